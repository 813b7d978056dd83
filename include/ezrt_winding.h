/* ezrt_winding.h -- stream-ordered winding-number queries on device memory (libezrt_hip.so only).
 *
 * How many times does the mesh wrap around a point: the generalised winding number (Jacobson, Kavan, Sorkine-Hornung 2013), the sum
 * over the triangles of the solid angle each subtends at the point, divided by 4 pi.  It is 1 inside and 0 outside a closed mesh
 * that faces outwards (-1 inside one that faces inwards), it degrades smoothly across a hole or a doubled sheet where the parity of
 * ezrt_inside.h is no topological fact and differs between axes, it is additive over meshes, and it needs no tree: occupancy grids,
 * signed-distance signs and containment tests of scanned or hand-made meshes -- holes, duplicated faces, self-crossings -- threshold
 * it at 0.5.
 *
 *   points3    n x 3 floats: the query points
 *
 * THE DEFINITION.  No contraction anywhere (-ffp-contract=off, as everywhere in the library); one rounding per written operation.
 * With d(x, y) = (double)x - (double)y, the term q_k of point p and triangle k (p1 p2 p3 of triangle k of the array given to
 * ezrt_scene_create):
 *
 * W1  The vertices are put in the order of their VALUES, v0 <= v1 <= v2, with
 *       less(x, y) = x.x < y.x || (x.x == y.x && (x.y < y.y || (x.y == y.y && x.z < y.z)))
 *       if less(p2, p1) swap(p1, p2);  if less(p3, p2) swap(p2, p3);  if less(p2, p1) swap(p1, p2);   (v0 v1 v2) = (p1 p2 p3)
 *     -- the three compare-and-swaps of ezrt_inside.h -- and sgn = -1 if an odd number of them swapped, else +1: the parity of the
 *     permutation.  This depends on the triangle alone, not on p.  q_k = 0 if any coordinate of the triangle or of p is not finite,
 *     or if v0 == v1 or v1 == v2 on all three coordinates (two vertices equal by value; -0 equals +0).
 * W2  fp64 (IEEE binary64, round to nearest even) on the fp32 values converted exactly:
 *       a = (d(v0.x,p.x), d(v0.y,p.y), d(v0.z,p.z)),  b and c likewise from v1 and v2
 *       nx = b.y*c.z - b.z*c.y    ny = b.z*c.x - b.x*c.z    nz = b.x*c.y - b.y*c.x
 *       det = (a.x*nx + a.y*ny) + a.z*nz
 *       la = sqrt((a.x*a.x + a.y*a.y) + a.z*a.z),  lb and lc likewise            (IEEE sqrt: correctly rounded)
 *       ab = (a.x*b.x + a.y*b.y) + a.z*b.z,  bc = (b.x*c.x + b.y*c.y) + b.z*c.z,  ca = (c.x*a.x + c.y*a.y) + c.z*a.z
 *       den = (((la*lb)*lc + ab*lc) + bc*la) + ca*lb
 *     Van Oosterom and Strackee (1983): the solid angle of the triangle at p is Omega = 2 atan2(det, den).
 * W3  q_k = 0 if det == 0, or det or den is not finite, or m = max(|det|, |den|) is 0.  A point in the plane of a triangle, on it or
 *     not, contributes nothing: the mean of the two one-sided limits (+-2 pi on the triangle, 0 off it), independent of the winding.
 *     Otherwise
 *       t = ez_atan2((float)(det / m), (float)(den / m))        the fp32 definition of ezrt_detmath.h; t in [-pi, pi]
 *       t = sgn * t                                             (exact)
 * W4  q_k = llrint((double)t * 0x1p36)                          round to nearest even; the product is exact
 * W5  fixed(p)   = S = sum over k in [0, n_tri) of q_k          an int64 sum; S = 0 for a p with a non-finite coordinate
 *     winding(p) = (float)(((double)S * 0x1p-36) * 0x1.45f306dc9c883p-3)        the constant is 1 / (2 pi) rounded to binary64
 *
 * The budget of the sum.  |t| <= pi < 4, so |q_k| < 2^38; n_tri <= 2^24 (a leaf reference holds 24 bits); |S| < 2^62: S cannot
 * overflow an int64, and neither can the sum of the `fixed` of two scenes.
 *
 * What the rule guarantees, all of it on the bits of `fixed`.
 * - The sum is an integer sum: the order of the triangles does not matter to a bit, and neither does the tree, the split of the work
 *   across workgroups or the order of atomic additions.  NOTHING DEPENDS ON THE TREE; no entry point here reads it.
 * - Any re-ordering of a triangle's vertices that keeps its winding leaves q_k unchanged: the vertices are sorted before any
 *   arithmetic, and the parity is the same.  Flipping a triangle's winding negates q_k exactly (sgn changes, nothing else; llrint is
 *   odd).
 * - A mesh given twice has exactly twice the `fixed`; `fixed` of two scenes may be added by the caller -- for parts of a mesh, and
 *   for one mesh split over several devices.
 * - From fp32 inputs no fp64 operation of W2 overflows (|a| < 2^129: det and den below 2^390).
 *
 * Accuracy against the real-number value (derived).  det and den carry a relative error of a few 2^-53 of their terms' magnitudes,
 * far below fp32; per term the error is a few fp32 ulps of |t| from ez_atan2 and the two conversions to float, plus 2^-37 from W4:
 *   |winding - exact| <= (2^-22 * sum_k |t_k| + n_tri * 2^-37) / (2 pi) + 2^-24 |winding|
 * tests/test_winding_expected.py holds the numpy restatement of this rule to that bound against a float64 evaluation.  Within a few
 * 2^-53 (relative to the triangle's and the point's extent) of a triangle's plane the sign of det -- and over the triangle itself a
 * jump of half a winding -- is the rounded expression's: the value is pinned there as everywhere, and is that of one of the two sides.
 *
 * ezrt_query_winding_device writes fixed and, where asked for, winding.  `fixed` is REQUIRED: it is the accumulator of the call as
 * well as an output.  `chunks` splits the triangle range into that many slices, each summed by workgroups of its own and added into
 * `fixed` with 64-bit integer atomics (so the answer does not depend on it): chunks == 0 lets the library choose -- a pure function
 * of n and n_tri, which ezrt_winding_chunks returns: one slice where the points alone fill the device, otherwise enough to, of at
 * least 256 triangles each -- chunks >= 1 forces that many (clamped to n_tri, and to 65535), chunks < 0 is EZRT_ERR_INVALID.  With
 * more than one slice `fixed` is zeroed on the stream first, whatever it held.
 * ezrt_winding_at_device writes the single term q_k (and its winding, the same conversion) of point i and triangle tri_id[i], for
 * pairs the caller holds; an id outside the scene gives 0.
 *
 * How it is computed.  There is no pruning in an exact sum: one point per lane, every lane of a workgroup loops over the same slice of
 * the triangles and keeps its S in registers.  W1 -- the sort and sgn, which depend on the triangle alone -- is evaluated once per
 * triangle and workgroup: each lane sorts one triangle of a tile of 64 into LDS, and the wave reads the tile as a broadcast.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its n elements (anything else is rejected before any launch, never dereferenced); work is enqueued on `stream` and the
 * call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the other queries on
 * other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them, and a call
 * issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, points3 or fixed; NULL tri_id (ezrt_winding_at_device);
 * n < 0; chunks < 0; a pointer that is not device memory of the scene's device.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_WINDING_H
#define EZRT_WINDING_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_winding_device(EzrtScene* s, const float* points3 /* n x 3 */, int n, int chunks,
                              int64_t* fixed /* n, required: accumulator and output */, float* winding /* n or NULL */, void* stream);
int ezrt_winding_at_device(EzrtScene* s, const float* points3 /* n x 3 */, const int32_t* tri_id /* n */, int n, int64_t* fixed /* n */,
                           float* winding /* n or NULL */, void* stream);
/* the number of slices a call with chunks == 0 uses for n points and a scene of n_tri triangles (no device work; never fails) */
int ezrt_winding_chunks(int n, int n_tri);

#ifdef __cplusplus
}
#endif
#endif
