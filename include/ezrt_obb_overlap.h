/* ezrt_obb_overlap.h -- stream-ordered oriented-box queries on device memory (libezrt_hip.so only).
 *
 * Which triangles touch this ROTATED box: a robot link, a vehicle's footprint, a rotated tool holder, a brick of a rotated grid, a
 * part's own oriented bounding box, a picking volume along the view direction.  ezrt_query_box_overlap_device (ezrt_box_overlap.h)
 * takes axis-aligned boxes only; asked for the hull of a rotated box it returns far too many triangles -- a thin box along a diagonal
 * fills a few per cent of its hull -- and its row of at most 64 ids is then a truncated list that no filter can mend.  The rule
 * below is the exact separating-axis test of a closed triangle against a closed parallelepiped, it is defined on the triangle array
 * alone, and it is pinned operation by operation.
 *
 *   centre3    n x 3 floats: the centre c of every box
 *   axes9      n x 9 floats: its three half-axis vectors u0 u1 u2
 *
 * Box i is the set c + s0 u0 + s1 u1 + s2 u2 with |s_j| <= 1 for every j.  The vectors need not be unit or orthogonal: a sheared box
 * (a parallelepiped) is allowed, and the thirteen directions below are the complete separating-axis set for it too -- its three face
 * normals, the triangle's normal, and the nine cross products of a box edge with a triangle edge.
 *
 * THE DEFINITION.  No contraction anywhere (-ffp-contract=off, as everywhere in the library); one rounding per written operation.
 * Everything is fp64 (IEEE binary64, round to nearest even) on the fp32 inputs converted exactly.  With
 *   d(x, y)     = (double)x - (double)y,      U_j = (double)u_j  (component by component),      j + 1 and j + 2 taken modulo 3,
 *   dot(a, b)   = (a[0]*b[0] + a[1]*b[1]) + a[2]*b[2]
 *   cross(a, b) = (a[1]*b[2] - a[2]*b[1],  a[2]*b[0] - a[0]*b[2],  a[0]*b[1] - a[1]*b[0])
 * per box:
 *   n_j        = cross(U_{j+1}, U_{j+2}),   r_j = |dot(n_j, U_j)|                                 (the three face directions)
 *   h[c]       = (|U_0[c]| + |U_1[c]|) + |U_2[c]|,   hull_lo[c] = (double)c[c] - h[c],   hull_hi[c] = (double)c[c] + h[c]
 * Box i is LIVE when its twelve numbers are finite and r_0 > 0 && r_1 > 0 && r_2 > 0.  A box that is not live overlaps nothing.
 * A box without volume -- a zero axis, two parallel axes, three coplanar axes -- has lost the directions that would separate a
 * coplanar triangle from it, so it is not live; a caller who means a rectangle or a segment gives a THIN box in its place.
 *
 * Triangle k (p1 p2 p3 of triangle k of the array given to ezrt_scene_create) OVERLAPS the live box when all its nine coordinates are
 * finite and H0 .. H3 hold.  H0 and H1 are on the three vertices x in any order:
 *   H0  on every axis c: some vertex has (double)x[c] <= hull_hi[c] and some vertex has (double)x[c] >= hull_lo[c]      (the hull)
 *   p_j(x) = dot(n_j, (d(x[0],c[0]), d(x[1],c[1]), d(x[2],c[2])))
 *   H1  for every j: some vertex has p_j(x) <= r_j and some vertex has p_j(x) >= -r_j                     (the three face directions)
 * The vertices are then put in the order of their VALUES, v0 <= v1 <= v2, by the three compare-and-swaps of ezrt_inside.h (`less`
 * and the swaps as written out in ezrt_box_overlap.h), and
 *   e1  = (d(v1[0],v0[0]), d(v1[1],v0[1]), d(v1[2],v0[2])),   e2 the same of v2 and v0,   N = cross(e1, e2)
 *   s   = dot(N, (d(c[0],v0[0]), d(c[1],v0[1]), d(c[2],v0[2]))),   R = (|dot(N,U_0)| + |dot(N,U_1)|) + |dot(N,U_2)|
 *   H2  |s| <= R                                                                                        (the triangle's plane)
 *   for each edge (A, B; C) of (v0, v1; v2), (v1, v2; v0), (v0, v2; v1), with e = (d(B[0],A[0]), d(B[1],A[1]), d(B[2],A[2])),
 *   and for each j = 0, 1, 2:
 *     a   = cross(U_j, e)
 *     t   = dot(a, (d(C[0],A[0]), d(C[1],A[1]), d(C[2],A[2])))                                   (A and B project to 0, C to t)
 *     s   = dot(a, (d(c[0],A[0]), d(c[1],A[1]), d(c[2],A[2]))),   R = |dot(a,U_{j+1})| + |dot(a,U_{j+2})|
 *     the direction SEPARATES when s - R > max(0, t) || s + R < min(0, t)
 *   H3  none of the nine directions separates
 *   overlaps(i, k) = box i is live && triangle k is finite && H0 && H1 && H2 && H3
 *
 * What the rule guarantees.
 * - It is the separating-axis test of a CLOSED triangle against a CLOSED parallelepiped.  Every comparison admits equality, so
 *   touching counts: a vertex on a corner, on an edge or in a face, a box corner on the triangle.
 * - A degenerate triangle overlaps as the segment or point it is.  Its normal is zero -- s = R = 0 and H2 holds -- and the remaining
 *   directions test it completely: the three of H1 and the cross products of the box edges with the segment's direction are the
 *   complete set of a segment against the box; with three equal vertices every e is zero and H1, point in box, decides alone.
 * - A triangle with a non-finite vertex never overlaps, not even a box that holds everything.
 * - From finite fp32 inputs no fp64 operation here overflows, underflows to zero or yields a NaN.  |U| < 2^128 and |d| < 2^129.  Every
 *   component of a cross product is a difference of two products of two such numbers: below 2^259.  Every dot is a sum of three
 *   products of such a component with a U or a d: each product below 2^388, the dot below 2^390, R and s +- R below 2^392 -- far from
 *   2^1024.  A non-zero fp32 number or difference of two has magnitude >= 2^-149, so a non-zero product of two is >= 2^-298 and of
 *   three >= 2^-447, far above 2^-1022: no product of non-zero factors is a zero or a subnormal, and nothing here multiplies more
 *   than three.  A zero times a finite number is a zero; no infinity arises, hence no NaN.
 * - Exactness.  On integer or fixed-point coordinates of b bits (centres, axes and triangles on one grid, |x| < 2^b steps) every U
 *   has b bits and every d b + 1.  n_j and a are below 2^(2b+2) and N below 2^(2b+3); p_j is below 2^(3b+4), the t and s of an edge
 *   direction below 2^(3b+5) and s +- R below 2^(3b+6); the plane's s is below 2^(3b+6) and its R below 2^(3b+7).  All of them are
 *   integers, exact while 3 b + 7 <= 53: up to b = 15, a grid of 2^15 steps.  Within that budget every number above is the exact one
 *   and the rule is THE exact answer: the separating-axis theorem for these thirteen directions.  Beyond it every product and sum is
 *   rounded once (2^-53): the answers are still pinned, operation by operation, but a triangle within about 2^-50, relative to the
 *   extent of the triangle and the box, of touching the box may be given either answer.
 * - H0 changes nothing in exact arithmetic: a triangle outside the hull is outside the box, and one of the thirteen directions says
 *   so.  It is part of the definition so that a traversal may skip a box on comparisons alone, with no slack and no proof, even
 *   where the fp64 predicates are no longer exact: by H0 an overlapping triangle's own bounding box passes `lo[c] <= hull_hi[c] &&
 *   hi[c] >= hull_lo[c]`, and so does every box that holds it.  Comparing an fp32 value with an fp64 bound is the same as comparing
 *   it with that bound rounded INWARD to fp32 (hull_hi toward minus infinity, hull_lo toward plus infinity).
 * - H1 lets a traversal prune on the box's own face directions, again without slack.  For a box [lo, hi] of fp32 numbers let
 *     pmin_j = p_j(the corner with lo[c] where n_j[c] >= 0 and hi[c] otherwise),   pmax_j = p_j(the opposite corner)
 *   evaluated by the very expression of p_j.  Rounding to nearest is monotone; d(x, c) is monotone in x, a product with a fixed
 *   factor is monotone (rising or falling with the factor's sign) and a sum is monotone in each operand.  So pmin_j <= p_j(v) <=
 *   pmax_j ON THE BITS for every fp32 point v inside [lo, hi], and a box with pmin_j > r_j || pmax_j < -r_j holds only triangles
 *   that fail H1.  (A NaN -- 0 times an infinite bound -- fails both comparisons: such a box is not skipped.)
 * - The vertex order and the winding of a triangle do not matter to a single bit, and neither does the order of the triangles: H0 and
 *   H1 ask "some vertex", the vertices are sorted before any other arithmetic, the count is an integer sum and the list is a set of
 *   lowest indices.  NOTHING DEPENDS ON THE TREE.
 * - NOT promised: the same bits for two parametrisations of one box.  Permuting or negating the axes gives the same set of points
 *   but other roundings off the grid, and a triangle within a rounding of touching may then be answered differently.
 *
 * ezrt_query_obb_overlap_device writes, for box i,
 *   n_overlap[i]    the full number of overlapping triangles                                       (may be NULL when max_k > 0)
 *   tri_id row i    the min(max_k, n_overlap[i]) LOWEST indices of them in ascending order, then -1
 * A row of K entries is therefore a prefix of every longer one, the answer does not depend on the tree, and it survives a retree or
 * a refit of unchanged geometry.  max_k is in 0 .. EZRT_OBB_OVERLAP_MAX; with max_k == 0 tri_id is ignored and n_overlap is
 * required: a count-only call.  A caller who needs every triangle of a box with n_overlap[i] > max_k reads n_overlap and asks again
 * with the box split into smaller ones (a triangle that several parts touch is reported by each), or pages by triangle ranges
 * itself: scenes created from slices of the array, or ezrt_obb_overlap_at_device on the ranges it holds.
 *
 * ezrt_obb_overlap_at_device writes overlaps[i] = overlaps(box i, triangle tri_id[i]) as 0 / 1; an id outside the scene writes 0.
 * It narrows candidates the caller already holds, as ezrt_box_overlap_at_device does, and it is the direct probe of the per-triangle
 * function.
 *
 * How it is computed.  n_j, r_j and the hull are computed once per box.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1;
 * decided per call, a refit can change it) one box per lane walks the 4-wide records depth-first and descends a slot when it passes
 * two gates: the six fp32 comparisons of H0 against the hull rounded inward, and behind them pmin_j <= r_j && pmax_j >= -r_j for the
 * three face directions -- see H0 and H1.  Triangles below no leaf are swept after the walk.  Otherwise (malformed or tiny scenes)
 * the same per-triangle function sweeps all n_tri triangles.  The list is kept sorted in the box's own output row.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its n (or n x 3, n x 9, n x max_k) elements (anything else is rejected before any launch, never dereferenced); work is
 * enqueued on `stream` and the call returns without synchronising; no scratch set is used; the calls may run beside
 * ezrt_render_device and the other queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit
 * (ezrt_refit.h) waits for them, and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, centre3 or axes9; max_k outside 0 ..
 * EZRT_OBB_OVERLAP_MAX; max_k > 0 with NULL tri_id; max_k == 0 with NULL n_overlap; NULL tri_id or overlaps
 * (ezrt_obb_overlap_at_device); n < 0; a pointer that is not device memory of the scene's device.  n == 0 returns 0 and launches
 * nothing. */
#ifndef EZRT_OBB_OVERLAP_H
#define EZRT_OBB_OVERLAP_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_OBB_OVERLAP_MAX 64

int ezrt_query_obb_overlap_device(EzrtScene* s, const float* centre3 /* n x 3 */, const float* axes9 /* n x 9: u0 u1 u2 */, int n, int max_k,
                                  int32_t* tri_id /* n x max_k, or NULL when max_k == 0 */, int32_t* n_overlap /* n, or NULL */, void* stream);
int ezrt_obb_overlap_at_device(EzrtScene* s, const float* centre3 /* n x 3 */, const float* axes9 /* n x 9 */, const int32_t* tri_id /* n */,
                               int n, uint8_t* overlaps /* n */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
