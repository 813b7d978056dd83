/* ezrt_plane.h -- stream-ordered plane queries on device memory (libezrt_hip.so only).
 *
 * Cut the mesh with a plane: which triangles does the plane cross, and in which segment each -- the cross-section of the mesh as a
 * soup of oriented segments that chain into closed loops by comparing bits.  Slicing for additive manufacturing, section views and
 * contour lines, silhouettes against a clipping plane, girths and cross-section areas.  A zero-thickness ezrt_box_overlap.h box gives
 * ids without the section, counts a vertex on the plane for every triangle around it, and stops at 64 ids; a section is useless
 * truncated, so this is also the library's first COMPLETE variable-length answer: count, offsets, fill (CSR), in a pinned order.
 *
 *   planes4    n x 4 floats (a, b, c, d): the points with a x + b y + c z = d.  The normal (a, b, c) need not be unit.
 *
 * THE DEFINITION.  No contraction anywhere (-ffp-contract=off, as everywhere in the library); one rounding per written operation;
 * everything is fp64 (IEEE binary64, round to nearest even) on the fp32 inputs converted exactly, except where fp32 is written.
 *
 * P1  Plane i is LIVE when a, b, c and d are finite and (a, b, c) != (0, 0, 0).  A plane that is not live crosses nothing.
 * P2  The side of a vertex v (three fp32 values) of a live plane:
 *       s(v) = (((double)a*v.x + (double)b*v.y) + (double)c*v.z) - (double)d
 *     Each product of two fp32 values is exact in fp64, so s costs three roundings.  v is UP when s(v) >= 0 and DOWN when s(v) < 0:
 *     a vertex ON the plane counts as UP, the half-open rule (-0 is >= 0).  s depends on the vertex's VALUE and the plane alone,
 *     never on the triangle: a vertex shared by value has one side in every triangle that holds it.
 * P3  Triangle k (p1 p2 p3 of triangle k of the array given to ezrt_scene_create) is CROSSED by a live plane when its nine
 *     coordinates are finite and its vertices are neither all UP nor all DOWN.  So
 *     - a triangle lying in the plane (three zeros: all UP) is NOT crossed.  This is the slicer's convention: a face in the cutting
 *       plane belongs to the layer boundary of the solid on one side only, and its outline is already drawn by its neighbours;
 *     - a triangle that touches the plane from the DOWN side with one vertex is crossed, in a segment of length zero; with an edge,
 *       in that edge; one that touches from the UP side is not crossed;
 *     - the planes (a, b, c, d) and (-a, -b, -c, -d) are the same set of points and differ in exactly these cases.
 * P4  The end point on an edge.  A crossed triangle has exactly two edges whose ends differ in side.  The ends of such an edge are
 *     put in the order of their VALUES, A < B, with the `less` of ezrt_inside.h and ezrt_winding.h on (x, y, z):
 *       less(x, y) = x.x < y.x || (x.x == y.x && (x.y < y.y || (x.y == y.y && x.z < y.z)))          A = less(Y, X) ? Y : X
 *     (ends that differ in side differ in value, and -0 == +0 gives one side to both).  Then, per coordinate c:
 *       if s(A) == 0   P = A                                       (the fp32 values themselves, the sign of a zero included)
 *       elif s(B) == 0 P = B
 *       else           t = s(A) / (s(A) - s(B))                    opposite strict signs: no cancellation, 0 <= t <= 1
 *                      P[c] = (float)((double)A[c] + t * ((double)B[c] - (double)A[c]))
 *                      lo = B[c] < A[c] ? B[c] : A[c],  hi = B[c] < A[c] ? A[c] : B[c]                 (fp32)
 *                      P[c] = P[c] < lo ? lo : (P[c] > hi ? hi : P[c])                                (fp32: the clamp)
 *     The point is a function of the edge's two values and the plane ALONE: two triangles that share an edge by value get the same
 *     point ON THE BITS, whichever way round each holds it.
 * P5  Orientation.  Walk the boundary in the stored order p1 -> p2 -> p3 -> p1: exactly one of the three directed edges goes from
 *     UP to DOWN and exactly one from DOWN to UP.  q0 is P4's point of the first, q1 that of the second; the row of the triangle is
 *     seg = (q0.x q0.y q0.z q1.x q1.y q1.z).  With N the triangle's normal (p2 - p1) x (p3 - p1) and n = (a, b, c), q0 -> q1 runs
 *     along n x N: for a mesh with outward counter-clockwise windings the material is on the segment's LEFT seen from the side the
 *     plane's normal points to, outer loops run counter-clockwise and holes clockwise -- for (a, b, c, d) and for its negation alike.
 *     Re-ordering a triangle's vertices within its winding changes nothing to a bit (the same three directed edges); flipping the
 *     winding swaps q0 and q1 and changes nothing else.  A degenerate triangle (two vertices equal by value, or three in a line) is
 *     cut as the segment it is: two equal vertices give q0 == q1 on the bits.
 * P6  The answer of plane i is the list of its crossed triangles in ASCENDING id with their rows; the answers of the planes follow
 *     one another in the order of the planes (CSR: offsets[i] .. offsets[i + 1]).
 *
 * What the rule guarantees.
 * - NOTHING DEPENDS ON THE TREE (no entry point here reads it), on the order of the triangles beyond the ids themselves, or on the
 *   split of the work (`slices`): the classification and the points are per-pair functions, and the order is by id.
 * - Loops.  On a closed, consistently wound manifold every edge is held by two triangles in opposite directions, so the directed
 *   edge that is UP -> DOWN in one is DOWN -> UP in the other, and by P4 both get the same bits: every bit pattern of an end point
 *   occurs exactly as often as a q0 as it does as a q1.  Sections chain into closed loops by a dictionary on the 12 bytes of an end
 *   point, without tolerance.  (A vertex stored as -0 in one triangle and +0 in another is two bit patterns where P4 copies it.)
 * - No overflow.  From finite fp32 inputs |a v.x| < 2^256 and |s| < 2^259; |s(A) - s(B)| < 2^260; |B[c] - A[c]| < 2^129: no fp64
 *   operation of P2 or P4 overflows, and none yields a NaN (t is a quotient of finite numbers with a non-zero divisor).
 * - Exactness of the classification.  Let the coordinates be integer multiples of a power of two u, at most 2^25 u in magnitude,
 *   a, b, c integer multiples of a power of two w, at most 2^25 w, and d an integer multiple of u w with |d| <= 2^51 u w (integer
 *   coordinates and coefficients up to 2^25; a grid of spacing 2^-j, j <= 26, for both; ...).  Then every term of P2 is an integer
 *   multiple of u w, the partial sums are at most 2^51, 1.5 * 2^51 and 2.5 * 2^51 < 2^53 of them: every s is EXACT, and UP / DOWN / on-the-plane is
 *   the exact classification.  Beyond that each s carries at most three roundings: the classification is still pinned and still
 *   one per vertex value, but a vertex within a few 2^-53 (relative to |a v.x| + |b v.y| + |c v.z| + |d|) of the plane may be given
 *   either side.
 * - Accuracy of the end point (derived) on such a grid, against the exact rational point P* of the edge's line and the plane.  s(A)
 *   and s(B) are exact and so is s(A) - s(B) = n . (A - B), an integer multiple of u w below 2^53.  t carries ONE rounding (the
 *   division: relative 2^-53); B[c] - A[c] is exact; the product t * (B[c] - A[c]) is rounded once (relative 2^-53), and so is the
 *   sum.  With M = max(|A[c]|, |B[c]|), |B[c] - A[c]| <= 2 M and |A[c] + t (B[c] - A[c])| <= M: the fp64 value v is within
 *   (2^-52 + 2^-52 + 2^-53) M (1 + 2^-52) < 2^-50 M of P*[c].  The conversion to fp32 adds at most 2^-24 |v|, and the clamp can only
 *   move P[c] towards P*[c], which lies in [lo, hi].  So
 *       |P[c] - P*[c]| <= 2^-24 |P*[c]| + 2^-49 max(|A[c]|, |B[c]|)
 *   -- the final rounding to fp32, plus THREE fp64 roundings (t, the product, the sum), not one; the fp64 part is 2^-25 of the
 *   fp32 part and never shows in an fp32 result unless v lands within it of a rounding boundary.  tests/test_plane_expected.py holds
 *   the numpy restatement of this rule to that bound against exact rational arithmetic.
 *
 * THE CALLS.
 * ezrt_plane_slices(n, n_tri, slices) does no device work and returns S, the effective number of slices of the triangle range for
 * a call with n planes on a scene of n_tri triangles: slices == 0 is the library's choice, a pure function of n and n_tri (enough
 * slices that the waves -- one per slice and tile of 64 planes -- number 16384, none below 256 triangles); slices >= 1 is
 * clamped to ceil(n_tri / 64) and to 4096; S >= 1 always (also for n <= 0, n_tri <= 0 or slices < 0).  Slice j is the triangle
 * range [j L, min((j + 1) L, n_tri)) with L = 64 * ceil(ceil(n_tri / S) / 64); trailing slices may be empty.
 * ezrt_query_plane_count_device writes part[i S + j], the number of crossed triangles of plane i in slice j (n x S, REQUIRED: it is
 * what the fill call places its rows by), n_cross[i], their sum, and -- where asked for -- offsets, the exclusive prefix sum of
 * n_cross in int64 with the total in offsets[n].
 * ezrt_query_plane_section_device takes planes4, n and slices as given to the count call and part and offsets exactly as it left
 * them, and writes P6: rows offsets[i] .. offsets[i + 1] of tri_id and seg hold plane i's crossed triangles in ascending id.  A row
 * index >= capacity is not written: the caller sees the overflow in offsets[n] > capacity and may call again with larger arrays
 * (the count need not be repeated).  seg may be NULL (ids only).  Rows below capacity that belong to no plane are not touched.
 * ezrt_plane_section_at_device answers pairs the caller holds, plane i against triangle tri_id[i]: crosses (0 / 1), side (-1 / 0 / +1:
 * the sign of s of p1 p2 p3; 0 is ON the plane, which P2 counts as UP -- what lets a caller apply a closed touching rule of their
 * own) and seg.  An id outside the scene, a plane that is not live or a triangle with a non-finite coordinate writes zeros
 * everywhere; a pair that is not crossed has a zero seg.  The sum of crosses over all ids is n_cross.
 *
 * How it is computed.  There is no tree walk: a plane's candidates are no small set, and the all-pairs sweep is what fills the device
 * when there are few planes.  One wave per (slice, tile of 64 planes): each lane holds one triangle of a round of 64, converted to
 * fp64 once; the plane is uniform across the wave (the tile's planes are staged in LDS and read as a broadcast); per plane 18 fp64
 * operations, a ballot of the crossed lanes and its population count into the plane's counter.  The fill pass repeats the sweep
 * and numbers the crossed lanes by the count of set ballot bits below each: ascending ids without a sort or a barrier between
 * waves; P4 runs for crossed lanes only.  The prefix sum over the planes is a small kernel of its own.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its elements (anything else is rejected before any launch, never dereferenced); work is enqueued on `stream` and the
 * call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the other queries on
 * other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them, and a call
 * issued after the refit returned sees the new geometry (count and fill must see the same).
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene or planes4; NULL part or n_cross (count); NULL part,
 * offsets or tri_id (section); NULL tri_id or crosses (section_at); n < 0; slices < 0; capacity < 0; a pointer that is not device
 * memory of the scene's device.  n == 0 returns 0 and launches nothing (offsets[0] is then not written either). */
#ifndef EZRT_PLANE_H
#define EZRT_PLANE_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the effective number of slices (no device work; never fails) */
int ezrt_plane_slices(int n, int n_tri, int slices);
int ezrt_query_plane_count_device(EzrtScene* s, const float* planes4 /* n x 4 */, int n, int slices, int32_t* part /* n x S, required */,
                                  int32_t* n_cross /* n */, int64_t* offsets /* n + 1, or NULL */, void* stream);
int ezrt_query_plane_section_device(EzrtScene* s, const float* planes4 /* n x 4 */, int n, int slices, const int32_t* part /* n x S */,
                                    const int64_t* offsets /* n + 1 */, int64_t capacity, int32_t* tri_id /* capacity */,
                                    float* seg /* capacity x 6: q0 then q1, or NULL */, void* stream);
int ezrt_plane_section_at_device(EzrtScene* s, const float* planes4 /* n x 4 */, const int32_t* tri_id /* n */, int n, uint8_t* crosses /* n */,
                                 int8_t* side /* n x 3 or NULL */, float* seg /* n x 6 or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
