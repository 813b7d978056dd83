/* ezrt_box_overlap.h -- stream-ordered box-overlap queries on device memory (libezrt_hip.so only).
 *
 * Which triangles touch this axis-aligned box: the question behind voxelisation and occupancy grids (which cells does the surface
 * pass through -- ezrt_query_inside_device answers for the cells' centres only), collision broad phase and clearance boxes, binning
 * triangles into tiles or bricks, cutting a working set out of a large mesh, picking with a marquee.  ezrt_query_nearest_device with a
 * radius returns a ball, not a box, and cannot say "touches".  The rule below can: it is the exact separating-axis test, it is
 * defined on the triangle array alone, and it is pinned operation by operation.
 *
 *   box_lo3    n x 3 floats: the lower corner of every box
 *   box_hi3    n x 3 floats: the upper corner
 *
 * THE DEFINITION.  No contraction anywhere (-ffp-contract=off, as everywhere in the library); one rounding per written operation.
 *
 * Box i is LIVE when its six numbers are finite and lo[c] <= hi[c] on every axis c.  A box of zero thickness, or a single point, is
 * live.  A box that is not live overlaps nothing.
 *
 * Triangle k (p1 p2 p3 of triangle k of the array given to ezrt_scene_create) OVERLAPS the live box [lo, hi] when all its nine
 * coordinates are finite and H1 .. H3 hold.  H1 is fp32 comparisons on the three vertices in any order:
 *   H1  on every axis c: some vertex has x[c] <= hi[c] and some vertex has x[c] >= lo[c]          (the three box axes)
 * The vertices are then put in the order of their VALUES, v0 <= v1 <= v2, lexicographic on (x, y, z), with
 *   less(x, y) = x[0] < y[0] || (x[0] == y[0] && (x[1] < y[1] || (x[1] == y[1] && x[2] < y[2])))
 *   if less(p2, p1) swap(p1, p2);  if less(p3, p2) swap(p2, p3);  if less(p2, p1) swap(p1, p2);   (v0 v1 v2) = (p1 p2 p3)
 * -- the three compare-and-swaps of ezrt_inside.h -- and everything below is fp64 (IEEE binary64, round to nearest even) on the fp32
 * values converted exactly; with d(x, y) = (double)x - (double)y:
 *   the box's interval on an axis a, relative to a point A:
 *     bmin(a, A) = (t0 + t1) + t2,   t_c = a[c] >= 0 ? a[c]*d(lo[c],A[c]) : a[c]*d(hi[c],A[c])
 *     bmax(a, A) = (t0 + t1) + t2,   t_c = a[c] >= 0 ? a[c]*d(hi[c],A[c]) : a[c]*d(lo[c],A[c])
 *   e1  = (d(v1[0],v0[0]), d(v1[1],v0[1]), d(v1[2],v0[2])),   e2 the same of v2 and v0
 *   N   = (e1[1]*e2[2] - e1[2]*e2[1],  e1[2]*e2[0] - e1[0]*e2[2],  e1[0]*e2[1] - e1[1]*e2[0])
 *   H2  bmin(N, v0) <= 0 && bmax(N, v0) >= 0                                                     (the triangle's plane)
 *   for each edge (A, B; C) of (v0, v1; v2), (v1, v2; v0), (v0, v2; v1), with e = (d(B[0],A[0]), d(B[1],A[1]), d(B[2],A[2])),
 *   and for each box axis j = 0, 1, 2:
 *     a   has a[(j+1)%3] = -e[(j+2)%3],  a[(j+2)%3] = e[(j+1)%3],  a[j] = 0                       (e x the box axis j)
 *     t   = (a[0]*d(C[0],A[0]) + a[1]*d(C[1],A[1])) + a[2]*d(C[2],A[2])                          (A and B project to 0, C to t)
 *     the axis SEPARATES when bmin(a, A) > max(0, t) || bmax(a, A) < min(0, t)
 *   H3  none of the nine axes separates
 *   overlaps(i, k) = box i is live && triangle k is finite && H1 && H2 && H3
 *
 * What the rule guarantees.
 * - It is the separating-axis test of a CLOSED triangle against a CLOSED box: the three box axes (H1), the triangle's normal (H2)
 *   and the nine cross products of an edge with a box axis (H3).  Every comparison admits equality, so touching counts: a vertex on
 *   a face, an edge through a corner, a triangle in the plane of a face, a point box on the triangle.
 * - A degenerate triangle overlaps as the segment or point it is.  Its normal is zero -- bmin = bmax = 0 and H2 holds -- and its
 *   edge axes are those of a segment (its edges are parallel, so three of the nine directions are left, which with H1 is the
 *   complete test of a segment against a box); with three equal vertices every e is zero and H1, point in box, decides alone.
 * - A triangle with a non-finite vertex never overlaps, not even a box that holds everything.
 * - From finite fp32 inputs no fp64 operation here overflows or yields a NaN: |d| < 2^129, so |e| and |a| < 2^129, |N| < 2^259,
 *   every product is below 2^388 and every sum below 2^390, far from 2^1024; a zero times a finite number is a zero.
 * - Exactness.  On integer or fixed-point coordinates of b bits (triangles and boxes on one grid of 2^b steps) every d is exact and
 *   has b + 1 bits.  An edge axis needs 2 b + 3 bits for its sums -- exact up to 2^25 steps; the plane needs 3 b + 6 bits -- exact
 *   up to 2^15 steps.  Within that budget every number above is the exact one and the rule is THE exact answer: the separating-axis
 *   theorem for these thirteen directions.  Beyond it every product and sum is rounded once (2^-53): the answers are still pinned,
 *   operation by operation, but a triangle within about 2^-50, relative to the extent of the triangle and the box, of touching
 *   the box may be given either answer.
 * - H1 changes nothing in exact arithmetic.  It is part of the definition so that a traversal may skip a box on fp32 comparisons
 *   alone, with no slack and no proof, even where the fp64 predicates are no longer exact: by H1 an overlapping triangle's own
 *   bounding box passes `lo[c] <= box.hi[c] && hi[c] >= box.lo[c]`, and so does every box that holds it.
 * - The vertex order and the winding of a triangle do not matter to a single bit, and neither does the order of the triangles: the
 *   vertices are sorted before any arithmetic, the count is an integer sum and the list is a set of lowest indices.  NOTHING DEPENDS
 *   ON THE TREE.
 *
 * ezrt_query_box_overlap_device writes, for box i,
 *   n_overlap[i]    the full number of overlapping triangles                                       (may be NULL when max_k > 0)
 *   tri_id row i    the min(max_k, n_overlap[i]) LOWEST indices of them in ascending order, then -1
 * A row of K entries is therefore a prefix of every longer one, the answer does not depend on the tree, and it survives a retree or
 * a refit of unchanged geometry.  max_k is in 0 .. EZRT_BOX_OVERLAP_MAX; with max_k == 0 tri_id is ignored and n_overlap is
 * required: a count-only call.  A caller who needs every triangle of a box with n_overlap[i] > max_k reads n_overlap and asks again
 * with the box split into smaller ones (a triangle that several parts touch is reported by each), or pages by triangle ranges
 * itself: scenes created from slices of the array, or ezrt_box_overlap_at_device on the ranges it holds.
 *
 * ezrt_box_overlap_at_device writes overlaps[i] = overlaps(box i, triangle tri_id[i]) as 0 / 1; an id outside the scene writes 0.
 * It narrows candidates the caller already holds, as ezrt_closest_point_at_device and ezrt_surface_at_device do, and it is the
 * direct probe of the per-triangle function.
 *
 * How it is computed.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1; decided per call, a refit can change it) one box
 * per lane walks the 4-wide records depth-first and descends a slot when slot.lo[c] <= hi[c] && slot.hi[c] >= lo[c] on all three
 * axes -- comparisons only, see H1.  Triangles below no leaf are swept after the walk.  Otherwise (malformed or tiny scenes) the
 * same per-triangle function sweeps all n_tri triangles.  The list is kept sorted in the box's own output row.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its n (or n x 3, n x max_k) elements (anything else is rejected before any launch, never dereferenced); work is enqueued
 * on `stream` and the call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the
 * other queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them,
 * and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, box_lo3 or box_hi3; max_k outside 0 ..
 * EZRT_BOX_OVERLAP_MAX; max_k > 0 with NULL tri_id; max_k == 0 with NULL n_overlap; NULL tri_id or overlaps
 * (ezrt_box_overlap_at_device); n < 0; a pointer that is not device memory of the scene's device.  n == 0 returns 0 and launches
 * nothing. */
#ifndef EZRT_BOX_OVERLAP_H
#define EZRT_BOX_OVERLAP_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_BOX_OVERLAP_MAX 64

int ezrt_query_box_overlap_device(EzrtScene* s, const float* box_lo3 /* n x 3 */, const float* box_hi3 /* n x 3 */, int n, int max_k,
                                  int32_t* tri_id /* n x max_k, or NULL when max_k == 0 */, int32_t* n_overlap /* n, or NULL */, void* stream);
int ezrt_box_overlap_at_device(EzrtScene* s, const float* box_lo3 /* n x 3 */, const float* box_hi3 /* n x 3 */, const int32_t* tri_id /* n */,
                               int n, uint8_t* overlaps /* n */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
