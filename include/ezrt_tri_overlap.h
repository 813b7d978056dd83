/* ezrt_tri_overlap.h -- stream-ordered triangle-overlap queries on device memory (libezrt_hip.so only).
 *
 * Which triangles of the scene does this triangle cross or touch: the narrow phase behind ezrt_box_overlap.h's broad phase, for a
 * caller who holds a second mesh -- a tool against a part, a character against a level, a cutting surface, or the scene's own
 * triangles in a self-intersection check.  The rule below is the exact separating-axis test of two closed triangles, it is defined on
 * the triangle array alone, and it is pinned operation by operation.
 *
 *   tris9      n x 9 floats: p1 p2 p3 of every query triangle
 *
 * THE DEFINITION.  No contraction anywhere (-ffp-contract=off, as everywhere in the library); one rounding per written operation.
 *
 * The vertices of a triangle with nine finite coordinates are put in the order of their VALUES, v0 <= v1 <= v2, lexicographic on
 * (x, y, z), with
 *   less(x, y) = x[0] < y[0] || (x[0] == y[0] && (x[1] < y[1] || (x[1] == y[1] && x[2] < y[2])))
 *   if less(p2, p1) swap(p1, p2);  if less(p3, p2) swap(p2, p3);  if less(p2, p1) swap(p1, p2);   (v0 v1 v2) = (p1 p2 p3)
 * -- the three compare-and-swaps of ezrt_inside.h.  Arithmetic is fp64 (IEEE binary64, round to nearest even) on the fp32 values
 * converted exactly; with d(x, y) = (double)x - (double)y and d3(X, Y) = (d(X[0],Y[0]), d(X[1],Y[1]), d(X[2],Y[2])) the NORMAL of the
 * triangle is
 *   e1 = d3(v1, v0),  e2 = d3(v2, v0)
 *   N  = (e1[1]*e2[2] - e1[2]*e2[1],  e1[2]*e2[0] - e1[0]*e2[2],  e1[0]*e2[1] - e1[1]*e2[0])
 * A triangle is LIVE when its nine coordinates are finite and N != (0, 0, 0).  The query triangle i and the scene triangle k (p1 p2
 * p3 of triangle k of the array given to ezrt_scene_create) are held to the same two conditions, and a triangle that is not live
 * overlaps nothing.
 *
 * THIS DEPARTS FROM THE BOX RULE, where a degenerate triangle overlaps as the segment or point it is.  There the other body has an
 * interior and the thirteen directions are complete for a segment or a point against it.  Here the directions below are complete for
 * two proper triangles; they are not for two collinear segments (the common line's in-plane normal is among them only by accident) or
 * for a point against a segment.  A pinned "nothing" is better than an unpinned "sometimes": a caller who needs segments asks with
 * thin proper triangles, or with ezrt_box_overlap.h.
 *
 * Live triangles Q (the query) and S (the scene's) OVERLAP when T1 and T2 hold.  T1 is fp32 comparisons on the six vertices in any
 * order:
 *   T1  on every axis c: some vertex of Q has x[c] <= some vertex of S, and some vertex of S has x[c] <= some vertex of Q
 * -- the closed overlap of the two bounding boxes.  For T2 the two triangles are put in the order of their values too: with
 * (q0 q1 q2) and (s0 s1 s2) the sorted vertices,
 *   (A, B) = (S, Q) when less(s0, q0) || (s0 == q0 && (less(s1, q1) || (s1 == q1 && less(s2, q2)))), else (Q, S)
 * (== on all three coordinates; when neither is less the two hold the same values and the choice changes nothing).  With a0 a1 a2 and
 * b0 b1 b2 their sorted vertices, every point is taken relative to a0,
 *   D1 = d3(a1, a0),  D2 = d3(a2, a0),  D3 = d3(b0, a0),  D4 = d3(b1, a0),  D5 = d3(b2, a0)
 * and a direction x = (x0, x1, x2) projects a point with difference D to
 *   p(x, D) = (x0*D[0] + x1*D[1]) + x2*D[2]
 * so that A spans the interval of {0, p(x, D1), p(x, D2)} (a0 projects to 0 by definition: nothing is computed for it) and B that of
 * {p(x, D3), p(x, D4), p(x, D5)}.  The direction SEPARATES when
 *   max(0, p(x,D1), p(x,D2)) < min(p(x,D3), p(x,D4), p(x,D5))  ||  max(p(x,D3), p(x,D4), p(x,D5)) < min(0, p(x,D1), p(x,D2))
 * The edges of a triangle with sorted vertices v0 v1 v2 are E0 = d3(v1, v0), E1 = d3(v2, v1), E2 = d3(v2, v0): e_i those of A, f_j
 * those of B.  The 29 directions, ALL of them always part of the rule (none is chosen or left out by a computed number):
 *   N_A, N_B                                     the two normals, as defined above                                        (2)
 *   e_i x f_j, i, j = 0, 1, 2                    (e[1]*f[2] - e[2]*f[1],  e[2]*f[0] - e[0]*f[2],  e[0]*f[1] - e[1]*f[0])      (9)
 *   g x axis_j, g = e_0 e_1 e_2 f_0 f_1 f_2, j = 0, 1, 2:   x[(j+1)%3] = -g[(j+2)%3],  x[(j+2)%3] = g[(j+1)%3],  x[j] = 0        (18)
 *   T2  none of the 29 directions separates
 *   overlaps(i, k) = Q is live && S is live && T1 && T2
 *
 * What the rule guarantees.
 * - It is the separating-axis test of two CLOSED triangles: they overlap when they share at least one point.  Every comparison that
 *   separates is strict, so touching counts: a vertex on a face, on an edge or on a vertex, edges that cross in a point, coplanar
 *   triangles that share an edge or a point.
 * - Every direction is sound: intervals of projections of sets that meet have a common point, so no direction separates them.
 * - The set is complete for two proper triangles.  Planes that are not parallel: the difference body A - B is a polytope whose
 *   faces are a face of one plus a vertex of the other (normals N_A, N_B) or two edges that are not parallel (e_i x f_j).  Parallel
 *   planes that differ: N_A separates.  ONE plane: the difference body is a polygon in that plane whose sides are edges g of A or
 *   B, and what separates is the in-plane normal of a side; g x axis_j is perpendicular to g, and it is parallel to N (useless in
 *   the plane) or zero exactly when N[j] == 0 -- so with an axis j that has N[j] != 0, which a live triangle has, it acts in the
 *   plane as that normal.  COPLANAR TRIANGLES ARE THEREFORE ANSWERED BY THE SAME RULE; nothing is decided by "are they coplanar",
 *   a question that a rounded number could not settle.
 * - From finite fp32 inputs no fp64 operation here overflows, underflows to a wrong zero or yields a NaN.  |d| < 2^129, so every
 *   component of an edge or a D is below 2^129, of a normal or a cross product below 2^259, a product with a D below 2^388 and a
 *   projection below 2^390: far from 2^1024, and no infinity arises, hence no NaN (0 times a finite number is a zero).  A d that
 *   is not zero is at least 2^-149 in magnitude, so a product of up to three factors that are not zero is at least 2^-447: a normal
 *   number, far above 2^-1022.  A product is therefore zero only when a factor is, and a sum or difference is zero only when its
 *   operands cancel as written.
 * - Exactness.  The highest degree in the coordinates is 3 (a normal or a cross product, degree 2, times a difference).  On integer
 *   or fixed-point coordinates of b bits (both triangles on one grid of 2^b steps) every d is exact and has b + 1 bits; a product
 *   of two has 2 b + 2 bits and a component of a normal or cross product 2 b + 3; times a D, 3 b + 4; the projection, a sum of three,
 *   3 b + 6 bits.  That fits binary64's 53 up to b = 15: exact on a grid of up to about 2^15 steps.  The 18 directions g x axis_j
 *   have degree 2 and need 2 b + 3 bits (exact to 2^25 steps).  Within that budget every number above is the exact one and the rule
 *   is THE exact answer.  Beyond it every product and sum is rounded once (2^-53): the answers are still pinned, operation by
 *   operation, but two triangles within about 2^-50, relative to their extent, of touching may be given either answer.
 * - T1 changes nothing in exact arithmetic (the three coordinate axes are sound directions).  It is part of the definition so that a
 *   traversal may skip a box on fp32 comparisons alone, with no slack and no proof, even where the fp64 projections are no longer
 *   exact: by T1 an overlapping scene triangle's own bounding box passes `lo[c] <= q.hi[c] && hi[c] >= q.lo[c]` against the query
 *   triangle's bounding box [q.lo, q.hi], and so does every box that holds it -- the argument of H1 in ezrt_box_overlap.h.
 * - The vertex order and the winding of EITHER triangle do not matter to a single bit, and neither does the order of the scene's
 *   triangles: both vertex triples are sorted before any arithmetic, the count is an integer sum and the list is a set of lowest
 *   indices.  NOTHING DEPENDS ON THE TREE.
 * - Swapping the roles gives the same answer to a bit: overlaps(Q against a scene that holds S) == overlaps(S against a scene that
 *   holds Q).  Liveness is a function of one triangle, T1 is symmetric as written, and T2 is computed on (A, B), which is chosen by
 *   the values and not by the roles.  A self-intersection check may therefore test each pair once.
 *
 * ezrt_query_tri_overlap_device writes, for query triangle i,
 *   n_overlap[i]    the full number of overlapping triangles                                       (may be NULL when max_k > 0)
 *   tri_id row i    the min(max_k, n_overlap[i]) LOWEST indices of them in ascending order, then -1
 * -- exactly the list of ezrt_query_box_overlap_device: a row of K entries is a prefix of every longer one, the answer does not
 * depend on the tree, and it survives a retree or a refit of unchanged geometry.  max_k is in 0 .. EZRT_TRI_OVERLAP_MAX; with
 * max_k == 0 tri_id is ignored and n_overlap is required: a count-only call.  A query triangle that is a triangle of the scene
 * overlaps itself and every triangle that shares a vertex with it; a self-intersection check is ezrt_self_overlap.h, whose rule
 * leaves out what two triangles share by value and nothing else.
 *
 * ezrt_tri_overlap_at_device writes overlaps[i] = overlaps(query triangle i, triangle tri_id[i]) as 0 / 1; an id outside the scene
 * writes 0.  It narrows candidates the caller already holds -- rows of ezrt_query_box_overlap_device, or rows of this query after
 * the query mesh has moved -- and it is the direct probe of the per-pair function.
 *
 * How it is computed.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1; decided per call, a refit can change it) one
 * query triangle per lane walks the 4-wide records depth-first and descends a slot when slot.lo[c] <= q.hi[c] && slot.hi[c] >=
 * q.lo[c] on all three axes -- comparisons only, see T1.  Triangles below no leaf are swept after the walk.  Otherwise (malformed or
 * tiny scenes) the same per-pair function sweeps all n_tri triangles.  The list is kept sorted in the query's own output row.
 *
 * Memory, streams, ordering and errors are those of ezrt_box_overlap.h (which takes them from ezrt_closest_point.h): every pointer is
 * device memory of the scene's device, large enough for its n (or n x 9, n x max_k) elements (anything else is rejected before any
 * launch, never dereferenced); work is enqueued on `stream` and the call returns without synchronising; no scratch set is used; the
 * calls may run beside ezrt_render_device and the other queries on other streams and leave ezrt_counters and ezrt_last_render_ms
 * alone; a later refit (ezrt_refit.h) waits for them, and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene or tris9; max_k outside 0 .. EZRT_TRI_OVERLAP_MAX;
 * max_k > 0 with NULL tri_id; max_k == 0 with NULL n_overlap; NULL tri_id or overlaps (ezrt_tri_overlap_at_device); n < 0; a pointer
 * that is not device memory of the scene's device.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_TRI_OVERLAP_H
#define EZRT_TRI_OVERLAP_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_TRI_OVERLAP_MAX 64

int ezrt_query_tri_overlap_device(EzrtScene* s, const float* tris9 /* n x 9 */, int n, int max_k,
                                  int32_t* tri_id /* n x max_k, or NULL when max_k == 0 */, int32_t* n_overlap /* n, or NULL */, void* stream);
int ezrt_tri_overlap_at_device(EzrtScene* s, const float* tris9 /* n x 9 */, const int32_t* tri_id /* n */, int n,
                               uint8_t* overlaps /* n */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
