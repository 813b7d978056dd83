/* ezrt_self_overlap.h -- stream-ordered self-overlap queries on device memory (libezrt_hip.so only).
 *
 * Where does the mesh cross itself: for a triangle of the scene, the OTHER triangles of the scene that meet it anywhere except in
 * what the two share by value.  ezrt_tri_overlap.h cannot answer this: there touching counts, so a triangle overlaps its whole
 * vertex umbrella, and dropping the neighbours by their ids is wrong -- two triangles that share a vertex can pierce each other, two
 * that share an edge can fold onto each other, and those are the defects a deformation driven through ezrt_refit.h produces first.
 * The scene is a triangle soup: "shared" can only mean shared by VALUE, and the rule below is defined on the triangle array alone.
 * It is what a caller checks between two refits before asking ezrt_inside.h, whose answers assume a mesh that does not cross itself.
 *
 * THE DEFINITION.  No contraction anywhere (-ffp-contract=off, as everywhere in the library); one rounding per written operation.
 * less, ==, the sorted vertices, d, d3, the normal N, LIVE, p(x, D), the edges E0 E1 E2 of a sorted triangle, T1, T2, the order
 * (A, B) of two triangles and overlaps are those of ezrt_tri_overlap.h.  Arithmetic is fp64 on the fp32 values converted exactly,
 * and the vertices of both triangles are sorted by value before any of it.
 *
 * Take triangles I and J of the scene with I != J as ids.  Both must be live; a triangle that is not live crosses nothing.  With
 * (i0 i1 i2) and (j0 j1 j2) their sorted vertices, s is the number of vertices of I that are == on all three coordinates to a
 * vertex of J.  A live triangle has three distinct vertices, so the shared vertices pair off and s is 0 .. 3; -0 == +0.
 *
 *   s = 0   crosses(I, J) = overlaps(I, J) of ezrt_tri_overlap.h: T1 and T2, to the bit.
 *   s = 3   (the same three values: a duplicated face)  crosses(I, J) = true.
 *   s = 1   the shared vertex is v; the other two vertices of I, in the order of their values, are (a, b), those of J are (c, d):
 *             crosses(I, J) = seg_meets(a, b; J) || seg_meets(c, d; I)
 *   s = 2   the shared vertices, in the order of their values, are (u, v).  The two triangles are put in the order (A, B) of T2,
 *           and with a the vertex of A and b the vertex of B that are not shared (u and v are read from A):
 *             e = d3(v, u),  Da = d3(a, u),  Db = d3(b, u)
 *             X_a = e x Da,  X_b = e x Db            (e[1]*D[2] - e[2]*D[1],  e[2]*D[0] - e[0]*D[2],  e[0]*D[1] - e[1]*D[0])
 *             coplanar  = p(X_a, Db) == 0
 *             same_side = for some component c:  (X_a[c] > 0 && X_b[c] > 0) || (X_a[c] < 0 && X_b[c] < 0)
 *             crosses(I, J) = coplanar && same_side
 *
 * seg_meets(a, b; T) is the separating-axis test of the closed segment a b, (a, b) in the order of their values, against the closed
 * live triangle T with sorted vertices t0 t1 t2 and edges f_0 = d3(t1, t0), f_1 = d3(t2, t1), f_2 = d3(t2, t0).  With g_0 = d3(b, a)
 * the segment's direction, every point is taken relative to t0,
 *   D1 = d3(t1, t0),  D2 = d3(t2, t0),  D3 = d3(a, t0),  D4 = d3(b, t0)
 * and a direction x SEPARATES when
 *   max(0, p(x,D1), p(x,D2)) < min(p(x,D3), p(x,D4))  ||  max(p(x,D3), p(x,D4)) < min(0, p(x,D1), p(x,D2))
 * The 16 directions, ALL of them always part of the rule:
 *   N_T                                          the normal of T                                                        (1)
 *   g_0 x f_j, j = 0, 1, 2                       the cross product as written above                                       (3)
 *   g x axis_j, g = g_0 f_0 f_1 f_2, j = 0, 1, 2:   x[(j+1)%3] = -g[(j+2)%3],  x[(j+2)%3] = g[(j+1)%3],  x[j] = 0                (12)
 *   seg_meets(a, b; T) = none of the 16 directions separates
 *
 * What the rule guarantees.
 * - It answers "do I and J share a point outside the convex hull of the vertices they share": outside nothing (s = 0: any common
 *   point), outside the point v (s = 1), outside the segment u v (s = 2); for s = 3 the hull is the triangle itself and the answer
 *   is true by definition -- a duplicated face is a defect.  A manifold mesh, a mesh with T-free non-manifold edges or vertex
 *   contacts, every mesh whose triangles meet only in whole shared vertices and edges, crosses itself nowhere.
 * - s = 1 is complete.  Let p != v be a common point.  The segment v p lies in both triangles (both are convex and hold v and p).
 *   Extend it beyond p until it first leaves one of them, say I: it leaves I through I's edge opposite v, the segment a b, at a point
 *   that still lies in J -- so a b meets J.  Conversely a b does not hold v (I is live), so a point of a b in J is a common point
 *   other than v.  Every direction of seg_meets is sound (projections of sets that meet have a common point), and the 16 are
 *   complete for a proper segment against a proper triangle: segment not parallel to the plane of T -- the difference body T - S
 *   is a prism whose faces have the normals N_T (the two caps) and g_0 x f_j (the three sides); parallel to the plane but off it
 *   -- N_T separates; in the plane -- the difference body is a polygon whose sides are parallel to g_0 or to an f_j, and g x axis_j
 *   acts as the in-plane normal of such a side for an axis j with N_T[j] != 0, the argument of ezrt_tri_overlap.h.  a != b, since
 *   I is live.
 * - s = 2 is complete.  Both triangles hold the line u v.  If their planes differ they meet in that line only, and on it each holds
 *   exactly the segment u v: nothing outside the hull.  If they are one plane, the two triangles lie on the two sides of the line
 *   u v or on one; on two sides they meet in the segment only; on one side both hold a neighbourhood, in their half-plane, of the
 *   segment's interior points.  X_a and X_b are normals of the two planes: Db lies in A's plane exactly when p(X_a, Db) == 0, and
 *   then X_a and X_b are parallel and neither is zero (both triangles are live), so they point the same way exactly when some
 *   component has one strict sign in both.  No product of the two is formed.
 * - It is symmetric to a bit: crosses(I, J) == crosses(J, I).  s does not depend on the roles; T2 is computed on (A, B); for s = 1
 *   the two seg_meets are evaluated whichever triangle is called I, and || commutes; for s = 2 the roles are given by (A, B) -- beyond
 *   the exact range p(X_a, Db) and p(X_b, Da) need not agree, so one of them is THE rule.  A pair therefore appears in both
 *   triangles' rows.
 * - It is independent of the tree, of the order of the triangles (ids only name the rows), and of the vertex order and winding of
 *   every triangle: all vertices are sorted by value before any arithmetic.
 * - Exactness.  Every expression has degree at most 3 in the coordinates (a cross product, degree 2, times a difference).  By the
 *   bit count of ezrt_tri_overlap.h the rule is exact on a grid of up to 2^15 steps -- there it is THE exact answer to the question
 *   above -- and beyond that every product and sum is rounded once: still pinned operation by operation, but pairs within about
 *   2^-50 of their extent of touching, or of being coplanar, may be given either answer.
 * - T1 holds for s >= 1 without being asked: the shared value lies in both bounding boxes.  T1 is part of s = 0.  So for EVERY case a
 *   crossing triangle's bounding box passes the fp32 comparisons against the bounding box of triangle I, and so does every box
 *   that holds it: the walk of ezrt_tri_overlap.h gates every case, unchanged.
 * - From finite fp32 inputs no fp64 operation here overflows, underflows to a wrong zero or yields a NaN: the expressions have the
 *   shapes of ezrt_tri_overlap.h's (differences below 2^129, cross products below 2^259, projections below 2^390; a product of up
 *   to three non-zero factors is at least 2^-447), and its bound argument applies as it stands.
 *
 * ezrt_query_self_overlap_device writes, for query i -- triangle ids[i] of the scene, or triangle i when ids is NULL (then n <= the
 * scene's number of triangles) --
 *   n_overlap[i]    the full number of triangles k != ids[i] with crosses(ids[i], k)                  (may be NULL when max_k > 0)
 *   tri_id row i    the min(max_k, n_overlap[i]) LOWEST indices of them in ascending order, then -1
 * -- the list of ezrt_query_tri_overlap_device: a row of K entries is a prefix of every longer one, nothing depends on the tree, and
 * the answer survives a retree or a refit of unchanged geometry.  max_k is in 0 .. EZRT_SELF_OVERLAP_MAX; with max_k == 0 tri_id is
 * ignored and n_overlap is required: a count-only call.  An id outside 0 .. n_tri - 1 is a dead query: an empty row and a count of
 * 0, as for a triangle that is not live.  ids may repeat.
 *
 * ezrt_self_overlap_at_device writes crosses[i] = crosses(tri_a[i], tri_b[i]) as 0 / 1; an id outside the scene, equal ids and a
 * triangle that is not live write 0.  It narrows pairs the caller already holds -- rows of this query after a refit -- and is the
 * direct probe of the per-pair function.
 *
 * How it is computed.  As ezrt_tri_overlap.h: where the scene prunes, one query per lane walks the 4-wide records depth-first with the
 * bounding box of its own triangle as the gate; otherwise the per-pair function sweeps all triangles.  The list is kept sorted in
 * the query's own output row.
 *
 * Memory, streams, ordering and errors are those of ezrt_tri_overlap.h: every pointer is device memory of the scene's device, large
 * enough for its n (or n x max_k) elements (anything else is rejected before any launch, never dereferenced); work is enqueued on
 * `stream` and the call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the
 * other queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for
 * them, and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene; n < 0; NULL ids with n above the scene's number of
 * triangles; max_k outside 0 .. EZRT_SELF_OVERLAP_MAX; max_k > 0 with NULL tri_id; max_k == 0 with NULL n_overlap; NULL tri_a, tri_b
 * or crosses (ezrt_self_overlap_at_device); a pointer that is not device memory of the scene's device.  n == 0 returns 0 and
 * launches nothing. */
#ifndef EZRT_SELF_OVERLAP_H
#define EZRT_SELF_OVERLAP_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_SELF_OVERLAP_MAX 64

int ezrt_query_self_overlap_device(EzrtScene* s, const int32_t* ids /* n, or NULL: query i is triangle i, n <= n_tri */, int n, int max_k,
                                   int32_t* tri_id /* n x max_k, or NULL when max_k == 0 */, int32_t* n_overlap /* n, or NULL */, void* stream);
int ezrt_self_overlap_at_device(EzrtScene* s, const int32_t* tri_a /* n */, const int32_t* tri_b /* n */, int n, uint8_t* crosses /* n */,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif
