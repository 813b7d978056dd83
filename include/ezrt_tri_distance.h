/* ezrt_tri_distance.h -- stream-ordered triangle-distance queries on device memory (libezrt_hip.so only).
 *
 * How far is this triangle from the mesh, and where do the two come closest: the proximity counterpart of ezrt_tri_overlap.h, as
 * ezrt_closest_point.h is that of ezrt_inside.h.  A caller who holds a second mesh -- a tool moving against a part -- learns from
 * the overlap query that the tool cuts the part only after it has cut; this query says how close the tool is to touching, and
 * whether anything lies within a clearance of it.  Closest-point calls on the tool's vertices do not answer that: they miss an edge
 * that passes an edge, and a vertex of the part that lies near the interior of a face of the tool.
 *
 *   tris9      n x 9 floats: p1 p2 p3 of every query triangle
 *   d_max      n floats, or NULL (= +inf for every triangle): only triangles within this distance are candidates
 *
 * THE DEFINITION.  All arithmetic is fp32 (IEEE binary32, round to nearest even), one rounding per written operation, no contraction
 * (-ffp-contract=off, as everywhere in the library), with ezrt_closest_point.h's conventions: + - * componentwise on vectors,
 * dot(u, w) = u.x*w.x + u.y*w.y + u.z*w.z evaluated left to right, IEEE divisions, min(x, y) = (y < x) ? y : x and
 * max(x, y) = (x < y) ? y : x (ez_min, ez_max).  clamp01(v) = min(max(v, 0), 1) with these two: a NaN stays a NaN.  The only fp64
 * arithmetic is that of the two rules taken from ezrt_tri_overlap.h as they stand: LIVE and overlaps.
 *
 * Liveness.  The query triangle Q = (p1, p2, p3) and the scene triangle S = (a, b, c) (the scene's p1 p2 p3 of triangle k) are LIVE by
 * the rule of ezrt_tri_overlap.h: nine finite coordinates and a normal N != (0, 0, 0) of the sorted vertices -- a non-finite number
 * and collinear or repeated vertices make a triangle not live.  A query triangle that is not live misses; a scene triangle that is
 * not live is never a candidate.
 *
 * Sub-candidates.  The distance of the pair (Q, S) is taken over 15 sub-candidates in this order; each yields a point x on Q, a point y
 * on S and d2 = dot(e, e), e = x - y.  BOTH TRIANGLES' VERTICES ARE TAKEN IN THE ORDER GIVEN (not in the sorted order of the live rule).
 *    0 ..  2   vertex p1, p2, p3 of Q against S: closest_point_triangle of ezrt_closest_point.h as it stands, with p the vertex and
 *              (a, b, c) = S.  x = the vertex, y = its q (already clamped to S's bounding box), d2 = its dist2.
 *    3 ..  5   vertex a, b, c of S against Q: the same function with the roles swapped, p the vertex and (a, b, c) = (p1, p2, p3).
 *              y = the vertex, x = its q (clamped to Q's bounding box), d2 = its dist2 (dot(y - x, y - x): the same bits as dot(x - y, x - y)).
 *    6 .. 14   edge i of Q against edge j of S, i outer: 6 + 3 i + j.  The edges of Q are (p1, p2), (p2, p3), (p3, p1), those of S
 *              (a, b), (b, c), (c, a).  The closest points of two closed segments [P1, Q1] (of Q) and [P2, Q2] (of S):
 *                d1 = Q1-P1; d2 = Q2-P2; r = P1-P2
 *                a = dot(d1,d1); e = dot(d2,d2); f = dot(d2,r); c = dot(d1,r); b = dot(d1,d2)
 *                den = a*e - b*b
 *                s = den > 0 ? clamp01((b*f - c*e)/den) : 0
 *                t = (b*s + f)/e
 *                if t < 0:       t = 0; s = clamp01(-c/a)
 *                else if t > 1:  t = 1; s = clamp01((b - c)/a)
 *                x' = P1 + d1*s;  lo = min(P1, Q1); hi = max(P1, Q1);  x = x' < lo ? lo : (x' > hi ? hi : x')     per axis
 *                y' = P2 + d2*t;  lo = min(P2, Q2); hi = max(P2, Q2);  y = y' < lo ? lo : (y' > hi ? hi : y')     per axis
 *                e = x - y;  d2 = dot(e, e)
 *              (a NaN x' or y' stays NaN; parallel segments have den <= 0 up to rounding and start from s = 0.)
 * The clamps change nothing in exact arithmetic -- a point of a segment lies in the segment's bounding box, which lies in its
 * triangle's -- and are what lets the traversal prune without any slack (below).
 *
 * Pair result.  A sub-candidate whose d2 is not finite (NaN, +inf: an overflow, a 0/0 of an edge whose squared length underflows) is
 * skipped.  dist2 of the pair is the smallest finite d2; the FIRST sub-candidate in the order above wins on equality and supplies the
 * pair's (x, y).  If no d2 is finite the pair is no candidate.
 *
 * Crossing.  If overlaps(Q, S) of ezrt_tri_overlap.h holds (unchanged: T1 and the 29 directions), the pair's dist2 is 0 and its
 * `crosses` is 1.  (x, y) stay those of the 15-way minimum: THEY ARE THE NEAREST FEATURES OF THE TWO TRIANGLES, NOT A COMMON POINT.
 * The step is required: an edge that pierces the interior of a face has positive vertex-face and edge-edge distances.  A pair that
 * touches in a vertex or along an edge already has a sub-candidate with d2 = 0 on exact inputs; its `crosses` is 1 all the same,
 * because the overlap rule counts touching.
 *
 * The answer for Q, with B = d_max*d_max (fp32; +inf when d_max is NULL; a d_max that is not >= 0 -- NaN, negative -- gives no
 * candidates): the candidates are the pairs with a dist2 (finite by construction) <= B.  The smallest dist2 wins.  Among equal dist2
 * a pair that crosses comes before a pair that does not, and then the smallest scene index k wins.  The first of the two matters at
 * dist2 = 0 alone -- all the triangles that Q crosses have 0, and so has a triangle that is apart from Q by less than fp32 resolves,
 * whose nearest sub-candidate rounds to 0 (a vertex of Q computed as the midpoint of an edge of S lies next to that edge, not on it)
 * -- and it is what makes `crosses` the answer of ezrt_tri_overlap.h for the whole scene: crosses is 1 EXACTLY when Q overlaps some
 * triangle of the scene by that header's rule, and tri_id is then the lowest index among them, the first entry of that query's row.
 * THE ANSWER NEVER DEPENDS ON THE TREE.
 *
 * What is NOT promised.  The rule is not symmetric in the two roles (Q against a scene that holds S may differ in the last bits from
 * S against a scene that holds Q: the sub-candidates come in another order and the segment formula treats its two segments
 * differently), and it is not invariant under reordering the vertices of Q or of S (the order decides which of two equal d2 supplies
 * the points, and rounding differs between the orders).  `crosses`, liveness and a dist of 0 by crossing are invariant: they are the
 * overlap rule's.
 *
 * Outputs per query triangle:
 *   tri_id        the winning scene triangle, -1 for a miss
 *   dist          sqrtf(dist2) of the winner, +inf for a miss                                         (may be NULL)
 *   point_query   x of the winner, on the query triangle; zeros for a miss                            (may be NULL)
 *   point_scene   y of the winner, on the scene triangle; zeros for a miss                            (may be NULL)
 *   crosses       uint8: 1 when the winner crosses or touches Q, else 0; 0 for a miss                 (may be NULL)
 *
 * ezrt_tri_distance_at_device evaluates the pair rule for (query triangle i, triangle tri_id[i]) the caller holds -- the winners of
 * an earlier call after the query mesh has moved a little, rows of ezrt_query_tri_overlap_device or ezrt_query_nearest_device -- and
 * writes dist, point_query, point_scene and crosses as above (no d_max).  An id outside the scene, a triangle that is not live on
 * either side or a pair without a finite sub-candidate writes the miss values (+inf, zeros, zeros, 0).  At least one output is required.
 *
 * How it is computed.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1; decided per call, a refit can change it) one
 * query triangle per lane walks the 4-wide records best-first, as ezrt_closest_point.h's points do, with the lower bound of a box
 * [lo, hi] taken against Q's fp32 bounding box [qlo, qhi]:
 *   g = max(lo - qhi, 0, qlo - hi) per axis;  lb = dot(g, g)
 * A subtree is skipped only when lb > the best dist2 so far (or lb is not finite) and descended on equality; an entry popped from the
 * stack is checked again.  WHY NO MARGIN IS NEEDED: every x is a vertex of Q or is clamped into the bounding box of Q or of an edge
 * of Q, so qlo <= x <= qhi per axis; every y is a vertex of S or is clamped into the bounding box of S or of an edge of S, which
 * lies in every box above S.  Per axis either g = 0 <= |e|, or g = fl(lo - qhi) with y >= lo > qhi >= x: y - x >= lo - qhi in the
 * reals, rounding is monotone and |fl(x - y)| = fl(y - x), so |e| >= g (the same on the other side).  fl(x*x) is monotone in |x| and
 * fl(fl(X + Y) + Z) in each of X, Y, Z >= 0, so lb <= d2 ON THE BITS for every sub-candidate with a finite d2, overflow of lb
 * included, hence lb <= the pair's dist2; a pair that crosses passes T1, so the boxes overlap on every axis and lb = 0 = dist2.  The
 * same lb of S's own bounding box gates the pair before its 15 sub-candidates and the fp64 overlap rule: a triangle with lb > best
 * can neither win nor tie.  Triangles below no leaf are swept after the walk.  Otherwise (malformed or tiny scenes) the same pair
 * function sweeps all n_tri triangles without a tree.  Both give the answer defined above, bit for bit.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its n (or n x 3, n x 9) elements (anything else is rejected before any launch, never dereferenced); work is enqueued on
 * `stream` and the call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the
 * other queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them,
 * and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, tris9 or tri_id; n < 0; no output at all
 * (ezrt_tri_distance_at_device); a pointer that is not device memory of the scene's device.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_TRI_DISTANCE_H
#define EZRT_TRI_DISTANCE_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_tri_distance_device(EzrtScene* s, const float* tris9 /* n x 9 */, const float* d_max /* n or NULL */, int n,
                                   int32_t* tri_id /* n */, float* dist /* n or NULL */, float* point_query /* n x 3 or NULL */,
                                   float* point_scene /* n x 3 or NULL */, uint8_t* crosses /* n or NULL */, void* stream);
int ezrt_tri_distance_at_device(EzrtScene* s, const float* tris9 /* n x 9 */, const int32_t* tri_id /* n */, int n,
                                float* dist /* n or NULL */, float* point_query /* n x 3 or NULL */, float* point_scene /* n x 3 or NULL */,
                                uint8_t* crosses /* n or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
