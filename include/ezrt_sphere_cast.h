/* ezrt_sphere_cast.h -- stream-ordered sphere-cast queries on device memory (libezrt_hip.so only).
 *
 * How far can a sphere of radius r move along a ray before it touches the mesh: the query a character controller, a tool path, a
 * robot link or a camera boom asks.  A ray (ezrt_query.h) has no thickness -- it slips through a gap the body does not fit through
 * and passes an edge the body would clip --, and sampling ezrt_closest_point.h along the path is neither exact nor cheap.
 *
 *   rays6      n x 6 floats: origin o and direction d of every query; d NEED NOT HAVE UNIT LENGTH
 *   radius     n floats: r, in world units
 *   t_max      n floats, or NULL (= +inf for every query): only contacts at t <= t_max are candidates
 * t IS IN UNITS OF d: the centre of the sphere at time t is o + d*t.
 *
 * THE DEFINITION.  All arithmetic is fp32 (IEEE binary32, round to nearest even), one rounding per written operation, no contraction
 * (-ffp-contract=off, as everywhere in the library), with ezrt_closest_point.h's conventions: + - * componentwise on vectors,
 * dot(u, w) = u.x*w.x + u.y*w.y + u.z*w.z evaluated left to right, cross(u, w) = (u.y*w.z - u.z*w.y, u.z*w.x - u.x*w.z,
 * u.x*w.y - u.y*w.x), IEEE division and square root, min(x, y) = (y < x) ? y : x and max(x, y) = (x < y) ? y : x (ez_min, ez_max).
 * Negating a value is exact.  This rule is the library's own: the reference has no such query.
 *
 * 1. Liveness.  A query is LIVE when o, d and r are finite, r >= 0, dd = dot(d, d) is finite and > 0, and for every axis with
 *    d != 0 the reciprocal inv = 1/d is finite.  A query that is not live misses.  A t_max that is not >= 0 (negative, NaN) gives
 *    no candidates in step 3 (step 2 does not look at t_max).  A scene triangle (a, b, c) -- the scene's p1 p2 p3 of triangle k, IN
 *    THE ORDER GIVEN -- is LIVE when its nine coordinates are finite.  A degenerate triangle is met as the segment or point it is:
 *    its face sub-candidate is never valid (below), its edges and vertices are.
 *
 * 2. Touching at the start.  If ezrt_closest_point.h's rule for the point o with d_max = r (B = r*r; unchanged: the candidates have
 *    a finite dist2 <= B, the smallest dist2 wins, then the lowest index) finds a triangle, the answer is that triangle, t = 0,
 *    point = its nearest point q and touching = 1.  So where touching is set, (tri_id, point) are those of
 *    ezrt_query_closest_point_device(o, d_max = r) on the bits.
 *
 * 3. Otherwise the swept rule, per pair (query, live triangle).  rr = r*r.
 *    Gate.  lo = min(min(a, b), c), hi = max(max(a, b), c) per axis: the triangle's own bounding box.  slab(lo, hi):
 *        tnear = 0; tfar = +inf
 *        per axis x, y, z:   L = lo - r;  H = hi + r
 *          d == 0 (or -0):   the gate fails if o < L or o > H; the axis bounds nothing
 *          else:             x = (L - o)*inv;  y = (H - o)*inv;   near, far = (d < 0) ? (y, x) : (x, y)
 *                            tnear = max(tnear, near);  tfar = min(tfar, far)
 *        the gate passes if no flat axis failed and tnear <= tfar
 *    A pair whose gate fails is no candidate.  In exact arithmetic the gate rejects no pair that touches; like H1 and T1 of the
 *    overlap headers it is part of the rule.
 *    Seven sub-candidates, in this order; each yields a time tt and a contact point x, or is not valid.
 *      root(B, C, disc): the first time A*t*t + 2*B*t + C reaches 0 for a centre outside (C > 0) that approaches (B < 0), in the
 *      form without cancellation; 0 where the feature already holds the centre at t = 0.  disc is B*B - A*C in Lagrange's form,
 *      A*rr - |m x d|^2: written so, a thin sphere far from the feature does not hit it by rounding.
 *        C <= 0                      -> 0
 *        B < 0 and disc >= 0         -> C / (sqrt(disc) - B)
 *        otherwise                   -> not valid
 *      box(x, P, Q): x clamped per axis into [min(P, Q), max(P, Q)]: x < lo ? lo : (x > hi ? hi : x).
 *      0  the face.   ab = b - a; ac = c - a; m = o - a; n0 = cross(ab, ac); h0 = dot(n0, m)
 *                     h0 < 0:  n = -n0, h = -h0   else  n = n0, h = h0               (the normal on o's side)
 *                     nd = dot(n, d);  valid only if nd < 0                             (the centre approaches the plane)
 *                     len = sqrt(dot(n, n));  g = h - r*len;  tt = g <= 0 ? 0 : g / (-nd)
 *                     x' = (o + d*tt) - n*(r/len)                                       (the foot)
 *                     e0 = dot(cross(ab, x' - a), n0);  e1 = dot(cross(c - b, x' - b), n0);  e2 = dot(cross(a - c, x' - c), n0)
 *                     valid if e0 >= 0 and e1 >= 0 and e2 >= 0;   x = x' clamped into [lo, hi]
 *                     (a degenerate triangle has n0 = 0 up to rounding: nd = 0, or len = 0 and a NaN foot -- not valid)
 *      1 2 3  the edges (u, v) = (a, b), (b, c), (c, a): the infinite cylinder of radius r about the edge, in the plane across it.
 *                     e = v - u; m = o - u; ee = dot(e, e);  sd = dot(e, d)/ee;  sm = dot(e, m)/ee
 *                     dp = d - e*sd;  mp = m - e*sm                                     (d and m without their parts along e)
 *                     k = cross(mp, dp);  tt = root(dot(mp, dp), dot(mp, mp) - rr, dot(dp, dp)*rr - dot(k, k))
 *                     s = sm + sd*tt;  valid if 0 <= s <= 1;   x = box(u + e*s, u, v)
 *      4 5 6  the vertices p = a, b, c: the sphere of radius r about the vertex.
 *                     m = o - p;  k = cross(m, d);  tt = root(dot(m, d), dot(m, m) - rr, dd*rr - dot(k, k));  x = p
 *    A sub-candidate whose tt is not finite (NaN: a 0/0 of an edge of length 0, an overflow) is skipped.  The smallest tt wins, the
 *    FIRST in the order above on equality, and supplies x.  The pair's t = max(that tt, tnear); if no sub-candidate is valid or t is
 *    not finite the pair is no candidate.  In exact arithmetic the clamp to tnear changes nothing -- the sphere cannot touch the
 *    triangle before its centre enters the inflated box -- and it is what lets the traversal prune with no slack (below).  The rule
 *    "C <= 0 yields 0" matters for a sphere that step 2 finds an ulp clear of the surface and that moves inward: its root would be
 *    negative or cancel, and it must not tunnel.
 *    The answer: the candidates are the pairs with t <= t_max.  The smallest t wins, then the lowest triangle index k.
 *    touching = 0.  THE ANSWER NEVER DEPENDS ON THE TREE: triangles below no leaf take part as in every point query.
 *
 * What is NOT promised: invariance under reordering a triangle's vertices (the order decides which of two equal tt supplies the point,
 * and rounding differs), or agreement to the last bit with marching the closest-point query along the ray.
 * tests/test_sphere_cast_expected.py measures the residual |dist(o + d*t, triangle) - r| of the answers against float64.
 *
 * Outputs per query:
 *   tri_id     the winning triangle, -1 for a miss
 *   t          the time of first contact, 0 where touching; +inf for a miss                            (may be NULL)
 *   point      the contact point on the triangle; zeros for a miss                                     (may be NULL)
 *              (the contact normal is (o + d*t - point) / r)
 *   touching   uint8: 1 when the sphere touches the mesh at t = 0 by step 2, else 0; 0 for a miss      (may be NULL)
 * A miss is the point queries' (-1, +inf, zeros, 0), not the ray queries' 114514.
 *
 * ezrt_sphere_cast_at_device evaluates the pair rule for (query i, triangle tri_id[i]) the caller holds -- the winners of an earlier
 * call after the body has moved, rows of ezrt_query_nearest_device -- and writes t, point and touching as above (no t_max): touching
 * where closest_point_triangle's dist2 of (o, triangle) is finite and <= r*r (then t = 0 and point = its q), otherwise the swept pair
 * of step 3.  An id outside the scene, a query or triangle that is not live or a pair that is no candidate writes the miss values
 * (+inf, zeros, 0).  At least one output is required.
 *
 * How it is computed.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1; decided per call, a refit can change it) one
 * query per lane walks the 4-wide records twice: first ezrt_closest_point.h's search with B = r*r, and, if that finds nothing,
 * best-first in t.  The lower bound of a node box [lo, hi] is tnear of slab(lo, hi) above, +inf where that gate fails; a subtree is
 * skipped only when its bound > the best t so far (t_max until a candidate is found) and descended on equality; an entry popped from
 * the stack is checked again.  WHY NO MARGIN IS NEEDED: for a box [L, H] that holds [l, h], every step of near and far is monotone
 * under rounding -- subtracting or adding r, subtracting o, multiplying by inv (a constant of fixed sign; the two are swapped where
 * it is negative), max and min, and the flat-axis comparisons.  So tnear(outer) <= tnear(inner) and tfar(outer) >= tfar(inner) on
 * the bits, and an outer box passes whenever an inner one does.  o, r and inv are finite and inv != 0, so 0 * inf cannot arise; a
 * difference that overflows is an infinity of the right sign and stays ordered; inf - inf cannot arise from a finite o; a NaN bound
 * of a node box constrains nothing.  With the clamp, tnear(any box above T) <= tnear(T) <= t(pair): a skipped subtree holds neither
 * a winner nor a tie.  The same slab test of the triangle's own box gates the pair before its seven sub-candidates.  Triangles
 * below no leaf are swept after each walk.  Otherwise (malformed or tiny scenes) the same functions sweep all n_tri triangles without
 * a tree.  Both give the answer defined above, bit for bit.
 *
 * Memory, streams, ordering and errors are those of ezrt_tri_distance.h: every pointer is device memory of the scene's device, large
 * enough for its n (or n x 3, n x 6) elements (anything else is rejected before any launch, never dereferenced); work is enqueued on
 * `stream` and the call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the
 * other queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them,
 * and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, rays6, radius or tri_id; n < 0; no output at all
 * (ezrt_sphere_cast_at_device); a pointer that is not device memory of the scene's device.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_SPHERE_CAST_H
#define EZRT_SPHERE_CAST_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_sphere_cast_device(EzrtScene* s, const float* rays6 /* n x 6 */, const float* radius /* n */, const float* t_max /* n or NULL */,
                                  int n, int32_t* tri_id /* n */, float* t /* n or NULL */, float* point /* n x 3 or NULL */,
                                  uint8_t* touching /* n or NULL */, void* stream);
int ezrt_sphere_cast_at_device(EzrtScene* s, const float* rays6 /* n x 6 */, const float* radius /* n */, const int32_t* tri_id /* n */, int n,
                               float* t /* n or NULL */, float* point /* n x 3 or NULL */, uint8_t* touching /* n or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
