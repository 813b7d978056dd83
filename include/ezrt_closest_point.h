/* ezrt_closest_point.h -- stream-ordered closest-point queries on device memory (libezrt_hip.so only).
 *
 * Which point of the mesh is nearest to a given point, and how far away is it: the question behind distance fields, collision and
 * clearance checks, snapping a point to a surface, point-cloud-to-mesh error and proximity-based ambient occlusion.  Every other
 * query of the library asks about a ray; this one cannot be emulated with them.
 *
 *   points3    n x 3 floats: the query points
 *   d_max      n floats, or NULL (= +inf for every point): only triangles within this distance are candidates
 *
 * THE DEFINITION.  All arithmetic is fp32 (IEEE binary32, round to nearest even), one rounding per written operation, no contraction
 * (-ffp-contract=off, as everywhere in the library).  On vectors, + - * are componentwise and dot(u, w) = u.x*w.x + u.y*w.y + u.z*w.z,
 * evaluated left to right.  Divisions are IEEE divisions.  min(x, y) = (y < x) ? y : x and max(x, y) = (x < y) ? y : x (ez_min,
 * ez_max of ezrt_detmath.h: fminf / fmaxf with the sign of a zero result and the NaN case pinned).
 *
 * For a query point p and triangle k with vertices a, b, c (the scene's p1, p2, p3 of triangle k), the closest point q_k is the
 * region form of the point-triangle projection, evaluated in this order; the first case that applies wins:
 *
 *   ab = b-a; ac = c-a; ap = p-a; d1 = dot(ab,ap); d2 = dot(ac,ap)
 *     d1 <= 0 && d2 <= 0                       -> (v,w) = (0,0)
 *   bp = p-b; d3 = dot(ab,bp); d4 = dot(ac,bp)
 *     d3 >= 0 && d4 <= d3                      -> (v,w) = (1,0)
 *   vc = d1*d4 - d3*d2
 *     vc <= 0 && d1 >= 0 && d3 <= 0            -> (v,w) = (d1/(d1-d3), 0)
 *   cp = p-c; d5 = dot(ab,cp); d6 = dot(ac,cp)
 *     d6 >= 0 && d5 <= d6                      -> (v,w) = (0,1)
 *   vb = d5*d2 - d1*d6
 *     vb <= 0 && d2 >= 0 && d6 <= 0            -> (v,w) = (0, d2/(d2-d6))
 *   va = d3*d6 - d5*d4
 *     va <= 0 && d4-d3 >= 0 && d5-d6 >= 0      -> w = (d4-d3)/((d4-d3)+(d5-d6)); (v,w) = (1-w, w)
 *     otherwise                                -> s = va+vb+vc; (v,w) = (vb/s, vc/s)
 *   q' = (a + ab*v) + ac*w
 *   lo = min(min(a,b),c); hi = max(max(a,b),c)                    per axis
 *   q  = q' < lo ? lo : (q' > hi ? hi : q')                       per axis (a NaN q' stays NaN)
 *   e  = p - q;  dist2_k = dot(e,e)
 *
 * The clamp changes nothing in exact arithmetic -- a point of a triangle lies in the triangle's bounding box -- and is what lets the
 * traversal prune without any slack (below).
 *
 * The answer for p, with B = d_max*d_max (fp32; +inf when d_max is NULL):
 *   the candidates are the triangles k in [0, n_tri) whose dist2_k is finite and <= B; a d_max that is not >= 0 (NaN, negative)
 *   gives no candidates; a non-finite dist2_k is never a candidate (a NaN vertex, a degenerate triangle that reaches 0/0, an
 *   overflow, a non-finite p).  The winner is the candidate with the smallest dist2_k; among equal dist2_k the smallest k wins -- k
 *   is the index in the array given to ezrt_scene_create, the id space of every other query.  THE ANSWER NEVER DEPENDS ON THE TREE.
 *
 * Outputs per point:
 *   tri_id   the winner, -1 for a miss
 *   point    q of the winner, zeros for a miss                                              (may be NULL)
 *   dist     sqrtf(dist2) of the winner, +inf for a miss (NOT EZ_INF: that is hitTriangle's ray-parameter convention, and
 *            distances here are not bounded by it)                                           (may be NULL)
 *   bary     (v, w) of the winner, zeros for a miss; normals or attributes interpolate with (1-v-w, v, w) over (p1, p2, p3)
 *                                                                                            (may be NULL)
 *
 * How it is computed.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1: the boxes are nested and every leaf box holds
 * its triangles; decided per call, a refit can change it) one point per lane walks the 4-wide records best-first: children ordered
 * by their box distance lb = dot(g,g), g = max(lo - p, 0, p - hi) per axis, nearest first; a subtree is skipped only when
 * lb > best dist2 so far (or lb is not finite) and descended on equality, and an entry popped from the stack is checked again.  No
 * margin is needed: q lies inside every box above its triangle, and fp32 subtraction, squaring and the two additions of dot are
 * monotone, so lb <= dist2_k holds ON THE BITS for every triangle below the box.  Otherwise (malformed or tiny scenes) the same
 * per-triangle function sweeps all n_tri triangles without a tree.  Both give the answer defined above, bit for bit.
 *
 * Memory, streams, ordering and errors are those of ezrt_multihit.h: every pointer is device memory of the scene's device, large
 * enough for its n elements (anything else is rejected before any launch, never dereferenced); work is enqueued on `stream` and the
 * call returns without synchronising; no scratch set is used; the call may run beside ezrt_render_device and the other queries on
 * other streams and leaves ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for it, and a call
 * issued after the refit returned sees the new geometry.
 *
 * Returns 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, points3 or tri_id; n < 0; a pointer that is not device
 * memory of the scene's device.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_CLOSEST_POINT_H
#define EZRT_CLOSEST_POINT_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_closest_point_device(EzrtScene* s, const float* points3 /* n x 3 */, const float* d_max /* n or NULL */, int n,
                                    int32_t* tri_id /* n */, float* point /* n x 3 or NULL */, float* dist /* n or NULL */,
                                    float* bary /* n x 2 or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
