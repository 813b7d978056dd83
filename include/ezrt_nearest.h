/* ezrt_nearest.h -- stream-ordered nearest-K queries on device memory (libezrt_hip.so only).
 *
 * Which triangles of the mesh lie around a given point: the K nearest in order, and how many lie within a radius.  The question behind
 * a collision broad-phase ("everything within r"), contact manifolds, distance fields that blend several nearby triangles,
 * point-to-mesh registration with outlier rejection and proximity-based ambient occlusion.  ezrt_closest_point.h gives the winner;
 * this gives the list and the full count, as ezrt_multihit.h does beside the closest hit of a ray.
 *
 *   points3    n x 3 floats: the query points
 *   d_max      n floats, or NULL (= +inf for every point): only triangles within this distance are candidates
 *   max_k      K, the slots per point, 1 .. EZRT_NEAREST_MAX
 *
 * THE DEFINITION of ezrt_query_nearest_device is that of ezrt_closest_point.h, extended.  For a query point p, dist2_k of triangle k
 * (all fp32, operation by operation) and the candidate set C are exactly those of that header: with B = d_max*d_max (fp32; +inf when
 * d_max is NULL), C holds the triangles k in [0, n_tri) whose dist2_k is finite and <= B; a d_max that is not >= 0 (NaN, negative)
 * gives no candidates, and so does a non-finite p (every dist2_k is then inf or NaN).  L is C sorted ascending by the pair
 * (dist2_k, k): equal dist2 are ordered by ascending triangle index -- the index in the array given to ezrt_scene_create.  THE ANSWER
 * NEVER DEPENDS ON THE TREE or on the order in which the triangles are met.
 *
 * Outputs per point i, K = max_k:
 *   tri_id[i*K + j]   the j-th entry of L, for j < min(|C|, K); -1 in the other slots
 *   dist[i*K + j]     sqrtf(dist2) of that entry; +inf in the other slots (NOT EZ_INF, as in ezrt_closest_point.h)
 *   n_within[i]       |C|: the full number of triangles within d_max, which may exceed K                       (may be NULL)
 *
 * What follows from it:
 *   slot 0 is, bit for bit, ezrt_query_closest_point_device's {tri_id, dist} for the same p and d_max (the smallest dist2, the
 *   lowest index among equals; {-1, +inf} for a miss);
 *   the first j slots of a K-row equal the j-row: a larger K only appends;
 *   a triangle id appears at most once in a row (a triangle is one element of C, whatever copies of it the array holds);
 *   dist is ascending along a row, and tri_id ascending among equal dist2.
 * The nearest points and barycentrics of the entries of a row come from ezrt_closest_point_at_device.
 *
 * WHAT n_within COSTS.  Without it (n_within == NULL) the search radius is B until the K slots are full and then shrinks to the
 * dist2 of the K-th entry, so the work is that of a closest-point query reaching a little further.  With it the count ranges over
 * EVERYTHING within d_max, so the walk cannot shrink its radius below B: every triangle within d_max of the point is evaluated, and
 * with d_max == NULL every triangle of the scene is, for every point.  Ask for the count together with a d_max, or not at all.
 *
 * ezrt_closest_point_at_device is to ezrt_query_nearest_device what ezrt_surface_at_device is to ezrt_query_all_hits_device: for
 * pairs the caller holds -- point j against triangle tri_id[j] -- it returns what ezrt_query_closest_point_device returns for its
 * winner, by the same per-triangle evaluation:
 *   point   q of triangle tri_id[j] for point j                                                      (may be NULL)
 *   dist    sqrtf(dist2_k)                                                                           (may be NULL)
 *   bary    (v, w) of the projection; attributes interpolate with (1-v-w, v, w) over (p1, p2, p3)    (may be NULL)
 * An element whose tri_id[j] < 0 or >= n_tri, or whose dist2 is not finite, gets (zeros, +inf, zeros).  Not all three outputs may be
 * NULL.  For the rows of a nearest-K answer pass each point K times (the Python wrapper broadcasts).  d_max plays no part here.
 *
 * How it is computed.  One point per lane.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1; decided per call) the
 * best-first walk of ezrt_closest_point.h over the 4-wide records, its stack column in LDS, carrying the sorted list in the point's
 * own output rows: dist holds dist2 during the walk, the pair of the K-th entry is kept in registers once the row is full, and a
 * candidate that does not precede it is only counted.  A subtree is skipped only when its box distance lb > radius (or lb is not
 * finite) and descended on equality -- a lower index at an equal dist2 displaces the last entry -- without any margin: lb <= dist2_k
 * holds on the bits (ezrt_closest_point.h).  Triangles below no leaf are swept after the walk.  Otherwise (malformed or tiny scenes)
 * every triangle is swept without a tree.  A final pass turns dist2 into dist and fills the unused slots.  Both routes, with and
 * without n_within, give the answer defined above, bit for bit.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its n (or n x max_k) elements (anything else is rejected before any launch, never dereferenced); work is enqueued on
 * `stream` and the call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the
 * other queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them,
 * and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, points3, tri_id or dist (ezrt_closest_point_at_device:
 * NULL scene, points3 or tri_id, or all three outputs NULL); n < 0; max_k outside [1, EZRT_NEAREST_MAX]; a pointer that is not
 * device memory of the scene's device.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_NEAREST_H
#define EZRT_NEAREST_H

#include <stdint.h>

#include "ezrt.h"

#define EZRT_NEAREST_MAX 64

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_nearest_device(EzrtScene* s, const float* points3 /* n x 3 */, const float* d_max /* n or NULL */, int n, int max_k,
                              int32_t* tri_id /* n x max_k */, float* dist /* n x max_k */, int32_t* n_within /* n or NULL */,
                              void* stream);
int ezrt_closest_point_at_device(EzrtScene* s, const float* points3 /* n x 3 */, const int32_t* tri_id /* n */, int n,
                                 float* point /* n x 3 or NULL */, float* dist /* n or NULL */, float* bary /* n x 2 or NULL */,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
