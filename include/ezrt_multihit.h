/* ezrt_multihit.h -- stream-ordered all-hits queries on device memory (libezrt_hip.so only).
 *
 * Every triangle a ray crosses, in order of distance, where ezrt_query.h answers with the nearest one alone: crossing counts for
 * inside/outside tests, thickness and penetration depth, transparency and cut-away views, CSG picking, the exit point behind an
 * entry point -- in one traversal per ray and without re-shooting from a nudged origin (which moves t and loses layers closer
 * together than 0.0005).
 *
 *   rays_od6   n_rays x 6 floats: origin, direction (any length; not normalised by the library)
 *   t_max      n_rays floats, or NULL (= +inf for every ray)
 *   max_hits   K, 1 .. EZRT_ALL_HITS_MAX: the length of a ray's output row
 *
 * The list of a ray.  The reference's hitBVH (P5/fsh:254-306) does not prune: which triangles a ray is tested against is fixed by
 * the tree, and in which order by the ray.  Let V be the sequence of triangles hitBVH hands to hitTriangle for ray i, in the order
 * it reaches them: the nearer child first (a tie: the right one), a leaf's range in ascending index, no pruning of any kind.  A ray
 * sees only the triangles below a leaf: a triangle below no leaf of the caller's node array is in no V and in no list.  Let H
 * be the members of V with isHit and t < min(t_max[i], EZ_INF) (EZ_INF = 114514, ezrt_detmath.h; t_max == NULL: the bound is
 * EZ_INF; a NaN t_max: H is empty), sorted by t ascending with a STABLE sort: equal t keep their visit order.
 *
 * ezrt_query_all_hits_device:
 *   n_hits[i]                       |H|: the full count, which may exceed max_hits
 *   tri_id[i K + j], t_hit[i K + j] the j-th entry of the sorted H for j < min(|H|, K); {-1, EZ_INF} for the other slots
 *   n_hits may be NULL, and so may t_hit; tri_id may not.
 *   Consequences: slot 0 is bit for bit what ezrt_query_closest_device returns for the same ray and t_max, the copy that wins an
 *   exact tie included (the closest hit is the first member of V with the smallest t); n_hits[i] > 0 is
 *   ezrt_query_occluded_device's answer; a triangle id appears at most once in a row.  As everywhere in the library there is no
 *   t_min: a triangle is accepted at t >= 0.0005 only.
 *   One ray per lane on the reference's binary tree in the reference's order: every scene ezrt_render_paths serves is served.
 *
 * ezrt_surface_at_device: the surface attributes of hits the caller already holds -- rows of the lists above, or the {tri, t}
 *   ezrt_query_closest_device returned.  Element j gets, for triangle tri_id[j] at distance t_hit[j] along ray j (rays_od6[6 j ..],
 *   as given), what ezrt_query_surface_device (ezrt_surface.h) gives for its winner, computed by the same device function:
 *   hit_point = S + d * t, normal = the smooth normal in the form `integrator` selects (ezrt_surface.h), negated when inside,
 *   inside = the ray meets the triangle's back.  tri_id[j] < 0 or >= the scene's triangle count: zeros.  hit_point, normal and
 *   inside may each be NULL (not written), not all three.
 *
 * Memory, streams, ordering and errors are those of ezrt_shade.h: every pointer is device memory of the scene's device, large
 * enough for its n_rays x max_hits, n_rays or n elements (anything else is rejected before any launch, never dereferenced); work is
 * enqueued on `stream` and the call returns without synchronising; the calls use no scratch set -- the sorted list of a ray is
 * kept in its own output row -- may run beside ezrt_render_device and the other queries on other streams, and leave ezrt_counters
 * and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them, and a call issued after the refit returned sees the
 * new geometry.
 *
 * Returns 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, rays or tri_id; n_rays < 0 (n < 0); max_hits outside
 * [1, EZRT_ALL_HITS_MAX]; ezrt_surface_at_device: NULL t_hit, all three outputs NULL, an integrator not listed in ezrt_surface.h;
 * a pointer that is not device memory of the scene's device.  n_rays == 0 (n == 0) returns 0 and launches nothing. */
#ifndef EZRT_MULTIHIT_H
#define EZRT_MULTIHIT_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_ALL_HITS_MAX 64

int ezrt_query_all_hits_device(EzrtScene* s, const float* rays_od6, const float* t_max, int n_rays, int max_hits,
                               int32_t* tri_id /* n_rays x max_hits */, float* t_hit /* n_rays x max_hits */,
                               int32_t* n_hits /* n_rays */, void* stream);
int ezrt_surface_at_device(EzrtScene* s, const float* rays_od6 /* n x 6 */, const int32_t* tri_id /* n */,
                           const float* t_hit /* n */, int n, int integrator, float* hit_point /* n x 3 */,
                           float* normal /* n x 3 */, uint8_t* inside /* n */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
