/* ezrt_query.h -- stream-ordered ray queries on device memory (libezrt_hip.so only).
 *
 * Closest-hit and occlusion queries for rays that already live in device memory, enqueued on the caller's stream with no host
 * round trip: ambient occlusion, shadow rays to a light, visibility between two points, picking along a bounded segment.  They run
 * the render calls' traversal kernels (the persistent 4-wide kernel with its redo launch, or the binary kernel for scenes whose
 * boxes are not nested) and return exactly the reference's answers.
 *
 * "The reference's hit" of a ray means exactly what ezrt_query_hits (ezrt.h) returns for it: {tri, t}, and on a miss tri = -1 and
 * t = EZ_INF (114514, the reference's "infinity", ezrt_detmath.h).  Every hit has t < EZ_INF.  That is hitBVH on the caller's node
 * array: a ray sees only the triangles below a leaf it reaches -- a triangle below no leaf is never hit (the point and overlap
 * queries sweep such triangles; the ray queries do not) -- and of two triangles at one distance the one whose leaf the reference's
 * walk reaches first wins.
 *
 *   rays_od6   n_rays x 6 floats: origin, direction (any length; not normalised by the library)
 *   t_max      n_rays floats, or NULL (= +inf for every ray)
 *
 * ezrt_query_closest_device: {tri_id[i], t_hit[i]} = the reference's hit if tri >= 0 && t < t_max[i], else {-1, EZ_INF}.  With
 *   t_max == NULL this is bit for bit ezrt_query_hits.
 * ezrt_query_occluded_device: occluded[i] = (tri >= 0 && t < t_max[i]) ? 1 : 0.  A NaN t_max gives 0, as does one <= 0.0005 (no
 *   hit is closer); with t_max == NULL occluded[i] = (tri >= 0).  The traversal stops at the first triangle it accepts below
 *   t_max and skips every part of the tree that provably lies beyond it ("Occlusion queries").
 *
 * There is no t_min: like the reference's hitTriangle, a triangle is only accepted at t >= 0.0005.  Offsetting an origin off the
 * surface it starts on (along the normal, say) is the caller's job.
 *
 * Memory and streams:
 *   - Every non-NULL pointer is DEVICE memory of the scene's device (hipMalloc, a torch CUDA tensor), large enough for n_rays
 *     entries; anything else -- host memory included -- is rejected before anything is launched, never dereferenced.
 *   - Work is enqueued on `stream` (a hipStream_t of the scene's device; NULL = the default stream) and the call returns without
 *     waiting for it: the outputs are complete when the stream says so.  There is no host synchronisation in steady state.
 *   - Queries use a scratch set of their own (not the render calls'): it grows to the largest n_rays seen and is released with the
 *     scene.  Growing it may synchronise the device.
 *   - Queries on one scene must be ordered among themselves: issue them on one stream, or synchronise between them.
 *   - Queries may run concurrently with ezrt_render_device calls of the same scene on another stream: a scene's records are read
 *     only after ezrt_scene_create.  A refit (ezrt_refit.h) is the one call that rewrites them: it waits for the queries already
 *     issued on the scene, and queries issued after it returns see the new geometry.
 *   - A query changes no scene state a caller can observe: ezrt_counters and ezrt_last_render_ms report the render calls only.
 *
 * Returns 0 or a negative EZRT_ERR_* code (ezrt.h; message in ezrt_last_error()):
 *   EZRT_ERR_INVALID  NULL scene, rays or output; n_rays < 0; a pointer that is not device memory of the scene's device
 *   n_rays == 0 returns 0 and launches nothing. */
#ifndef EZRT_QUERY_H
#define EZRT_QUERY_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_closest_device(EzrtScene* s, const float* rays_od6, const float* t_max, int n_rays, int32_t* tri_id, float* t_hit,
                              void* stream);
int ezrt_query_occluded_device(EzrtScene* s, const float* rays_od6, const float* t_max, int n_rays, uint8_t* occluded,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif
