/* ezrt_path.h -- stream-ordered path queries on device memory (libezrt_hip.so only).
 *
 * The layer the other device queries feed (ezrt_query.h, ezrt_surface.h, ezrt_shade.h): the render's own primary rays, and the
 * radiance an integrator's pathTracing returns along rays of the caller's choosing -- computed by the device functions a render
 * call runs (the ray generator of main() and the one-lane bounce loop behind ezrt_render_paths), so the values are the render's --
 * and the reference's -- on the bits.  Light-map and probe baking, non-pinhole cameras or a denoiser's reference radiance at chosen
 * pixels need no re-implementation of the seed rules, the Sobol / Cranley-Patterson dimensions of a bounce, the MIS weights, the
 * break conditions or the order of a multiplication.
 *
 *   sample_xyf  n x 3 uint32: sample_xyf[3 i .. 3 i + 2] = (ix, iy, frame) names the PIXEL-SAMPLE whose random numbers element i
 *               uses -- the pixel (ix, iy) of frame `frame` (EzrtRenderParams: frame0 + k).  It does not say where a ray points.
 *   rays_od6    n x 6 floats: origin, direction.
 *   integrator  EZRT_INTEGRATOR_P3_DIFFUSE, _P4_DISNEY, _P5_SOBOL, _P5_MIS or _P5_MIS_ANISO (ezrt.h).
 *
 * ezrt_camera_rays_device: rays_od6[6 i .. 6 i + 5] = the primary ray main() shoots for pixel-sample i: the origin is p->eye; the
 *   direction is seeded with (ix * 1973 + iy * 9277 + frame * 26699) | 1, jittered by two draws of the RNG, turned by
 *   p->camera_rotate and normalised -- the bits a render call of `p` traces for that pixel of that frame.  Of `p` only width,
 *   height, eye and camera_rotate are read: the pixel rect, the tiles and the shard are not applied, and ix / iy are not checked
 *   against width / height (a pixel beyond the frame is computed like any other).  `s` supplies the device; its records are not
 *   read.
 *
 * ezrt_query_radiance_device: radiance[3 i .. 3 i + 2] = the `colour` the pathTracing of `integrator` gives with max_bounce bounces
 *   and env_clamp (both as in EzrtRenderParams) for the primary ray rays_od6[6 i ..], used as given: never normalised.  The RNG
 *   state is the pixel-sample's seed ADVANCED BY THE TWO JITTER DRAWS, the state main() has when it reaches hitBVH; the
 *   Cranley-Patterson offsets come from (ix, iy), the Sobol index is the Gray code of frame + 1; the scene's sampler setting
 *   (ezrt_scene_set_sampler) and environment (ezrt_scene_set_env, in whichever device layout the options selected) are used.  A
 *   ray that misses gives hdrColor(direction) with the clamp; max_bounce == 0 gives the emission of what it hits.
 *   Consequence: with the rays ezrt_camera_rays_device returns for the same sample_xyf, the result is bit for bit the `colour`
 *   ezrt_render_paths reports for that pixel and frame (a NaN equals a NaN: ezrt.h "Numerical contract").
 *   One path per lane, as the kernel behind ezrt_render_paths: every scene that one serves is served.
 *
 * Memory, streams, ordering and errors are those of ezrt_shade.h: every pointer is device memory of the scene's device, large
 * enough for n elements (anything else is rejected before any launch, never dereferenced); work is enqueued on `stream` and the
 * call returns without synchronising; the calls use no scratch memory, may run beside ezrt_render_device and the other queries on
 * other streams, and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them, and a call
 * issued after the refit returned sees the new geometry.
 *
 * Returns 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, params or pointer; n < 0; a pointer that is not device
 * memory of the scene's device; ezrt_camera_rays_device: width or height <= 0; ezrt_query_radiance_device: max_bounce outside
 * [0, 64] (the range of a render call), an integrator not listed above, a scene without an environment (ezrt_scene_set_env),
 * integrator 51 or 52 on a scene whose environment has no cache.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_PATH_H
#define EZRT_PATH_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_camera_rays_device(EzrtScene* s, const EzrtRenderParams* p, const uint32_t* sample_xyf /* n x 3 */, int n,
                            float* rays_od6 /* n x 6 */, void* stream);
int ezrt_query_radiance_device(EzrtScene* s, int integrator, int max_bounce, float env_clamp, const float* rays_od6 /* n x 6 */,
                               const uint32_t* sample_xyf /* n x 3 */, int n, float* radiance /* n x 3 */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
