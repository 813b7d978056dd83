/* ezrt_shade.h -- stream-ordered shading queries on device memory (libezrt_hip.so only).
 *
 * What lies behind a hit (ezrt_query.h, ezrt_surface.h): the material of a triangle, what it reflects towards a direction, the
 * direction an integrator would continue in, and what the environment returns along a direction -- computed on the device by the
 * functions the render's shading kernels call (brdf_evaluate, brdf_evaluate_pdf, sample_brdf, sample_brdf_aniso, the hemisphere
 * sampler, hdr_color, hdr_pdf, hdr_color_pdf, sample_hdr), on the scene's own material table, so the values are the render's -- and
 * the reference's -- on the bits.  Direct lighting, light baking, a custom estimator or a denoiser's albedo buffer need no
 * re-implementation of the Disney BRDF or of the environment sampler.
 *
 *   tri_id      n int32: triangle ids as ezrt_query_closest_device / ezrt_query_surface_device return them.  The material of
 *               element i is the one the scene holds for tri_id[i] (per-triangle record -> material index -> material table row:
 *               the road of every shaded hit of a render call).  tri_id[i] < 0 (a miss) or >= the scene's triangle count gives
 *               zeros in every output of element i.
 *   V, N, L     n x 3 floats each, used as given: never normalised by the library.  V points AWAY from the surface (the render's
 *               -viewDir, i.e. minus the ray direction), N is the shading normal ezrt_query_surface_device returned, L the
 *               direction towards the light / of the next ray.
 *   integrator  EZRT_INTEGRATOR_P3_DIFFUSE, _P4_DISNEY, _P5_SOBOL, _P5_MIS or _P5_MIS_ANISO (ezrt.h): whose bounce loop is meant.
 *
 * ezrt_query_material_device: mat18[18 i .. 18 i + 17] = the 18 material floats of the triangle as given to ezrt_scene_create
 *   (texels 6-11 of its record: emissive, baseColor, subsurface, metallic, specular, specularTint, roughness, anisotropic, sheen,
 *   sheenTint, clearcoat, clearcoatGloss, IOR, transmission), on the bits, the sign of a zero included.
 *
 * ezrt_shade_eval_device: f_r[3 i .. 3 i + 2] and (pdf != NULL) pdf[i] as the integrator's bounce loop computes them for the
 *   direction L it continues in:
 *     3        f_r = baseColor / PI                                        pdf = 1 / (2 PI)
 *     4        f_r = BRDF_Evaluate_aniso with X, Y = getTangent(N)         pdf = 1 / (2 PI)
 *     50       f_r = BRDF_Evaluate (isotropic)                             pdf = 1 / (2 PI)
 *     51       f_r, pdf = BRDF_Evaluate and BRDF_Pdf (isotropic), the pair the MIS loop evaluates together
 *     52       f_r, pdf = their anisotropic forms with X, Y = getTangent(N)
 *
 * ezrt_shade_sample_device: L[3 i .. 3 i + 2] = the direction the integrator continues in for the random numbers xi[3 i .. 3 i + 2]:
 *     3, 4, 50 toNormalHemisphere(SampleHemisphere(xi1, xi2), N): xi3, V and the material are not read (tri_id still selects the
 *              zeros of a miss)
 *     51       SampleBRDF(xi1, xi2, xi3, V, N, material)
 *     52       its anisotropic form with X, Y = getTangent(N)
 *
 * ezrt_env_eval_device: colour[3 i .. 3 i + 2] = hdrColor(L) (colour != NULL) and pdf[i] = hdrPdf(L) (pdf != NULL); at least one
 *   of the two.  env_clamp as in EzrtRenderParams: > 0 clamps every channel to it (chapter 3 uses 10), else no clamp.  Each value
 *   is the same whichever outputs are requested.
 * ezrt_env_sample_device: L[3 i .. 3 i + 2] = SampleHdr(xi[2 i], xi[2 i + 1]), a direction drawn from the environment's importance
 *   cache.
 *   Both read the environment in whichever device layout the scene's options selected (env_rgbe, env_pairs, env_planes, the filter of
 *   ezrt_scene_set_env).
 *
 * Memory, streams, ordering and errors are those of ezrt_query.h: every non-NULL pointer is device memory of the scene's device,
 * large enough for n elements (anything else is rejected before any launch, never dereferenced); work is enqueued on `stream` and
 * the call returns without synchronising; the calls may run beside ezrt_render_device on another stream, leave ezrt_counters and
 * ezrt_last_render_ms alone, and a later refit (ezrt_refit.h: it rewrites the per-triangle records these calls read) waits for
 * them.  They use no scratch memory at all.
 *
 * Returns 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene or required pointer (every pointer not marked "may be
 * NULL"; both outputs of ezrt_env_eval_device NULL); n < 0; an integrator not listed above; a pointer that is not device memory of
 * the scene's device; an environment call on a scene without an environment (ezrt_scene_set_env); ezrt_env_sample_device, or
 * ezrt_env_eval_device with a pdf output, on a scene whose environment has no cache.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_SHADE_H
#define EZRT_SHADE_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_material_device(EzrtScene* s, const int32_t* tri_id, int n, float* mat18, void* stream);
int ezrt_shade_eval_device(EzrtScene* s, int integrator, const int32_t* tri_id, const float* V, const float* N, const float* L,
                           int n, float* f_r /* n x 3 */, float* pdf /* n, may be NULL */, void* stream);
int ezrt_shade_sample_device(EzrtScene* s, int integrator, const int32_t* tri_id, const float* xi /* n x 3 */, const float* V,
                             const float* N, int n, float* L /* n x 3 */, void* stream);
int ezrt_env_eval_device(EzrtScene* s, const float* L, int n, float env_clamp, float* colour /* n x 3, may be NULL */,
                         float* pdf /* n, may be NULL */, void* stream);
int ezrt_env_sample_device(EzrtScene* s, const float* xi /* n x 2 */, int n, float* L /* n x 3 */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
