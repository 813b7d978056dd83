/* ezrt_surface.h -- stream-ordered surface queries on device memory (libezrt_hip.so only).
 *
 * The closest hit of every ray (ezrt_query.h) together with the rest of the reference's HitResult for it (P5/fsh:74-82,
 * hitTriangle P5/fsh:165-214): the hit point, the shading normal and the side the ray came from.  What a bounce ray, a shadow
 * ray or an ambient-occlusion ray needs to start from a surface, computed on the device by the same function that shades every hit
 * of a render call, so the values are the render's -- and the reference's -- on the bits.
 *
 *   rays_od6    n_rays x 6 floats: origin S, direction d (any length; not normalised by the library)
 *   t_max       n_rays floats, or NULL (= +inf for every ray)
 *   integrator  which form of the smooth-normal interpolation, as the render call picks it:
 *                 EZRT_INTEGRATOR_P3_DIFFUSE, EZRT_INTEGRATOR_P4_DISNEY        the +-0.00005 form (P3/fsh:273-274, P4/fsh:196-197)
 *                 EZRT_INTEGRATOR_P5_SOBOL, _P5_MIS, _P5_MIS_ANISO            the +1e-7 form (P5/fsh:206-207)
 *
 * Outputs (tri_id and t_hit required; hit_point, normal and inside each optional: NULL = not written):
 *   tri_id[i], t_hit[i]      bit for bit what ezrt_query_closest_device returns for the same rays and t_max
 *   hit_point[3i..3i+2]      P = S + d * t
 *   normal[3i..3i+2]         the smooth normal: the vertex normals interpolated at P, normalised, negated when inside
 *   inside[i]                1 if dot(N_geom, d) > 0 (the ray meets the triangle's back), else 0; N_geom = normalize(cross(p2 - p1,
 *                            p3 - p1))
 * For a miss -- including a hit at t >= t_max and a ray whose t_max no hit can beat -- hit_point, normal and inside are zeros.
 * As in ezrt_query.h a ray sees only the triangles below a leaf of the caller's node array: a triangle below no leaf is never the
 * winner.  (ezrt_surface_at_device, ezrt_multihit.h, takes any triangle id of the scene: it walks no tree.)
 *
 * There is no material output: the winner's material is tri36[tri_id * 36 + 18 .. + 36) of the caller's own triangle array.
 *
 * Memory, streams, scratch, ordering and errors are those of ezrt_query.h: every non-NULL pointer is device memory of the scene's
 * device (anything else is rejected before any launch); the call returns without synchronising; it uses the query scratch set, may
 * run beside ezrt_render_device on another stream, leaves ezrt_counters and ezrt_last_render_ms alone, and a later refit
 * (ezrt_refit.h) waits for it.
 *
 * Returns 0 or EZRT_ERR_INVALID (NULL scene, rays, tri_id or t_hit; n_rays < 0; an integrator not listed above; a pointer that is
 * not device memory of the scene's device).  n_rays == 0 returns 0 and launches nothing. */
#ifndef EZRT_SURFACE_H
#define EZRT_SURFACE_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_surface_device(EzrtScene* s, const float* rays_od6, const float* t_max, int n_rays, int integrator,
                              int32_t* tri_id, float* t_hit, float* hit_point, float* normal, uint8_t* inside, void* stream);

#ifdef __cplusplus
}
#endif
#endif
