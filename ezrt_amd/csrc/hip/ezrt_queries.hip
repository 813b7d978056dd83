// ezrt_queries.hip -- the device queries that are ONE kernel on the caller's stream and need no scratch: shading queries
// (include/ezrt_shade.h), path queries (include/ezrt_path.h), all-hits queries and surface_at (include/ezrt_multihit.h), closest-point,
// nearest-K, inside / signed-distance, box-overlap, triangle-overlap, self-overlap, triangle-distance, sphere-cast, segment,
// oriented-box, winding-number, plane, plane-loop and overlap-list queries (include/ezrt_closest_point.h, ezrt_nearest.h, ezrt_inside.h,
// ezrt_box_overlap.h, ezrt_tri_overlap.h, ezrt_self_overlap.h, ezrt_tri_distance.h, ezrt_sphere_cast.h, ezrt_segment.h,
// ezrt_obb_overlap.h, ezrt_winding.h, ezrt_plane.h, ezrt_plane_loops.h, ezrt_overlap_list.h).  The few that are more than one kernel
// are a handful of launches each: the sliced winding call is a memset, a kernel and a finishing kernel, the plane count a sweep and two
// small kernels, an overlap list's fill a routed kernel and, on the walk route, a sort, and the plane loops six launches over the
// caller's `work`.  The mesh processing, whose calls are many launches over a work buffer, is in ezrt_mesh.hip.  A translation unit of
// its own: none of its kernels is compiled together with the render pipeline's (ezrt_launch.hip), so a change here cannot move a
// register of a timed kernel.  The ray queries that run the pipeline's trace kernels (ezrt_query_closest_device,
// ezrt_query_occluded_device, ezrt_query_surface_device) are in ezrt_launch.hip.  Every call here goes through query_call
// (ezrt_internal.h).  DESIGN.md 5.
#include "ezrt_internal.h"
#include "ezrt_shade.h"
#include "ezrt_path.h"
#include "ezrt_multihit.h"
#include "ezrt_closest_point.h"
#include "ezrt_inside.h"
#include "ezrt_nearest.h"
#include "ezrt_box_overlap.h"
#include "ezrt_tri_overlap.h"
#include "ezrt_self_overlap.h"
#include "ezrt_tri_distance.h"
#include "ezrt_sphere_cast.h"
#include "ezrt_segment.h"
#include "ezrt_obb_overlap.h"
#include "ezrt_winding.h"
#include "ezrt_plane.h"
#include "ezrt_plane_loops.h"
#include "ezrt_overlap_list.h"
#include "ezrt_query_kernels.h"
#include "ezrt_scan_kernels.h"
#include "ezrt_point_queries.h"

using ezi::known_integrator;
using ezi::stack_lds_bytes;

template <int INTEG>
static void launch_shade_eval(EzrtScene* s, dim3 g, dim3 b, hipStream_t st, const int32_t* tri_id, const float* V, const float* N,
                              const float* L, int n, float* f_r, float* pdf) {
  if (pdf)
    hipLaunchKernelGGL((shade_eval_kernel<INTEG, true>), g, b, 0, st, s->tri_shade.p, s->mat_table.p, (int32_t)s->n_tri, tri_id, V, N, L,
                       (uint32_t)n, f_r, pdf);
  else
    hipLaunchKernelGGL((shade_eval_kernel<INTEG, false>), g, b, 0, st, s->tri_shade.p, s->mat_table.p, (int32_t)s->n_tri, tri_id, V, N, L,
                       (uint32_t)n, f_r, pdf);
}
// ---- point queries on device memory: what their kernels read of the scene, and the route of this call -- chosen per call: a refit
// can change whether the scene prunes.  lds = the lane's stack column of the best-first walk (ezrt_point_queries.h: point_walk):
// {lb, ref} per pending entry (+ 1 of slack).  A tree so lopsided that the column exceeds the 64 KiB of a launch without opt-in
// (> 127 entries: (need + 1) * 512 B <= 65 536 B admits 127; none of the builders comes near, and under the depth cap of 63 no
// caller's tree does -- at most 3 entries per two levels of its 62: 93) is swept instead, as is a scene that does not prune.
struct PointRoute {
  bool walk;
  size_t lds;
};
static PointRoute point_scene(const EzrtScene* s, PointScene& sc) {
  sc.tri_geom = s->tri_geom.p;
  sc.inner4 = s->inner4.p;
  sc.uncovered = s->cp_uncovered.p;
  sc.n_uncovered = s->n_cp_uncovered;
  sc.n_tri = s->n_tri;
  const size_t lds = ((size_t)s->stack_need_cp + 1) * 2 * CP_BLOCK * sizeof(int);
  return {s->prunable && s->n_inner4 > 0 && lds <= 64 * 1024, lds};
}
// the launch of a routed kernel for n points or boxes, CP_BLOCK per workgroup: the walking instance on `lds` bytes of stack column, or
// the sweeping one
template <class Args>
static void launch_routed(void (*walk)(Args), void (*sweep)(Args), const PointRoute& r, size_t lds, size_t n, hipStream_t st, const Args& a) {
  const dim3 g((unsigned)((n + CP_BLOCK - 1) / CP_BLOCK)), b(CP_BLOCK);
  if (r.walk) hipLaunchKernelGGL(walk, g, b, lds, st, a);
  else hipLaunchKernelGGL(sweep, g, b, 0, st, a);
}

// ---- overlap lists on device memory (include/ezrt_overlap_list.h): the fill call that the five entry points at the end of this file
// share.  in0 and in1 are the query's inputs (a null one is skipped), set(a) fills the query's own members of Args, walk and sweep are
// its list kernel, and lds_div is 2 for slot_walk's column of bare references and 1 for point_walk's, as in the max_k sibling.  One
// routed kernel on `st`, and on the walk route overlap_sort_kernel behind it; no scratch; checked, launched and ordered against a
// refit by query_call.
template <class Args, class Set>
static int overlap_list_call(const char* name, EzrtScene* s, bool inputs, ezi::DeviceBuf in0, ezi::DeviceBuf in1, int n, const int64_t* offsets,
                             int64_t capacity, int32_t* tri_id, int32_t* n_found, void* stream, void (*walk)(Args), void (*sweep)(Args),
                             size_t lds_div, Set set) {
  return ezi::guarded(name, [&]() -> int {
    if (!s || !inputs || !offsets || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (capacity < 0) return fail(EZRT_ERR_INVALID, "capacity < 0");
    // (the byte count below must not wrap: a wrapped one would pass the buffer check and leave list_row a capacity that is none)
    if (capacity > (int64_t)(PTRDIFF_MAX / sizeof(int32_t))) return fail(EZRT_ERR_INVALID, "capacity exceeds what an array can hold");
    if (!tri_id && capacity > 0) return fail(EZRT_ERR_INVALID, "NULL tri_id with capacity > 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, cap = (size_t)capacity;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {in0, in1, {offsets, (N + 1) * sizeof(int64_t)}, {tri_id, cap * sizeof(int32_t)}, {n_found, N * sizeof(int32_t)}}, N, st,
                      [&](dim3, dim3) {
      Args a;
      const PointRoute r = point_scene(s, a.sc);
      a.offsets = (const long long*)offsets;
      a.capacity = (long long)capacity;
      a.tri = tri_id;
      a.n_found = n_found;
      a.n = (uint32_t)n;
      set(a);
      launch_routed(walk, sweep, r, r.lds / lds_div, N, st, a);
      // pass 2: the sweep fills in ascending id, and no row longer than OL_INSERT_MAX fits a smaller capacity
      if (!OL_SKIP_SORT && r.walk && capacity > (OL_INSERT_MAX > 1 ? OL_INSERT_MAX : 1)) {
        OverlapSortArgs o;
        o.offsets = a.offsets;
        o.capacity = a.capacity;
        o.tri = tri_id;
        o.n = a.n;
        o.n_tri = a.sc.n_tri;
        hipLaunchKernelGGL(overlap_sort_kernel, dim3((unsigned)((N + OL_SORT_ROWS - 1) / OL_SORT_ROWS)), dim3(OL_SORT_BLOCK), 0, st, o);
      }
    });
  });
}

// ---- the lowest max_k overlapping triangles per query, on device memory (include/ezrt_box_overlap.h, ezrt_obb_overlap.h,
// ezrt_tri_overlap.h, ezrt_self_overlap.h, ezrt_segment.h): the call that the five max_k entry points share, overlap_list_call's
// sibling with the same in0, in1, set, walk, sweep and lds_div.  `max` is the query's EZRT_*_OVERLAP_MAX.  One routed kernel on `st`,
// no scratch (a query's list is kept in its own output row); checked, launched and ordered against a refit by query_call.
template <class Args, class Set>
static int overlap_rows_call(const char* name, EzrtScene* s, bool inputs, ezi::DeviceBuf in0, ezi::DeviceBuf in1, int n, int max_k, int max,
                             int32_t* tri_id, int32_t* n_overlap, void* stream, void (*walk)(Args), void (*sweep)(Args), size_t lds_div,
                             Set set) {
  return ezi::guarded(name, [&]() -> int {
    if (!s || !inputs || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (max_k < 0 || max_k > max) return fail(EZRT_ERR_INVALID, "max_k out of range [0,%d]", max);
    if (max_k > 0 && !tri_id) return fail(EZRT_ERR_INVALID, "tri_id is required when max_k > 0");
    if (max_k == 0 && !n_overlap) return fail(EZRT_ERR_INVALID, "n_overlap is required when max_k == 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, K = (size_t)max_k;
    if (max_k == 0) tri_id = nullptr; // ignored
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {in0, in1, {tri_id, N * K * sizeof(int32_t)}, {n_overlap, N * sizeof(int32_t)}}, N, st, [&](dim3, dim3) {
      Args a;
      const PointRoute r = point_scene(s, a.sc);
      a.n = (uint32_t)n;
      a.K = max_k;
      a.div_k = make_fastdiv((uint32_t)(max_k > 0 ? max_k : 1));
      a.tri = tri_id;
      a.n_overlap = n_overlap;
      set(a);
      launch_routed(walk, sweep, r, r.lds / lds_div, N, st, a);
    });
  });
}

extern "C" {
// ---- shading queries on device memory (include/ezrt_shade.h)
int ezrt_query_material_device(EzrtScene* s, const int32_t* tri_id, int n, float* mat18, void* stream) {
  return ezi::guarded("ezrt_query_material_device", [&]() -> int {
    if (!s || !tri_id || !mat18 || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri_id, N * sizeof(int32_t)}, {mat18, N * 18 * sizeof(float)}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(shade_material_kernel, g, b, 0, st, s->tri_shade.p, s->mat_table.p, (int32_t)s->n_tri, tri_id, (uint32_t)n, mat18);
    });
  });
}
int ezrt_shade_eval_device(EzrtScene* s, int integrator, const int32_t* tri_id, const float* V, const float* N, const float* L, int n,
                           float* f_r, float* pdf, void* stream) {
  return ezi::guarded("ezrt_shade_eval_device", [&]() -> int {
    if (!s || !tri_id || !V || !N || !L || !f_r || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!known_integrator(integrator)) return fail(EZRT_ERR_INVALID, "unknown integrator %d", integrator);
    if (n == 0) return 0;
    const size_t K = (size_t)n, v3 = K * 3 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri_id, K * sizeof(int32_t)}, {V, v3}, {N, v3}, {L, v3}, {f_r, v3}, {pdf, K * sizeof(float)}}, K, st,
                      [&](dim3 g, dim3 b) { // each kernel is compiled for its integrator
                        ezi::with_integrator(integrator, [&](auto I) { launch_shade_eval<decltype(I)::value>(s, g, b, st, tri_id, V, N, L, n, f_r, pdf); });
                      });
  });
}
int ezrt_shade_sample_device(EzrtScene* s, int integrator, const int32_t* tri_id, const float* xi, const float* V, const float* N, int n,
                             float* L, void* stream) {
  return ezi::guarded("ezrt_shade_sample_device", [&]() -> int {
    if (!s || !tri_id || !xi || !V || !N || !L || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!known_integrator(integrator)) return fail(EZRT_ERR_INVALID, "unknown integrator %d", integrator);
    if (n == 0) return 0;
    const size_t K = (size_t)n, v3 = K * 3 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri_id, K * sizeof(int32_t)}, {xi, v3}, {V, v3}, {N, v3}, {L, v3}}, K, st, [&](dim3 g, dim3 b) {
      const float4 *ts = s->tri_shade.p, *mt = s->mat_table.p;
      const int32_t nt = (int32_t)s->n_tri;
      if (integrator == EZRT_INTEGRATOR_P5_MIS)
        hipLaunchKernelGGL(shade_sample_kernel<EZRT_INTEGRATOR_P5_MIS>, g, b, 0, st, ts, mt, nt, tri_id, xi, V, N, (uint32_t)n, L);
      else if (integrator == EZRT_INTEGRATOR_P5_MIS_ANISO)
        hipLaunchKernelGGL(shade_sample_kernel<EZRT_INTEGRATOR_P5_MIS_ANISO>, g, b, 0, st, ts, mt, nt, tri_id, xi, V, N, (uint32_t)n, L);
      else // 3, 4 and 50 continue in the same direction: the uniform hemisphere about N
        hipLaunchKernelGGL(shade_sample_kernel<EZRT_INTEGRATOR_P5_SOBOL>, g, b, 0, st, ts, mt, nt, tri_id, xi, V, N, (uint32_t)n, L);
    });
  });
}
int ezrt_env_eval_device(EzrtScene* s, const float* L, int n, float env_clamp, float* colour, float* pdf, void* stream) {
  return ezi::guarded("ezrt_env_eval_device", [&]() -> int {
    if (!s || !L || (!colour && !pdf) || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument (one of colour and pdf is required) or n < 0");
    if (!s->hdr.p) return fail(EZRT_ERR_INVALID, "the scene has no environment (ezrt_scene_set_env)");
    if (pdf && !s->has_cache) return fail(EZRT_ERR_INVALID, "the pdf needs the env cache (ezrt_scene_set_env)");
    if (n == 0) return 0;
    const size_t K = (size_t)n, v3 = K * 3 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{L, v3}, {colour, v3}, {pdf, K * sizeof(float)}}, K, st, [&](dim3 g, dim3 b) {
      const DevScene sc = s->dev();
      if (colour && pdf) hipLaunchKernelGGL((env_eval_kernel<true, true>), g, b, 0, st, sc, L, (uint32_t)n, env_clamp, colour, pdf);
      else if (colour) hipLaunchKernelGGL((env_eval_kernel<true, false>), g, b, 0, st, sc, L, (uint32_t)n, env_clamp, colour, pdf);
      else hipLaunchKernelGGL((env_eval_kernel<false, true>), g, b, 0, st, sc, L, (uint32_t)n, env_clamp, colour, pdf);
    });
  });
}
int ezrt_env_sample_device(EzrtScene* s, const float* xi, int n, float* L, void* stream) {
  return ezi::guarded("ezrt_env_sample_device", [&]() -> int {
    if (!s || !xi || !L || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!s->hdr.p) return fail(EZRT_ERR_INVALID, "the scene has no environment (ezrt_scene_set_env)");
    if (!s->has_cache) return fail(EZRT_ERR_INVALID, "sampling needs the env cache (ezrt_scene_set_env)");
    if (n == 0) return 0;
    const size_t K = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{xi, K * 2 * sizeof(float)}, {L, K * 3 * sizeof(float)}}, K, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(env_sample_kernel, g, b, 0, st, s->dev(), xi, (uint32_t)n, L);
    });
  });
}

// ---- path queries on device memory (include/ezrt_path.h): one kernel each on `st`, no scratch; checked, launched and ordered
// against a refit by query_call
int ezrt_camera_rays_device(EzrtScene* s, const EzrtRenderParams* p, const uint32_t* sample_xyf, int n, float* rays_od6, void* stream) {
  return ezi::guarded("ezrt_camera_rays_device", [&]() -> int {
    if (!s || !sample_xyf || !rays_od6 || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!p) return fail(EZRT_ERR_INVALID, "params is NULL");
    if (p->width <= 0 || p->height <= 0) return fail(EZRT_ERR_INVALID, "width/height must be positive");
    if (n == 0) return 0;
    const size_t K = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{sample_xyf, K * 3 * sizeof(uint32_t)}, {rays_od6, K * 6 * sizeof(float)}}, K, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(camera_rays_kernel, g, b, 0, st, *p, sample_xyf, (uint32_t)n, rays_od6);
    });
  });
}
int ezrt_query_radiance_device(EzrtScene* s, int integrator, int max_bounce, float env_clamp, const float* rays_od6,
                               const uint32_t* sample_xyf, int n, float* radiance, void* stream) {
  return ezi::guarded("ezrt_query_radiance_device", [&]() -> int {
    if (!s || !rays_od6 || !sample_xyf || !radiance || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    // (the states a render call rejects, in its words: validate_params)
    if (max_bounce < 0 || max_bounce > 64) return fail(EZRT_ERR_INVALID, "max_bounce out of range [0,64]");
    if (!known_integrator(integrator)) return fail(EZRT_ERR_INVALID, "unknown integrator");
    if (!s->hdr.p) return fail(EZRT_ERR_INVALID, "the scene has no environment (ezrt_scene_set_env)");
    if ((integrator == EZRT_INTEGRATOR_P5_MIS || integrator == EZRT_INTEGRATOR_P5_MIS_ANISO) && !s->has_cache)
      return fail(EZRT_ERR_INVALID, "integrator 51 needs the env cache (ezrt_scene_set_env)");
    if (n == 0) return 0;
    const size_t K = (size_t)n, v3 = K * 3 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{rays_od6, 2 * v3}, {sample_xyf, K * 3 * sizeof(uint32_t)}, {radiance, v3}}, K, st, [&](dim3 g, dim3 b) {
      RadianceArgs a;
      a.sc = s->dev();
      a.rays = rays_od6;
      a.xyf = sample_xyf;
      a.n = (uint32_t)n;
      a.max_bounce = max_bounce;
      a.env_clamp = env_clamp;
      a.radiance = radiance;
      const size_t lds = stack_lds_bytes(s); // the traversal stack of the megakernel launch: s->depth entries per lane
      // each kernel is compiled for its integrator
      ezi::with_integrator(integrator, [&](auto I) { hipLaunchKernelGGL(radiance_query_kernel<decltype(I)::value>, g, b, lds, st, a); });
    });
  });
}

// ---- all-hits queries on device memory (include/ezrt_multihit.h): one kernel each on `st`, no scratch (a ray's sorted list is kept
// in its own output row); checked, launched and ordered against a refit by query_call
int ezrt_query_all_hits_device(EzrtScene* s, const float* rays_od6, const float* t_max, int n_rays, int max_hits, int32_t* tri_id,
                               float* t_hit, int32_t* n_hits, void* stream) {
  return ezi::guarded("ezrt_query_all_hits_device", [&]() -> int {
    if (!s || !rays_od6 || !tri_id || n_rays < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n_rays < 0");
    if (max_hits < 1 || max_hits > EZRT_ALL_HITS_MAX) return fail(EZRT_ERR_INVALID, "max_hits out of range [1,%d]", EZRT_ALL_HITS_MAX);
    if (n_rays == 0) return 0;
    const size_t N = (size_t)n_rays, K = (size_t)max_hits;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{rays_od6, N * 6 * sizeof(float)}, {t_max, N * sizeof(float)}, {tri_id, N * K * sizeof(int32_t)},
                          {t_hit, N * K * sizeof(float)}, {n_hits, N * sizeof(int32_t)}}, N, st, [&](dim3 g, dim3 b) {
      AllHitsArgs a;
      a.sc = s->dev();
      a.rays = rays_od6;
      a.t_max = t_max;
      a.n = (uint32_t)n_rays;
      a.K = max_hits;
      a.div_k = make_fastdiv((uint32_t)max_hits);
      a.tri = tri_id;
      a.t = t_hit;
      a.n_hits = n_hits;
      const size_t lds = stack_lds_bytes(s); // the traversal stack of the megakernel launch: s->depth entries per lane
      if (t_hit) hipLaunchKernelGGL(all_hits_kernel<true>, g, b, lds, st, a);
      else hipLaunchKernelGGL(all_hits_kernel<false>, g, b, lds, st, a);
    });
  });
}
int ezrt_surface_at_device(EzrtScene* s, const float* rays_od6, const int32_t* tri_id, const float* t_hit, int n, int integrator,
                           float* hit_point, float* normal, uint8_t* inside, void* stream) {
  return ezi::guarded("ezrt_surface_at_device", [&]() -> int {
    if (!s || !rays_od6 || !tri_id || !t_hit || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!hit_point && !normal && !inside) return fail(EZRT_ERR_INVALID, "one of hit_point, normal and inside is required");
    if (!known_integrator(integrator)) return fail(EZRT_ERR_INVALID, "unknown integrator %d", integrator);
    if (n == 0) return 0;
    const bool p5 = integrator >= EZRT_INTEGRATOR_P5_SOBOL; // the render's choice of the smooth-normal form, as ezrt_query_surface_device
    const size_t K = (size_t)n, v3 = K * 3 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{rays_od6, 2 * v3}, {tri_id, K * sizeof(int32_t)}, {t_hit, K * sizeof(float)}, {hit_point, v3}, {normal, v3},
                          {inside, K}}, K, st, [&](dim3 g, dim3 b) {
      const DevScene sc = s->dev();
      if (p5)
        hipLaunchKernelGGL(surface_at_kernel<true>, g, b, 0, st, sc.tri_geom, sc.tri_shade, (int32_t)s->n_tri, rays_od6, tri_id, t_hit,
                           (uint32_t)n, hit_point, normal, inside);
      else
        hipLaunchKernelGGL(surface_at_kernel<false>, g, b, 0, st, sc.tri_geom, sc.tri_shade, (int32_t)s->n_tri, rays_od6, tri_id, t_hit,
                           (uint32_t)n, hit_point, normal, inside);
    });
  });
}

// ---- closest-point queries on device memory (include/ezrt_closest_point.h): one kernel on `st`, no scratch; checked, launched and
// ordered against a refit by query_call.
int ezrt_query_closest_point_device(EzrtScene* s, const float* points3, const float* d_max, int n, int32_t* tri_id, float* point,
                                    float* dist, float* bary, void* stream) {
  return ezi::guarded("ezrt_query_closest_point_device", [&]() -> int {
    if (!s || !points3 || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{points3, N * 3 * sizeof(float)}, {d_max, N * sizeof(float)}, {tri_id, N * sizeof(int32_t)},
                          {point, N * 3 * sizeof(float)}, {dist, N * sizeof(float)}, {bary, N * 2 * sizeof(float)}}, N, st, [&](dim3, dim3) {
      ClosestPointArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.points = points3;
      a.d_max = d_max;
      a.n = (uint32_t)n;
      a.tri = tri_id;
      a.point = point;
      a.dist = dist;
      a.bary = bary;
      launch_routed(closest_point_kernel<true>, closest_point_kernel<false>, r, r.lds, N, st, a);
    });
  });
}

// ---- nearest-K queries on device memory (include/ezrt_nearest.h): one kernel each on `st`, no scratch (a point's sorted list is kept
// in its own output rows); checked, launched and ordered against a refit by query_call.  The route is chosen per call, by point_scene;
// n_within selects the counting instance, which cannot shrink its radius below d_max.
int ezrt_query_nearest_device(EzrtScene* s, const float* points3, const float* d_max, int n, int max_k, int32_t* tri_id, float* dist,
                              int32_t* n_within, void* stream) {
  return ezi::guarded("ezrt_query_nearest_device", [&]() -> int {
    if (!s || !points3 || !tri_id || !dist || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (max_k < 1 || max_k > EZRT_NEAREST_MAX) return fail(EZRT_ERR_INVALID, "max_k out of range [1,%d]", EZRT_NEAREST_MAX);
    if (n == 0) return 0;
    const size_t N = (size_t)n, K = (size_t)max_k;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{points3, N * 3 * sizeof(float)}, {d_max, N * sizeof(float)}, {tri_id, N * K * sizeof(int32_t)},
                          {dist, N * K * sizeof(float)}, {n_within, N * sizeof(int32_t)}}, N, st, [&](dim3, dim3) {
      NearestArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.points = points3;
      a.d_max = d_max;
      a.n = (uint32_t)n;
      a.K = max_k;
      a.div_k = make_fastdiv((uint32_t)max_k);
      a.tri = tri_id;
      a.dist = dist;
      a.n_within = n_within;
      if (n_within) launch_routed(nearest_kernel<true, true>, nearest_kernel<false, true>, r, r.lds, N, st, a);
      else launch_routed(nearest_kernel<true, false>, nearest_kernel<false, false>, r, r.lds, N, st, a);
    });
  });
}
int ezrt_closest_point_at_device(EzrtScene* s, const float* points3, const int32_t* tri_id, int n, float* point, float* dist, float* bary,
                                 void* stream) {
  return ezi::guarded("ezrt_closest_point_at_device", [&]() -> int {
    if (!s || !points3 || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!point && !dist && !bary) return fail(EZRT_ERR_INVALID, "one of point, dist and bary is required");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{points3, N * 3 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {point, N * 3 * sizeof(float)},
                          {dist, N * sizeof(float)}, {bary, N * 2 * sizeof(float)}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(closest_point_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, points3, tri_id, (uint32_t)n, point, dist,
                         bary);
    });
  });
}

// ---- inside and signed-distance queries on device memory (include/ezrt_inside.h): one kernel each on `st`, no scratch; checked,
// launched and ordered against a refit by query_call.  The route is chosen per call, by point_scene.
int ezrt_query_inside_device(EzrtScene* s, const float* points3, int n, int axis, uint8_t* inside, int32_t* crossings, void* stream) {
  return ezi::guarded("ezrt_query_inside_device", [&]() -> int {
    if (!s || !points3 || !inside || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (axis < 0 || axis > 5) return fail(EZRT_ERR_INVALID, "axis out of range [0,5]");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{points3, N * 3 * sizeof(float)}, {inside, N}, {crossings, N * sizeof(int32_t)}}, N, st, [&](dim3, dim3) {
      InsideArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.points = points3;
      a.n = (uint32_t)n;
      a.axis = axis;
      a.inside = inside;
      a.crossings = crossings;
      // this walk's entries are bare references, one row each: half of the column that decides the route
      launch_routed(inside_kernel<true>, inside_kernel<false>, r, r.lds / 2, N, st, a);
    });
  });
}
int ezrt_query_signed_distance_device(EzrtScene* s, const float* points3, const float* d_max, int n, int axis, int32_t* tri_id,
                                      float* point, float* sdist, float* bary, uint8_t* inside, void* stream) {
  return ezi::guarded("ezrt_query_signed_distance_device", [&]() -> int {
    if (!s || !points3 || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (axis < 0 || axis > 5) return fail(EZRT_ERR_INVALID, "axis out of range [0,5]");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{points3, N * 3 * sizeof(float)}, {d_max, N * sizeof(float)}, {tri_id, N * sizeof(int32_t)},
                          {point, N * 3 * sizeof(float)}, {sdist, N * sizeof(float)}, {bary, N * 2 * sizeof(float)}, {inside, N}}, N, st,
                      [&](dim3, dim3) {
      SignedDistanceArgs a;
      const PointRoute r = point_scene(s, a.cp.sc);
      a.cp.points = points3;
      a.cp.d_max = d_max;
      a.cp.n = (uint32_t)n;
      a.cp.tri = tri_id;
      a.cp.point = point;
      a.cp.dist = sdist;
      a.cp.bary = bary;
      a.axis = axis;
      a.inside = inside;
      // the crossing walk runs first, on the same column
      launch_routed(signed_distance_kernel<true>, signed_distance_kernel<false>, r, r.lds, N, st, a);
    });
  });
}

// ---- box-overlap queries on device memory (include/ezrt_box_overlap.h): one kernel each on `st`, no scratch (a box's list is kept in
// its own output row); checked, launched and ordered against a refit by query_call.  The route is chosen per call, by point_scene.
int ezrt_query_box_overlap_device(EzrtScene* s, const float* box_lo3, const float* box_hi3, int n, int max_k, int32_t* tri_id,
                                  int32_t* n_overlap, void* stream) {
  const size_t b3 = (size_t)n * 3 * sizeof(float);
  // this walk's entries are bare references, one row each: half of the column that decides the route
  return overlap_rows_call<BoxOverlapArgs>("ezrt_query_box_overlap_device", s, box_lo3 && box_hi3, {box_lo3, b3}, {box_hi3, b3}, n, max_k,
                                           EZRT_BOX_OVERLAP_MAX, tri_id, n_overlap, stream, box_overlap_kernel<true>, box_overlap_kernel<false>, 2,
                                           [&](BoxOverlapArgs& a) { a.lo = box_lo3, a.hi = box_hi3; });
}
int ezrt_box_overlap_at_device(EzrtScene* s, const float* box_lo3, const float* box_hi3, const int32_t* tri_id, int n, uint8_t* overlaps,
                               void* stream) {
  return ezi::guarded("ezrt_box_overlap_at_device", [&]() -> int {
    if (!s || !box_lo3 || !box_hi3 || !tri_id || !overlaps || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{box_lo3, N * 3 * sizeof(float)}, {box_hi3, N * 3 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {overlaps, N}}, N,
                      st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(box_overlap_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, box_lo3, box_hi3, tri_id, (uint32_t)n, overlaps);
    });
  });
}

// ---- oriented-box queries on device memory (include/ezrt_obb_overlap.h): one kernel each on `st`, no scratch (a box's list is kept in
// its own output row); checked, launched and ordered against a refit by query_call.  The route is chosen per call, by point_scene.
int ezrt_query_obb_overlap_device(EzrtScene* s, const float* centre3, const float* axes9, int n, int max_k, int32_t* tri_id,
                                  int32_t* n_overlap, void* stream) {
  const size_t b3 = (size_t)n * 3 * sizeof(float);
  // slot_walk's entries are bare references, one row each: half of the column that decides the route (stack_need_cp + 1 rows)
  return overlap_rows_call<ObbOverlapArgs>("ezrt_query_obb_overlap_device", s, centre3 && axes9, {centre3, b3}, {axes9, 3 * b3}, n, max_k,
                                           EZRT_OBB_OVERLAP_MAX, tri_id, n_overlap, stream, obb_overlap_kernel<true>, obb_overlap_kernel<false>, 2,
                                           [&](ObbOverlapArgs& a) { a.centre = centre3, a.axes = axes9; });
}
int ezrt_obb_overlap_at_device(EzrtScene* s, const float* centre3, const float* axes9, const int32_t* tri_id, int n, uint8_t* overlaps,
                               void* stream) {
  return ezi::guarded("ezrt_obb_overlap_at_device", [&]() -> int {
    if (!s || !centre3 || !axes9 || !tri_id || !overlaps || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{centre3, N * 3 * sizeof(float)}, {axes9, N * 9 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {overlaps, N}}, N,
                      st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(obb_overlap_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, centre3, axes9, tri_id, (uint32_t)n, overlaps);
    });
  });
}

// ---- winding-number queries on device memory (include/ezrt_winding.h): no scratch (`fixed` is the caller's accumulator); checked,
// launched and ordered against a refit by query_call.  No tree is read, so there is no route.
//
// The slices of a call with chunks == 0 -- a pure function of n and n_tri.  A workgroup is one wave of WN_BLOCK points; an MI355X
// has 256 CUs of 4 SIMDs, and WN_FILL = 8192 waves is eight per SIMD, what the kernel's registers allow: the pair function is a long
// dependent chain of fp64 operations (three square roots, two divisions), and the measured rate still rises from 2 to 8 waves per SIMD
// (DESIGN.md has the figures).  Where the points alone give that many, one slice (no zeroing, no atomics, no finishing kernel);
// otherwise enough slices to reach it, but none shorter than WN_MIN_SLICE triangles, below which the per-workgroup cost (the point,
// the atomic) is no longer small beside the slice.
constexpr int WN_FILL = 8192, WN_MIN_SLICE = 256, WN_MAX_SLICES = 65535; // (65535: the y extent of a grid)
int ezrt_winding_chunks(int n, int n_tri) {
  if (n <= 0 || n_tri <= 0) return 1;
  const long long blocks = ((long long)n + WN_BLOCK - 1) / WN_BLOCK;
  if (blocks >= WN_FILL) return 1;
  const long long want = (WN_FILL + blocks - 1) / blocks, most = n_tri / WN_MIN_SLICE;
  const long long c = want < most ? want : most;
  return (int)(c < 1 ? 1 : c);
}
int ezrt_query_winding_device(EzrtScene* s, const float* points3, int n, int chunks, int64_t* fixed, float* winding, void* stream) {
  return ezi::guarded("ezrt_query_winding_device", [&]() -> int {
    if (!s || !points3 || !fixed || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (chunks < 0) return fail(EZRT_ERR_INVALID, "chunks < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    static const bool tile = [] { // the triangles through an LDS tile (the default: the faster) or by scalar loads (kept for measuring)
      const char* e = getenv("EZRT_WINDING_SCALAR");
      return !(e && e[0] == '1');
    }();
    return query_call(s, {{points3, N * 3 * sizeof(float)}, {fixed, N * sizeof(int64_t)}, {winding, N * sizeof(float)}}, N, st,
                      [&](dim3, dim3) -> int {
      const int n_tri = (int)s->n_tri;
      int c = chunks == 0 ? ezrt_winding_chunks(n, n_tri) : chunks;
      if (c > n_tri) c = n_tri;
      if (c > WN_MAX_SLICES) c = WN_MAX_SLICES;
      if (c < 1) c = 1;
      WindingArgs a;
      a.tri_geom = s->tri_geom.p;
      a.n_tri = n_tri;
      a.per_slice = (n_tri + c - 1) / c;
      if (a.per_slice > 0) c = (n_tri + a.per_slice - 1) / a.per_slice; // no empty slice
      a.points = points3;
      a.n = (uint32_t)n;
      a.fixed = (long long*)fixed;
      a.winding = winding;
      const dim3 g((unsigned)((N + WN_BLOCK - 1) / WN_BLOCK), (unsigned)c), b(WN_BLOCK);
      if (c == 1) {
        if (tile) hipLaunchKernelGGL((winding_kernel<false, true>), g, b, 0, st, a);
        else hipLaunchKernelGGL((winding_kernel<false, false>), g, b, 0, st, a);
        return 0;
      }
      HIP_TRY(hipMemsetAsync(fixed, 0, N * sizeof(int64_t), st));
      if (tile) hipLaunchKernelGGL((winding_kernel<true, true>), g, b, 0, st, a);
      else hipLaunchKernelGGL((winding_kernel<true, false>), g, b, 0, st, a);
      if (winding)
        hipLaunchKernelGGL(winding_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const long long*)fixed, (uint32_t)n,
                           winding);
      return 0;
    });
  });
}
int ezrt_winding_at_device(EzrtScene* s, const float* points3, const int32_t* tri_id, int n, int64_t* fixed, float* winding, void* stream) {
  return ezi::guarded("ezrt_winding_at_device", [&]() -> int {
    if (!s || !points3 || !tri_id || !fixed || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{points3, N * 3 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {fixed, N * sizeof(int64_t)},
                          {winding, N * sizeof(float)}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(winding_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, points3, tri_id, (uint32_t)n, (long long*)fixed,
                         winding);
    });
  });
}

// ---- plane queries on device memory (include/ezrt_plane.h): no scratch (`part` and `offsets` are the caller's); checked, launched and
// ordered against a refit by query_call.  No tree is read, so there is no route.
//
// The slices.  A workgroup is one wave for a slice of the triangle range and a tile of PL_TILE planes.  slices == 0: where the tiles
// alone give PL_FILL = 16384 waves one slice; otherwise enough slices to reach that, but none below PL_MIN_SLICE = 256 triangles,
// where the tile's conversion and the counters' store are no longer small beside the slice.  16384 is two waves for each of the
// 8 x 1024 wave slots of an MI355X that the sweep's 40 VGPRs allow.  Measured (profiles/r24/plane_rates.txt): the COUNT
// pass of 10 000 planes gets faster with more waves well past the slots (4 239 waves 690 to 730 Gpairs/s, 10 048 840 to 930, 16 485
// 920 to 1 020, 40 192 1 050 to 1 100: the sides of one plane are three short dependent chains of fp64 operations, and short
// workgroups leave a shorter tail), but the FILL pass pays for every slice before its own -- the sum of part[i][0 .. j) per plane of
// the tile -- and 40960 waves, tried, lost 15 % on the fill of 10 000 random planes against 64 slices.  16384 is within the
// run-to-run spread of the best of 1, 8 and 64 forced slices in both passes wherever a call takes longer than a launch.
constexpr int PL_FILL = 16384, PL_MIN_SLICE = 256, PL_MAX_SLICES = 4096;
int ezrt_plane_slices(int n, int n_tri, int slices) {
  const long long rounds = n_tri > 0 ? ((long long)n_tri + PL_BLOCK - 1) / PL_BLOCK : 1;
  long long c = 1;
  if (slices >= 1) {
    c = slices;
  } else if (n > 0 && n_tri > 0) {
    const long long tiles = ((long long)n + PL_TILE - 1) / PL_TILE;
    const long long want = tiles >= PL_FILL ? 1 : (PL_FILL + tiles - 1) / tiles, most = n_tri / PL_MIN_SLICE;
    c = want < most ? want : most;
  }
  if (c > rounds) c = rounds;
  if (c > PL_MAX_SLICES) c = PL_MAX_SLICES;
  return (int)(c < 1 ? 1 : c);
}
// L of the header: the triangles of a slice, a multiple of 64
static int32_t plane_per_slice(int n_tri, int S) {
  const long long per = ((long long)(n_tri > 0 ? n_tri : 0) + S - 1) / S;
  const long long L = (per + PL_BLOCK - 1) / PL_BLOCK * PL_BLOCK;
  return (int32_t)(L < PL_BLOCK ? PL_BLOCK : L);
}
int ezrt_query_plane_count_device(EzrtScene* s, const float* planes4, int n, int slices, int32_t* part, int32_t* n_cross, int64_t* offsets,
                                  void* stream) {
  return ezi::guarded("ezrt_query_plane_count_device", [&]() -> int {
    if (!s || !planes4 || !part || !n_cross || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (slices < 0) return fail(EZRT_ERR_INVALID, "slices < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    const int n_tri = (int)s->n_tri, S = ezrt_plane_slices(n, n_tri, slices);
    return query_call(s, {{planes4, N * 4 * sizeof(float)}, {part, N * (size_t)S * sizeof(int32_t)}, {n_cross, N * sizeof(int32_t)},
                          {offsets, (N + 1) * sizeof(int64_t)}}, N, st, [&](dim3, dim3) {
      PlaneArgs a{};
      a.tri_geom = s->tri_geom.p;
      a.n_tri = n_tri;
      a.per_slice = plane_per_slice(n_tri, S);
      a.slices = S;
      a.planes = planes4;
      a.n = (uint32_t)n;
      a.part = part;
      hipLaunchKernelGGL((plane_kernel<false>), dim3((unsigned)((N + PL_TILE - 1) / PL_TILE), (unsigned)S), dim3(PL_BLOCK), 0, st, a);
      hipLaunchKernelGGL(plane_total_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const int32_t*)part, (int32_t)S, (uint32_t)n, n_cross);
      if (offsets) hipLaunchKernelGGL(plane_offsets_kernel, dim3(1), dim3(PL_SCAN), 0, st, (const int32_t*)n_cross, (uint32_t)n, (long long*)offsets);
    });
  });
}
int ezrt_query_plane_section_device(EzrtScene* s, const float* planes4, int n, int slices, const int32_t* part, const int64_t* offsets,
                                    int64_t capacity, int32_t* tri_id, float* seg, void* stream) {
  return ezi::guarded("ezrt_query_plane_section_device", [&]() -> int {
    if (!s || !planes4 || !part || !offsets || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (slices < 0) return fail(EZRT_ERR_INVALID, "slices < 0");
    if (capacity < 0) return fail(EZRT_ERR_INVALID, "capacity < 0");
    if (!tri_id && capacity > 0) return fail(EZRT_ERR_INVALID, "NULL tri_id with capacity > 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, cap = (size_t)capacity;
    hipStream_t st = (hipStream_t)stream;
    const int n_tri = (int)s->n_tri, S = ezrt_plane_slices(n, n_tri, slices);
    return query_call(s, {{planes4, N * 4 * sizeof(float)}, {part, N * (size_t)S * sizeof(int32_t)}, {offsets, (N + 1) * sizeof(int64_t)},
                          {tri_id, cap * sizeof(int32_t)}, {seg, cap * 6 * sizeof(float)}}, N, st, [&](dim3, dim3) {
      if (capacity == 0) return; // no row can be written
      PlaneArgs a{};
      a.tri_geom = s->tri_geom.p;
      a.n_tri = n_tri;
      a.per_slice = plane_per_slice(n_tri, S);
      a.slices = S;
      a.planes = planes4;
      a.n = (uint32_t)n;
      a.part = const_cast<int32_t*>(part);
      a.offsets = (const long long*)offsets;
      a.capacity = (long long)capacity;
      a.tri_id = tri_id;
      a.seg = seg;
      hipLaunchKernelGGL((plane_kernel<true>), dim3((unsigned)((N + PL_TILE - 1) / PL_TILE), (unsigned)S), dim3(PL_BLOCK), 0, st, a);
    });
  });
}
int ezrt_plane_section_at_device(EzrtScene* s, const float* planes4, const int32_t* tri_id, int n, uint8_t* crosses, int8_t* side, float* seg,
                                 void* stream) {
  return ezi::guarded("ezrt_plane_section_at_device", [&]() -> int {
    if (!s || !planes4 || !tri_id || !crosses || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{planes4, N * 4 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {crosses, N}, {side, N * 3},
                          {seg, N * 6 * sizeof(float)}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(plane_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, planes4, tri_id, (uint32_t)n, crosses, side, seg);
    });
  });
}

// ---- plane loops on device memory (include/ezrt_plane_loops.h): six launches on `st` -- the two routes of loops_chain_kernel, the
// planes' scan, the lengths, the loops' scan, the scatter -- over the caller's `work`; checked, launched and ordered against a refit
// by query_call.  `work` is lofs (capacity + 1 int64) and then 14 x capacity ints: nxt prd hd ps hl lo li ro, and rep oh ih twice as long.
size_t ezrt_plane_loops_work_bytes(int64_t capacity) {
  const size_t cap = capacity > 0 ? (size_t)capacity : 0;
  return cap * (sizeof(int64_t) + 14 * sizeof(int32_t)) + sizeof(int64_t);
}
void ezrt_plane_loops_limits(int* tile_rows_max) {
  if (tile_rows_max) *tile_rows_max = LP_TILE_MAX;
}
int ezrt_plane_loops_device(EzrtScene* s, const int64_t* offsets, int n, const float* seg, int64_t capacity, int tile_rows, int64_t* next,
                            int64_t* order, int64_t* plane_loops, int64_t loop_capacity, int64_t* loop_offsets, uint8_t* closed, void* work,
                            size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_plane_loops_device", [&]() -> int {
    if (!s || !offsets || !plane_loops || !loop_offsets || !work || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (capacity < 0 || loop_capacity < 0) return fail(EZRT_ERR_INVALID, "capacity < 0 or loop_capacity < 0");
    if (tile_rows < 0) return fail(EZRT_ERR_INVALID, "tile_rows < 0");
    // (the byte counts below must not wrap)
    if (capacity > (int64_t)(PTRDIFF_MAX / 64) || loop_capacity > (int64_t)(PTRDIFF_MAX / 16))
      return fail(EZRT_ERR_INVALID, "capacity exceeds what an array can hold");
    if ((!seg || !order) && capacity > 0) return fail(EZRT_ERR_INVALID, "NULL seg or order with capacity > 0");
    if (work_bytes < ezrt_plane_loops_work_bytes(capacity)) return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_plane_loops_work_bytes(capacity)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n == 0) return 0;
    const size_t N = (size_t)n, cap = (size_t)capacity, lcap = (size_t)loop_capacity;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{offsets, (N + 1) * sizeof(int64_t)}, {seg, cap * 6 * sizeof(float)}, {next, cap * sizeof(int64_t)},
                          {order, cap * sizeof(int64_t)}, {plane_loops, (N + 1) * sizeof(int64_t)}, {loop_offsets, (lcap + 1) * sizeof(int64_t)},
                          {closed, lcap}, {work, ezrt_plane_loops_work_bytes(capacity)}}, N, st, [&](dim3, dim3) {
      LoopsArgs a{};
      a.offsets = (const long long*)offsets;
      a.seg = (const uint32_t*)seg;
      a.capacity = (long long)capacity;
      a.n_tri = (int32_t)s->n_tri;
      a.n = (uint32_t)n;
      a.tile = (uint32_t)(tile_rows == 0 || tile_rows > LP_TILE_MAX ? LP_TILE_MAX : tile_rows);
      a.lofs = (long long*)work;
      int32_t* w = (int32_t*)(a.lofs + cap + 1);
      a.nxt = w, a.prd = w + cap, a.hd = w + 2 * cap, a.ps = w + 3 * cap, a.hl = w + 4 * cap, a.lo = w + 5 * cap, a.li = w + 6 * cap;
      a.ro = w + 7 * cap, a.rep = w + 8 * cap, a.oh = w + 10 * cap, a.ih = w + 12 * cap;
      a.next = (long long*)next, a.order = (long long*)order, a.plane_loops = (long long*)plane_loops;
      a.loop_offsets = (long long*)loop_offsets, a.loop_capacity = (long long)loop_capacity, a.closed = closed;
      const dim3 g((unsigned)n);
      hipLaunchKernelGGL((loops_chain_kernel<true>), g, dim3(LP_LDS_BLOCK), 0, st, a);
      hipLaunchKernelGGL((loops_chain_kernel<false>), g, dim3(LP_GLB_BLOCK), 0, st, a);
      scan_small(st, a.plane_loops, nullptr, (long long)n);
      hipLaunchKernelGGL(loops_length_kernel, g, dim3(LP_BLOCK), 0, st, a);
      scan_small(st, a.lofs, (const long long*)(a.plane_loops + n), (long long)capacity);
      hipLaunchKernelGGL(loops_scatter_kernel, g, dim3(LP_BLOCK), 0, st, a);
    });
  });
}

// ---- triangle-overlap queries on device memory (include/ezrt_tri_overlap.h): one kernel each on `st`, no scratch (a query's list is
// kept in its own output row); checked, launched and ordered against a refit by query_call.  The route is chosen per call, by
// point_scene.
int ezrt_query_tri_overlap_device(EzrtScene* s, const float* tris9, int n, int max_k, int32_t* tri_id, int32_t* n_overlap, void* stream) {
  // this walk's entries are bare references, one row each: half of the column that decides the route
  return overlap_rows_call<TriOverlapArgs>("ezrt_query_tri_overlap_device", s, tris9 != nullptr, {tris9, (size_t)n * 9 * sizeof(float)}, {nullptr, 0},
                                           n, max_k, EZRT_TRI_OVERLAP_MAX, tri_id, n_overlap, stream, tri_overlap_kernel<true>,
                                           tri_overlap_kernel<false>, 2, [&](TriOverlapArgs& a) { a.tris = tris9; });
}
int ezrt_tri_overlap_at_device(EzrtScene* s, const float* tris9, const int32_t* tri_id, int n, uint8_t* overlaps, void* stream) {
  return ezi::guarded("ezrt_tri_overlap_at_device", [&]() -> int {
    if (!s || !tris9 || !tri_id || !overlaps || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tris9, N * 9 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {overlaps, N}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(tri_overlap_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, tris9, tri_id, (uint32_t)n, overlaps);
    });
  });
}

// ---- self-overlap queries on device memory (include/ezrt_self_overlap.h): one kernel each on `st`, no scratch (a query's list is
// kept in its own output row); checked, launched and ordered against a refit by query_call.  The route is chosen per call, by
// point_scene.
int ezrt_query_self_overlap_device(EzrtScene* s, const int32_t* ids, int n, int max_k, int32_t* tri_id, int32_t* n_overlap, void* stream) {
  // (between the shared call's first and second test, which a scene and an n >= 0 pass)
  if (s && !ids && n > 0 && (size_t)n > (size_t)s->n_tri)
    return fail(EZRT_ERR_INVALID, "n exceeds the scene's %d triangles (ids is NULL)", (int)s->n_tri);
  // this walk's entries are bare references, one row each: half of the column that decides the route
  return overlap_rows_call<SelfOverlapArgs>("ezrt_query_self_overlap_device", s, true, {ids, (size_t)n * sizeof(int32_t)}, {nullptr, 0}, n, max_k,
                                            EZRT_SELF_OVERLAP_MAX, tri_id, n_overlap, stream, self_overlap_kernel<true>,
                                            self_overlap_kernel<false>, 2, [&](SelfOverlapArgs& a) { a.ids = ids; });
}
int ezrt_self_overlap_at_device(EzrtScene* s, const int32_t* tri_a, const int32_t* tri_b, int n, uint8_t* crosses, void* stream) {
  return ezi::guarded("ezrt_self_overlap_at_device", [&]() -> int {
    if (!s || !tri_a || !tri_b || !crosses || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri_a, N * sizeof(int32_t)}, {tri_b, N * sizeof(int32_t)}, {crosses, N}}, N, st, [&](dim3 g, dim3 b) {
      PointScene sc;
      point_scene(s, sc);
      hipLaunchKernelGGL(self_overlap_at_kernel, g, b, 0, st, sc, tri_a, tri_b, (uint32_t)n, crosses);
    });
  });
}

// ---- triangle-distance queries on device memory (include/ezrt_tri_distance.h): one kernel each on `st`, no scratch; checked,
// launched and ordered against a refit by query_call.  The route is chosen per call, by point_scene.
int ezrt_query_tri_distance_device(EzrtScene* s, const float* tris9, const float* d_max, int n, int32_t* tri_id, float* dist,
                                   float* point_query, float* point_scene, uint8_t* crosses, void* stream) {
  return ezi::guarded("ezrt_query_tri_distance_device", [&]() -> int {
    if (!s || !tris9 || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tris9, N * 9 * sizeof(float)}, {d_max, N * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {dist, N * sizeof(float)},
                          {point_query, N * 3 * sizeof(float)}, {point_scene, N * 3 * sizeof(float)}, {crosses, N}}, N, st, [&](dim3, dim3) {
      TriDistanceArgs a;
      const PointRoute r = ::point_scene(s, a.sc); // (the function: the parameter of that name is the output)
      a.tris = tris9;
      a.d_max = d_max;
      a.n = (uint32_t)n;
      a.tri = tri_id;
      a.dist = dist;
      a.point_query = point_query;
      a.point_scene = point_scene;
      a.crosses = crosses;
      launch_routed(tri_distance_kernel<true>, tri_distance_kernel<false>, r, r.lds, N, st, a);
    });
  });
}
int ezrt_tri_distance_at_device(EzrtScene* s, const float* tris9, const int32_t* tri_id, int n, float* dist, float* point_query,
                                float* point_scene, uint8_t* crosses, void* stream) {
  return ezi::guarded("ezrt_tri_distance_at_device", [&]() -> int {
    if (!s || !tris9 || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!dist && !point_query && !point_scene && !crosses)
      return fail(EZRT_ERR_INVALID, "one of dist, point_query, point_scene and crosses is required");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tris9, N * 9 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {dist, N * sizeof(float)},
                          {point_query, N * 3 * sizeof(float)}, {point_scene, N * 3 * sizeof(float)}, {crosses, N}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(tri_distance_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, tris9, tri_id, (uint32_t)n, dist, point_query,
                         point_scene, crosses);
    });
  });
}

// ---- sphere-cast queries on device memory (include/ezrt_sphere_cast.h): one kernel each on `st`, no scratch; checked, launched and
// ordered against a refit by query_call.  The route is chosen per call, by point_scene.
int ezrt_query_sphere_cast_device(EzrtScene* s, const float* rays6, const float* radius, const float* t_max, int n, int32_t* tri_id, float* t,
                                  float* point, uint8_t* touching, void* stream) {
  return ezi::guarded("ezrt_query_sphere_cast_device", [&]() -> int {
    if (!s || !rays6 || !radius || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{rays6, N * 6 * sizeof(float)}, {radius, N * sizeof(float)}, {t_max, N * sizeof(float)}, {tri_id, N * sizeof(int32_t)},
                          {t, N * sizeof(float)}, {point, N * 3 * sizeof(float)}, {touching, N}}, N, st, [&](dim3, dim3) {
      SphereCastArgs a;
      const PointRoute r = point_scene(s, a.cp.sc);
      a.cp.points = nullptr;
      a.cp.d_max = radius;
      a.cp.n = (uint32_t)n;
      a.cp.tri = tri_id;
      a.cp.point = point;
      a.cp.dist = nullptr;
      a.cp.bary = nullptr;
      a.rays = rays6;
      a.t_max = t_max;
      a.t = t;
      a.touching = touching;
      launch_routed(sphere_cast_kernel<true>, sphere_cast_kernel<false>, r, r.lds, N, st, a);
    });
  });
}
int ezrt_sphere_cast_at_device(EzrtScene* s, const float* rays6, const float* radius, const int32_t* tri_id, int n, float* t, float* point,
                               uint8_t* touching, void* stream) {
  return ezi::guarded("ezrt_sphere_cast_at_device", [&]() -> int {
    if (!s || !rays6 || !radius || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!t && !point && !touching) return fail(EZRT_ERR_INVALID, "one of t, point and touching is required");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{rays6, N * 6 * sizeof(float)}, {radius, N * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {t, N * sizeof(float)},
                          {point, N * 3 * sizeof(float)}, {touching, N}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(sphere_cast_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, rays6, radius, tri_id, (uint32_t)n, t, point,
                         touching);
    });
  });
}

// ---- segment queries on device memory (include/ezrt_segment.h): one kernel each on `st`, no scratch (a capsule's list is kept in its
// own output row); checked, launched and ordered against a refit by query_call.  The route is chosen per call, by point_scene.
int ezrt_query_segment_distance_device(EzrtScene* s, const float* segs6, const float* d_max, int n, int32_t* tri_id, float* dist,
                                       float* point_query, float* point_scene, uint8_t* crosses, void* stream) {
  return ezi::guarded("ezrt_query_segment_distance_device", [&]() -> int {
    if (!s || !segs6 || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{segs6, N * 6 * sizeof(float)}, {d_max, N * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {dist, N * sizeof(float)},
                          {point_query, N * 3 * sizeof(float)}, {point_scene, N * 3 * sizeof(float)}, {crosses, N}}, N, st, [&](dim3, dim3) {
      SegmentDistanceArgs a;
      const PointRoute r = ::point_scene(s, a.sc); // (the function: the parameter of that name is the output)
      a.segs = segs6;
      a.d_max = d_max;
      a.n = (uint32_t)n;
      a.tri = tri_id;
      a.dist = dist;
      a.point_query = point_query;
      a.point_scene = point_scene;
      a.crosses = crosses;
      launch_routed(segment_distance_kernel<true>, segment_distance_kernel<false>, r, r.lds, N, st, a);
    });
  });
}
int ezrt_segment_distance_at_device(EzrtScene* s, const float* segs6, const int32_t* tri_id, int n, float* dist, float* point_query,
                                    float* point_scene, uint8_t* crosses, void* stream) {
  return ezi::guarded("ezrt_segment_distance_at_device", [&]() -> int {
    if (!s || !segs6 || !tri_id || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!dist && !point_query && !point_scene && !crosses)
      return fail(EZRT_ERR_INVALID, "one of dist, point_query, point_scene and crosses is required");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{segs6, N * 6 * sizeof(float)}, {tri_id, N * sizeof(int32_t)}, {dist, N * sizeof(float)},
                          {point_query, N * 3 * sizeof(float)}, {point_scene, N * 3 * sizeof(float)}, {crosses, N}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(segment_distance_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, segs6, tri_id, (uint32_t)n, dist,
                         point_query, point_scene, crosses);
    });
  });
}
int ezrt_query_capsule_overlap_device(EzrtScene* s, const float* segs6, const float* radius, int n, int max_k, int32_t* tri_id,
                                      int32_t* n_overlap, void* stream) {
  // this walk is point_walk: {lb, ref} entries, the whole column
  return overlap_rows_call<CapsuleOverlapArgs>("ezrt_query_capsule_overlap_device", s, segs6 && radius, {segs6, (size_t)n * 6 * sizeof(float)},
                                               {radius, (size_t)n * sizeof(float)}, n, max_k, EZRT_CAPSULE_OVERLAP_MAX, tri_id, n_overlap, stream,
                                               capsule_overlap_kernel<true>, capsule_overlap_kernel<false>, 1,
                                               [&](CapsuleOverlapArgs& a) { a.segs = segs6, a.radius = radius; });
}

// ---- overlap lists on device memory (include/ezrt_overlap_list.h): count (the max_k == 0 calls above), offsets, fill.
void ezrt_overlap_list_limits(int* insert_max, int* tile_max) {
  if (insert_max) *insert_max = OL_INSERT_MAX;
  if (tile_max) *tile_max = OL_TILE_MAX;
}
int ezrt_overlap_offsets_device(EzrtScene* s, const int32_t* n_overlap, int n, int64_t* offsets, void* stream) {
  return ezi::guarded("ezrt_overlap_offsets_device", [&]() -> int {
    if (!s || !n_overlap || !offsets || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{n_overlap, N * sizeof(int32_t)}, {offsets, (N + 1) * sizeof(int64_t)}}, N, st, [&](dim3, dim3) {
      hipLaunchKernelGGL(plane_offsets_kernel, dim3(1), dim3(PL_SCAN), 0, st, n_overlap, (uint32_t)n, (long long*)offsets);
    });
  });
}
int ezrt_query_box_overlap_list_device(EzrtScene* s, const float* box_lo3, const float* box_hi3, int n, const int64_t* offsets, int64_t capacity,
                                       int32_t* tri_id, int32_t* n_found, void* stream) {
  const size_t b3 = (size_t)n * 3 * sizeof(float);
  return overlap_list_call<BoxOverlapListArgs>("ezrt_query_box_overlap_list_device", s, box_lo3 && box_hi3, {box_lo3, b3}, {box_hi3, b3}, n, offsets,
                                               capacity, tri_id, n_found, stream, box_overlap_list_kernel<true>, box_overlap_list_kernel<false>, 2,
                                               [&](BoxOverlapListArgs& a) { a.lo = box_lo3, a.hi = box_hi3; });
}
int ezrt_query_obb_overlap_list_device(EzrtScene* s, const float* centre3, const float* axes9, int n, const int64_t* offsets, int64_t capacity,
                                       int32_t* tri_id, int32_t* n_found, void* stream) {
  const size_t b3 = (size_t)n * 3 * sizeof(float);
  return overlap_list_call<ObbOverlapListArgs>("ezrt_query_obb_overlap_list_device", s, centre3 && axes9, {centre3, b3}, {axes9, 3 * b3}, n, offsets,
                                               capacity, tri_id, n_found, stream, obb_overlap_list_kernel<true>, obb_overlap_list_kernel<false>, 2,
                                               [&](ObbOverlapListArgs& a) { a.centre = centre3, a.axes = axes9; });
}
int ezrt_query_tri_overlap_list_device(EzrtScene* s, const float* tris9, int n, const int64_t* offsets, int64_t capacity, int32_t* tri_id,
                                       int32_t* n_found, void* stream) {
  return overlap_list_call<TriOverlapListArgs>("ezrt_query_tri_overlap_list_device", s, tris9 != nullptr, {tris9, (size_t)n * 9 * sizeof(float)},
                                               {nullptr, 0}, n, offsets, capacity, tri_id, n_found, stream, tri_overlap_list_kernel<true>,
                                               tri_overlap_list_kernel<false>, 2, [&](TriOverlapListArgs& a) { a.tris = tris9; });
}
int ezrt_query_self_overlap_list_device(EzrtScene* s, const int32_t* ids, int n, const int64_t* offsets, int64_t capacity, int32_t* tri_id,
                                        int32_t* n_found, void* stream) {
  if (s && !ids && n > 0 && (size_t)n > (size_t)s->n_tri)
    return fail(EZRT_ERR_INVALID, "n exceeds the scene's %d triangles (ids is NULL)", (int)s->n_tri);
  return overlap_list_call<SelfOverlapListArgs>("ezrt_query_self_overlap_list_device", s, true, {ids, (size_t)n * sizeof(int32_t)}, {nullptr, 0}, n,
                                                offsets, capacity, tri_id, n_found, stream, self_overlap_list_kernel<true>,
                                                self_overlap_list_kernel<false>, 2, [&](SelfOverlapListArgs& a) { a.ids = ids; });
}
int ezrt_query_capsule_overlap_list_device(EzrtScene* s, const float* segs6, const float* radius, int n, const int64_t* offsets, int64_t capacity,
                                           int32_t* tri_id, int32_t* n_found, void* stream) {
  // this walk is point_walk: {lb, ref} entries, the whole column
  return overlap_list_call<CapsuleOverlapListArgs>("ezrt_query_capsule_overlap_list_device", s, segs6 && radius,
                                                   {segs6, (size_t)n * 6 * sizeof(float)}, {radius, (size_t)n * sizeof(float)}, n, offsets, capacity,
                                                   tri_id, n_found, stream, capsule_overlap_list_kernel<true>, capsule_overlap_list_kernel<false>, 1,
                                                   [&](CapsuleOverlapListArgs& a) { a.segs = segs6, a.radius = radius; });
}

} // extern "C"
