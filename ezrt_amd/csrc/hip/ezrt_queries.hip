// ezrt_queries.hip -- the device queries that are ONE kernel on the caller's stream and need no scratch: shading queries
// (include/ezrt_shade.h), path queries (include/ezrt_path.h), all-hits queries and surface_at (include/ezrt_multihit.h), closest-point,
// nearest-K, inside / signed-distance, box-overlap, triangle-overlap, self-overlap, triangle-distance, sphere-cast, segment,
// oriented-box, winding-number, plane, plane-loop and overlap-list queries (include/ezrt_closest_point.h, ezrt_nearest.h, ezrt_inside.h, ezrt_box_overlap.h,
// ezrt_tri_overlap.h, ezrt_self_overlap.h, ezrt_tri_distance.h, ezrt_sphere_cast.h, ezrt_segment.h, ezrt_obb_overlap.h, ezrt_winding.h,
// ezrt_plane.h, ezrt_plane_loops.h, ezrt_overlap_list.h; the mesh topology of include/ezrt_topology.h, whose kernels are in
// ezrt_topology_kernels.h, and the vertex weld and smooth normals of include/ezrt_vertices.h, whose kernels are in
// ezrt_vertex_kernels.h, the mesh orientation of include/ezrt_orient.h, whose kernels are in ezrt_orient_kernels.h, and the boundary
// loops and caps of include/ezrt_boundary.h, whose kernels are in ezrt_boundary_kernels.h, the plane clipping of include/ezrt_clip.h,
// whose kernels are in ezrt_clip_kernels.h, the subdivision of include/ezrt_subdivide.h, whose kernels are in ezrt_subdiv_kernels.h, and the decimation of
// include/ezrt_decimate.h, whose kernels are in ezrt_decimate_kernels.h; the sliced winding call is a memset, a kernel and a finishing kernel on the caller's stream, the plane count a sweep
// and two small kernels, an overlap list's fill a routed kernel and, on the walk route, a sort).  A translation unit of its own: none
// of its kernels is compiled together with the render pipeline's (ezrt_launch.hip), so a change here cannot move a register of a timed
// kernel.  The ray queries that run the pipeline's trace kernels (ezrt_query_closest_device, ezrt_query_occluded_device,
// ezrt_query_surface_device) are in ezrt_launch.hip.  DESIGN.md 5.
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
#include "ezrt_topology.h"
#include "ezrt_vertices.h"
#include "ezrt_orient.h"
#include "ezrt_boundary.h"
#include "ezrt_clip.h"
#include "ezrt_subdivide.h"
#include "ezrt_decimate.h"
#include "ezrt_query_kernels.h"
#include "ezrt_point_queries.h"
#include "ezrt_topology_kernels.h"
#include "ezrt_vertex_kernels.h"
#include "ezrt_orient_kernels.h"
#include "ezrt_boundary_kernels.h"
#include "ezrt_clip_kernels.h"
#include "ezrt_subdiv_kernels.h"
#include "ezrt_decimate_kernels.h"

using ezi::known_integrator;
using ezi::stack_lds_bytes;

// Every call here goes through ezi::device_call: buffers checked against the scene's device, launch(grid, block), then the event of
// the scratch-free queries (QueryScratch::ev_shade_end), which a later refit waits for.
template <class Launch>
static int query_call(EzrtScene* s, std::initializer_list<ezi::DeviceBuf> bufs, size_t n, hipStream_t st, Launch&& launch) {
  return ezi::device_call(s, s->tri_shade.p, bufs, n, "inputs and outputs", "elements", &QueryScratch::ev_shade_end, st, launch);
}

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
  return ezi::guarded("ezrt_query_box_overlap_device", [&]() -> int {
    if (!s || !box_lo3 || !box_hi3 || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (max_k < 0 || max_k > EZRT_BOX_OVERLAP_MAX) return fail(EZRT_ERR_INVALID, "max_k out of range [0,%d]", EZRT_BOX_OVERLAP_MAX);
    if (max_k > 0 && !tri_id) return fail(EZRT_ERR_INVALID, "tri_id is required when max_k > 0");
    if (max_k == 0 && !n_overlap) return fail(EZRT_ERR_INVALID, "n_overlap is required when max_k == 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, K = (size_t)max_k;
    if (max_k == 0) tri_id = nullptr; // ignored
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{box_lo3, N * 3 * sizeof(float)}, {box_hi3, N * 3 * sizeof(float)}, {tri_id, N * K * sizeof(int32_t)},
                          {n_overlap, N * sizeof(int32_t)}}, N, st, [&](dim3, dim3) {
      BoxOverlapArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.lo = box_lo3;
      a.hi = box_hi3;
      a.n = (uint32_t)n;
      a.K = max_k;
      a.div_k = make_fastdiv((uint32_t)(max_k > 0 ? max_k : 1));
      a.tri = tri_id;
      a.n_overlap = n_overlap;
      // this walk's entries are bare references, one row each: half of the column that decides the route
      launch_routed(box_overlap_kernel<true>, box_overlap_kernel<false>, r, r.lds / 2, N, st, a);
    });
  });
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
  return ezi::guarded("ezrt_query_obb_overlap_device", [&]() -> int {
    if (!s || !centre3 || !axes9 || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (max_k < 0 || max_k > EZRT_OBB_OVERLAP_MAX) return fail(EZRT_ERR_INVALID, "max_k out of range [0,%d]", EZRT_OBB_OVERLAP_MAX);
    if (max_k > 0 && !tri_id) return fail(EZRT_ERR_INVALID, "tri_id is required when max_k > 0");
    if (max_k == 0 && !n_overlap) return fail(EZRT_ERR_INVALID, "n_overlap is required when max_k == 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, K = (size_t)max_k;
    if (max_k == 0) tri_id = nullptr; // ignored
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{centre3, N * 3 * sizeof(float)}, {axes9, N * 9 * sizeof(float)}, {tri_id, N * K * sizeof(int32_t)},
                          {n_overlap, N * sizeof(int32_t)}}, N, st, [&](dim3, dim3) {
      ObbOverlapArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.centre = centre3;
      a.axes = axes9;
      a.n = (uint32_t)n;
      a.K = max_k;
      a.div_k = make_fastdiv((uint32_t)(max_k > 0 ? max_k : 1));
      a.tri = tri_id;
      a.n_overlap = n_overlap;
      // slot_walk's entries are bare references, one row each: half of the column that decides the route (stack_need_cp + 1 rows)
      launch_routed(obb_overlap_kernel<true>, obb_overlap_kernel<false>, r, r.lds / 2, N, st, a);
    });
  });
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
      hipLaunchKernelGGL(loops_scan_kernel, dim3(1), dim3(LP_SCAN), 0, st, a.plane_loops, (const long long*)nullptr, (long long)n);
      hipLaunchKernelGGL(loops_length_kernel, g, dim3(LP_BLOCK), 0, st, a);
      hipLaunchKernelGGL(loops_scan_kernel, dim3(1), dim3(LP_SCAN), 0, st, a.lofs, (const long long*)(a.plane_loops + n), (long long)capacity);
      hipLaunchKernelGGL(loops_scatter_kernel, g, dim3(LP_BLOCK), 0, st, a);
    });
  });
}

// ---- mesh topology on device memory (include/ezrt_topology.h): up to eight launches on `st` -- init, join, rank, and with the
// component group unite, flatten, loops_scan_kernel, scatter -- over the caller's `work`; checked, launched and ordered against a
// refit by query_call.  `work` is scan (n_tri + 1 int64), then rep and head (T ints each, T the power of two >= 6 n_tri), link and
// slot (3 n_tri ints each), parent, csize and cflag (n_tri ints each).
static uint64_t topo_slots(int n_tri) {
  if (n_tri <= 0) return 0;
  uint64_t T = 8;
  while (T < 6ull * (uint64_t)n_tri) T <<= 1;
  return T;
}
size_t ezrt_topology_work_bytes(int n_tri) {
  if (n_tri <= 0) return 8;
  const uint64_t n = (uint64_t)n_tri, bytes = (n + 1) * 8 + topo_slots(n_tri) * 8 + 6 * n * 4 + 3 * n * 4;
  return (size_t)((bytes + 7) / 8 * 8);
}
int ezrt_mesh_topology_device(EzrtScene* s, int32_t* twin, uint8_t* edge_class, int32_t* mult, int32_t* root, int32_t* component,
                              int32_t* comp_root, int32_t* comp_size, uint8_t* comp_flags, int64_t* summary, void* work, size_t work_bytes,
                              void* stream) {
  return ezi::guarded("ezrt_mesh_topology_device", [&]() -> int {
    if (!s || !twin || !edge_class || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    const int group = (root ? 1 : 0) + (component ? 1 : 0) + (comp_root ? 1 : 0) + (comp_size ? 1 : 0) + (comp_flags ? 1 : 0);
    if (group != 0 && group != 5)
      return fail(EZRT_ERR_INVALID, "root, component, comp_root, comp_size and comp_flags are given together or not at all");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    const int n_tri = (int)s->n_tri;
    if (work_bytes < ezrt_topology_work_bytes(n_tri)) return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_topology_work_bytes(n_tri)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{twin, H * i4}, {edge_class, H}, {mult, H * i4}, {root, N * i4}, {component, N * i4}, {comp_root, N * i4},
                          {comp_size, N * i4}, {comp_flags, N}, {summary, 8 * sizeof(int64_t)}, {work, ezrt_topology_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      TopoArgs a{};
      a.tri_geom = s->tri_geom.p;
      a.n_tri = (int32_t)n_tri;
      a.T = topo_slots(n_tri);
      a.scan = (long long*)work;
      a.rep = (int32_t*)(a.scan + N + 1);
      a.head = (uint32_t*)(a.rep + a.T);
      a.link = a.head + a.T;
      a.slot = a.link + H;
      a.parent = (int32_t*)(a.slot + H);
      a.csize = a.parent + N;
      a.cflag = (uint32_t*)(a.csize + N);
      a.twin = twin, a.edge_class = edge_class, a.mult = mult;
      a.root = root, a.component = component, a.comp_root = comp_root, a.comp_size = comp_size, a.comp_flags = comp_flags;
      a.summary = (unsigned long long*)summary;
      // grid-stride loops: at most TP_GRID_MAX workgroups, a few per CU
      const auto grid = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + TP_BLOCK - 1) / TP_BLOCK, TP_GRID_MAX)); };
      const dim3 b(TP_BLOCK), gh = grid(H), gt = grid(N);
      hipLaunchKernelGGL(topo_init_kernel, grid(a.T), b, 0, st, a, group == 5);
      hipLaunchKernelGGL(topo_join_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(topo_rank_kernel, gh, b, 0, st, a);
      if (group == 5) {
        hipLaunchKernelGGL(topo_unite_kernel, gh, b, 0, st, a);
        hipLaunchKernelGGL(topo_flatten_kernel, gt, b, 0, st, a);
        hipLaunchKernelGGL(loops_scan_kernel, dim3(1), dim3(LP_SCAN), 0, st, a.scan, (const long long*)nullptr, (long long)n_tri);
        hipLaunchKernelGGL(topo_scatter_kernel, gt, b, 0, st, a);
      }
    });
  });
}
int ezrt_mesh_topology_at_device(EzrtScene* s, const int32_t* tri_a, const int32_t* edge_a, const int32_t* tri_b, int n, int8_t* shared,
                                 int8_t* opposite, void* stream) {
  return ezi::guarded("ezrt_mesh_topology_at_device", [&]() -> int {
    if (!s || !tri_a || !edge_a || !tri_b || !shared || !opposite || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri_a, N * sizeof(int32_t)}, {edge_a, N * sizeof(int32_t)}, {tri_b, N * sizeof(int32_t)}, {shared, N}, {opposite, N}},
                      N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(topo_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, tri_a, edge_a, tri_b, (uint32_t)n, shared, opposite);
    });
  });
}

// ---- vertex weld and smooth normals on device memory (include/ezrt_vertices.h): up to fifteen launches on `st` for the weld -- init,
// join, flag, a prefix sum (sums, loops_scan_kernel, scan), id, the prefix sum again, scatter, rank, and with the flags group link,
// fans, finish -- over the caller's `work`: ids and cnt (3 n_tri + 1 int64 each), tiles (one int64 per 2048 corners, and one), rep
// (T ints, T the topology's power of two >= 6 n_tri), then slot, cur, tmp,
// parent, flagw and fanc (3 n_tri ints each); two launches for the normals over 3 n_tri floats of `work`.  Checked, launched and
// ordered against a refit by query_call.
static uint64_t weld_tiles(int n_tri) { return (3ull * (uint64_t)n_tri + WD_TILE - 1) / WD_TILE; }
size_t ezrt_weld_work_bytes(int n_tri) {
  if (n_tri <= 0) return 8;
  const uint64_t h = 3ull * (uint64_t)n_tri, bytes = 2 * (h + 1) * 8 + (weld_tiles(n_tri) + 1) * 8 + topo_slots(n_tri) * 4 + 6 * h * 4;
  return (size_t)((bytes + 7) / 8 * 8);
}
int ezrt_mesh_weld_device(EzrtScene* s, int32_t* vertex, int32_t* vert_corner, int32_t* star_offsets, int32_t* star, int32_t* fans,
                          uint8_t* vert_flags, int64_t* summary, void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_mesh_weld_device", [&]() -> int {
    if (!s || !vertex || !vert_corner || !star_offsets || !star || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (!fans != !vert_flags) return fail(EZRT_ERR_INVALID, "fans and vert_flags are given together or not at all");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    const int n_tri = (int)s->n_tri;
    if (work_bytes < ezrt_weld_work_bytes(n_tri)) return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_weld_work_bytes(n_tri)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_tri <= 0) return 0;
    const size_t H = 3 * (size_t)n_tri, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{vertex, H * i4}, {vert_corner, H * i4}, {star_offsets, (H + 1) * i4}, {star, H * i4}, {fans, H * i4}, {vert_flags, H},
                          {summary, 8 * sizeof(int64_t)}, {work, ezrt_weld_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      WeldArgs a{};
      a.tri_geom = s->tri_geom.p;
      a.n_tri = (int32_t)n_tri;
      a.T = topo_slots(n_tri);
      a.ids = (long long*)work;
      a.cnt = a.ids + H + 1;
      a.tiles = a.cnt + H + 1;
      const uint64_t B = weld_tiles(n_tri);
      a.rep = (int32_t*)(a.tiles + B + 1);
      a.slot = (uint32_t*)(a.rep + a.T);
      a.cur = (int32_t*)(a.slot + H);
      a.tmp = a.cur + H;
      a.parent = a.tmp + H;
      a.flagw = (uint32_t*)(a.parent + H);
      a.fanc = (int32_t*)(a.flagw + H);
      a.vertex = vertex, a.vert_corner = vert_corner, a.star_offsets = star_offsets, a.star = star, a.fans = fans, a.vert_flags = vert_flags;
      a.summary = (unsigned long long*)summary;
      const auto grid = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + WD_BLOCK - 1) / WD_BLOCK, WD_GRID_MAX)); };
      const dim3 b(WD_BLOCK), gh = grid(H), scan(LP_SCAN);
      hipLaunchKernelGGL(weld_init_kernel, grid(a.T), b, 0, st, a, fans != nullptr);
      hipLaunchKernelGGL(weld_join_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(weld_flag_kernel, gh, b, 0, st, a);
      // a prefix sum of x in place over B tiles (ezrt_vertex_kernels.h: weld_scan_kernel); n_dev: its length, read on the device
      const auto prefix = [&](long long* x, const long long* n_dev) {
        hipLaunchKernelGGL(weld_sums_kernel, dim3((unsigned)B), b, 0, st, (const long long*)x, a.tiles, n_dev, (long long)H);
        hipLaunchKernelGGL(loops_scan_kernel, dim3(1), scan, 0, st, a.tiles, (const long long*)nullptr, (long long)B);
        hipLaunchKernelGGL(weld_scan_kernel, dim3((unsigned)B), b, 0, st, x, (const long long*)a.tiles, n_dev, (long long)H);
      };
      prefix(a.ids, nullptr);
      hipLaunchKernelGGL(weld_id_kernel, gh, b, 0, st, a);
      prefix(a.cnt, (const long long*)(a.ids + H));
      hipLaunchKernelGGL(weld_scatter_kernel, grid(H + 1), b, 0, st, a);
      hipLaunchKernelGGL(weld_rank_kernel, gh, b, 0, st, a);
      if (fans) {
        hipLaunchKernelGGL(weld_link_kernel, gh, b, 0, st, a);
        hipLaunchKernelGGL(weld_fans_kernel, gh, b, 0, st, a);
        hipLaunchKernelGGL(weld_finish_kernel, gh, b, 0, st, a);
      }
    });
  });
}
int ezrt_mesh_weld_at_device(EzrtScene* s, const int32_t* corner_a, const int32_t* corner_b, int n, int8_t* same, void* stream) {
  return ezi::guarded("ezrt_mesh_weld_at_device", [&]() -> int {
    if (!s || !corner_a || !corner_b || !same || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{corner_a, N * sizeof(int32_t)}, {corner_b, N * sizeof(int32_t)}, {same, N}}, N, st, [&](dim3 g, dim3 b) {
      hipLaunchKernelGGL(weld_at_kernel, g, b, 0, st, s->tri_geom.p, (int32_t)s->n_tri, corner_a, corner_b, (uint32_t)n, same);
    });
  });
}
size_t ezrt_vertex_normals_work_bytes(int n_tri) {
  if (n_tri <= 0) return 8;
  return (size_t)((3ull * (uint64_t)n_tri * sizeof(float) + 7) / 8 * 8);
}
int ezrt_vertex_normals_device(EzrtScene* s, float* tri36, int n_tri, const int32_t* vertex, const int32_t* star_offsets, const int32_t* star,
                               void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_vertex_normals_device", [&]() -> int {
    if (!s || !tri36 || !vertex || !star_offsets || !star || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)n_tri != (int64_t)s->n_tri) return fail(EZRT_ERR_INVALID, "n_tri is %d, the scene has %lld triangles", n_tri, (long long)s->n_tri);
    if (n_tri > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    if (work_bytes < ezrt_vertex_normals_work_bytes(n_tri))
      return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_vertex_normals_work_bytes(n_tri)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * 36 * sizeof(float)}, {vertex, H * i4}, {star_offsets, (H + 1) * i4}, {star, H * i4},
                          {work, ezrt_vertex_normals_work_bytes(n_tri)}},
                      N, st, [&](dim3 g, dim3 b) {
      VertexNormalArgs a{};
      a.tri36 = tri36;
      a.n_tri = (int32_t)n_tri;
      a.vertex = vertex, a.star_offsets = star_offsets, a.star = star;
      a.face = (float*)work;
      hipLaunchKernelGGL(vn_face_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(vn_corner_kernel, dim3((unsigned)((H + WD_BLOCK - 1) / WD_BLOCK)), b, 0, st, a);
    });
  });
}

// ---- mesh orientation on device memory (include/ezrt_orient.h): nine launches on `st` -- init, union, flatten, check, the weld's
// prefix sum (sums, loops_scan_kernel, scan), volume, finish -- over the caller's `work`: scan (n_tri + 1 int64), tiles (one int64 per
// 2048 triangles, and one), vol (n_tri int64), then par, flat, pf and psz (n_tri ints each) and two words for A; one launch for the
// rewind.  Checked, launched and ordered against a refit by query_call.
static uint64_t orient_tiles(int n_tri) { return ((uint64_t)n_tri + WD_TILE - 1) / WD_TILE; }
size_t ezrt_orient_work_bytes(int n_tri) {
  if (n_tri <= 0) return 8;
  return (size_t)(32ull * (uint64_t)n_tri + 8ull * orient_tiles(n_tri) + 24ull);
}
int ezrt_mesh_orient_device(EzrtScene* s, const int32_t* twin, const uint8_t* edge_class, int outward, uint8_t* flip, int32_t* patch_root,
                            int32_t* patch, int32_t* proot, int32_t* psize, uint8_t* pflags, int64_t* vol6, int64_t* summary, void* work,
                            size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_mesh_orient_device", [&]() -> int {
    if (!s || !twin || !edge_class || !flip || !patch_root || !patch || !proot || !psize || !pflags || !vol6 || !summary || !work)
      return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    const int n_tri = (int)s->n_tri;
    if (work_bytes < ezrt_orient_work_bytes(n_tri)) return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_orient_work_bytes(n_tri)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{twin, H * i4}, {edge_class, H}, {flip, N}, {patch_root, N * i4}, {patch, N * i4}, {proot, N * i4}, {psize, N * i4},
                          {pflags, N}, {vol6, N * sizeof(int64_t)}, {summary, 8 * sizeof(int64_t)}, {work, ezrt_orient_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      OrientArgs a{};
      a.tri_geom = s->tri_geom.p;
      a.n_tri = (int32_t)n_tri;
      a.twin = twin, a.edge_class = edge_class, a.outward = outward != 0 ? 1 : 0;
      const uint64_t B = orient_tiles(n_tri);
      a.scan = (long long*)work;
      a.tiles = a.scan + N + 1;
      a.vol = a.tiles + B + 1;
      a.par = (uint32_t*)(a.vol + N);
      a.flat = a.par + N;
      a.pf = a.flat + N;
      a.psz = (int32_t*)(a.pf + N);
      a.amax = (uint32_t*)(a.psz + N);
      a.flip = flip, a.patch_root = patch_root, a.patch = patch, a.proot = proot, a.psize = psize, a.pflags = pflags;
      a.vol6 = (long long*)vol6, a.summary = (unsigned long long*)summary;
      const auto grid = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + OR_BLOCK - 1) / OR_BLOCK, OR_GRID_MAX)); };
      const dim3 b(OR_BLOCK), gh = grid(H), gt = grid(N);
      hipLaunchKernelGGL(orient_init_kernel, gt, b, 0, st, a);
      hipLaunchKernelGGL(orient_union_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(orient_flatten_kernel, gt, b, 0, st, a);
      hipLaunchKernelGGL(orient_check_kernel, gt, b, 0, st, a);
      // the prefix sum of the roots' flags in place over B tiles (ezrt_vertex_kernels.h: weld_scan_kernel)
      hipLaunchKernelGGL(weld_sums_kernel, dim3((unsigned)B), dim3(WD_BLOCK), 0, st, (const long long*)a.scan, a.tiles, (const long long*)nullptr, (long long)N);
      hipLaunchKernelGGL(loops_scan_kernel, dim3(1), dim3(LP_SCAN), 0, st, a.tiles, (const long long*)nullptr, (long long)B);
      hipLaunchKernelGGL(weld_scan_kernel, dim3((unsigned)B), dim3(WD_BLOCK), 0, st, a.scan, (const long long*)a.tiles, (const long long*)nullptr, (long long)N);
      hipLaunchKernelGGL(orient_volume_kernel, gt, b, 0, st, a);
      hipLaunchKernelGGL(orient_finish_kernel, gt, b, 0, st, a);
    });
  });
}
int ezrt_rewind_device(EzrtScene* s, float* tri36, int n_tri, const uint8_t* flip, void* stream) {
  return ezi::guarded("ezrt_rewind_device", [&]() -> int {
    if (!s || !tri36 || !flip) return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)n_tri != (int64_t)s->n_tri) return fail(EZRT_ERR_INVALID, "n_tri is %d, the scene has %lld triangles", n_tri, (long long)s->n_tri);
    if (n_tri > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * 36 * sizeof(float)}, {flip, N}}, N, st, [&](dim3, dim3) {
      hipLaunchKernelGGL(rewind_kernel, dim3((unsigned)((N + OR_BLOCK - 1) / OR_BLOCK)), dim3(OR_BLOCK), 0, st, tri36, (uint32_t)n_tri, flip);
    });
  });
}

// ---- boundary loops on device memory (include/ezrt_boundary.h): 17 launches and the rounds of the ranking on `st` -- init, next,
// union, open, a prefix sum (sums, loops_scan_kernel, scan) that compacts the BOUNDARY half-edges, rank init, ceil(log2(3 n_tri)) jumping
// rounds, flag, the prefix sum over the compacted list that numbers the heads, number, the prefix sum of the lengths, scatter -- over the
// caller's `work`: scan_c and scan_n (3 n_tri + 1 int64 each), tiles (one int64 per 2048 half-edges, and one), the two buffers of the
// ranking (3 n_tri int64 each), four int64 of counts, then pred, par and comp (3 n_tri ints each); one launch for the cap.  Checked,
// launched and ordered against a refit by query_call.
static uint64_t boundary_tiles(int n_tri) { return (3ull * (uint64_t)n_tri + WD_TILE - 1) / WD_TILE; }
size_t ezrt_boundary_work_bytes(int n_tri) {
  if (n_tri <= 0) return 8;
  return (size_t)(132ull * (uint64_t)n_tri + 4ull * ((uint64_t)n_tri & 1ull) + 8ull * boundary_tiles(n_tri) + 56ull);
}
int ezrt_mesh_boundary_device(EzrtScene* s, const int32_t* twin, const uint8_t* edge_class, int32_t* next, int32_t* loop, int32_t* pos,
                              int32_t* order, int32_t* loop_offsets, uint8_t* lflags, int64_t* area2, int64_t* summary, void* work,
                              size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_mesh_boundary_device", [&]() -> int {
    if (!s || !twin || !edge_class || !next || !loop || !pos || !order || !loop_offsets || !lflags || !summary || !work)
      return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    const int n_tri = (int)s->n_tri;
    if (work_bytes < ezrt_boundary_work_bytes(n_tri)) return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_boundary_work_bytes(n_tri)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t), i8 = sizeof(int64_t);
    hipStream_t st = (hipStream_t)stream;
    // (a null area2 is skipped by the check, as a null input of the overlap lists is)
    return query_call(s, {{twin, H * i4}, {edge_class, H}, {next, H * i4}, {loop, H * i4}, {pos, H * i4}, {order, H * i4},
                          {loop_offsets, (H + 1) * i4}, {lflags, H}, {area2, 3 * H * i8}, {summary, 8 * i8},
                          {work, ezrt_boundary_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      BoundaryArgs a{};
      a.tri_geom = s->tri_geom.p;
      a.n_tri = (int32_t)n_tri;
      a.twin = twin, a.edge_class = edge_class;
      const uint64_t T = boundary_tiles(n_tri);
      a.scan_c = (long long*)work;
      a.scan_n = a.scan_c + H + 1;
      a.tiles = a.scan_n + H + 1;
      a.jump[0] = (unsigned long long*)(a.tiles + T + 1);
      a.jump[1] = a.jump[0] + H;
      a.cnt = (long long*)(a.jump[1] + H);
      a.pred = (int32_t*)(a.cnt + 4);
      a.par = (uint32_t*)(a.pred + H);
      a.comp = (int32_t*)(a.par + H);
      a.open = (uint32_t*)a.scan_n;
      a.lens = a.scan_c;
      int rounds = 0;
      while ((1ull << rounds) < (uint64_t)H) rounds++; // ceil(log2(3 n_tri)): at most 32
      a.rounds = rounds;
      a.next = next, a.loop = loop, a.pos = pos, a.order = order, a.loop_offsets = loop_offsets, a.lflags = lflags;
      a.area2 = (long long*)area2, a.summary = (unsigned long long*)summary;
      const dim3 b(BD_BLOCK), g((unsigned)std::min<uint64_t>((H + BD_BLOCK - 1) / BD_BLOCK, BD_GRID_MAX));
      // a prefix sum of x in place over T tiles (ezrt_vertex_kernels.h: weld_scan_kernel); n_dev: its length, read on the device
      const auto scan = [&](long long* x, const long long* n_dev) {
        hipLaunchKernelGGL(weld_sums_kernel, dim3((unsigned)T), dim3(WD_BLOCK), 0, st, (const long long*)x, a.tiles, n_dev, (long long)H);
        hipLaunchKernelGGL(loops_scan_kernel, dim3(1), dim3(LP_SCAN), 0, st, a.tiles, (const long long*)nullptr, (long long)T);
        hipLaunchKernelGGL(weld_scan_kernel, dim3((unsigned)T), dim3(WD_BLOCK), 0, st, x, (const long long*)a.tiles, n_dev, (long long)H);
      };
      hipLaunchKernelGGL(bd_init_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(bd_next_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(bd_union_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(bd_open_kernel, g, b, 0, st, a);
      scan(a.scan_c, nullptr);
      hipLaunchKernelGGL(bd_rank_init_kernel, g, b, 0, st, a);
      for (int r = 0; r < rounds; r++) hipLaunchKernelGGL(bd_jump_kernel, g, b, 0, st, a, r & 1); // rounds are separated by launches
      hipLaunchKernelGGL(bd_flag_kernel, g, b, 0, st, a);
      scan(a.scan_n, a.cnt);
      hipLaunchKernelGGL(bd_number_kernel, g, b, 0, st, a);
      scan(a.lens, a.cnt + 1);
      hipLaunchKernelGGL(bd_scatter_kernel, g, b, 0, st, a);
    });
  });
}
int ezrt_cap_rows_device(EzrtScene* s, const float* tri36, int n_tri, const int32_t* order, const int32_t* loop, const int32_t* pos,
                         const int32_t* loop_offsets, const uint8_t* lflags, const int64_t* summary, float* cap, uint8_t* cap_valid,
                         void* stream) {
  return ezi::guarded("ezrt_cap_rows_device", [&]() -> int {
    if (!s || !tri36 || !order || !loop || !pos || !loop_offsets || !lflags || !summary || !cap || !cap_valid)
      return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)n_tri != (int64_t)s->n_tri) return fail(EZRT_ERR_INVALID, "n_tri is %d, the scene has %lld triangles", n_tri, (long long)s->n_tri);
    if (n_tri > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * 36 * sizeof(float)}, {order, H * i4}, {loop, H * i4}, {pos, H * i4}, {loop_offsets, (H + 1) * i4},
                          {lflags, H}, {summary, 8 * sizeof(int64_t)}, {cap, H * 36 * sizeof(float)}, {cap_valid, H}},
                      H, st, [&](dim3, dim3) {
      hipLaunchKernelGGL(cap_rows_kernel, dim3((unsigned)((H + BD_BLOCK - 1) / BD_BLOCK)), dim3(BD_BLOCK), 0, st, tri36, (int32_t)n_tri, order, loop,
                         pos, loop_offsets, lflags, (const long long*)summary, cap, cap_valid);
    });
  });
}

// ---- plane clipping on device memory (include/ezrt_clip.h).  Count: a memset of the summary, clip_count_kernel, and the weld's tiled
// prefix sum (sums, loops_scan_kernel, scan) of offsets in place over the caller's `work`, the tiles' sums and their total.  Fill: one
// launch, the staged instance where tri36 and out are 16-byte aligned, else the per-lane one (always, in the measurement variant
// EZRT_CLIP_PER_LANE).  Checked, launched and ordered against a refit by query_call; the scene's records are not read.
#ifndef EZRT_CLIP_PER_LANE
#define EZRT_CLIP_PER_LANE 0
#endif
static uint64_t clip_tiles(int n_rows) { return ((uint64_t)n_rows + WD_TILE - 1) / WD_TILE; }
size_t ezrt_clip_work_bytes(int n_rows) {
  if (n_rows <= 0) return 8;
  return (size_t)(8ull * clip_tiles(n_rows) + 8ull);
}
int ezrt_clip_count_device(EzrtScene* s, const float* tri36, int n_rows, const float* plane4, int64_t* offsets, int64_t* summary, void* work,
                           size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_clip_count_device", [&]() -> int {
    if (!s || !tri36 || !plane4 || !offsets || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 2) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 2 rows");
    if (work_bytes < ezrt_clip_work_bytes(n_rows)) return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_clip_work_bytes(n_rows)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, i8 = sizeof(int64_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * 36 * sizeof(float)}, {plane4, 4 * sizeof(float)}, {offsets, (N + 1) * i8}, {summary, 8 * i8},
                          {work, ezrt_clip_work_bytes(n_rows)}},
                      N, st, [&](dim3, dim3) -> int {
      const uint64_t T = clip_tiles(n_rows);
      long long *x = (long long*)offsets, *tiles = (long long*)work;
      HIP_TRY(hipMemsetAsync(summary, 0, 8 * i8, st));
      hipLaunchKernelGGL(clip_count_kernel, dim3((unsigned)((N + CL_BLOCK - 1) / CL_BLOCK)), dim3(CL_BLOCK), 0, st, tri36, (int32_t)n_rows, plane4, x,
                         (unsigned long long*)summary);
      // the prefix sum of the counts in place over T tiles (ezrt_vertex_kernels.h: weld_scan_kernel); the total lands in offsets[n_rows]
      hipLaunchKernelGGL(weld_sums_kernel, dim3((unsigned)T), dim3(WD_BLOCK), 0, st, (const long long*)x, tiles, (const long long*)nullptr, (long long)N);
      hipLaunchKernelGGL(loops_scan_kernel, dim3(1), dim3(LP_SCAN), 0, st, tiles, (const long long*)nullptr, (long long)T);
      hipLaunchKernelGGL(weld_scan_kernel, dim3((unsigned)T), dim3(WD_BLOCK), 0, st, x, (const long long*)tiles, (const long long*)nullptr, (long long)N);
      return 0;
    });
  });
}
int ezrt_clip_rows_device(EzrtScene* s, const float* tri36, int n_rows, const float* plane4, const int64_t* offsets, int64_t capacity, float* out,
                          int32_t* src, int8_t* cut_edge, void* stream) {
  return ezi::guarded("ezrt_clip_rows_device", [&]() -> int {
    if (!s || !tri36 || !plane4 || !offsets) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 2) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 2 rows");
    if (capacity < 0) return fail(EZRT_ERR_INVALID, "capacity < 0");
    // (the byte count below must not wrap: a wrapped one would pass the buffer check and leave the kernel a capacity that is none)
    if (capacity > (int64_t)(PTRDIFF_MAX / (36 * sizeof(float)))) return fail(EZRT_ERR_INVALID, "capacity exceeds what an array can hold");
    if (!out && capacity > 0) return fail(EZRT_ERR_INVALID, "NULL out with capacity > 0");
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, cap = (size_t)capacity, row = 36 * sizeof(float);
    if (out && cap > 0) {
      const uintptr_t i0 = (uintptr_t)tri36, i1 = i0 + N * row, o0 = (uintptr_t)out, o1 = o0 + cap * row;
      if (i0 < o1 && o0 < i1) return fail(EZRT_ERR_INVALID, "out overlaps tri36");
    }
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * row}, {plane4, 4 * sizeof(float)}, {offsets, (N + 1) * sizeof(int64_t)}, {cap ? out : nullptr, cap * row},
                          {cap ? src : nullptr, cap * sizeof(int32_t)}, {cap ? cut_edge : nullptr, cap}},
                      N, st, [&](dim3, dim3) {
      if (cap == 0) return; // nothing fits: nothing is written
      ClipFillArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.plane4 = plane4, a.offsets = (const long long*)offsets, a.capacity = (long long)capacity;
      a.out = out, a.src = src, a.cut_edge = cut_edge;
      const dim3 g((unsigned)((N + CL_BLOCK - 1) / CL_BLOCK)), b(CL_BLOCK);
      const bool staged = !EZRT_CLIP_PER_LANE && ((uintptr_t)tri36 | (uintptr_t)out) % 16 == 0;
      if (staged) hipLaunchKernelGGL(clip_fill_kernel<true>, g, b, 0, st, a);
      else hipLaunchKernelGGL(clip_fill_kernel<false>, g, b, 0, st, a);
    });
  });
}

// ---- subdivision on device memory (include/ezrt_subdivide.h): a memset of the summary, in Loop mode subdiv_vertex_kernel over the
// caller's `work` (four words per possible vertex), and one fill launch, the staged instance where tri36 and out are 16-byte aligned,
// else the per-lane one (always, in the measurement variant EZRT_SUBDIV_PER_LANE).  The output's size is known, so there is no count.
// Checked, launched and ordered against a refit by query_call; the scene's records are not read.
#ifndef EZRT_SUBDIV_PER_LANE
#define EZRT_SUBDIV_PER_LANE 0
#endif
#ifndef EZRT_SUBDIV_SKIP_VERTEX // measurement variant: Loop mode without its vertex pass, for timing the fill alone (the slots are whatever `work` held)
#define EZRT_SUBDIV_SKIP_VERTEX 0
#endif
size_t ezrt_subdivide_work_bytes(int n_rows, int mode) {
  if (n_rows <= 0 || mode != EZRT_SUBDIVIDE_LOOP) return 8;
  return (size_t)(48ull * (uint64_t)n_rows + 8ull);
}
int ezrt_subdivide_rows_device(EzrtScene* s, const float* tri36, int n_rows, int mode, const int32_t* twin, const uint8_t* edge_class,
                               const int32_t* vertex, const int32_t* star_offsets, const int32_t* star, const uint8_t* vert_flags, float* out,
                               int64_t* summary, void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_subdivide_rows_device", [&]() -> int {
    if (!s || !tri36 || !out || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 12) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 12 rows");
    if (mode != EZRT_SUBDIVIDE_MIDPOINT && mode != EZRT_SUBDIVIDE_LOOP) return fail(EZRT_ERR_INVALID, "mode %d is neither MIDPOINT nor LOOP", mode);
    const int given = !!twin + !!edge_class + !!vertex + !!star_offsets + !!star + !!vert_flags;
    if (given != 0 && given != 6)
      return fail(EZRT_ERR_INVALID, "twin, edge_class, vertex, star_offsets, star and vert_flags are given together or not at all");
    if (mode == EZRT_SUBDIVIDE_MIDPOINT && given) return fail(EZRT_ERR_INVALID, "the topology and weld arrays must be NULL in MIDPOINT mode");
    if (mode == EZRT_SUBDIVIDE_LOOP && !given) return fail(EZRT_ERR_INVALID, "LOOP mode needs the topology and weld arrays");
    if (work_bytes < ezrt_subdivide_work_bytes(n_rows, mode))
      return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_subdivide_work_bytes(n_rows, mode)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, H = 3 * N, row = 36 * sizeof(float), i4 = sizeof(int32_t);
    {
      const uintptr_t i0 = (uintptr_t)tri36, i1 = i0 + N * row, o0 = (uintptr_t)out, o1 = o0 + 4 * N * row;
      if (i0 < o1 && o0 < i1) return fail(EZRT_ERR_INVALID, "out overlaps tri36");
    }
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * row}, {out, 4 * N * row}, {summary, 8 * sizeof(int64_t)}, {work, ezrt_subdivide_work_bytes(n_rows, mode)},
                          {twin, H * i4}, {edge_class, H}, {vertex, H * i4}, {star_offsets, (H + 1) * i4}, {star, H * i4}, {vert_flags, H}},
                      N, st, [&](dim3, dim3) -> int {
      SubdivArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.mode = (int32_t)mode;
      a.twin = twin, a.edge_class = edge_class, a.vertex = vertex, a.star_offsets = star_offsets, a.star = star, a.vert_flags = vert_flags;
      a.out = out, a.summary = (unsigned long long*)summary, a.slot = (uint32_t*)work;
      HIP_TRY(hipMemsetAsync(summary, 0, 8 * sizeof(int64_t), st));
      const dim3 b(SD_BLOCK);
      if (mode == EZRT_SUBDIVIDE_LOOP && !EZRT_SUBDIV_SKIP_VERTEX) hipLaunchKernelGGL(subdiv_vertex_kernel, dim3((unsigned)((H + SD_BLOCK - 1) / SD_BLOCK)), b, 0, st, a);
      const bool staged = !EZRT_SUBDIV_PER_LANE && ((uintptr_t)tri36 | (uintptr_t)out) % 16 == 0;
      if (staged) hipLaunchKernelGGL(subdiv_fill_kernel<true>, dim3((unsigned)std::min<uint64_t>((N + SD_TILE - 1) / SD_TILE, SD_GRID_MAX)), b, 0, st, a);
      else hipLaunchKernelGGL(subdiv_fill_kernel<false>, dim3((unsigned)((N + SD_BLOCK - 1) / SD_BLOCK)), b, 0, st, a);
      return 0;
    });
  });
}

// ---- decimation on device memory (include/ezrt_decimate.h).  Count: init, insert, flag, the weld's tiled prefix sum (sums,
// loops_scan_kernel, scan) over the corners, cells, with EZRT_DECIMATE_DEDUP classify, keep, and the prefix sum again over the rows,
// in place in offsets -- up to twelve launches over the caller's `work`: ids (3 n_rows + 1 int64), tiles (one int64 per 2048 corners,
// and one), key (T int64, T the topology's power of two >= 6 n_rows), sum (3 T int64), cnt, low (T ints each), mn, mx (3 T ints each),
// slot (3 n_rows ints), rep2 (T2 ints, T2 the power of two >= 2 n_rows), slot2 (n_rows ints).  Fill: one launch, the staged instance
// where tri36 and out are 16-byte aligned, else the per-lane one (always, in the measurement variant EZRT_DECIMATE_PER_LANE).
// Checked, launched and ordered against a refit by query_call; the scene's records are not read.
#ifndef EZRT_DECIMATE_PER_LANE
#define EZRT_DECIMATE_PER_LANE 0
#endif
static uint64_t dec_slots2(int n_rows) {
  uint64_t T = 8;
  while (T < 2ull * (uint64_t)n_rows) T <<= 1;
  return T;
}
size_t ezrt_decimate_work_bytes(int n_rows) {
  if (n_rows <= 0) return 8;
  const uint64_t n = (uint64_t)n_rows;
  return (size_t)(40ull * n + 8ull * weld_tiles(n_rows) + 64ull * topo_slots(n_rows) + 4ull * dec_slots2(n_rows) + 16ull);
}
int ezrt_decimate_count_device(EzrtScene* s, const float* tri36, int n_rows, const float* grid4, int flags, int32_t* cell, int32_t* cell_corner,
                               float* cell_point, int64_t* offsets, int64_t* summary, void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_decimate_count_device", [&]() -> int {
    if (!s || !tri36 || !grid4 || !cell || !cell_corner || !cell_point || !offsets || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 rows");
    if (flags & ~EZRT_DECIMATE_DEDUP) return fail(EZRT_ERR_INVALID, "flags %d has a bit that is not EZRT_DECIMATE_DEDUP", flags);
    if (work_bytes < ezrt_decimate_work_bytes(n_rows)) return fail(EZRT_ERR_INVALID, "work_bytes is below ezrt_decimate_work_bytes(n_rows)");
    if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, H = 3 * N, i4 = sizeof(int32_t), i8 = sizeof(int64_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * 36 * sizeof(float)}, {grid4, 4 * sizeof(float)}, {cell, H * i4}, {cell_corner, H * i4},
                          {cell_point, H * 3 * sizeof(float)}, {offsets, (N + 1) * i8}, {summary, 8 * i8}, {work, ezrt_decimate_work_bytes(n_rows)}},
                      H, st, [&](dim3, dim3) {
      DecArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.grid4 = grid4, a.flags = (int32_t)flags;
      a.T = topo_slots(n_rows), a.T2 = dec_slots2(n_rows);
      const uint64_t B = weld_tiles(n_rows), R = clip_tiles(n_rows);
      a.ids = (long long*)work;
      a.tiles = a.ids + H + 1;
      a.key = (unsigned long long*)(a.tiles + B + 1);
      a.sum = a.key + a.T;
      a.cnt = (uint32_t*)(a.sum + 3 * a.T);
      a.low = (int32_t*)(a.cnt + a.T);
      a.mn = (uint32_t*)(a.low + a.T);
      a.mx = a.mn + 3 * a.T;
      a.slot = a.mx + 3 * a.T;
      a.rep2 = (int32_t*)(a.slot + H);
      a.slot2 = (uint32_t*)(a.rep2 + a.T2);
      a.cell = cell, a.cell_corner = cell_corner, a.cell_point = cell_point, a.offsets = (long long*)offsets;
      a.summary = (unsigned long long*)summary;
      const auto grid = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + DC_BLOCK - 1) / DC_BLOCK, DC_GRID_MAX)); };
      const dim3 b(DC_BLOCK), gh = grid(H), scan(LP_SCAN), wb(WD_BLOCK);
      // a prefix sum of x[0 .. n) in place over `tl` tiles (ezrt_vertex_kernels.h: weld_scan_kernel); the total lands in x[n]
      const auto prefix = [&](long long* x, uint64_t n, uint64_t tl) {
        hipLaunchKernelGGL(weld_sums_kernel, dim3((unsigned)tl), wb, 0, st, (const long long*)x, a.tiles, (const long long*)nullptr, (long long)n);
        hipLaunchKernelGGL(loops_scan_kernel, dim3(1), scan, 0, st, a.tiles, (const long long*)nullptr, (long long)tl);
        hipLaunchKernelGGL(weld_scan_kernel, dim3((unsigned)tl), wb, 0, st, x, (const long long*)a.tiles, (const long long*)nullptr, (long long)n);
      };
      hipLaunchKernelGGL(dec_init_kernel, grid(3 * a.T), b, 0, st, a);
      hipLaunchKernelGGL(dec_insert_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(dec_flag_kernel, gh, b, 0, st, a);
      prefix(a.ids, H, B);
      hipLaunchKernelGGL(dec_cells_kernel, gh, b, 0, st, a);
      if (flags & EZRT_DECIMATE_DEDUP) hipLaunchKernelGGL(dec_classify_kernel, grid(N), b, 0, st, a);
      hipLaunchKernelGGL(dec_keep_kernel, dim3((unsigned)((N + DC_BLOCK - 1) / DC_BLOCK)), b, 0, st, a);
      prefix(a.offsets, N, R);
    });
  });
}
int ezrt_decimate_rows_device(EzrtScene* s, const float* tri36, int n_rows, const int32_t* cell, const float* cell_point, const int64_t* offsets,
                              int64_t capacity, float* out, int32_t* src, void* stream) {
  return ezi::guarded("ezrt_decimate_rows_device", [&]() -> int {
    if (!s || !tri36 || !cell || !cell_point || !offsets) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 rows");
    if (capacity < 0) return fail(EZRT_ERR_INVALID, "capacity < 0");
    // (the byte count below must not wrap: a wrapped one would pass the buffer check and leave the kernel a capacity that is none)
    if (capacity > (int64_t)(PTRDIFF_MAX / (36 * sizeof(float)))) return fail(EZRT_ERR_INVALID, "capacity exceeds what an array can hold");
    if (!out && capacity > 0) return fail(EZRT_ERR_INVALID, "NULL out with capacity > 0");
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, H = 3 * N, cap = (size_t)capacity, row = 36 * sizeof(float);
    if (out && cap > 0) {
      const uintptr_t i0 = (uintptr_t)tri36, i1 = i0 + N * row, o0 = (uintptr_t)out, o1 = o0 + cap * row;
      if (i0 < o1 && o0 < i1) return fail(EZRT_ERR_INVALID, "out overlaps tri36");
    }
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * row}, {cell, H * sizeof(int32_t)}, {cell_point, H * 3 * sizeof(float)}, {offsets, (N + 1) * sizeof(int64_t)},
                          {cap ? out : nullptr, cap * row}, {cap ? src : nullptr, cap * sizeof(int32_t)}},
                      N, st, [&](dim3, dim3) {
      if (cap == 0) return; // nothing fits: nothing is written
      DecFillArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.cell = cell, a.cell_point = cell_point, a.offsets = (const long long*)offsets;
      a.capacity = (long long)capacity, a.out = out, a.src = src;
      const dim3 g((unsigned)((N + DC_BLOCK - 1) / DC_BLOCK)), b(DC_BLOCK);
      const bool staged = !EZRT_DECIMATE_PER_LANE && ((uintptr_t)tri36 | (uintptr_t)out) % 16 == 0;
      if (staged) hipLaunchKernelGGL(dec_fill_kernel<true>, g, b, 0, st, a);
      else hipLaunchKernelGGL(dec_fill_kernel<false>, g, b, 0, st, a);
    });
  });
}

// ---- triangle-overlap queries on device memory (include/ezrt_tri_overlap.h): one kernel each on `st`, no scratch (a query's list is
// kept in its own output row); checked, launched and ordered against a refit by query_call.  The route is chosen per call, by
// point_scene.
int ezrt_query_tri_overlap_device(EzrtScene* s, const float* tris9, int n, int max_k, int32_t* tri_id, int32_t* n_overlap, void* stream) {
  return ezi::guarded("ezrt_query_tri_overlap_device", [&]() -> int {
    if (!s || !tris9 || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (max_k < 0 || max_k > EZRT_TRI_OVERLAP_MAX) return fail(EZRT_ERR_INVALID, "max_k out of range [0,%d]", EZRT_TRI_OVERLAP_MAX);
    if (max_k > 0 && !tri_id) return fail(EZRT_ERR_INVALID, "tri_id is required when max_k > 0");
    if (max_k == 0 && !n_overlap) return fail(EZRT_ERR_INVALID, "n_overlap is required when max_k == 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, K = (size_t)max_k;
    if (max_k == 0) tri_id = nullptr; // ignored
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tris9, N * 9 * sizeof(float)}, {tri_id, N * K * sizeof(int32_t)}, {n_overlap, N * sizeof(int32_t)}}, N, st,
                      [&](dim3, dim3) {
      TriOverlapArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.tris = tris9;
      a.n = (uint32_t)n;
      a.K = max_k;
      a.div_k = make_fastdiv((uint32_t)(max_k > 0 ? max_k : 1));
      a.tri = tri_id;
      a.n_overlap = n_overlap;
      // this walk's entries are bare references, one row each: half of the column that decides the route
      launch_routed(tri_overlap_kernel<true>, tri_overlap_kernel<false>, r, r.lds / 2, N, st, a);
    });
  });
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
  return ezi::guarded("ezrt_query_self_overlap_device", [&]() -> int {
    if (!s || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (!ids && (size_t)n > (size_t)s->n_tri) return fail(EZRT_ERR_INVALID, "n exceeds the scene's %d triangles (ids is NULL)", (int)s->n_tri);
    if (max_k < 0 || max_k > EZRT_SELF_OVERLAP_MAX) return fail(EZRT_ERR_INVALID, "max_k out of range [0,%d]", EZRT_SELF_OVERLAP_MAX);
    if (max_k > 0 && !tri_id) return fail(EZRT_ERR_INVALID, "tri_id is required when max_k > 0");
    if (max_k == 0 && !n_overlap) return fail(EZRT_ERR_INVALID, "n_overlap is required when max_k == 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, K = (size_t)max_k;
    if (max_k == 0) tri_id = nullptr; // ignored
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{ids, N * sizeof(int32_t)}, {tri_id, N * K * sizeof(int32_t)}, {n_overlap, N * sizeof(int32_t)}}, N, st,
                      [&](dim3, dim3) {
      SelfOverlapArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.ids = ids;
      a.n = (uint32_t)n;
      a.K = max_k;
      a.div_k = make_fastdiv((uint32_t)(max_k > 0 ? max_k : 1));
      a.tri = tri_id;
      a.n_overlap = n_overlap;
      // this walk's entries are bare references, one row each: half of the column that decides the route
      launch_routed(self_overlap_kernel<true>, self_overlap_kernel<false>, r, r.lds / 2, N, st, a);
    });
  });
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
  return ezi::guarded("ezrt_query_capsule_overlap_device", [&]() -> int {
    if (!s || !segs6 || !radius || n < 0) return fail(EZRT_ERR_INVALID, "NULL argument or n < 0");
    if (max_k < 0 || max_k > EZRT_CAPSULE_OVERLAP_MAX) return fail(EZRT_ERR_INVALID, "max_k out of range [0,%d]", EZRT_CAPSULE_OVERLAP_MAX);
    if (max_k > 0 && !tri_id) return fail(EZRT_ERR_INVALID, "tri_id is required when max_k > 0");
    if (max_k == 0 && !n_overlap) return fail(EZRT_ERR_INVALID, "n_overlap is required when max_k == 0");
    if (n == 0) return 0;
    const size_t N = (size_t)n, K = (size_t)max_k;
    if (max_k == 0) tri_id = nullptr; // ignored
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{segs6, N * 6 * sizeof(float)}, {radius, N * sizeof(float)}, {tri_id, N * K * sizeof(int32_t)},
                          {n_overlap, N * sizeof(int32_t)}}, N, st, [&](dim3, dim3) {
      CapsuleOverlapArgs a;
      const PointRoute r = point_scene(s, a.sc);
      a.segs = segs6;
      a.radius = radius;
      a.n = (uint32_t)n;
      a.K = max_k;
      a.div_k = make_fastdiv((uint32_t)(max_k > 0 ? max_k : 1));
      a.tri = tri_id;
      a.n_overlap = n_overlap;
      // this walk is point_walk: {lb, ref} entries, the whole column
      launch_routed(capsule_overlap_kernel<true>, capsule_overlap_kernel<false>, r, r.lds, N, st, a);
    });
  });
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
