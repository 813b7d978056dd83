// ezrt_mesh.hip -- the mesh processing on device memory: the calls that make SEVERAL launches on the caller's stream, most of them over a
// `work` buffer the caller brings.  Mesh topology (include/ezrt_topology.h, kernels in ezrt_topology_kernels.h), vertex weld and smooth
// normals (ezrt_vertices.h, ezrt_vertex_kernels.h), mesh orientation and rewind (ezrt_orient.h, ezrt_orient_kernels.h), boundary loops
// and caps (ezrt_boundary.h, ezrt_boundary_kernels.h), plane clipping (ezrt_clip.h, ezrt_clip_kernels.h), subdivision
// (ezrt_subdivide.h, ezrt_subdiv_kernels.h), decimation (ezrt_decimate.h, ezrt_decimate_kernels.h) and isosurface extraction
// (ezrt_isosurface.h, ezrt_iso_kernels.h) and smoothing (ezrt_smooth.h, ezrt_smooth_kernels.h).  What the families share is
// stated once: the prefix sums are scan_small and scan_tiled (ezrt_scan_kernels.h); a `work` buffer is described by ONE layout function
// over a WorkCarver (ezrt_work_carver.h), which ezrt_*_work_bytes runs over a null pointer and the call over the caller's; the argument
// checks and the grids are the helpers below.  A translation unit of its own, as ezrt_queries.hip is: none of its kernels is compiled
// together with the render pipeline's or the one-kernel queries'.  Every call goes through query_call (ezrt_internal.h).  DESIGN.md 5.
#include "ezrt_internal.h"
#include "ezrt_topology.h"
#include "ezrt_vertices.h"
#include "ezrt_orient.h"
#include "ezrt_boundary.h"
#include "ezrt_clip.h"
#include "ezrt_subdivide.h"
#include "ezrt_decimate.h"
#include "ezrt_isosurface.h"
#include "ezrt_smooth.h"
#include "ezrt_work_carver.h"
#define EZRT_SCAN_TILED 1 // this unit launches the tiled prefix sum too
#include "ezrt_scan_kernels.h"
#include "ezrt_topology_kernels.h"
#include "ezrt_vertex_kernels.h"
#include "ezrt_orient_kernels.h"
#include "ezrt_boundary_kernels.h"
#include "ezrt_clip_kernels.h"
#include "ezrt_subdiv_kernels.h"
#include "ezrt_decimate_kernels.h"
#include "ezrt_iso_kernels.h"
#include "ezrt_smooth_kernels.h"

using ezi::WorkCarver;

// ---- what the calls share
constexpr unsigned MESH_GRID_MAX = 4096;         // workgroups of a grid-stride launch: 16 per CU
constexpr size_t ROW_BYTES = 36 * sizeof(float); // a triangle row
// the grid of a grid-stride launch over n elements: at most MESH_GRID_MAX workgroups, a few per CU
static dim3 mesh_grid(uint64_t n, unsigned block) { return dim3((unsigned)std::min<uint64_t>((n + block - 1) / block, MESH_GRID_MAX)); }
// the grid of a launch with one lane per element
static dim3 mesh_blocks(uint64_t n, unsigned block) { return dim3((unsigned)((n + block - 1) / block)); }
// the caller's `work`: at least `need` bytes, which `need_name` spells in the message, and aligned for its int64 pieces
static int work_check(const void* work, size_t work_bytes, size_t need, const char* need_name) {
  if (work_bytes < need) return fail(EZRT_ERR_INVALID, "work_bytes is below %s", need_name);
  if ((uintptr_t)work % sizeof(int64_t)) return fail(EZRT_ERR_INVALID, "work is not 8-byte aligned");
  return 0;
}
// a fill call's capacity, in rows, and the `out` that goes with it
static int capacity_check(int64_t capacity, const void* out) {
  if (capacity < 0) return fail(EZRT_ERR_INVALID, "capacity < 0");
  // (the byte count must not wrap: a wrapped one would pass the buffer check and leave the kernel a capacity that is none)
  if (capacity > (int64_t)(PTRDIFF_MAX / ROW_BYTES)) return fail(EZRT_ERR_INVALID, "capacity exceeds what an array can hold");
  if (!out && capacity > 0) return fail(EZRT_ERR_INVALID, "NULL out with capacity > 0");
  return 0;
}
// a fill call's out_rows rows of `out` against the n_rows rows of tri36 it reads
static int overlap_check(const float* tri36, size_t n_rows, const float* out, size_t out_rows) {
  const uintptr_t i0 = (uintptr_t)tri36, i1 = i0 + n_rows * ROW_BYTES, o0 = (uintptr_t)out, o1 = o0 + out_rows * ROW_BYTES;
  if (out && out_rows > 0 && i0 < o1 && o0 < i1) return fail(EZRT_ERR_INVALID, "out overlaps tri36");
  return 0;
}
// a fill's instance: the staged one where both ends are 16-byte aligned, else -- and always in a per-lane measurement variant -- the
// one whose lanes copy their own rows
static bool fill_staged(bool per_lane, const void* tri36, const void* out) { return !per_lane && ((uintptr_t)tri36 | (uintptr_t)out) % 16 == 0; }
// the slots of a hash table: the power of two >= max(8, least)
static uint64_t table_slots(uint64_t least) {
  uint64_t T = 8;
  while (T < least) T <<= 1;
  return T;
}

extern "C" {
// ---- mesh topology on device memory (include/ezrt_topology.h): up to eight launches on `st` -- init, join, rank, and with the
// component group unite, flatten, scan_block_kernel, scatter -- over the caller's `work`; checked, launched and ordered against a
// refit by query_call.  `work` is scan (n_tri + 1 int64), then rep and head (T ints each, T the power of two >= 6 n_tri), link and
// slot (3 n_tri ints each), parent, csize and cflag (n_tri ints each).
static size_t topo_layout(void* work, int n_tri, TopoArgs& a) {
  const uint64_t N = (uint64_t)n_tri, H = 3 * N;
  WorkCarver w(work);
  a.T = table_slots(6 * N);
  a.scan = w.take<long long>(N + 1);
  a.rep = w.take<int32_t>(a.T), a.head = w.take<uint32_t>(a.T);
  a.link = w.take<uint32_t>(H), a.slot = w.take<uint32_t>(H);
  a.parent = w.take<int32_t>(N), a.csize = w.take<int32_t>(N), a.cflag = w.take<uint32_t>(N);
  return w.bytes();
}
size_t ezrt_topology_work_bytes(int n_tri) {
  TopoArgs a{};
  return n_tri <= 0 ? 8 : topo_layout(nullptr, n_tri, a);
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
    if (int rc = work_check(work, work_bytes, ezrt_topology_work_bytes(n_tri), "ezrt_topology_work_bytes(n_tri)")) return rc;
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{twin, H * i4}, {edge_class, H}, {mult, H * i4}, {root, N * i4}, {component, N * i4}, {comp_root, N * i4},
                          {comp_size, N * i4}, {comp_flags, N}, {summary, 8 * sizeof(int64_t)}, {work, ezrt_topology_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      TopoArgs a{};
      a.tri_geom = s->tri_geom.p, a.n_tri = (int32_t)n_tri;
      topo_layout(work, n_tri, a);
      a.twin = twin, a.edge_class = edge_class, a.mult = mult;
      a.root = root, a.component = component, a.comp_root = comp_root, a.comp_size = comp_size, a.comp_flags = comp_flags;
      a.summary = (unsigned long long*)summary;
      const dim3 b(TP_BLOCK), gh = mesh_grid(H, TP_BLOCK), gt = mesh_grid(N, TP_BLOCK);
      hipLaunchKernelGGL(topo_init_kernel, mesh_grid(a.T, TP_BLOCK), b, 0, st, a, group == 5);
      hipLaunchKernelGGL(topo_join_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(topo_rank_kernel, gh, b, 0, st, a);
      if (group == 5) {
        hipLaunchKernelGGL(topo_unite_kernel, gh, b, 0, st, a);
        hipLaunchKernelGGL(topo_flatten_kernel, gt, b, 0, st, a);
        scan_small(st, a.scan, nullptr, (long long)n_tri);
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
// join, flag, a prefix sum (scan_tiled), id, the prefix sum again, scatter, rank, and with the flags group link, fans, finish -- over
// the caller's `work`: ids and cnt (3 n_tri + 1 int64 each), tiles (one int64 per 2048 corners, and one), rep (T ints, T the
// topology's power of two >= 6 n_tri), then slot, cur, tmp, parent, flagw and fanc (3 n_tri ints each); two launches for the normals
// over 3 n_tri floats of `work`.  Checked, launched and ordered against a refit by query_call.
static size_t weld_layout(void* work, int n_tri, WeldArgs& a) {
  const uint64_t H = 3ull * (uint64_t)n_tri;
  WorkCarver w(work);
  a.T = table_slots(2 * H);
  a.ids = w.take<long long>(H + 1), a.cnt = w.take<long long>(H + 1);
  a.tiles = w.take<long long>(scan_tile_count(H) + 1);
  a.rep = w.take<int32_t>(a.T);
  a.slot = w.take<uint32_t>(H), a.cur = w.take<int32_t>(H), a.tmp = w.take<int32_t>(H);
  a.parent = w.take<int32_t>(H), a.flagw = w.take<uint32_t>(H), a.fanc = w.take<int32_t>(H);
  return w.bytes();
}
size_t ezrt_weld_work_bytes(int n_tri) {
  WeldArgs a{};
  return n_tri <= 0 ? 8 : weld_layout(nullptr, n_tri, a);
}
int ezrt_mesh_weld_device(EzrtScene* s, int32_t* vertex, int32_t* vert_corner, int32_t* star_offsets, int32_t* star, int32_t* fans,
                          uint8_t* vert_flags, int64_t* summary, void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_mesh_weld_device", [&]() -> int {
    if (!s || !vertex || !vert_corner || !star_offsets || !star || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (!fans != !vert_flags) return fail(EZRT_ERR_INVALID, "fans and vert_flags are given together or not at all");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    const int n_tri = (int)s->n_tri;
    if (int rc = work_check(work, work_bytes, ezrt_weld_work_bytes(n_tri), "ezrt_weld_work_bytes(n_tri)")) return rc;
    if (n_tri <= 0) return 0;
    const size_t H = 3 * (size_t)n_tri, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{vertex, H * i4}, {vert_corner, H * i4}, {star_offsets, (H + 1) * i4}, {star, H * i4}, {fans, H * i4}, {vert_flags, H},
                          {summary, 8 * sizeof(int64_t)}, {work, ezrt_weld_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      WeldArgs a{};
      a.tri_geom = s->tri_geom.p, a.n_tri = (int32_t)n_tri;
      weld_layout(work, n_tri, a);
      a.vertex = vertex, a.vert_corner = vert_corner, a.star_offsets = star_offsets, a.star = star, a.fans = fans, a.vert_flags = vert_flags;
      a.summary = (unsigned long long*)summary;
      const uint64_t B = scan_tile_count(H);
      const dim3 b(WD_BLOCK), gh = mesh_grid(H, WD_BLOCK);
      hipLaunchKernelGGL(weld_init_kernel, mesh_grid(a.T, WD_BLOCK), b, 0, st, a, fans != nullptr);
      hipLaunchKernelGGL(weld_join_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(weld_flag_kernel, gh, b, 0, st, a);
      scan_tiled(st, a.ids, a.tiles, B, nullptr, (long long)H);
      hipLaunchKernelGGL(weld_id_kernel, gh, b, 0, st, a);
      scan_tiled(st, a.cnt, a.tiles, B, (const long long*)(a.ids + H), (long long)H); // its length V is read on the device
      hipLaunchKernelGGL(weld_scatter_kernel, mesh_grid(H + 1, WD_BLOCK), b, 0, st, a);
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
static size_t normals_layout(void* work, int n_tri, VertexNormalArgs& a) {
  WorkCarver w(work);
  a.face = w.take<float>(3ull * (uint64_t)n_tri);
  return w.bytes();
}
size_t ezrt_vertex_normals_work_bytes(int n_tri) {
  VertexNormalArgs a{};
  return n_tri <= 0 ? 8 : normals_layout(nullptr, n_tri, a);
}
int ezrt_vertex_normals_device(EzrtScene* s, float* tri36, int n_tri, const int32_t* vertex, const int32_t* star_offsets, const int32_t* star,
                               void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_vertex_normals_device", [&]() -> int {
    if (!s || !tri36 || !vertex || !star_offsets || !star || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)n_tri != (int64_t)s->n_tri) return fail(EZRT_ERR_INVALID, "n_tri is %d, the scene has %lld triangles", n_tri, (long long)s->n_tri);
    if (n_tri > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    if (int rc = work_check(work, work_bytes, ezrt_vertex_normals_work_bytes(n_tri), "ezrt_vertex_normals_work_bytes(n_tri)")) return rc;
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * ROW_BYTES}, {vertex, H * i4}, {star_offsets, (H + 1) * i4}, {star, H * i4},
                          {work, ezrt_vertex_normals_work_bytes(n_tri)}},
                      N, st, [&](dim3 g, dim3 b) {
      VertexNormalArgs a{};
      a.tri36 = tri36, a.n_tri = (int32_t)n_tri;
      a.vertex = vertex, a.star_offsets = star_offsets, a.star = star;
      normals_layout(work, n_tri, a);
      hipLaunchKernelGGL(vn_face_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(vn_corner_kernel, mesh_blocks(H, WD_BLOCK), b, 0, st, a);
    });
  });
}

// ---- mesh orientation on device memory (include/ezrt_orient.h): nine launches on `st` -- init, union, flatten, check, the prefix sum
// (scan_tiled), volume, finish -- over the caller's `work`: scan (n_tri + 1 int64), tiles (one int64 per 2048 triangles, and one),
// vol (n_tri int64), then par, flat, pf and psz (n_tri ints each) and two words for A; one launch for the rewind.  Checked, launched
// and ordered against a refit by query_call.
static size_t orient_layout(void* work, int n_tri, OrientArgs& a) {
  const uint64_t N = (uint64_t)n_tri;
  WorkCarver w(work);
  a.scan = w.take<long long>(N + 1);
  a.tiles = w.take<long long>(scan_tile_count(N) + 1);
  a.vol = w.take<long long>(N);
  a.par = w.take<uint32_t>(N), a.flat = w.take<uint32_t>(N), a.pf = w.take<uint32_t>(N), a.psz = w.take<int32_t>(N);
  a.amax = w.take<uint32_t>(2);
  return w.bytes();
}
size_t ezrt_orient_work_bytes(int n_tri) {
  OrientArgs a{};
  return n_tri <= 0 ? 8 : orient_layout(nullptr, n_tri, a);
}
int ezrt_mesh_orient_device(EzrtScene* s, const int32_t* twin, const uint8_t* edge_class, int outward, uint8_t* flip, int32_t* patch_root,
                            int32_t* patch, int32_t* proot, int32_t* psize, uint8_t* pflags, int64_t* vol6, int64_t* summary, void* work,
                            size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_mesh_orient_device", [&]() -> int {
    if (!s || !twin || !edge_class || !flip || !patch_root || !patch || !proot || !psize || !pflags || !vol6 || !summary || !work)
      return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    const int n_tri = (int)s->n_tri;
    if (int rc = work_check(work, work_bytes, ezrt_orient_work_bytes(n_tri), "ezrt_orient_work_bytes(n_tri)")) return rc;
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{twin, H * i4}, {edge_class, H}, {flip, N}, {patch_root, N * i4}, {patch, N * i4}, {proot, N * i4}, {psize, N * i4},
                          {pflags, N}, {vol6, N * sizeof(int64_t)}, {summary, 8 * sizeof(int64_t)}, {work, ezrt_orient_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      OrientArgs a{};
      a.tri_geom = s->tri_geom.p, a.n_tri = (int32_t)n_tri;
      a.twin = twin, a.edge_class = edge_class, a.outward = outward != 0 ? 1 : 0;
      orient_layout(work, n_tri, a);
      a.flip = flip, a.patch_root = patch_root, a.patch = patch, a.proot = proot, a.psize = psize, a.pflags = pflags;
      a.vol6 = (long long*)vol6, a.summary = (unsigned long long*)summary;
      const dim3 b(OR_BLOCK), gh = mesh_grid(H, OR_BLOCK), gt = mesh_grid(N, OR_BLOCK);
      hipLaunchKernelGGL(orient_init_kernel, gt, b, 0, st, a);
      hipLaunchKernelGGL(orient_union_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(orient_flatten_kernel, gt, b, 0, st, a);
      hipLaunchKernelGGL(orient_check_kernel, gt, b, 0, st, a);
      scan_tiled(st, a.scan, a.tiles, scan_tile_count(N), nullptr, (long long)N); // the roots' flags, in place
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
    return query_call(s, {{tri36, N * ROW_BYTES}, {flip, N}}, N, st, [&](dim3, dim3) {
      hipLaunchKernelGGL(rewind_kernel, mesh_blocks(N, OR_BLOCK), dim3(OR_BLOCK), 0, st, tri36, (uint32_t)n_tri, flip);
    });
  });
}

// ---- boundary loops on device memory (include/ezrt_boundary.h): 17 launches and the rounds of the ranking on `st` -- init, next,
// union, open, a prefix sum (scan_tiled) that compacts the BOUNDARY half-edges, rank init, ceil(log2(3 n_tri)) jumping rounds, flag, the
// prefix sum over the compacted list that numbers the heads, number, the prefix sum of the lengths, scatter -- over the caller's
// `work`: scan_c and scan_n (3 n_tri + 1 int64 each), tiles (one int64 per 2048 half-edges, and one), the two buffers of the ranking
// (3 n_tri int64 each), four int64 of counts, then pred, par and comp (3 n_tri ints each); open lies over scan_n and lens over scan_c.
// One launch for the cap.  Checked, launched and ordered against a refit by query_call.
static size_t boundary_layout(void* work, int n_tri, BoundaryArgs& a) {
  const uint64_t H = 3ull * (uint64_t)n_tri;
  WorkCarver w(work);
  a.scan_c = w.take<long long>(H + 1), a.scan_n = w.take<long long>(H + 1);
  a.tiles = w.take<long long>(scan_tile_count(H) + 1);
  a.jump[0] = w.take<unsigned long long>(H), a.jump[1] = w.take<unsigned long long>(H);
  a.cnt = w.take<long long>(4);
  a.pred = w.take<int32_t>(H), a.par = w.take<uint32_t>(H), a.comp = w.take<int32_t>(H);
  a.open = (uint32_t*)a.scan_n, a.lens = a.scan_c;
  return w.bytes();
}
size_t ezrt_boundary_work_bytes(int n_tri) {
  BoundaryArgs a{};
  return n_tri <= 0 ? 8 : boundary_layout(nullptr, n_tri, a);
}
int ezrt_mesh_boundary_device(EzrtScene* s, const int32_t* twin, const uint8_t* edge_class, int32_t* next, int32_t* loop, int32_t* pos,
                              int32_t* order, int32_t* loop_offsets, uint8_t* lflags, int64_t* area2, int64_t* summary, void* work,
                              size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_mesh_boundary_device", [&]() -> int {
    if (!s || !twin || !edge_class || !next || !loop || !pos || !order || !loop_offsets || !lflags || !summary || !work)
      return fail(EZRT_ERR_INVALID, "NULL argument");
    if ((int64_t)s->n_tri > (int64_t)(INT32_MAX / 3)) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 triangles");
    const int n_tri = (int)s->n_tri;
    if (int rc = work_check(work, work_bytes, ezrt_boundary_work_bytes(n_tri), "ezrt_boundary_work_bytes(n_tri)")) return rc;
    if (n_tri <= 0) return 0;
    const size_t N = (size_t)n_tri, H = 3 * N, i4 = sizeof(int32_t), i8 = sizeof(int64_t);
    hipStream_t st = (hipStream_t)stream;
    // (a null area2 is skipped by the check, as a null input of the overlap lists is)
    return query_call(s, {{twin, H * i4}, {edge_class, H}, {next, H * i4}, {loop, H * i4}, {pos, H * i4}, {order, H * i4},
                          {loop_offsets, (H + 1) * i4}, {lflags, H}, {area2, 3 * H * i8}, {summary, 8 * i8},
                          {work, ezrt_boundary_work_bytes(n_tri)}},
                      H, st, [&](dim3, dim3) {
      BoundaryArgs a{};
      a.tri_geom = s->tri_geom.p, a.n_tri = (int32_t)n_tri;
      a.twin = twin, a.edge_class = edge_class;
      boundary_layout(work, n_tri, a);
      int rounds = 0;
      while ((1ull << rounds) < (uint64_t)H) rounds++; // ceil(log2(3 n_tri)): at most 32
      a.rounds = rounds;
      a.next = next, a.loop = loop, a.pos = pos, a.order = order, a.loop_offsets = loop_offsets, a.lflags = lflags;
      a.area2 = (long long*)area2, a.summary = (unsigned long long*)summary;
      const uint64_t T = scan_tile_count(H);
      const dim3 b(BD_BLOCK), g = mesh_grid(H, BD_BLOCK);
      hipLaunchKernelGGL(bd_init_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(bd_next_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(bd_union_kernel, g, b, 0, st, a);
      hipLaunchKernelGGL(bd_open_kernel, g, b, 0, st, a);
      scan_tiled(st, a.scan_c, a.tiles, T, nullptr, (long long)H);
      hipLaunchKernelGGL(bd_rank_init_kernel, g, b, 0, st, a);
      for (int r = 0; r < rounds; r++) hipLaunchKernelGGL(bd_jump_kernel, g, b, 0, st, a, r & 1); // rounds are separated by launches
      hipLaunchKernelGGL(bd_flag_kernel, g, b, 0, st, a);
      scan_tiled(st, a.scan_n, a.tiles, T, a.cnt, (long long)H); // the lengths of this one and the next are read on the device
      hipLaunchKernelGGL(bd_number_kernel, g, b, 0, st, a);
      scan_tiled(st, a.lens, a.tiles, T, a.cnt + 1, (long long)H);
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
    return query_call(s, {{tri36, N * ROW_BYTES}, {order, H * i4}, {loop, H * i4}, {pos, H * i4}, {loop_offsets, (H + 1) * i4},
                          {lflags, H}, {summary, 8 * sizeof(int64_t)}, {cap, H * ROW_BYTES}, {cap_valid, H}},
                      H, st, [&](dim3, dim3) {
      hipLaunchKernelGGL(cap_rows_kernel, mesh_blocks(H, BD_BLOCK), dim3(BD_BLOCK), 0, st, tri36, (int32_t)n_tri, order, loop, pos, loop_offsets,
                         lflags, (const long long*)summary, cap, cap_valid);
    });
  });
}

// ---- plane clipping on device memory (include/ezrt_clip.h).  Count: a memset of the summary, clip_count_kernel, and the tiled prefix
// sum (scan_tiled) of offsets in place over the caller's `work`, the tiles' sums and their total.  Fill: one launch, the staged
// instance where tri36 and out are 16-byte aligned, else the per-lane one (always, in the measurement variant EZRT_CLIP_PER_LANE).
// Checked, launched and ordered against a refit by query_call; the scene's records are not read.
#ifndef EZRT_CLIP_PER_LANE
#define EZRT_CLIP_PER_LANE 0
#endif
static size_t clip_layout(void* work, int n_rows, long long*& tiles) {
  WorkCarver w(work);
  tiles = w.take<long long>(scan_tile_count((uint64_t)n_rows) + 1);
  return w.bytes();
}
size_t ezrt_clip_work_bytes(int n_rows) {
  long long* tiles;
  return n_rows <= 0 ? 8 : clip_layout(nullptr, n_rows, tiles);
}
int ezrt_clip_count_device(EzrtScene* s, const float* tri36, int n_rows, const float* plane4, int64_t* offsets, int64_t* summary, void* work,
                           size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_clip_count_device", [&]() -> int {
    if (!s || !tri36 || !plane4 || !offsets || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 2) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 2 rows");
    if (int rc = work_check(work, work_bytes, ezrt_clip_work_bytes(n_rows), "ezrt_clip_work_bytes(n_rows)")) return rc;
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, i8 = sizeof(int64_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * ROW_BYTES}, {plane4, 4 * sizeof(float)}, {offsets, (N + 1) * i8}, {summary, 8 * i8},
                          {work, ezrt_clip_work_bytes(n_rows)}},
                      N, st, [&](dim3, dim3) -> int {
      long long *x = (long long*)offsets, *tiles;
      clip_layout(work, n_rows, tiles);
      HIP_TRY(hipMemsetAsync(summary, 0, 8 * i8, st));
      hipLaunchKernelGGL(clip_count_kernel, mesh_blocks(N, CL_BLOCK), dim3(CL_BLOCK), 0, st, tri36, (int32_t)n_rows, plane4, x,
                         (unsigned long long*)summary);
      scan_tiled(st, x, tiles, scan_tile_count(N), nullptr, (long long)N); // the counts, in place; the total lands in offsets[n_rows]
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
    if (int rc = capacity_check(capacity, out)) return rc;
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, cap = (size_t)capacity;
    if (int rc = overlap_check(tri36, N, out, cap)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * ROW_BYTES}, {plane4, 4 * sizeof(float)}, {offsets, (N + 1) * sizeof(int64_t)},
                          {cap ? out : nullptr, cap * ROW_BYTES}, {cap ? src : nullptr, cap * sizeof(int32_t)}, {cap ? cut_edge : nullptr, cap}},
                      N, st, [&](dim3, dim3) {
      if (cap == 0) return; // nothing fits: nothing is written
      ClipFillArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.plane4 = plane4, a.offsets = (const long long*)offsets, a.capacity = (long long)capacity;
      a.out = out, a.src = src, a.cut_edge = cut_edge;
      const dim3 g = mesh_blocks(N, CL_BLOCK), b(CL_BLOCK);
      if (fill_staged(EZRT_CLIP_PER_LANE, tri36, out)) hipLaunchKernelGGL(clip_fill_kernel<true>, g, b, 0, st, a);
      else hipLaunchKernelGGL(clip_fill_kernel<false>, g, b, 0, st, a);
    });
  });
}

// ---- subdivision on device memory (include/ezrt_subdivide.h): a memset of the summary, in Loop mode subdiv_vertex_kernel over the
// caller's `work` (four words per possible vertex; in either mode one int64 behind them that nobody touches: no buffer is empty), and
// one fill launch, the staged instance where tri36 and out are 16-byte aligned, else the per-lane one (always, in the measurement
// variant EZRT_SUBDIV_PER_LANE).  The output's size is known, so there is no count.  Checked, launched and ordered against a refit by
// query_call; the scene's records are not read.
#ifndef EZRT_SUBDIV_PER_LANE
#define EZRT_SUBDIV_PER_LANE 0
#endif
#ifndef EZRT_SUBDIV_SKIP_VERTEX // measurement variant: Loop mode without its vertex pass, for timing the fill alone (the slots are whatever `work` held)
#define EZRT_SUBDIV_SKIP_VERTEX 0
#endif
static size_t subdiv_layout(void* work, int n_rows, int mode, SubdivArgs& a) {
  WorkCarver w(work);
  a.slot = w.take<uint32_t>(mode == EZRT_SUBDIVIDE_LOOP ? 4 * 3ull * (uint64_t)n_rows : 0);
  w.take<int64_t>(1);
  return w.bytes();
}
size_t ezrt_subdivide_work_bytes(int n_rows, int mode) {
  SubdivArgs a{};
  return n_rows <= 0 ? 8 : subdiv_layout(nullptr, n_rows, mode, a);
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
    if (int rc = work_check(work, work_bytes, ezrt_subdivide_work_bytes(n_rows, mode), "ezrt_subdivide_work_bytes(n_rows, mode)")) return rc;
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, H = 3 * N, i4 = sizeof(int32_t);
    if (int rc = overlap_check(tri36, N, out, 4 * N)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * ROW_BYTES}, {out, 4 * N * ROW_BYTES}, {summary, 8 * sizeof(int64_t)},
                          {work, ezrt_subdivide_work_bytes(n_rows, mode)}, {twin, H * i4}, {edge_class, H}, {vertex, H * i4},
                          {star_offsets, (H + 1) * i4}, {star, H * i4}, {vert_flags, H}},
                      N, st, [&](dim3, dim3) -> int {
      SubdivArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.mode = (int32_t)mode;
      a.twin = twin, a.edge_class = edge_class, a.vertex = vertex, a.star_offsets = star_offsets, a.star = star, a.vert_flags = vert_flags;
      a.out = out, a.summary = (unsigned long long*)summary;
      subdiv_layout(work, n_rows, mode, a);
      HIP_TRY(hipMemsetAsync(summary, 0, 8 * sizeof(int64_t), st));
      const dim3 b(SD_BLOCK);
      if (mode == EZRT_SUBDIVIDE_LOOP && !EZRT_SUBDIV_SKIP_VERTEX) hipLaunchKernelGGL(subdiv_vertex_kernel, mesh_blocks(H, SD_BLOCK), b, 0, st, a);
      if (fill_staged(EZRT_SUBDIV_PER_LANE, tri36, out))
        hipLaunchKernelGGL(subdiv_fill_kernel<true>, dim3((unsigned)std::min<uint64_t>((N + SD_TILE - 1) / SD_TILE, SD_GRID_MAX)), b, 0, st, a);
      else hipLaunchKernelGGL(subdiv_fill_kernel<false>, mesh_blocks(N, SD_BLOCK), b, 0, st, a);
      return 0;
    });
  });
}

// ---- decimation on device memory (include/ezrt_decimate.h).  Count: init, insert, flag, the tiled prefix sum (scan_tiled) over the
// corners, cells, with EZRT_DECIMATE_DEDUP classify, keep, and the prefix sum again over the rows, in place in offsets -- up to twelve
// launches over the caller's `work`: ids (3 n_rows + 1 int64), tiles (one int64 per 2048 corners, and one), key (T int64, T the
// topology's power of two >= 6 n_rows), sum (3 T int64), cnt, low (T ints each), mn, mx (3 T ints each), slot (3 n_rows ints), rep2
// (T2 ints, T2 the power of two >= 2 n_rows), slot2 (n_rows ints).  Fill: one launch, the staged instance where tri36 and out are
// 16-byte aligned, else the per-lane one (always, in the measurement variant EZRT_DECIMATE_PER_LANE).  Checked, launched and ordered
// against a refit by query_call; the scene's records are not read.
#ifndef EZRT_DECIMATE_PER_LANE
#define EZRT_DECIMATE_PER_LANE 0
#endif
static size_t dec_layout(void* work, int n_rows, DecArgs& a) {
  const uint64_t N = (uint64_t)n_rows, H = 3 * N;
  WorkCarver w(work);
  a.T = table_slots(6 * N), a.T2 = table_slots(2 * N);
  a.ids = w.take<long long>(H + 1);
  a.tiles = w.take<long long>(scan_tile_count(H) + 1);
  a.key = w.take<unsigned long long>(a.T), a.sum = w.take<unsigned long long>(3 * a.T);
  a.cnt = w.take<uint32_t>(a.T), a.low = w.take<int32_t>(a.T);
  a.mn = w.take<uint32_t>(3 * a.T), a.mx = w.take<uint32_t>(3 * a.T);
  a.slot = w.take<uint32_t>(H);
  a.rep2 = w.take<int32_t>(a.T2), a.slot2 = w.take<uint32_t>(N);
  return w.bytes();
}
size_t ezrt_decimate_work_bytes(int n_rows) {
  DecArgs a{};
  return n_rows <= 0 ? 8 : dec_layout(nullptr, n_rows, a);
}
int ezrt_decimate_count_device(EzrtScene* s, const float* tri36, int n_rows, const float* grid4, int flags, int32_t* cell, int32_t* cell_corner,
                               float* cell_point, int64_t* offsets, int64_t* summary, void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_decimate_count_device", [&]() -> int {
    if (!s || !tri36 || !grid4 || !cell || !cell_corner || !cell_point || !offsets || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 rows");
    if (flags & ~EZRT_DECIMATE_DEDUP) return fail(EZRT_ERR_INVALID, "flags %d has a bit that is not EZRT_DECIMATE_DEDUP", flags);
    if (int rc = work_check(work, work_bytes, ezrt_decimate_work_bytes(n_rows), "ezrt_decimate_work_bytes(n_rows)")) return rc;
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, H = 3 * N, i4 = sizeof(int32_t), i8 = sizeof(int64_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * ROW_BYTES}, {grid4, 4 * sizeof(float)}, {cell, H * i4}, {cell_corner, H * i4},
                          {cell_point, H * 3 * sizeof(float)}, {offsets, (N + 1) * i8}, {summary, 8 * i8}, {work, ezrt_decimate_work_bytes(n_rows)}},
                      H, st, [&](dim3, dim3) {
      DecArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.grid4 = grid4, a.flags = (int32_t)flags;
      dec_layout(work, n_rows, a);
      a.cell = cell, a.cell_corner = cell_corner, a.cell_point = cell_point, a.offsets = (long long*)offsets;
      a.summary = (unsigned long long*)summary;
      const dim3 b(DC_BLOCK), gh = mesh_grid(H, DC_BLOCK);
      hipLaunchKernelGGL(dec_init_kernel, mesh_grid(3 * a.T, DC_BLOCK), b, 0, st, a);
      hipLaunchKernelGGL(dec_insert_kernel, gh, b, 0, st, a);
      hipLaunchKernelGGL(dec_flag_kernel, gh, b, 0, st, a);
      scan_tiled(st, a.ids, a.tiles, scan_tile_count(H), nullptr, (long long)H);
      hipLaunchKernelGGL(dec_cells_kernel, gh, b, 0, st, a);
      if (flags & EZRT_DECIMATE_DEDUP) hipLaunchKernelGGL(dec_classify_kernel, mesh_grid(N, DC_BLOCK), b, 0, st, a);
      hipLaunchKernelGGL(dec_keep_kernel, mesh_blocks(N, DC_BLOCK), b, 0, st, a);
      scan_tiled(st, a.offsets, a.tiles, scan_tile_count(N), nullptr, (long long)N); // the rows kept, in place; the total in offsets[n_rows]
    });
  });
}
int ezrt_decimate_rows_device(EzrtScene* s, const float* tri36, int n_rows, const int32_t* cell, const float* cell_point, const int64_t* offsets,
                              int64_t capacity, float* out, int32_t* src, void* stream) {
  return ezi::guarded("ezrt_decimate_rows_device", [&]() -> int {
    if (!s || !tri36 || !cell || !cell_point || !offsets) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 rows");
    if (int rc = capacity_check(capacity, out)) return rc;
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, H = 3 * N, cap = (size_t)capacity;
    if (int rc = overlap_check(tri36, N, out, cap)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * ROW_BYTES}, {cell, H * sizeof(int32_t)}, {cell_point, H * 3 * sizeof(float)}, {offsets, (N + 1) * sizeof(int64_t)},
                          {cap ? out : nullptr, cap * ROW_BYTES}, {cap ? src : nullptr, cap * sizeof(int32_t)}},
                      N, st, [&](dim3, dim3) {
      if (cap == 0) return; // nothing fits: nothing is written
      DecFillArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.cell = cell, a.cell_point = cell_point, a.offsets = (const long long*)offsets;
      a.capacity = (long long)capacity, a.out = out, a.src = src;
      const dim3 g = mesh_blocks(N, DC_BLOCK), b(DC_BLOCK);
      if (fill_staged(EZRT_DECIMATE_PER_LANE, tri36, out)) hipLaunchKernelGGL(dec_fill_kernel<true>, g, b, 0, st, a);
      else hipLaunchKernelGGL(dec_fill_kernel<false>, g, b, 0, st, a);
    });
  });
}

// ---- isosurface extraction on device memory (include/ezrt_isosurface.h).  Count: a memset of the summary, iso_count_kernel with a
// workgroup per block of 256 cells, and the tiled prefix sum (scan_tiled) of offsets in place over the caller's `work`, the tiles'
// sums and their total.  Fill: one launch with a workgroup per block, the staged instance where out is 16-byte aligned, else the
// per-lane one (always, in the measurement variant EZRT_ISO_PER_LANE).  Checked, launched and ordered against a refit by query_call;
// the scene's records are not read.
#ifndef EZRT_ISO_PER_LANE
#define EZRT_ISO_PER_LANE 0
#endif
// the cells of a grid whose dimensions are >= 1 and whose vertices are at most INT32_MAX
static uint64_t iso_cells(int nx, int ny, int nz) { return (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1); }
static uint64_t iso_blocks(uint64_t n_cells) { return (n_cells + ISO_BLOCK - 1) / ISO_BLOCK; }
// what both calls reject in the dimensions
static int iso_dims_check(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1) return fail(EZRT_ERR_INVALID, "a dimension < 1");
  if ((uint64_t)nx * (uint64_t)ny * (uint64_t)nz > (uint64_t)INT32_MAX) return fail(EZRT_ERR_INVALID, "nx ny nz exceeds INT32_MAX");
  return 0;
}
static size_t iso_layout(void* work, uint64_t n_blocks, long long*& tiles) {
  WorkCarver w(work);
  tiles = w.take<long long>(scan_tile_count(n_blocks) + 1);
  return w.bytes();
}
size_t ezrt_iso_work_bytes(int nx, int ny, int nz) {
  long long* tiles;
  if (nx < 2 || ny < 2 || nz < 2) return 8;
  // (a grid the calls reject for its size counts as the largest they take: the function stays monotone and never wraps)
  const unsigned __int128 cells = (unsigned __int128)iso_cells(nx, ny, 2) * (unsigned __int128)(nz - 1);
  return iso_layout(nullptr, iso_blocks(cells > (unsigned __int128)INT32_MAX ? (uint64_t)INT32_MAX : (uint64_t)cells), tiles);
}
int ezrt_iso_count_device(EzrtScene* s, const float* values, int nx, int ny, int nz, const float* grid8, int64_t* offsets, int64_t* summary,
                          void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_iso_count_device", [&]() -> int {
    if (!s || !values || !grid8 || !offsets || !summary || !work) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (int rc = iso_dims_check(nx, ny, nz)) return rc;
    if (int rc = work_check(work, work_bytes, ezrt_iso_work_bytes(nx, ny, nz), "ezrt_iso_work_bytes(nx, ny, nz)")) return rc;
    const uint64_t n_cells = iso_cells(nx, ny, nz), B = iso_blocks(n_cells);
    if (n_cells == 0) return 0;
    const size_t n_values = (size_t)nx * (size_t)ny * (size_t)nz, i8 = sizeof(int64_t);
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{values, n_values * sizeof(float)}, {grid8, 8 * sizeof(float)}, {offsets, (B + 1) * i8}, {summary, 8 * i8},
                          {work, ezrt_iso_work_bytes(nx, ny, nz)}},
                      n_cells, st, [&](dim3, dim3) -> int {
      long long *x = (long long*)offsets, *tiles;
      iso_layout(work, B, tiles);
      HIP_TRY(hipMemsetAsync(summary, 0, 8 * i8, st));
      hipLaunchKernelGGL(iso_count_kernel, dim3((unsigned)B), dim3(ISO_BLOCK), 0, st, values, nx, ny, (uint32_t)n_cells, grid8, x,
                         (unsigned long long*)summary);
      scan_tiled(st, x, tiles, scan_tile_count(B), nullptr, (long long)B); // the blocks' counts, in place; the total lands in offsets[n_blocks]
      return 0;
    });
  });
}
int ezrt_iso_rows_device(EzrtScene* s, const float* values, int nx, int ny, int nz, const float* grid8, const float* material18,
                         const int64_t* offsets, int64_t capacity, float* out, int32_t* cell, void* stream) {
  return ezi::guarded("ezrt_iso_rows_device", [&]() -> int {
    if (!s || !values || !grid8 || !material18 || !offsets) return fail(EZRT_ERR_INVALID, "NULL argument");
    if (int rc = iso_dims_check(nx, ny, nz)) return rc;
    if (int rc = capacity_check(capacity, out)) return rc;
    const uint64_t n_cells = iso_cells(nx, ny, nz), B = iso_blocks(n_cells);
    if (n_cells == 0) return 0;
    const size_t n_values = (size_t)nx * (size_t)ny * (size_t)nz, cap = (size_t)capacity;
    const uintptr_t v0 = (uintptr_t)values, v1 = v0 + n_values * sizeof(float), o0 = (uintptr_t)out, o1 = o0 + cap * ROW_BYTES;
    if (out && cap > 0 && v0 < o1 && o0 < v1) return fail(EZRT_ERR_INVALID, "out overlaps values");
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{values, n_values * sizeof(float)}, {grid8, 8 * sizeof(float)}, {material18, 18 * sizeof(float)},
                          {offsets, (B + 1) * sizeof(int64_t)}, {cap ? out : nullptr, cap * ROW_BYTES}, {cap ? cell : nullptr, cap * sizeof(int32_t)}},
                      n_cells, st, [&](dim3, dim3) {
      if (cap == 0) return; // nothing fits: nothing is written
      IsoFillArgs a{};
      a.values = values, a.nx = (int32_t)nx, a.ny = (int32_t)ny, a.n_cells = (uint32_t)n_cells, a.grid8 = grid8, a.material18 = material18;
      a.offsets = (const long long*)offsets, a.capacity = (long long)capacity, a.out = out, a.cell = cell;
      const dim3 g((unsigned)B), b(ISO_BLOCK);
      if (fill_staged(EZRT_ISO_PER_LANE, out, out)) hipLaunchKernelGGL(iso_fill_kernel<true>, g, b, 0, st, a);
      else hipLaunchKernelGGL(iso_fill_kernel<false>, g, b, 0, st, a);
    });
  });
}

// ---- smoothing on device memory (include/ezrt_smooth.h): a memset of the summary; the plan -- smooth_plan_kernel, the tiled prefix
// sum (scan_tiled) of the workgroups' counts, smooth_terms_kernel -- over the caller's `work`: counts (one int64 per 256 corners, and
// one), tiles (one int64 per 2048 counts, and one), the two position buffers (9 n_rows floats each), term (6 n_rows words), rec (9 n_rows
// words), state (3 n_rows bytes); the steps, one launch each or, where the rows fit tile_rows, one launch of one workgroup for all of
// them; and one fill launch, the staged instance where tri36 and out are 16-byte aligned, else the per-lane one.  Checked, launched
// and ordered against a refit by query_call; the scene's records are not read.
static size_t smooth_layout(void* work, int n_rows, SmoothArgs& a) {
  const uint64_t H = 3ull * (uint64_t)n_rows, B = (H + SM_BLOCK - 1) / SM_BLOCK;
  WorkCarver w(work);
  a.counts = w.take<long long>(B + 1);
  a.tiles = w.take<long long>(scan_tile_count(B) + 1);
  a.pos[0] = w.take<float>(3 * H), a.pos[1] = w.take<float>(3 * H);
  a.term = w.take<uint32_t>(2 * H), a.rec = w.take<uint32_t>(3 * H);
  a.state = w.take<uint8_t>(H);
  return w.bytes();
}
size_t ezrt_smooth_work_bytes(int n_rows) {
  SmoothArgs a{};
  // (a count the call rejects for its size counts as the largest it takes: the function stays monotone)
  return n_rows <= 0 ? 8 : smooth_layout(nullptr, std::min(n_rows, INT32_MAX / 3), a);
}
void ezrt_smooth_limits(int* tile_rows_max) {
  if (tile_rows_max) *tile_rows_max = SM_TILE_MAX;
}
int ezrt_smooth_rows_device(EzrtScene* s, const float* tri36, int n_rows, const uint8_t* edge_class, const int32_t* vertex,
                            const int32_t* star_offsets, const int32_t* star, const uint8_t* vert_flags, int steps, float lambda, float mu,
                            int flags, int tile_rows, float* out, int64_t* summary, void* work, size_t work_bytes, void* stream) {
  return ezi::guarded("ezrt_smooth_rows_device", [&]() -> int {
    if (!s || !tri36 || !edge_class || !vertex || !star_offsets || !star || !vert_flags || !out || !summary || !work)
      return fail(EZRT_ERR_INVALID, "NULL argument");
    if (n_rows < 0) return fail(EZRT_ERR_INVALID, "n_rows < 0");
    if (n_rows > INT32_MAX / 3) return fail(EZRT_ERR_INVALID, "more than INT32_MAX / 3 rows");
    if (steps < 1 || steps > EZRT_SMOOTH_STEPS_MAX) return fail(EZRT_ERR_INVALID, "steps %d is outside 1 .. EZRT_SMOOTH_STEPS_MAX", steps);
    if (!std::isfinite(lambda) || !std::isfinite(mu)) return fail(EZRT_ERR_INVALID, "lambda or mu is not finite");
    if (flags & ~EZRT_SMOOTH_PIN_BORDER) return fail(EZRT_ERR_INVALID, "flags %d has a bit that is not EZRT_SMOOTH_PIN_BORDER", flags);
    if (tile_rows < 0) return fail(EZRT_ERR_INVALID, "tile_rows < 0");
    if (int rc = work_check(work, work_bytes, ezrt_smooth_work_bytes(n_rows), "ezrt_smooth_work_bytes(n_rows)")) return rc;
    if (n_rows == 0) return 0;
    const size_t N = (size_t)n_rows, H = 3 * N, i4 = sizeof(int32_t);
    if (out != tri36) // the same rows exactly: in place
      if (int rc = overlap_check(tri36, N, out, N)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return query_call(s, {{tri36, N * ROW_BYTES}, {out, N * ROW_BYTES}, {summary, 8 * sizeof(int64_t)}, {work, ezrt_smooth_work_bytes(n_rows)},
                          {edge_class, H}, {vertex, H * i4}, {star_offsets, (H + 1) * i4}, {star, H * i4}, {vert_flags, H}},
                      N, st, [&](dim3, dim3) -> int {
      SmoothArgs a{};
      a.tri36 = tri36, a.n_rows = (int32_t)n_rows, a.steps = (int32_t)steps, a.flags = (int32_t)flags, a.lambda = lambda, a.mu = mu;
      a.edge_class = edge_class, a.vertex = vertex, a.star_offsets = star_offsets, a.star = star, a.vert_flags = vert_flags;
      a.out = out, a.summary = (unsigned long long*)summary;
      smooth_layout(work, n_rows, a);
      HIP_TRY(hipMemsetAsync(summary, 0, 8 * sizeof(int64_t), st));
      const uint64_t B = (H + SM_BLOCK - 1) / SM_BLOCK;
      const dim3 b(SM_BLOCK), gh((unsigned)B);
      hipLaunchKernelGGL(smooth_plan_kernel, gh, b, 0, st, a);
      scan_tiled(st, a.counts, a.tiles, scan_tile_count(B), nullptr, (long long)B); // the counts, in place; the total lands in counts[B]
      hipLaunchKernelGGL(smooth_terms_kernel, gh, b, 0, st, a);
      const int tile = tile_rows == 0 || tile_rows > SM_TILE_MAX ? SM_TILE_MAX : tile_rows;
      if (n_rows <= tile) {
        hipLaunchKernelGGL(smooth_steps_lds_kernel, dim3(1), dim3(SM_LDS_BLOCK), 0, st, a);
      } else {
        const dim3 gs((unsigned)std::min<uint64_t>(B, SM_GRID_MAX));
        for (int j = 0; j < steps; j++) hipLaunchKernelGGL(smooth_step_kernel, gs, b, 0, st, a, (int32_t)j); // steps are separated by launches
      }
      if (fill_staged(false, tri36, out))
        hipLaunchKernelGGL(smooth_fill_kernel<true>, dim3((unsigned)std::min<uint64_t>((N + SM_FILL_TILE - 1) / SM_FILL_TILE, SM_GRID_MAX)), b, 0, st, a);
      else hipLaunchKernelGGL(smooth_fill_kernel<false>, mesh_blocks(N, SM_BLOCK), b, 0, st, a);
      return 0;
    });
  });
}
} // extern "C"
