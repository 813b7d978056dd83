// ezrt_query_kernels.h -- the gfx950 kernels of the device queries that are one launch on the caller's stream (ezrt_queries.hip, the
// only file that includes this): shading queries (include/ezrt_shade.h), path queries (include/ezrt_path.h), all-hits queries and
// surface_at (include/ezrt_multihit.h).  The point and box queries have a header of their own, ezrt_point_queries.h.
#pragma once
#include "ezrt_device.h"
#include "ezrt_records.h"
#include "ezrt_path_device.h"

namespace ezd {

// ---- shading queries (include/ezrt_shade.h): one element per lane, operands and results in the caller's device arrays.  The
// material of an element is the table row of its triangle, reached as shade_point reaches it: the third texel of the triangle's
// shade record holds the material index, and the row's 16-byte loads are issued right behind that load, ahead of the arithmetic.
// Every kernel is specialised at compile time for what it evaluates (the integrator, the outputs asked for): no lane carries a
// runtime switch, the registers of a lobe it never evaluates, or the loads of a row it never reads.
//
// The table row of triangle `tri`, or false for a miss / an id beyond the scene (the element's outputs are zeros then).  ROWS: how
// many of the row's MAT_REC_FLOAT4 texels are loaded, from the first; the others are zeros.
template <int ROWS>
EZD bool shade_mat_row(const float4* tri_shade, const float4* mat_table, int32_t n_tri, int32_t tri, float4 (&m)[MAT_REC_FLOAT4]) {
  if ((uint32_t)tri >= (uint32_t)n_tri) return false;
  const float4 r2 = tri_shade[(size_t)tri * SHADE_REC_FLOAT4 + 2];
  const float4* mq = mat_table + (size_t)__float_as_uint(r2.y) * MAT_REC_FLOAT4;
#pragma unroll
  for (int k = 0; k < MAT_REC_FLOAT4; k++) m[k] = k < ROWS ? mq[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return true;
}

// ezrt_query_material_device: the 18 floats the row starts with (texels 0-4; mat_pack_row)
__global__ __launch_bounds__(256) void shade_material_kernel(const float4* tri_shade, const float4* mat_table, int32_t n_tri,
                                                             const int32_t* tri_id, uint32_t n, float* mat18) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 m[MAT_REC_FLOAT4];
  const bool ok = shade_mat_row<5>(tri_shade, mat_table, n_tri, tri_id[i], m);
  float* o = mat18 + (size_t)i * 18;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    o[4 * k + 0] = ok ? m[k].x : 0.0f;
    o[4 * k + 1] = ok ? m[k].y : 0.0f;
    o[4 * k + 2] = ok ? m[k].z : 0.0f;
    o[4 * k + 3] = ok ? m[k].w : 0.0f;
  }
  o[16] = ok ? m[4].x : 0.0f;
  o[17] = ok ? m[4].y : 0.0f;
}

// ezrt_shade_eval_device: f_r and pdf of the direction L as the bounce loop of integrator INTEG computes them for its rayL
// (ezrt_wavefront.h "start bounce b").  Integrator 3 reads baseColor alone: the row's first two texels.
template <int INTEG, bool WANT_PDF>
__global__ __launch_bounds__(256) void shade_eval_kernel(const float4* tri_shade, const float4* mat_table, int32_t n_tri,
                                                         const int32_t* tri_id, const float* Vp, const float* Np, const float* Lp,
                                                         uint32_t n, float* f_out, float* pdf_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr bool MIS = integ_mis<INTEG>();
  float4 q[MAT_REC_FLOAT4];
  const bool ok = shade_mat_row<INTEG == EZRT_INTEGRATOR_P3_DIFFUSE ? 2 : MAT_REC_FLOAT4>(tri_shade, mat_table, n_tri, tri_id[i], q);
  f3 f_r = mk(0, 0, 0);
  float pdf = 0.0f;
  if (ok) {
    Mat m;
    mat_unpack_row(m, q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
    const f3 V = ld3(Vp + (size_t)i * 3), N = ld3(Np + (size_t)i * 3), L = ld3(Lp + (size_t)i * 3);
    if (MIS) {
      constexpr bool ANISO_IS = integ_aniso_is<INTEG>();
      f3 X = mk(0, 0, 0), Y = mk(0, 0, 0);
      if (ANISO_IS) get_tangent(N, X, Y);
      brdf_evaluate_pdf<ANISO_IS>(V, N, L, X, Y, m, f_r, pdf);
    } else {
      pdf = 1.0f / (2.0f * PI);
      if (INTEG == EZRT_INTEGRATOR_P3_DIFFUSE) {
        f_r = m.baseColor / PI;
      } else {
        f3 tangent, bitangent;
        get_tangent(N, tangent, bitangent);
        f_r = brdf_evaluate<INTEG == EZRT_INTEGRATOR_P4_DISNEY>(V, N, L, tangent, bitangent, m);
      }
    }
  }
  st3(f_out + (size_t)i * 3, f_r);
  if (WANT_PDF) pdf_out[i] = pdf;
}

// ezrt_shade_sample_device: the direction the bounce loop of integrator INTEG continues in.  Without MIS (3, 4, 50: one
// instantiation) it is the uniform hemisphere about N and no material is read.
template <int INTEG>
__global__ __launch_bounds__(256) void shade_sample_kernel(const float4* tri_shade, const float4* mat_table, int32_t n_tri,
                                                           const int32_t* tri_id, const float* xip, const float* Vp, const float* Np,
                                                           uint32_t n, float* L_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr bool MIS = integ_mis<INTEG>();
  const int32_t tri = tri_id[i];
  f3 L = mk(0, 0, 0);
  if (MIS) {
    float4 q[MAT_REC_FLOAT4];
    if (shade_mat_row<MAT_REC_FLOAT4>(tri_shade, mat_table, n_tri, tri, q)) {
      Mat m;
      mat_unpack_row(m, q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
      constexpr bool ANISO_IS = integ_aniso_is<INTEG>();
      const float* xi = xip + (size_t)i * 3;
      const f3 V = ld3(Vp + (size_t)i * 3), N = ld3(Np + (size_t)i * 3);
      f3 X = mk(0, 0, 0), Y = mk(0, 0, 0);
      if (ANISO_IS) get_tangent(N, X, Y);
      L = ANISO_IS ? sample_brdf_aniso(xi[0], xi[1], xi[2], V, N, X, Y, m) : sample_brdf(xi[0], xi[1], xi[2], V, N, m);
    }
  } else if ((uint32_t)tri < (uint32_t)n_tri) {
    const float* xi = xip + (size_t)i * 3;
    L = to_normal_hemisphere(sample_hemisphere(xi[0], xi[1]), ld3(Np + (size_t)i * 3));
  }
  st3(L_out + (size_t)i * 3, L);
}

// ezrt_env_eval_device: hdr_color and / or hdr_pdf of L; both = the fused lookup of the MIS loops
template <bool COLOUR, bool WANT_PDF>
__global__ __launch_bounds__(256) void env_eval_kernel(DevScene sc, const float* Lp, uint32_t n, float env_clamp, float* colour,
                                                       float* pdf_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Counters ctr = {0, 0, 0, 0, 0, 0, 0};
  const f3 L = ld3(Lp + (size_t)i * 3);
  f3 c = mk(0, 0, 0);
  float pdf = 0.0f;
  if (COLOUR && WANT_PDF) hdr_color_pdf<false>(sc, L, env_clamp, ctr, c, pdf);
  else if (COLOUR) c = hdr_color<false>(sc, L, env_clamp, ctr);
  else pdf = hdr_pdf<false>(sc, L, ctr);
  if (COLOUR) st3(colour + (size_t)i * 3, c);
  if (WANT_PDF) pdf_out[i] = pdf;
}

// ezrt_env_sample_device
__global__ __launch_bounds__(256) void env_sample_kernel(DevScene sc, const float* xip, uint32_t n, float* L_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Counters ctr = {0, 0, 0, 0, 0, 0, 0};
  st3(L_out + (size_t)i * 3, sample_hdr<false>(sc, xip[(size_t)i * 2], xip[(size_t)i * 2 + 1], ctr));
}

// ---- path queries (include/ezrt_path.h): one element per lane.  sample_xyf names the pixel-sample (ix, iy, frame) whose random
// numbers an element uses.
//
// ezrt_camera_rays_device: (eye, camera_dir) of each pixel-sample: the primary ray a render call shoots for it
__global__ __launch_bounds__(256) void camera_rays_kernel(EzrtRenderParams p, const uint32_t* xyf, uint32_t n, float* rays) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* q = xyf + (size_t)i * 3;
  uint32_t seed;
  const f3 dir = camera_dir(p, q[0], q[1], q[2], seed);
  float* o = rays + (size_t)i * 6;
  o[0] = p.eye[0], o[1] = p.eye[1], o[2] = p.eye[2];
  st3(o + 3, dir);
}

// ezrt_query_radiance_device: path_radiance along the caller's ray, a whole path per lane as in trace_kernel -- the same LDS
// traversal stack, a column per lane (the launch sizes it as the megakernel's: stack_lds_bytes).  The RNG starts where main() has
// it at its hitBVH call: the pixel-sample's seed behind the two jitter draws.  Work counters stay in the lane and are dropped.
struct RadianceArgs {
  DevScene sc;
  const float* rays;    // n x 6
  const uint32_t* xyf;  // n x 3
  uint32_t n;
  int32_t max_bounce;
  float env_clamp;
  float* radiance;      // n x 3
};
template <int INTEG>
__global__ __launch_bounds__(BLOCK) void radiance_query_kernel(RadianceArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const float* r = a.rays + (size_t)i * 6;
  const uint32_t* q = a.xyf + (size_t)i * 3;
  const uint32_t ix = q[0], iy = q[1], frame = q[2];
  uint32_t seed = pixel_seed(ix, iy, frame);
  (void)wang_hash(seed); // the jitter draws of main(): the ray is the caller's, the state behind them the pixel-sample's
  (void)wang_hash(seed);
  Counters ctr = {0, 0, 0, 0, 0, 0, 0};
  const PathLog none = {nullptr, nullptr};
  const f3 c = path_radiance<INTEG, false, false>(a.sc, ld3(r), ld3(r + 3), ix, iy, frame, seed, a.max_bounce, a.env_clamp,
                                                   lds_stack + threadIdx.x, ctr, none);
  st3(a.radiance + (size_t)i * 3, c);
}

// ---- all-hits queries (include/ezrt_multihit.h): one ray per lane.
//
// ezrt_query_all_hits_device: hit_bvh's walk -- the reference's binary records in the reference's order, unpruned, the LDS traversal
// stack a column per lane (launched with stack_lds_bytes, as radiance_query_kernel) -- that keeps EVERY triangle hit_triangle_t
// accepts below the ray's bound instead of the nearest: the visit order, and with it the order of equal t, is the reference's by
// construction.  The sorted list lives in the ray's own output row (global memory, K = max_hits entries): a ray is accepted by a
// handful of triangles and tests hundreds, so the row is touched a few times per ray, while K * 256 entries in LDS would not fit
// beside the stack at K = 64 (64 KiB of keys alone) and K entries in registers would cost the walk its occupancy.  `nb` entries
// are in the row, sorted; `last` holds the t of entry K - 1 once the row is full: a candidate that is not strictly below it is
// counted and touches no memory.  An insertion shifts the strictly greater entries up one slot (the K-th falls out), so equal t
// stay in visit order.  HAVE_T = false (no t_hit): the keys of the entries in the row are recomputed from their ids -- t is a pure
// function of (triangle, ray) -- by the same hit_triangle_t.
// Afterwards each wave fills the unused slots of its 64 rows with {-1, INF} together: consecutive lanes write consecutive words.
struct AllHitsArgs {
  DevScene sc;
  const float* rays;  // n x 6
  const float* t_max; // n, or null
  uint32_t n;
  int32_t K;
  FastDiv div_k;      // / K (the fill)
  int32_t* tri;       // n x K
  float* t;           // n x K, or null (HAVE_T = false)
  int32_t* n_hits;    // n, or null
};
template <bool HAVE_T>
__global__ __launch_bounds__(BLOCK) void all_hits_kernel(AllHitsArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  const int K = a.K;
  int nb = 0;
  if (i < a.n) {
    const DevScene& sc = a.sc;
    const float* r = a.rays + (size_t)i * 6;
    const f3 S = ld3(r), d = ld3(r + 3);
    // t < min(t_max, INF); a NaN t_max admits nothing (no hit has t < 0.0005)
    float bound = INF;
    if (a.t_max) {
      const float tm = a.t_max[i];
      bound = tm < INF ? tm : (tm >= INF ? INF : 0.0f);
    }
    int32_t* ri = a.tri + (size_t)i * K;
    float* rt = HAVE_T ? a.t + (size_t)i * K : nullptr;
    uint32_t count = 0;
    float last = INF;
    auto key = [&](int j) -> float {
      if (HAVE_T) return rt[j];
      float tj = INF;
      (void)hit_triangle_t(sc.tri_geom + (size_t)ri[j] * 3, S, d, tj);
      return tj;
    };
    auto put = [&](int j, int32_t id, float tj) {
      ri[j] = id;
      if (HAVE_T) rt[j] = tj;
      if (j == K - 1) last = tj;
    };
    int* stack = lds_stack + threadIdx.x;
    const f3 inv = mk(ez_rcp(d.x), ez_rcp(d.y), ez_rcp(d.z));
    int sp = 0;
    uint32_t ref = sc.root_ref;
    for (;;) {
      if (ref & LEAF_BIT) {
        const int first = (int)(ref & 0x00ffffffu);
        const int n = (int)((ref >> 24) & 0x7fu) + 1;
        for (int k = first; k < first + n; k++) {
          float t;
          if (!hit_triangle_t(sc.tri_geom + (size_t)k * 3, S, d, t) || !(t < bound)) continue;
          count++;
          if (nb == K && !(t < last)) continue; // behind a full row: counted only
          int j = nb < K ? nb++ : K - 1;
          while (j > 0) {
            const float tp = key(j - 1);
            if (!(tp > t)) break;
            put(j, ri[j - 1], tp);
            j--;
          }
          put(j, k, t);
        }
      } else {
        const float4* q = sc.inner + (size_t)ref * 4;
        const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        const float d1 = hit_aabb(S, inv, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y));
        const float d2 = hit_aabb(S, inv, mk(q1.z, q1.w, q2.x), mk(q2.y, q2.z, q2.w));
        const uint32_t left = __float_as_uint(q3.x), right = __float_as_uint(q3.y);
        if (d1 > 0.0f && d2 > 0.0f) {
          if (d1 < d2) { // left first: push right, continue with left
            stack[sp * BLOCK] = (int)right;
            sp++;
            ref = left;
          } else {
            stack[sp * BLOCK] = (int)left;
            sp++;
            ref = right;
          }
          continue;
        } else if (d1 > 0.0f) {
          ref = left;
          continue;
        } else if (d2 > 0.0f) {
          ref = right;
          continue;
        }
      }
      if (sp == 0) break;
      sp--;
      ref = (uint32_t)stack[sp * BLOCK];
    }
    if (a.n_hits) a.n_hits[i] = (int32_t)count;
  }
  // the unused slots of the wave's 64 rows: one flat run of 64 K words from the wave's first row
  const uint32_t lane = threadIdx.x & 63u;
  const size_t base = (size_t)(i - lane) * K;
  for (uint32_t e = lane; e < 64u * (uint32_t)K; e += 64u) {
    const uint32_t row = fastdiv(e, a.div_k);
    const uint32_t slot = e - row * (uint32_t)K;
    const int used = __shfl(nb, (int)row);
    if (i - lane + row < a.n && slot >= (uint32_t)used) {
      a.tri[base + e] = -1;
      if (HAVE_T) a.t[base + e] = INF;
    }
  }
}

// ezrt_surface_at_device: surface_point for hits the caller holds -- {triangle, t} of element i along ray i.  An id outside the
// scene writes zeros; point / normal / inside may each be null (not written).
template <bool P5TRI>
__global__ __launch_bounds__(256) void surface_at_kernel(const float4* tri_geom, const float4* tri_shade, int32_t n_tri, const float* rays,
                                                         const int32_t* tri_id, const float* t_hit, uint32_t n, float* point,
                                                         float* normal, uint8_t* inside) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  f3 P = mk(0.0f, 0.0f, 0.0f), N = mk(0.0f, 0.0f, 0.0f);
  bool in = false;
  if ((uint32_t)tri < (uint32_t)n_tri) {
    const float* r = rays + (size_t)i * 6;
    surface_point<P5TRI>(tri_geom, tri_shade, tri, t_hit[i], ld3(r), ld3(r + 3), P, N, in, [](float4) {});
  }
  if (point) st3(point + (size_t)i * 3, P);
  if (normal) st3(normal + (size_t)i * 3, N);
  if (inside) inside[i] = in ? 1u : 0u;
}

} // namespace ezd
