// ezrt_path_device.h -- the device functions of a whole path in one lane that more than one translation unit needs: the Sobol
// sequence, the primary ray of a pixel-sample (pixel_seed, camera_dir) and the bounce loop (path_radiance).  ezrt_launch.hip runs them
// in trace_kernel and the timed stages (ezrt_kernels.h, ezrt_wavefront.h, ezrt_traceq4.h), ezrt_queries.hip in camera_rays_kernel and
// radiance_query_kernel (ezrt_query_kernels.h).  EZD functions only: no kernel is defined here.
#pragma once
#include "ezrt_device.h"
#include "ezrt_records.h"

namespace ezd {

// dims 0-7: the shader literal (P5/fsh:351-353); dims 8-15: include/ezrt.h, ezrt_scene_set_sampler
// (static: every translation unit that includes this has a copy of its own)
static __constant__ uint32_t c_sobol_v[16 * 32] = {
#include "ezrt_sobol_v.inc"
#include "ezrt_sobol_v16.inc"
};

// sobol(d, i): P5/fsh:361-369
EZD float sobol(uint32_t d, uint32_t i) {
  uint32_t result = 0, offset = d * 32u;
  for (uint32_t j = 0; i != 0; i >>= 1, j++)
    if (i & 1u) result ^= c_sobol_v[j + offset];
  return (float)result * (1.0f / (float)0xFFFFFFFFu);
}
EZD uint32_t gray_code(uint32_t i) { return i ^ (i >> 1); }

// The seed of pixel-sample (ix, iy, frame): P5/fsh:315-318
EZD uint32_t pixel_seed(uint32_t ix, uint32_t iy, uint32_t frame) { return (ix * 1973u + iy * 9277u + frame * 26699u) | 1u; }

// The direction of the primary ray of pixel-sample (ix, iy, frame): main() up to the hitBVH call (P5/fsh:315-318 seed, 920-925
// jitter, camera, normalize).  `seed` returns the RNG state main() has when it reaches hitBVH: the pixel-sample's seed advanced by
// the two jitter draws.  ONE definition for every kernel that needs the direction -- the primary stage's trace and shading kernels
// (primary_dir), trace_kernel and ezrt_camera_rays_device -- so that the ray the trace follows, the ray the shading stage shades
// and the ray a caller is handed are the same bits.  Of `p` it reads width, height and camera_rotate alone.
// POW2: width and height are powers of two and (sw, sh) = (1 / W, 1 / H), both exact: x / W IS x * (1 / W) on the bits then (a scaling
// by a power of two is exact while nothing becomes subnormal, and the operands here are 2^-25 .. 2^14 in size), so the four correctly
// rounded divisions -- about eleven instructions each -- are four multiplications.  Otherwise (sw, sh) = (W, H) and the divisions are
// the reference's.  A template parameter, not a uniform branch: the branch was built and measured in round 4 -- C2 -3.3 %: more launch-
// invariant values in a kernel at its SGPR limit became three more VGPR spills in the refill block (profiles/r4/rcp_pow2_ab.txt) --
// while the compile-time form takes the reciprocals IN PLACE of W and H (traceq4_kernel WHOLE == 2).  m: EzrtRenderParams::camera_rotate.
template <bool POW2>
EZD f3 camera_dir_scaled(float sw, float sh, const float* m, uint32_t ix, uint32_t iy, uint32_t frame, uint32_t& seed) {
  seed = pixel_seed(ix, iy, frame);
  auto over = [](float v, float s) { return POW2 ? v * s : v / s; };
  float pixx = over((float)ix + 0.5f, sw) * 2.0f - 1.0f;
  float pixy = over((float)iy + 0.5f, sh) * 2.0f - 1.0f;
  float aax = over(rnd(seed) - 0.5f, sw);
  float aay = over(rnd(seed) - 0.5f, sh);
  float vx = pixx + aax, vy = pixy + aay, vz = -1.5f;
  f3 dir = mk(m[0] * vx + m[4] * vy + m[8] * vz, m[1] * vx + m[5] * vy + m[9] * vz, m[2] * vx + m[6] * vy + m[10] * vz);
  return normalize(dir);
}
EZD f3 camera_dir(const EzrtRenderParams& p, uint32_t ix, uint32_t iy, uint32_t frame, uint32_t& seed) {
  return camera_dir_scaled<false>((float)p.width, (float)p.height, p.camera_rotate, ix, iy, frame, seed);
}

// Where a path's ray slots are logged (ezrt_render_paths): the 1 + 2 * max_bounce ids and distances of ONE pixel
struct PathLog {
  int32_t* tri;
  float* t;
};
template <bool PATHLOG>
EZD void plog(const PathLog& lg, int slot, int32_t tri, float t) {
  if (PATHLOG) {
    lg.tri[slot] = tri;
    lg.t[slot] = (tri >= 0) ? t : INF;
  }
}

// pathTracing of integrator INTEG along ONE primary ray, a whole path in this lane: main() from its hitBVH call to `color`
// (P5/fsh:926-938 and the chapters' loops).  The ray enters through (org3, dir), used as given; the pixel-sample through
// (ix, iy, frame) -- Cranley-Patterson offsets, Gray-coded Sobol index -- and `seed`, the RNG state behind the two jitter draws
// (camera_dir returns it).  ONE definition of the bounce loop for every one-lane kernel: trace_kernel (the megakernel route of a
// render call and ezrt_render_paths, which logs every ray slot through `lg`) and radiance_query_kernel (caller rays).
template <int INTEG, bool FULLCTR, bool PATHLOG>
EZD f3 path_radiance(const DevScene& sc, f3 org3, f3 dir, uint32_t ix, uint32_t iy, uint32_t frame, uint32_t seed, int max_bounce,
                     float env_clamp, int* stack, Counters& ctr, const PathLog& lg) {
  constexpr bool P5TRI = (INTEG >= 50);
  constexpr bool MIS = integ_mis<INTEG>();
  constexpr bool ANISO_IS = integ_aniso_is<INTEG>();
  int32_t tri;
  float t;
  hit_bvh<FULLCTR, BLOCK>(sc, org3, dir, stack, tri, t, ctr);
  plog<PATHLOG>(lg, 0, tri, t);
  if (tri < 0) return hdr_color<FULLCTR>(sc, dir, env_clamp, ctr);
  Hit hit;
  shade_point<P5TRI>(sc, tri, t, org3, dir, hit);
  const f3 Le0 = hit.m.emissive;
  f3 Lo = mk(0, 0, 0), history = mk(1, 1, 1);
  float cpu = 0.0f, cpv = 0.0f;
  if (INTEG >= 50) cp_offsets(ix, iy, cpu, cpv);
  const uint32_t gray = gray_code(frame + 1u);

  for (int bounce = 0; bounce < max_bounce; bounce++) {
    const f3 V = -hit.viewDir, N = hit.N;
    f3 X = mk(0, 0, 0), Y = mk(0, 0, 0);
    if (ANISO_IS) get_tangent(N, X, Y);
    if (MIS) {
      // env importance sample + shadow ray: P5/fsh:819-842
      float h1 = rnd(seed);
      float h2 = rnd(seed);
      f3 Lh = sample_hdr<FULLCTR>(sc, h1, h2, ctr);
      if (dot(N, Lh) > 0.0f) {
        int32_t st;
        float stt;
        hit_bvh<FULLCTR, BLOCK>(sc, hit.P, Lh, stack, st, stt, ctr);
        plog<PATHLOG>(lg, 1 + 2 * bounce, st, stt);
        if (st < 0) {
          f3 color;
          float pdf_light;
          hdr_color_pdf<FULLCTR>(sc, Lh, env_clamp, ctr, color, pdf_light);
          f3 f_r;
          float pdf_brdf;
          brdf_evaluate_pdf<ANISO_IS>(V, N, Lh, X, Y, hit.m, f_r, pdf_brdf);
          float w = mis_mix_weight(pdf_light, pdf_brdf);
          Lo = Lo + (((history * w) * color) * f_r) * dot(N, Lh) / pdf_light;
        }
      }
    }
    // sample direction
    f3 L;
    float xi1, xi2;
    if (INTEG >= 50) { // sobolVec2 + CP: P5/fsh:771-772, 845-846 (dims wrap at 8)
      uint32_t d0 = ((uint32_t)bounce * 2u) & sc.sobol_mask, d1 = ((uint32_t)bounce * 2u + 1u) & sc.sobol_mask;
      xi1 = cp_rotate(sobol(d0, gray), cpu);
      xi2 = cp_rotate(sobol(d1, gray), cpv);
    } else { // P3/fsh:109-114: z = rand() then phi = 2 pi rand()
      xi1 = rnd(seed);
      xi2 = rnd(seed);
    }
    float cosine, pdf;
    f3 f_r;
    if (MIS) {
      float xi3 = rnd(seed);
      L = ANISO_IS ? sample_brdf_aniso(xi1, xi2, xi3, V, N, X, Y, hit.m) : sample_brdf(xi1, xi2, xi3, V, N, hit.m);
      cosine = dot(N, L);
      if (cosine <= 0.0f) break;
    } else {
      L = to_normal_hemisphere(sample_hemisphere(xi1, xi2), N);
      pdf = 1.0f / (2.0f * PI);
      cosine = ez_max(0.0f, dot(L, N));
      if (INTEG == EZRT_INTEGRATOR_P3_DIFFUSE) {
        f_r = hit.m.baseColor / PI;
      } else {
        f3 tangent, bitangent;
        get_tangent(N, tangent, bitangent);
        f_r = brdf_evaluate<INTEG == EZRT_INTEGRATOR_P4_DISNEY>(V, N, L, tangent, bitangent, hit.m);
      }
    }
    int32_t nt;
    float ntt;
    hit_bvh<FULLCTR, BLOCK>(sc, hit.P, L, stack, nt, ntt, ctr);
    plog<PATHLOG>(lg, 2 + 2 * bounce, nt, ntt);
    if (MIS) {
      brdf_evaluate_pdf<ANISO_IS>(V, N, L, X, Y, hit.m, f_r, pdf);
      if (pdf <= 0.0f) break;
    }
    if (nt < 0) {
      f3 sky;
      float pdf_light = 0.0f;
      if (MIS) hdr_color_pdf<FULLCTR>(sc, L, env_clamp, ctr, sky, pdf_light);
      else sky = hdr_color<FULLCTR>(sc, L, env_clamp, ctr);
      if (MIS) {
        float w = mis_mix_weight(pdf, pdf_light);
        Lo = Lo + (((history * w) * sky) * f_r) * cosine / pdf;
      } else {
        Lo = Lo + ((history * sky) * f_r) * cosine / pdf;
      }
      break;
    }
    Hit nh;
    shade_point<P5TRI>(sc, nt, ntt, hit.P, L, nh);
    Lo = Lo + ((history * nh.m.emissive) * f_r) * cosine / pdf;
    history = history * (f_r * cosine / pdf);
    hit = nh;
  }
  return Le0 + Lo;
}

} // namespace ezd
