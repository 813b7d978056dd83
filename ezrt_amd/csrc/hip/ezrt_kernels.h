// ezrt_kernels.h -- the gfx950 kernels of the trace path.
//
//   trace_kernel<INTEG, FULLCTR, PATHLOG>   one thread = one pixel-sample
//       (ray-gen + hitBVH x (1 + k*bounces) + Disney BRDF + env lookups);
//       a 256-thread workgroup owns a 16x16 pixel block of one frame, each of
//       its four wavefronts an 8x8 sub-tile, so the 64 primary rays of a wave
//       are coherent.  Sample radiance goes to a frame-major sample buffer.
//       Its primary-ray arithmetic (camera_dir) and its bounce loop (path_radiance)
//       are device functions of their own: camera_rays_kernel and
//       radiance_query_kernel<INTEG> (include/ezrt_path.h) hand the first out
//       and run the second along caller rays, one path per lane as here.
//   accumulate_kernel    the reference's running mean mix(last, c, 1/(k+1))
//       (P5/fsh:943-944) applied in frame order, one thread per pixel.
//   sobol_kernel / tonemap_kernel / query_kernel / math_kernel  small entry
//       points of the C ABI (KATs, pass3, probe rays, det-math audit).
//
// Grid shape: pixel-samples are independent, so the whole chunk of frames is
// one launch of n_blocks * n_frames workgroups (>> 256 CUs); the hardware
// dispatcher load-balances the wildly uneven per-pixel cost (sky pixel = 1 ray,
// bunny pixel = 5).  Block b lands on XCD b % 8 and blockIdx = frame * n_blocks
// + block, so with n_blocks % 8 == 0 one image block stays on one XCD's L2 for
// every frame of the chunk.
#pragma once
#include "ezrt_device.h"
#include "ezrt_records.h"

namespace ezd {

// dims 0-7: the shader literal (P5/fsh:351-353); dims 8-15: include/ezrt.h, ezrt_scene_set_sampler
__constant__ uint32_t c_sobol_v[16 * 32] = {
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

struct TraceArgs {
  DevScene sc;
  EzrtRenderParams p;
  const int2* blocks;   // origin (x, y) of each 16x16 pixel block to render
  int32_t n_blocks;
  uint32_t frame_first; // first frame of this launch
  Sample3* samples;     // [n_frames][n_blocks * 256]
  unsigned long long* counters; // EZRT_CTR_COUNT
  int32_t* log_tri;     // PATHLOG: [H][W][slots]
  float* log_t;
  float* log_colour;    // PATHLOG: [H][W][3]
  int32_t stack_entries;
};

EZD bool pixel_owned(const EzrtRenderParams& p, int x, int y) {
  if (x < p.x0 || x >= p.x1 || y < p.y0 || y >= p.y1) return false;
  if (p.shard_count <= 1) return true;
  int tw = p.tile_w > 0 ? p.tile_w : 32, th = p.tile_h > 0 ? p.tile_h : 32;
  int tiles_x = (p.width + tw - 1) / tw;
  int tile = (y / th) * tiles_x + (x / tw);
  return tile % p.shard_count == p.shard_index;
}

EZD unsigned long long wave_sum(uint32_t v) {
  unsigned long long s = v;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// ---- queue position -> pixel-sample -> primary ray (used by raygen_kernel, and by the primary stage's trace and shading
// kernels when the chunk's rays are generated where they are consumed: Tuning::gen_primary)
EZD void slot_to_pixel(const int2* blocks, const FastDiv& n_blocks, uint32_t slot, uint32_t frame_first, int& x, int& y,
                       uint32_t& frame) {
  uint32_t tid = slot & 255u;
  uint32_t b = slot >> 8;
  const uint32_t fk = fastdiv(b, n_blocks), blk = b - fk * n_blocks.d;
  int2 org = blocks[blk];
  uint32_t wave = tid >> 6, lane = tid & 63u;
  x = org.x + (int)((wave & 1u) * 8u + (lane & 7u));
  y = org.y + (int)((wave >> 1) * 8u + (lane >> 3));
  frame = frame_first + fk;
}

// Queue order of the primary rays.  Sample slots are laid out [frame][16x16 block][8x8 sub-block]
// [lane]; taking queue position = sample slot would hand a wave pools of 256 rays from ONE 16x16
// pixel block -- all cheap (sky) or all expensive (the Bunny), and the launch ends with the waves
// that drew the expensive ones.  So the 8x8 sub-blocks of a frame are visited in a scattered
// order, sub-block (r * scatter) mod n_sub at position r (scatter ~ 2531, coprime to n_sub): a pool is four
// sub-blocks from distant parts of the image and every pool costs about the same.
EZD uint32_t queue_to_sample(uint32_t qslot, const FastDiv& n_sub_div, uint32_t scatter, uint32_t sh = 6u) {
  const uint32_t n_sub = n_sub_div.d; // granules of 1 << sh slots per frame = (n_blocks * 256) >> sh
  const uint32_t q = qslot >> sh;
  const uint32_t fk = fastdiv(q, n_sub_div), r = q - fk * n_sub;
  const uint32_t p = r * scatter; // 32-bit: the host keeps n_sub <= 2^20 and scatter < 2^12 here
  const uint32_t r2 = p - fastdiv(p, n_sub_div) * n_sub;
  return ((fk * n_sub + r2) << sh) | (qslot & ((1u << sh) - 1u));
}

// The seed of pixel-sample (ix, iy, frame): P5/fsh:315-318
EZD uint32_t pixel_seed(uint32_t ix, uint32_t iy, uint32_t frame) { return (ix * 1973u + iy * 9277u + frame * 26699u) | 1u; }

// The direction of the primary ray of pixel-sample (ix, iy, frame): main() up to the hitBVH call (P5/fsh:315-318 seed, 920-925
// jitter, camera, normalize).  `seed` returns the RNG state main() has when it reaches hitBVH: the pixel-sample's seed advanced by
// the two jitter draws.  ONE definition for every kernel that needs the direction -- the primary stage's trace and shading kernels
// (primary_dir), trace_kernel and ezrt_camera_rays_device -- so that the ray the trace follows, the ray the shading stage shades
// and the ray a caller is handed are the same bits.  Of `p` it reads width, height and camera_rotate alone.
EZD f3 camera_dir(const EzrtRenderParams& p, uint32_t ix, uint32_t iy, uint32_t frame, uint32_t& seed) {
  seed = pixel_seed(ix, iy, frame);
  const float W = (float)p.width, H = (float)p.height;
  // (x / W for a power-of-two W IS x * (1 / W) on the bits, and every BASELINE frame is one: the four divisions below as
  // multiplications behind a uniform branch were built and measured in round 4 -- C2 -3.3 %: four more launch-invariant values
  // in a kernel at its SGPR limit became three more VGPR spills in the refill block; profiles/r4/rcp_pow2_ab.txt)
  float pixx = ((float)ix + 0.5f) / W * 2.0f - 1.0f;
  float pixy = ((float)iy + 0.5f) / H * 2.0f - 1.0f;
  float aax = (rnd(seed) - 0.5f) / W;
  float aay = (rnd(seed) - 0.5f) / H;
  float vx = pixx + aax, vy = pixy + aay, vz = -1.5f;
  const float* m = p.camera_rotate;
  f3 dir = mk(m[0] * vx + m[4] * vy + m[8] * vz, m[1] * vx + m[5] * vy + m[9] * vz, m[2] * vx + m[6] * vy + m[10] * vz);
  return normalize(dir);
}

// The primary ray of queue position `qslot`: (dir.xyz, 1), or w = 0 for a pixel this shard does not own.
EZD float4 primary_dir(const EzrtRenderParams& p, const int2* blocks, const FastDiv& div_blocks, const FastDiv& div_sub, uint32_t scatter,
                       uint32_t scatter_shift, uint32_t frame_first, uint32_t qslot) {
  int x, y;
  uint32_t frame;
  slot_to_pixel(blocks, div_blocks, queue_to_sample(qslot, div_sub, scatter, scatter_shift), frame_first, x, y, frame);
  if (!pixel_owned(p, x, y)) return make_float4(0, 0, 0, 0.0f);
  uint32_t seed;
  const f3 dir = camera_dir(p, (uint32_t)x, (uint32_t)y, frame, seed);
  return make_float4(dir.x, dir.y, dir.z, 1.0f);
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

template <int INTEG, bool FULLCTR, bool PATHLOG>
__global__ __launch_bounds__(BLOCK) void trace_kernel(TraceArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const int tid = threadIdx.x;
  const int blk = blockIdx.x % a.n_blocks;
  const int fk = blockIdx.x / a.n_blocks;
  const uint32_t frame = a.frame_first + (uint32_t)fk;
  const int wave = tid >> 6, lane = tid & 63;
  const int2 org = a.blocks[blk];
  const int x = org.x + (wave & 1) * 8 + (lane & 7);
  const int y = org.y + (wave >> 1) * 8 + (lane >> 3);
  int* stack = lds_stack + tid;
  const DevScene& sc = a.sc;
  const EzrtRenderParams& p = a.p;

  Counters ctr = {0, 0, 0, 0, 0, 0, 0};
  uint32_t samples = 0;
  f3 colour = mk(0, 0, 0);
  const bool active = pixel_owned(p, x, y);
  if (active) {
    samples = 1;
    const size_t pix = (size_t)y * p.width + x;
    PathLog lg = {nullptr, nullptr};
    if (PATHLOG) {
      int slots = 1 + 2 * p.max_bounce;
      lg.tri = a.log_tri + pix * slots;
      lg.t = a.log_t + pix * slots;
      for (int k = 0; k < slots; k++) {
        lg.tri[k] = -2;
        lg.t[k] = INF;
      }
    }
    const uint32_t ix = (uint32_t)x, iy = (uint32_t)y;
    uint32_t seed;
    const f3 dir = camera_dir(p, ix, iy, frame, seed);
    const f3 org3 = mk(p.eye[0], p.eye[1], p.eye[2]);
    colour = path_radiance<INTEG, FULLCTR, PATHLOG>(sc, org3, dir, ix, iy, frame, seed, p.max_bounce, p.env_clamp, stack, ctr, lg);
    if (PATHLOG) {
      a.log_colour[pix * 3 + 0] = colour.x;
      a.log_colour[pix * 3 + 1] = colour.y;
      a.log_colour[pix * 3 + 2] = colour.z;
    }
  }
  if (!PATHLOG) a.samples[((size_t)fk * a.n_blocks + blk) * BLOCK + tid] = Sample3{colour.x, colour.y, colour.z};

  // counters: one atomic per wave per slot
  unsigned long long r = wave_sum(ctr.rays), s = wave_sum(samples);
  if (lane == 0) {
    atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_RAYS], r);
    atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_SAMPLES], s);
  }
  if (FULLCTR) {
    unsigned long long v1 = wave_sum(ctr.pops), v2 = wave_sum(ctr.inner), v3 = wave_sum(ctr.tris),
                       v4 = wave_sum(ctr.mats), v5 = wave_sum(ctr.envmap), v6 = wave_sum(ctr.envcache);
    if (lane == 0) {
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_NODE_POPS], v1);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_INNER_POPS], v2);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_TRI_TESTS], v3);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_MAT_FETCH], v4);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_ENV_MAP], v5);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_ENV_CACHE], v6);
    }
  }
}

// mix(lastColor, color, 1.0/float(frameCounter+1)): P5/fsh:943-947, in frame order.
struct AccumArgs {
  EzrtRenderParams p;
  const int2* blocks;
  int32_t n_blocks;
  uint32_t frame_first, n_frames;
  const Sample3* samples;
  float4* accum; // [H][W] RGBA
};
__global__ __launch_bounds__(BLOCK) void accumulate_kernel(AccumArgs a) {
  const int tid = threadIdx.x, blk = blockIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int2 org = a.blocks[blk];
  const int x = org.x + (wave & 1) * 8 + (lane & 7);
  const int y = org.y + (wave >> 1) * 8 + (lane >> 3);
  if (!pixel_owned(a.p, x, y)) return;
  const size_t pix = (size_t)y * a.p.width + x;
  float4 last = a.accum[pix];
  f3 mean = mk(last.x, last.y, last.z);
  for (uint32_t k = 0; k < a.n_frames; k++) {
    const Sample3 c = a.samples[((size_t)k * a.n_blocks + blk) * BLOCK + tid];
    uint32_t frame = a.frame_first + k;
    if (frame == 0) {
      mean = mk(c.x, c.y, c.z);
    } else {
      float w = 1.0f / (float)(frame + 1u);
      mean = mix3(mean, mk(c.x, c.y, c.z), w);
    }
  }
  a.accum[pix] = make_float4(mean.x, mean.y, mean.z, 1.0f);
}

// inner records with both child boxes translated by -S (S = the eye): what hitAABB subtracts on every visit
__global__ void inner_rel_kernel(const float4* inner, int n_inner, float sx, float sy, float sz, float4* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_inner) return;
  const float4 q0 = inner[i * 4], q1 = inner[i * 4 + 1], q2 = inner[i * 4 + 2];
  out[i * 4] = make_float4(q0.x - sx, q0.y - sy, q0.z - sz, q0.w - sx);
  out[i * 4 + 1] = make_float4(q1.x - sy, q1.y - sz, q1.z - sx, q1.w - sy);
  out[i * 4 + 2] = make_float4(q2.x - sz, q2.y - sx, q2.z - sy, q2.w - sz);
  out[i * 4 + 3] = inner[i * 4 + 3];
}

__global__ void sobol_kernel(uint32_t index0, int n, int n_dims, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n_dims) return;
  int s = i / n_dims, d = i % n_dims;
  out[i] = sobol((uint32_t)d, gray_code(index0 + (uint32_t)s));
}

// ezrt_frame_nonfinite: pixels whose running mean is poisoned (the reference's 0/0 in misMixWeight, P5/fsh:754-757, reproduced:
// include/ezrt.h "Numerical contract").  One ballot per wave, one atomic per wave that saw any.
__global__ void nonfinite_kernel(const float4* rgba, size_t n, unsigned long long* count) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ((n + 63) & ~(size_t)63); i += (size_t)gridDim.x * blockDim.x) {
    bool bad = false;
    if (i < n) {
      const float4 v = rgba[i];
      // non-finite = exponent all ones
      bad = ((__float_as_uint(v.x) & 0x7f800000u) == 0x7f800000u) || ((__float_as_uint(v.y) & 0x7f800000u) == 0x7f800000u) ||
            ((__float_as_uint(v.z) & 0x7f800000u) == 0x7f800000u);
    }
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)__popcll(m));
  }
}

// pass3.fsh:14-24 + P1/main.cpp:187-189
__global__ void tonemap_kernel(const float4* rgba, int n, uint8_t* rgb8) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 c = rgba[i];
  float lum = 0.3f * c.x + 0.6f * c.y + 0.1f * c.z;
  float k = 1.0f + lum / 1.5f;
  float ch[3] = {c.x, c.y, c.z};
  for (int j = 0; j < 3; j++) {
    float v = ch[j] * 1.0f / k;
    v = ez_pow(v, 1.0f / 2.2f);
    float q = ez_clamp(v * 255.0f, 0.0f, 255.0f);
    if (!(q == q)) q = 0.0f;
    rgb8[(size_t)i * 3 + j] = (uint8_t)(int)q;
  }
}

struct QueryArgs {
  DevScene sc;
  const float* rays;
  int n;
  int32_t* tri;
  float* t;
  unsigned long long* counters;
};
template <bool FULLCTR>
__global__ __launch_bounds__(BLOCK) void query_kernel(QueryArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  int i = blockIdx.x * BLOCK + threadIdx.x;
  Counters ctr = {0, 0, 0, 0, 0, 0, 0};
  if (i < a.n) {
    const float* r = a.rays + (size_t)i * 6;
    int32_t tri;
    float t;
    hit_bvh<FULLCTR, BLOCK>(a.sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), lds_stack + threadIdx.x, tri, t, ctr);
    a.tri[i] = tri;
    a.t[i] = (tri >= 0) ? t : INF;
  }
  unsigned long long rr = wave_sum(ctr.rays);
  if ((threadIdx.x & 63) == 0) atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_RAYS], rr);
  if (FULLCTR) {
    unsigned long long v1 = wave_sum(ctr.pops), v2 = wave_sum(ctr.inner), v3 = wave_sum(ctr.tris), v4 = wave_sum(ctr.mats);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_NODE_POPS], v1);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_INNER_POPS], v2);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_TRI_TESTS], v3);
      atomicAdd(&ctr_slot(a.counters)[EZRT_CTR_MAT_FETCH], v4);
    }
  }
}

// ezrt_debug_math op 17: the launch-invariant division of the queue maps (FastDiv), bits in / bits out
__global__ void fastdiv_kernel(const float* a, FastDiv f, int n, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = __uint_as_float(fastdiv(__float_as_uint(a[i]), f));
}

__global__ void math_kernel(int op, const float* a, const float* b, int n, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = a[i], y = b[i], r;
  switch (op) {
    case 0: r = ez_sin(x); break;
    case 1: r = ez_cos(x); break;
    case 2: r = ez_atan2(x, y); break;
    case 3: r = ez_asin(x); break;
    case 4: r = ez_log(x); break;
    case 5: r = ez_exp(x); break;
    case 6: r = ez_pow(x, y); break;
    case 7: r = __builtin_sqrtf(x); break;
    case 8: r = x / y; break;
    default: {
      uint32_t sd = __float_as_uint(x);
      r = rnd(sd);
    }
  }
  out[i] = r;
}

// Intersector audit (ezrt_debug_math ops 10-12): the device functions the traversal kernels call,
// evaluated on caller-supplied operands so tests can compare them with the reference's C++ twins
// (P2/main.cpp:212-238, 449-463) directly.  op 10 = hit_aabb (exact select form), 12 = hit_aabb_tame
// (v_min3/v_max3 form; NaN for rays that are not tame = the caller must not have used it), 11 =
// hit_triangle_t on the 48-B record ezrt_scene_create builds (unit plane normal precomputed with the
// same fp32 operations), INF on a miss.
__global__ void isect_kernel(int op, const float* a, const float* b, int n, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = a + 6 * (size_t)i;
  f3 S = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
  if (op >= 13) { // integrator 52's sampler / pdf in the frame N = (0,0,1) (include/ezrt.h, ezrt_debug_math)
    const float* q = b + 6 * (size_t)i;
    Mat m;
    m.emissive = mk(0, 0, 0);
    m.baseColor = mk(0, 0, 0);
    m.subsurface = m.specular = m.specularTint = m.sheen = m.sheenTint = 0.0f;
    m.roughness = q[0];
    m.anisotropic = q[1];
    m.metallic = q[2];
    m.clearcoat = q[3];
    m.clearcoatGloss = q[4];
    m.anisotropic = q[1];
    mat_derive(m);
    const f3 N = mk(0, 0, 1);
    f3 X, Y;
    get_tangent(N, X, Y);
    if (op == 13) {
      out[i] = brdf_pdf_aniso(S, N, d, X, Y, m);
    } else {
      const f3 L = sample_brdf_aniso(r[0], r[1], r[2], d, N, X, Y, m);
      out[i] = op == 14 ? L.x : (op == 15 ? L.y : L.z);
    }
    return;
  }
  if (op == 11) {
    const float* t = b + 9 * (size_t)i;
    float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
    float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
    float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    float inv = 1.0f / __builtin_sqrtf(cx * cx + cy * cy + cz * cz);
    float4 g[3] = {make_float4(t[0], t[1], t[2], cx * inv), make_float4(t[3], t[4], t[5], cy * inv),
                   make_float4(t[6], t[7], t[8], cz * inv)};
    float tt;
    out[i] = hit_triangle_t(g, S, d, tt) ? tt : INF;
    return;
  }
  const float* q = b + 6 * (size_t)i;
  f3 inv = mk(ez_rcp(d.x), ez_rcp(d.y), ez_rcp(d.z));
  f3 AA = mk(q[0], q[1], q[2]), BB = mk(q[3], q[4], q[5]);
  if (op == 10) out[i] = hit_aabb(S, inv, AA, BB);
  else out[i] = ray_is_tame(S, inv) ? hit_aabb_tame(S, inv, AA, BB) : __uint_as_float(0x7fc00000u);
}

// Function-level audit (ezrt_debug_fn, include/ezrt.h): the BRDF, the samplers and the environment lookups the shading kernels
// call (the fused brdf_evaluate_pdf of the MIS loops and integrator 52's sampler included: ops 11-13), on caller-supplied operands.  op / chapter / layouts are the header's.  Materials arrive as mat_table rows packed on
// the host by mat_pack_row (what ezrt_scene_create does) and are read with shade_point's mat_unpack_row, or -- `inline_mat` --
// as their 18 floats, derived here by mat_derive.  The environment ops read `sc`, the scene's own DevScene.
struct FnArgs {
  DevScene sc;
  int op, chapter, inline_mat, n;
  const float* a;
  const float4* rows; // n x MAT_ROW_FLOAT4 (table mode)
  const float* m18;   // n x 18 (inline mode)
  float* out;
};
__global__ __launch_bounds__(256) void fn_kernel(FnArgs q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n) return;
  Counters ctr = {0, 0, 0, 0, 0, 0, 0};
  Mat m;
  if ((q.op >= 1 && q.op <= 4) || (q.op >= 11 && q.op <= 13)) {
    if (q.inline_mat) {
      mat_from18(m, q.m18 + (size_t)i * 18);
    } else {
      const float4* mq = q.rows + (size_t)i * MAT_ROW_FLOAT4;
      mat_unpack_row(m, mq[0], mq[1], mq[2], mq[3], mq[4], mq[5], mq[6]);
    }
  }
  const float env_clamp = q.chapter == 3 ? 10.0f : 0.0f;
  f3 r = mk(0, 0, 0);
  switch (q.op) {
    case 1: {
      const float* p = q.a + (size_t)i * 9;
      r = brdf_evaluate<false>(ld3(p), ld3(p + 3), ld3(p + 6), mk(0, 0, 0), mk(0, 0, 0), m);
      break;
    }
    case 2: {
      const float* p = q.a + (size_t)i * 9;
      const f3 N = ld3(p + 3);
      f3 X, Y;
      get_tangent(N, X, Y);
      r = q.chapter == 4 ? brdf_evaluate<true>(ld3(p), N, ld3(p + 6), X, Y, m) : brdf_evaluate<false>(ld3(p), N, ld3(p + 6), X, Y, m);
      break;
    }
    case 3: {
      const float* p = q.a + (size_t)i * 9;
      r = sample_brdf(p[0], p[1], p[2], ld3(p + 3), ld3(p + 6), m);
      break;
    }
    case 4: {
      const float* p = q.a + (size_t)i * 9;
      q.out[i] = brdf_pdf(ld3(p), ld3(p + 3), ld3(p + 6), m);
      return;
    }
    case 5: q.out[i] = hdr_pdf<false>(q.sc, ld3(q.a + (size_t)i * 3), ctr); return;
    case 6: {
      const float* p = q.a + (size_t)i * 2;
      r = sample_hdr<false>(q.sc, p[0], p[1], ctr);
      break;
    }
    case 7: r = hdr_color<false>(q.sc, ld3(q.a + (size_t)i * 3), env_clamp, ctr); break;
    case 9: {
      const float* p = q.a + (size_t)i * 5;
      r = to_normal_hemisphere(sample_hemisphere(p[0], p[1]), ld3(p + 2));
      break;
    }
    case 11:   // what the MIS loops of integrators 51 / 52 call per evaluated direction (ezrt_wavefront.h, mega_kernel)
    case 12: {
      const float* p = q.a + (size_t)i * 9;
      const f3 N = ld3(p + 3);
      f3 X, Y, f;
      float pdf;
      get_tangent(N, X, Y);
      if (q.op == 11) brdf_evaluate_pdf<false>(ld3(p), N, ld3(p + 6), X, Y, m, f, pdf);
      else brdf_evaluate_pdf<true>(ld3(p), N, ld3(p + 6), X, Y, m, f, pdf);
      float* o = q.out + (size_t)i * 4;
      o[0] = f.x, o[1] = f.y, o[2] = f.z, o[3] = pdf;
      return;
    }
    case 13: { // integrator 52's sampler
      const float* p = q.a + (size_t)i * 9;
      const f3 N = ld3(p + 6);
      f3 X, Y;
      get_tangent(N, X, Y);
      r = sample_brdf_aniso(p[0], p[1], p[2], ld3(p + 3), N, X, Y, m);
      break;
    }
    default: { // 10 (the host admits no other op)
      float pdf;
      hdr_color_pdf<false>(q.sc, ld3(q.a + (size_t)i * 3), env_clamp, ctr, r, pdf);
      float* o = q.out + (size_t)i * 4;
      o[0] = r.x, o[1] = r.y, o[2] = r.z, o[3] = pdf;
      return;
    }
  }
  float* o = q.out + (size_t)i * 3;
  o[0] = r.x, o[1] = r.y, o[2] = r.z;
}

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

// ezrt_debug_math op 18: ez_rcp(x) against the compiler's `1.0f / x` for ALL 2^32 bit patterns of x (a NaN equals a NaN).
// res[0] = mismatches, res[1] = the smallest mismatching pattern.
__global__ void rcp_audit_kernel(unsigned long long* res) {
  unsigned long long bad = 0ull, first = ~0ull;
  for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < (1ull << 32); k += (unsigned long long)gridDim.x * blockDim.x) {
    const float x = __uint_as_float((uint32_t)k);
    float want;
    asm volatile("" : "=v"(want) : "0"(1.0f / x)); // (keep the two expressions apart)
    const float got = ez_rcp(x);
    const bool same = __float_as_uint(got) == __float_as_uint(want) || (got != got && want != want);
    if (!same) {
      bad++;
      if (k < first) first = k;
    }
  }
  if (bad) {
    atomicAdd(&res[0], bad);
    atomicMin(&res[1], first);
  }
}

} // namespace ezd
