// ezrt_device.h -- device-side building blocks of the gfx950 trace: vector
// helpers with a fixed evaluation order, RNG/Sobol, the BVH traversal over the
// device scene layout, texture fetches, the Disney BRDF and its samplers.
//
// Results contract: every function here reproduces, bit for bit, the fp32
// arithmetic the reference's fragment shader specifies once its
// implementation-defined parts are pinned as in DESIGN.md ("arithmetic
// contract"): left-to-right evaluation, no fma contraction (-ffp-contract=off),
// GLSL built-ins from include/ezrt_detmath.h.  Reference lines are cited per
// function (P5/fsh = part 5 shaders/fshader.fsh, etc.).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ezrt.h"
#include "ezrt_detmath.h"

#define EZD __device__ __forceinline__

namespace ezd {

constexpr float PI = EZ_PI;
constexpr float INF = EZ_INF;

struct f3 {
  float x, y, z;
};
EZD f3 mk(float x, float y, float z) { return f3{x, y, z}; }
// one pixel-sample's radiance as the shading stages hand it to accumulate_kernel: 12 B (the alpha of P5/fsh:946 is the
// constant 1: a float4 here was 25 % more traffic on both sides)
struct Sample3 {
  float x, y, z;
};
EZD f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
EZD f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
EZD f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
EZD f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
EZD f3 operator/(f3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
EZD f3 operator-(f3 a) { return mk(-a.x, -a.y, -a.z); }
EZD float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
EZD f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// 1.0f / x, correctly rounded -- the same bits as the division the compiler emits for `1.0f / x` (IEEE binary32, round to nearest
// even: what gcc produces for the oracle), in 4 VALU instructions instead of the 10 + hazard nops of the general division macro
// (v_div_scale x2, v_rcp, 4 fma, v_div_fmas, v_div_fixup): v_rcp_f32 is within 1 ulp, one Newton step on the residual computed with
// a fused multiply-add (the rounding of THIS primitive's result is what the contract fixes, not how it is reached) lands on the
// correctly rounded quotient for every |x| in [2^-120, 2^120]; everything else -- zeros, denormals, huge values whose reciprocal is
// denormal, infinities, NaNs -- takes the compiler's division.  Not a claim: tests/test_gpu_parity.py runs ALL 2^32 bit patterns
// through both on the device (ezrt_debug_math op 18) and requires zero mismatches.  Rays per refill: three of these (1 / d) + the
// normalisation of a generated primary direction; the shading kernels' normalisations.
#ifndef EZRT_FAST_RCP
#define EZRT_FAST_RCP 1 // (0: A/B builds, tools/build_variant.sh)
#endif
EZD float ez_rcp(float x) {
  if (!EZRT_FAST_RCP) return 1.0f / x;
  const float ax = __builtin_fabsf(x);
  if (ax >= 7.5231638e-37f && ax <= 1.329228e36f) { // [2^-120, 2^120]
    float r = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, r, 1.0f);
    r = __builtin_fmaf(r, e, r);
    return r;
  }
  return 1.0f / x;
}
EZD f3 normalize(f3 a) {
  float inv = ez_rcp(__builtin_sqrtf(dot(a, a)));
  return a * inv;
}
EZD f3 mix3(f3 a, f3 b, float t) { return mk(ez_mix(a.x, b.x, t), ez_mix(a.y, b.y, t), ez_mix(a.z, b.z, t)); }
EZD f3 reflect(f3 i, f3 n) { // GLSL: I - 2.0 * dot(N, I) * N
  float k = 2.0f * dot(n, i);
  return i - n * k;
}
EZD float sqr(float x) { return x * x; }

// ---------------------------------------------------------------------------
// Device scene layout (built by ezrt_scene_create from the reference arrays).
//
//  tri_geom : 3 x float4 per triangle = 48 B, one cache line pair per test
//             (p1.xyz, N.x) (p2.xyz, N.y) (p3.xyz, N.z);  N = the unit plane
//             normal hitTriangle recomputes per call (P5/fsh:172) -- a pure
//             function of the triangle, evaluated once with the same fp32 ops.
//  tri_ref  : the reference's own 36-float records (144 B); only texels 3-11
//             (vertex normals + material) are read, once per *winning* hit.
//  inner    : 4 x float4 per inner node = 64 B: both children's boxes plus two
//             child references, so an inner visit is ONE 64-B fetch instead of
//             the reference's three 48-B getBVHNode calls (P5/fsh:266,281,285).
//             ref >= 0      : index of an inner record
//             ref bit31 set : leaf, bits 30..24 = n-1, bits 23..0 = first tri
struct DevScene {
  const float4* tri_geom;
  const float* tri_ref;
  const float4* inner;
  const float4* tri_shade; // 4 x float4 per triangle: what a WINNING hit needs besides tri_geom (see ShadeRec below)
  const float4* mat_table; // 7 x float4 per distinct material: its 18 floats + the constants brdf_evaluate derives from them
  uint32_t root_ref;
  int32_t n_tri;
  const float4* hdr;   // RGBA texels, row 0 = top
  const uint32_t* hdr_rgbe; // the same map as R | G << 8 | B << 16 | E << 24 when EVERY texel is exactly (m / 256) 2^(E - 128)
                            // per channel -- true by construction for maps HDRLoader decoded (hdrloader.cpp:97-114) -- else NULL
  const uint2* hdr_pairs;   // hdr_rgbe's rows in pairs (or NULL): (H + 1) x W entries, [j][x] = (texel(max(j - 1, 0), x), texel(min(j, H - 1), x)),
                            // so the 2x2 footprint of a bilinear lookup is ONE 16-byte load (tex_fetch_rgbe; knob env_pairs; W >= 2)
  const float4* cache; // (x/w, y/h, pdf, 0)
  const float2* cache_xy; // the same cache as two planes (or NULL): (x/w, y/h) for SampleHdr, pdf for hdrPdf -- the two
  const float* cache_pdf; // texels a bilinear lookup takes from a row are then ONE 16- or 8-byte load (tex_fetch_xy / _pdf)
  int32_t env_w, env_h, env_filter;
  uint32_t sobol_mask; // 7: Sobol dimensions wrap d & 7 (the reference's table), 15: sixteen dimensions (ezrt_scene_set_sampler)
};

// integrators 51 and 52 share pathTracingImportanceSampling's loop (P5/fsh:810-890); 52 swaps in the anisotropic lobe
template <int INTEG>
constexpr bool integ_mis() { return INTEG == EZRT_INTEGRATOR_P5_MIS || INTEG == EZRT_INTEGRATOR_P5_MIS_ANISO; }
template <int INTEG>
constexpr bool integ_aniso_is() { return INTEG == EZRT_INTEGRATOR_P5_MIS_ANISO; }

// Exact unsigned division by a launch-invariant divisor (Granlund-Montgomery, round-up form): with L = ceil(log2 d)
// and m = floor(2^32 (2^L - d) / d) + 1,  floor(n / d) = (((n - t) >> 1) + t) >> (L - 1),  t = mulhi(m, n),  for every
// 32-bit n.  The queue <-> sample-slot <-> pixel maps divide by the number of 16x16 blocks / of queue granules, values
// only known at launch: the compiler's 32-bit division is ~30 instructions, and ray generation runs it three times
// per sample (it was VALU-bound on them).  tests/test_host_scene.py checks the host twin over the divisors' range.
struct FastDiv {
  uint32_t d, m, s; // s = L - 1; d == 1: m = 0 and the quotient is n
};
inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d ? d : 1u;
  f.m = 0u;
  f.s = 0u;
  if (f.d > 1u) {
    uint32_t L = 0;
    while ((1ull << L) < f.d) L++;
    f.m = (uint32_t)((((1ull << L) - f.d) << 32) / f.d) + 1u;
    f.s = L - 1u;
  }
  return f;
}
__host__ __device__ inline uint32_t fastdiv(uint32_t n, const FastDiv& f) {
  if (f.d == 1u) return n;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t t = __umulhi(f.m, n);
#else
  const uint32_t t = (uint32_t)(((unsigned long long)f.m * n) >> 32);
#endif
  return (((n - t) >> 1) + t) >> f.s;
}

constexpr uint32_t LEAF_BIT = 0x80000000u;

struct Counters { // per-thread, registers
  uint32_t rays, pops, inner, tris, mats, envmap, envcache;
};

// ---------------------------------------------------------------------------
// RNG: P5/fsh:315-331
// Work counters live in CTR_SLOTS copies (one 64-byte line each) and are summed by ezrt_counters: every wave adds
// its totals when it retires, and ONE counter word only sustains ~88 atomics/us chip-wide -- the 32 768 waves of
// the primary shading stage needed 370 us just to report their sample counts.
constexpr int CTR_SLOTS = 64;
EZD unsigned long long* ctr_slot(unsigned long long* base) {
  return base + (size_t)((blockIdx.x * 5u + (threadIdx.x >> 6)) & (CTR_SLOTS - 1)) * EZRT_CTR_COUNT;
}

// Lane mask of a predicate.  (HIP's __ballot takes an int: the bool is first materialised as 0/1
// in a VGPR and compared again -- two VALU slots per test in a VALU-bound loop.)
EZD unsigned long long ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }

EZD uint32_t wang_hash(uint32_t& seed) {
  seed = (seed ^ 61u) ^ (seed >> 16);
  seed *= 9u;
  seed = seed ^ (seed >> 4);
  seed *= 0x27d4eb2du;
  seed = seed ^ (seed >> 15);
  return seed;
}
EZD float rnd(uint32_t& seed) { return (float)wang_hash(seed) / 4294967296.0f; }

// CranleyPattersonRotation: P5/fsh:378-396.  The offsets depend on the pixel only.
EZD void cp_offsets(uint32_t ix, uint32_t iy, float& u, float& v) {
  uint32_t pseed = (ix * 1973u + iy * 9277u + 59u * 26699u) | 1u;
  u = (float)wang_hash(pseed) / 4294967296.0f;
  v = (float)wang_hash(pseed) / 4294967296.0f;
}
EZD float cp_rotate(float p, float off) {
  p += off;
  if (p > 1.0f) p -= 1.0f;
  if (p < 0.0f) p += 1.0f;
  return p;
}

// ---------------------------------------------------------------------------
// hitAABB: P5/fsh:220-233 with invdir hoisted (1.0/dir is the same value on
// every call of one ray).
EZD float hit_aabb(f3 S, f3 inv, f3 AA, f3 BB) {
  f3 f = (BB - S) * inv;
  f3 n = (AA - S) * inv;
  float t1 = ez_min(ez_max(f.x, n.x), ez_min(ez_max(f.y, n.y), ez_max(f.z, n.z)));
  float t0 = ez_max(ez_min(f.x, n.x), ez_max(ez_min(f.y, n.y), ez_min(f.z, n.z)));
  return (t1 >= t0) ? ((t0 > 0.0f) ? t0 : t1) : -1.0f;
}

// Same slab test on v_min_f32 / v_max_f32 / v_min3 / v_max3 (one issue slot each instead of
// compare + hazard nop + select).  Hardware min/max differ from (b<a)?b:a only on NaN operands and on
// the sign of a zero result; the result is consumed by comparisons only (sign of zero is invisible) and
// no NaN can arise when the ray's origin and 1/direction are finite (finite box minus finite origin
// times a finite factor is finite or +-inf, never NaN).  Callers use it only for such rays
// (ray_is_tame) and fall back to hit_aabb otherwise, so decisions stay bit-identical.
// (v_min/v_max straight from inline asm: through fminf/fmaxf the compiler first canonicalises every operand
// with a v_max_f32 x, x -- six more instructions per inner step of a loop that is bound by VALU issue)
EZD float hw_min(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
EZD float hw_max(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
EZD float hw_min3(float a, float b, float c) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
EZD float hw_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// the two slab tests on boxes already translated by the ray origin (see TraceQArgs.inner_rel)
EZD float hit_aabb_rel(f3 inv, f3 AA, f3 BB) {
  f3 f = BB * inv;
  f3 n = AA * inv;
  float t1 = ez_min(ez_max(f.x, n.x), ez_min(ez_max(f.y, n.y), ez_max(f.z, n.z)));
  float t0 = ez_max(ez_min(f.x, n.x), ez_max(ez_min(f.y, n.y), ez_min(f.z, n.z)));
  return (t1 >= t0) ? ((t0 > 0.0f) ? t0 : t1) : -1.0f;
}
EZD float hit_aabb_tame_rel(f3 inv, f3 AA, f3 BB) {
  f3 f = BB * inv;
  f3 n = AA * inv;
  float t1 = hw_min3(hw_max(f.x, n.x), hw_max(f.y, n.y), hw_max(f.z, n.z));
  float t0 = hw_max3(hw_min(f.x, n.x), hw_min(f.y, n.y), hw_min(f.z, n.z));
  return (t1 >= t0) ? ((t0 > 0.0f) ? t0 : t1) : -1.0f;
}
EZD float hit_aabb_tame(f3 S, f3 inv, f3 AA, f3 BB) {
  f3 f = (BB - S) * inv;
  f3 n = (AA - S) * inv;
  float t1 = hw_min3(hw_max(f.x, n.x), hw_max(f.y, n.y), hw_max(f.z, n.z));
  float t0 = hw_max3(hw_min(f.x, n.x), hw_min(f.y, n.y), hw_min(f.z, n.z));
  return (t1 >= t0) ? ((t0 > 0.0f) ? t0 : t1) : -1.0f;
}
// hit_aabb_tame that also hands out the entry distance t0 = max_k of the near-plane products (for distance pruning)
EZD float hit_aabb_tame_e(f3 S, f3 inv, f3 AA, f3 BB, float& t0_out) {
  f3 f = (BB - S) * inv;
  f3 n = (AA - S) * inv;
  float t1 = hw_min3(hw_max(f.x, n.x), hw_max(f.y, n.y), hw_max(f.z, n.z));
  float t0 = hw_max3(hw_min(f.x, n.x), hw_min(f.y, n.y), hw_min(f.z, n.z));
  t0_out = t0;
  return (t1 >= t0) ? ((t0 > 0.0f) ? t0 : t1) : -1.0f;
}
EZD bool ray_is_tame(f3 S, f3 inv) {
  const float big = 3.0e38f;
  return ez_abs(S.x) < big && ez_abs(S.y) < big && ez_abs(S.z) < big && ez_abs(inv.x) < big && ez_abs(inv.y) < big &&
         ez_abs(inv.z) < big;
}

// a finite ray with at least one direction component exactly +-0 (1/d = +-inf there): see ezrt_traceq4.h
EZD bool ray_is_semi(f3 S, f3 d, f3 inv) {
  const float big = 3.0e38f;
  const bool okx = ez_abs(inv.x) < big || d.x == 0.0f, oky = ez_abs(inv.y) < big || d.y == 0.0f, okz = ez_abs(inv.z) < big || d.z == 0.0f;
  return ez_abs(S.x) < big && ez_abs(S.y) < big && ez_abs(S.z) < big && okx && oky && okz && (d.x == 0.0f || d.y == 0.0f || d.z == 0.0f);
}

// hitTriangle, distance part: P5/fsh:160-198.  Flipping N (fsh:175-178) negates
// numerator, denominator and all three edge signs exactly, so t and the hit
// decision do not depend on it; isInside is recomputed for the winner.
EZD bool hit_triangle_t(const float4* __restrict__ g, f3 S, f3 d, float& t_out) {
  float4 a = g[0], b = g[1], c = g[2];
  f3 p1 = mk(a.x, a.y, a.z), p2 = mk(b.x, b.y, b.z), p3 = mk(c.x, c.y, c.z);
  f3 N = mk(a.w, b.w, c.w);
  float Nd = dot(N, d);
  if (ez_abs(Nd) < 0.00001f) return false;
  float t = (dot(N, p1) - dot(S, N)) / Nd;
  if (t < 0.0005f) return false;
  f3 P = S + d * t;
  f3 c1 = cross(p2 - p1, P - p1);
  f3 c2 = cross(p3 - p2, P - p2);
  f3 c3 = cross(p1 - p3, P - p3);
  float s1 = dot(c1, N), s2 = dot(c2, N), s3 = dot(c3, N);
  bool r1 = (s1 > 0.0f) && (s2 > 0.0f) && (s3 > 0.0f);
  bool r2 = (s1 < 0.0f) && (s2 < 0.0f) && (s3 < 0.0f);
  t_out = t;
  return r1 || r2;
}

// ---- closest-point queries (include/ezrt_closest_point.h, where the definition is the contract): the region form of the
// point-triangle projection, case by case in the header's order, then q clamped to the triangle's bounding box.  Returns dist2 =
// dot(p - q, p - q); q and the barycentrics (v, w) of the projection come back by reference.
// (closest_point_abc: the same on vertices held in registers -- the triangle-distance rule below asks it with the roles swapped)
EZD float closest_point_abc(f3 a, f3 b, f3 c, f3 p, f3& q, float& v, float& w) {
  const f3 ab = b - a, ac = c - a, ap = p - a;
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  const f3 bp = p - b;
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  const f3 cp = p - c;
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (d1 <= 0.0f && d2 <= 0.0f) {
    v = 0.0f, w = 0.0f;
  } else if (d3 >= 0.0f && d4 <= d3) {
    v = 1.0f, w = 0.0f;
  } else {
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
      v = d1 / (d1 - d3), w = 0.0f;
    } else if (d6 >= 0.0f && d5 <= d6) {
      v = 0.0f, w = 1.0f;
    } else {
      const float vb = d5 * d2 - d1 * d6;
      if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        v = 0.0f, w = d2 / (d2 - d6);
      } else {
        const float va = d3 * d6 - d5 * d4;
        if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {
          w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
          v = 1.0f - w;
        } else {
          const float s = va + vb + vc;
          v = vb / s, w = vc / s;
        }
      }
    }
  }
  const f3 qp = (a + ab * v) + ac * w;
  const f3 lo = mk(ez_min(ez_min(a.x, b.x), c.x), ez_min(ez_min(a.y, b.y), c.y), ez_min(ez_min(a.z, b.z), c.z));
  const f3 hi = mk(ez_max(ez_max(a.x, b.x), c.x), ez_max(ez_max(a.y, b.y), c.y), ez_max(ez_max(a.z, b.z), c.z));
  q = mk(qp.x < lo.x ? lo.x : (qp.x > hi.x ? hi.x : qp.x), qp.y < lo.y ? lo.y : (qp.y > hi.y ? hi.y : qp.y),
         qp.z < lo.z ? lo.z : (qp.z > hi.z ? hi.z : qp.z));
  const f3 e = p - q;
  return dot(e, e);
}
EZD float closest_point_triangle(const float4* __restrict__ g, f3 p, f3& q, float& v, float& w) {
  const float4 ga = g[0], gb = g[1], gc = g[2];
  return closest_point_abc(mk(ga.x, ga.y, ga.z), mk(gb.x, gb.y, gb.z), mk(gc.x, gc.y, gc.z), p, q, v, w);
}
// The running answer of one query point.  A candidate is a triangle with a finite dist2 <= the bound; the smallest dist2 wins and,
// among equal dist2, the smallest index -- whatever the order in which the triangles are met.  `best` starts as the bound B
// (tri = -1): it is the pruning radius of the walk from the first step on.
struct ClosestBest {
  float best, v, w;
  int32_t tri;
  f3 q;
};
EZD void closest_point_candidate(ClosestBest& r, const float4* __restrict__ tri_geom, int32_t k, f3 p) {
  f3 q;
  float v, w;
  const float d2 = closest_point_triangle(tri_geom + (size_t)k * 3, p, q, v, w);
  // (d2 <= best is false for a NaN d2, d2 < inf for an infinite one; best is never NaN)
  if (d2 < __builtin_inff() && (d2 < r.best || (d2 == r.best && (r.tri < 0 || k < r.tri)))) {
    r.best = d2;
    r.tri = k;
    r.q = q;
    r.v = v;
    r.w = w;
  }
}
// lb of a box: dot(g, g), g = max(lo - p, 0, p - hi) per axis (fmaxf: a NaN difference counts as 0).  For a finite p and a box that
// holds the bounding box of a triangle, lb <= that triangle's dist2 on the bits (ezrt_point_queries.h: point_walk).
EZD float closest_point_box(f3 p, f3 lo, f3 hi) {
  const f3 g = mk(__builtin_fmaxf(__builtin_fmaxf(lo.x - p.x, 0.0f), p.x - hi.x), __builtin_fmaxf(__builtin_fmaxf(lo.y - p.y, 0.0f), p.y - hi.y),
                  __builtin_fmaxf(__builtin_fmaxf(lo.z - p.z, 0.0f), p.z - hi.z));
  return dot(g, g);
}
// ... and of a box against the query triangle's bounding box [qlo, qhi] (include/ezrt_tri_distance.h): g = max(lo - qhi, 0, qlo - hi)
// per axis.  For a box that holds the bounding box of a triangle, lb <= that pair's dist2 on the bits (ezrt_point_queries.h:
// tri_distance_kernel).
EZD float tri_distance_box(f3 qlo, f3 qhi, f3 lo, f3 hi) {
  const f3 g = mk(__builtin_fmaxf(__builtin_fmaxf(lo.x - qhi.x, 0.0f), qlo.x - hi.x), __builtin_fmaxf(__builtin_fmaxf(lo.y - qhi.y, 0.0f), qlo.y - hi.y),
                  __builtin_fmaxf(__builtin_fmaxf(lo.z - qhi.z, 0.0f), qlo.z - hi.z));
  return dot(g, g);
}
// The closest points of the closed segments [P1, Q1] and [P2, Q2], in the order of include/ezrt_tri_distance.h: x on the first, y on
// the second, each clamped to its segment's bounding box.  Returns dot(x - y, x - y).
EZD float seg_clamp01(float v) { return ez_min(ez_max(v, 0.0f), 1.0f); }
EZD f3 seg_point(f3 P, f3 Q, f3 d, float s) {
  const f3 r = P + d * s;
  const f3 lo = mk(ez_min(P.x, Q.x), ez_min(P.y, Q.y), ez_min(P.z, Q.z)), hi = mk(ez_max(P.x, Q.x), ez_max(P.y, Q.y), ez_max(P.z, Q.z));
  return mk(r.x < lo.x ? lo.x : (r.x > hi.x ? hi.x : r.x), r.y < lo.y ? lo.y : (r.y > hi.y ? hi.y : r.y),
            r.z < lo.z ? lo.z : (r.z > hi.z ? hi.z : r.z));
}
EZD float segment_segment_closest(f3 P1, f3 Q1, f3 P2, f3 Q2, f3& x, f3& y) {
  const f3 d1 = Q1 - P1, d2 = Q2 - P2, r = P1 - P2;
  const float a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2);
  const float den = a * e - b * b;
  float s = den > 0.0f ? seg_clamp01((b * f - c * e) / den) : 0.0f;
  float t = (b * s + f) / e;
  if (t < 0.0f) {
    t = 0.0f;
    s = seg_clamp01(-c / a);
  } else if (t > 1.0f) {
    t = 1.0f;
    s = seg_clamp01((b - c) / a);
  }
  x = seg_point(P1, Q1, d1, s);
  y = seg_point(P2, Q2, d2, t);
  const f3 g = x - y;
  return dot(g, g);
}

// ---- inside queries (include/ezrt_inside.h, where the definition is the contract): the frame of an axis and the crossing rule
// G1 .. G6 of one triangle, in the header's order.  The axis is a runtime permutation (uniform over the launch: the selects are on
// scalar conditions), not six instances.
struct InsideFrame {
  int c;    // the ray's coordinate: axis >> 1
  float g;  // -1 for the negative axes
  float ps, pt, pu; // the query point in the frame
};
EZD float inside_pick(float x, float y, float z, int c) { return c == 0 ? x : (c == 1 ? y : z); }
EZD InsideFrame inside_frame(int axis, f3 p) {
  InsideFrame f;
  f.c = axis >> 1;
  f.g = (axis & 1) ? -1.0f : 1.0f;
  f.ps = inside_pick(p.y, p.z, p.x, f.c);
  f.pt = inside_pick(p.z, p.x, p.y, f.c);
  f.pu = f.g * inside_pick(p.x, p.y, p.z, f.c);
  return f;
}
EZD bool inside_crossed(const float4* __restrict__ tg, const InsideFrame& f) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  float as = inside_pick(ga.y, ga.z, ga.x, f.c), at = inside_pick(ga.z, ga.x, ga.y, f.c), au = f.g * inside_pick(ga.x, ga.y, ga.z, f.c);
  float bs = inside_pick(gb.y, gb.z, gb.x, f.c), bt = inside_pick(gb.z, gb.x, gb.y, f.c), bu = f.g * inside_pick(gb.x, gb.y, gb.z, f.c);
  float cs = inside_pick(gc.y, gc.z, gc.x, f.c), ct = inside_pick(gc.z, gc.x, gc.y, f.c), cu = f.g * inside_pick(gc.x, gc.y, gc.z, f.c);
  const bool ka = as <= f.ps, kb = bs <= f.ps, kc = cs <= f.ps;
  if (!((ka || kb || kc) && !(ka && kb && kc))) return false;                                                   // G1
  if (!((at <= f.pt || bt <= f.pt || ct <= f.pt) && (at >= f.pt || bt >= f.pt || ct >= f.pt))) return false;    // G2
  if (!(au > f.pu || bu > f.pu || cu > f.pu)) return false;                                                     // G3
  auto cswap = [](float& xs, float& xt, float& xu, float& ys, float& yt, float& yu) {
    if (ys < xs || (ys == xs && (yt < xt || (yt == xt && yu < xu)))) { // less(y, x)
      float h = xs;
      xs = ys, ys = h;
      h = xt, xt = yt, yt = h;
      h = xu, xu = yu, yu = h;
    }
  };
  cswap(as, at, au, bs, bt, bu);
  cswap(bs, bt, bu, cs, ct, cu);
  cswap(as, at, au, bs, bt, bu);
  // fp64 from here: (v0 v1 v2) = (a b c)
  const double s0 = (double)as, t0 = (double)at, u0 = (double)au;
  const double s1 = (double)bs - s0, t1 = (double)bt - t0, s2 = (double)cs - s0, t2 = (double)ct - t0;
  const double A = s1 * t2 - t1 * s2;
  if (!(__builtin_fabs(A) < __builtin_inf() && A != 0.0)) return false;                                         // G4
  const double qs = (double)f.ps - s0, qt = (double)f.pt - t0;
  const double E02 = s2 * qt - t2 * qs;
  double E;
  if (bs <= f.ps) {
    const double s12 = (double)cs - (double)bs, t12 = (double)ct - (double)bt;
    const double rs = (double)f.ps - (double)bs, rt = (double)f.pt - (double)bt;
    E = s12 * rt - t12 * rs;
  } else {
    E = s1 * qt - t1 * qs;
  }
  if ((E02 < 0.0) == (E < 0.0)) return false;                                                                   // G5
  const double u1 = (double)bu - u0, u2 = (double)cu - u0;
  const double Ns = t1 * u2 - u1 * t2;
  const double Nt = u1 * s2 - s1 * u2;
  const double D = (Ns * qs + Nt * qt) + A * ((double)f.pu - u0);
  return __builtin_fabs(D) < __builtin_inf() && ((D < 0.0 && A > 0.0) || (D > 0.0 && A < 0.0));                 // G6
}

// ---- winding-number queries (include/ezrt_winding.h, where the definition is the contract): W1 of one triangle (winding_tri: the
// vertices in the order of their values, converted to fp64, and sgn -- which depend on the triangle alone, so where the triangle is
// uniform across a wave this is scalar work) and W2 .. W4 of one point against it (winding_term), in the header's order.
struct WindingTri {
  double v[9];  // v0 v1 v2
  float sgn;    // +-1: the parity of the sort; 0: the triangle has no term (a non-finite coordinate, two vertices equal by value)
};
EZD void winding_tri(const float4* __restrict__ tg, WindingTri& w) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  float ax = ga.x, ay = ga.y, az = ga.z, bx = gb.x, by = gb.y, bz = gb.z, cx = gc.x, cy = gc.y, cz = gc.z;
  const float inf = __builtin_inff();
  const bool finite = ez_abs(ax) < inf && ez_abs(ay) < inf && ez_abs(az) < inf && ez_abs(bx) < inf && ez_abs(by) < inf &&
                      ez_abs(bz) < inf && ez_abs(cx) < inf && ez_abs(cy) < inf && ez_abs(cz) < inf;
  // the three compare-and-swaps as selects, and the parity of the swaps that happened
  auto cswap = [](float& xx, float& xy, float& xz, float& yx, float& yy, float& yz) {
    const bool sw = yx < xx || (yx == xx && (yy < xy || (yy == xy && yz < xz))); // less(y, x)
    const float lx = sw ? yx : xx, ly = sw ? yy : xy, lz = sw ? yz : xz;
    const float hx = sw ? xx : yx, hy = sw ? xy : yy, hz = sw ? xz : yz;
    xx = lx, xy = ly, xz = lz, yx = hx, yy = hy, yz = hz;
    return sw;
  };
  const bool s1 = cswap(ax, ay, az, bx, by, bz);
  const bool s2 = cswap(bx, by, bz, cx, cy, cz);
  const bool s3 = cswap(ax, ay, az, bx, by, bz);
  const float sgn = ((s1 != s2) != s3) ? -1.0f : 1.0f;
  const bool repeated = (ax == bx && ay == by && az == bz) || (bx == cx && by == cy && bz == cz);
  w.v[0] = (double)ax, w.v[1] = (double)ay, w.v[2] = (double)az;
  w.v[3] = (double)bx, w.v[4] = (double)by, w.v[5] = (double)bz;
  w.v[6] = (double)cx, w.v[7] = (double)cy, w.v[8] = (double)cz;
  w.sgn = (finite && !repeated) ? sgn : 0.0f;
}
// q_k of the FINITE point (px, py, pz) and a triangle with w.sgn != 0
EZD long long winding_term(const WindingTri& w, double px, double py, double pz) {
  const double ax = w.v[0] - px, ay = w.v[1] - py, az = w.v[2] - pz;
  const double bx = w.v[3] - px, by = w.v[4] - py, bz = w.v[5] - pz;
  const double cx = w.v[6] - px, cy = w.v[7] - py, cz = w.v[8] - pz;
  const double nx = by * cz - bz * cy;
  const double ny = bz * cx - bx * cz;
  const double nz = bx * cy - by * cx;
  const double det = (ax * nx + ay * ny) + az * nz;
  const double la = __builtin_sqrt((ax * ax + ay * ay) + az * az);
  const double lb = __builtin_sqrt((bx * bx + by * by) + bz * bz);
  const double lc = __builtin_sqrt((cx * cx + cy * cy) + cz * cz);
  const double ab = (ax * bx + ay * by) + az * bz;
  const double bc = (bx * cx + by * cy) + bz * cz;
  const double ca = (cx * ax + cy * ay) + cz * az;
  const double den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
  const double fdet = __builtin_fabs(det), fden = __builtin_fabs(den), dinf = __builtin_inf();
  if (!(det != 0.0 && fdet < dinf && fden < dinf)) return 0;                                                      // W3
  const double m = fdet < fden ? fden : fdet;
  if (m == 0.0) return 0;
  const float t = w.sgn * ez_atan2((float)(det / m), (float)(den / m));
  return (long long)__builtin_rint((double)t * 0x1p36);                                                           // W4
}
// W5's conversion of the sum
EZD float winding_of(long long S) { return (float)(((double)S * 0x1p-36) * 0x1.45f306dc9c883p-3); }
// the single term of a pair, for ezrt_winding_at_device
EZD long long winding_pair(const float4* __restrict__ tg, f3 p) {
  const float inf = __builtin_inff();
  if (!(ez_abs(p.x) < inf && ez_abs(p.y) < inf && ez_abs(p.z) < inf)) return 0;
  WindingTri w;
  winding_tri(tg, w);
  if (w.sgn == 0.0f) return 0;
  return winding_term(w, (double)p.x, (double)p.y, (double)p.z);
}

// ---- plane queries (include/ezrt_plane.h, where the definition is the contract): P1 (plane_load), P2 (plane_side), P3
// (plane_crossed), P4 (plane_point) and P5 (plane_segment), in the header's order.  A triangle is held as nine doubles, the exact
// conversions of its fp32 coordinates (a conversion back is exact too), so a kernel converts it once for all planes.
struct PlaneEq {
  double a, b, c, d;
  int live; // P1
};
EZD void plane_load(const float* __restrict__ p4, PlaneEq& pl) {
  const float a = p4[0], b = p4[1], c = p4[2], d = p4[3], inf = __builtin_inff();
  pl.a = (double)a, pl.b = (double)b, pl.c = (double)c, pl.d = (double)d;
  pl.live = ez_abs(a) < inf && ez_abs(b) < inf && ez_abs(c) < inf && ez_abs(d) < inf && !(a == 0.0f && b == 0.0f && c == 0.0f);
}
EZD double plane_side(const PlaneEq& pl, double x, double y, double z) { return ((pl.a * x + pl.b * y) + pl.c * z) - pl.d; }
// the nine coordinates of tri_geom's rows as doubles; false where one of them is not finite
EZD bool plane_tri(const float4* __restrict__ tg, double v[9]) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  const float inf = __builtin_inff();
  v[0] = (double)ga.x, v[1] = (double)ga.y, v[2] = (double)ga.z;
  v[3] = (double)gb.x, v[4] = (double)gb.y, v[5] = (double)gb.z;
  v[6] = (double)gc.x, v[7] = (double)gc.y, v[8] = (double)gc.z;
  return ez_abs(ga.x) < inf && ez_abs(ga.y) < inf && ez_abs(ga.z) < inf && ez_abs(gb.x) < inf && ez_abs(gb.y) < inf &&
         ez_abs(gb.z) < inf && ez_abs(gc.x) < inf && ez_abs(gc.y) < inf && ez_abs(gc.z) < inf;
}
// P3 of a triangle with finite coordinates and a live plane, from the three sides
EZD bool plane_crossed(double s0, double s1, double s2) {
  const bool u0 = s0 >= 0.0, u1 = s1 >= 0.0, u2 = s2 >= 0.0;
  return !(u0 && u1 && u2) && (u0 || u1 || u2);
}
// P4: one coordinate of the point of the edge with the ends A < B (the order of their values), sides sa and sb, t = sa / (sa - sb)
EZD float plane_coord(double A, double B, double sa, double sb, double t) {
  const float a = (float)A, b = (float)B; // exact
  float p = (float)(A + t * (B - A));
  const float lo = b < a ? b : a, hi = b < a ? a : b;
  p = p < lo ? lo : (p > hi ? hi : p);
  return sa == 0.0 ? a : (sb == 0.0 ? b : p);
}
// P4: the point of the edge with the ends X and Y (sides sx and sy, one UP and one DOWN), whichever way round they are given
EZD f3 plane_point(double Xx, double Xy, double Xz, double sx, double Yx, double Yy, double Yz, double sy) {
  const bool sw = Yx < Xx || (Yx == Xx && (Yy < Xy || (Yy == Xy && Yz < Xz))); // less(Y, X)
  const double sa = sw ? sy : sx, sb = sw ? sx : sy;
  const double t = sa / (sa - sb);
  return mk(plane_coord(sw ? Yx : Xx, sw ? Xx : Yx, sa, sb, t), plane_coord(sw ? Yy : Xy, sw ? Xy : Yy, sa, sb, t),
            plane_coord(sw ? Yz : Xz, sw ? Xz : Yz, sa, sb, t));
}
// P5: (q0, q1) of a CROSSED triangle: the point of the directed edge that goes UP -> DOWN (p1 p2, p2 p3 or p3 p1), and of the one
// that goes DOWN -> UP.  (Written on the three edges' points under selects of scalars: nothing is indexed.)
EZD void plane_segment(const double v[9], double s0, double s1, double s2, f3& q0, f3& q1) {
  const double x0 = v[0], y0 = v[1], z0 = v[2], x1 = v[3], y1 = v[4], z1 = v[5], x2 = v[6], y2 = v[7], z2 = v[8];
  const bool u0 = s0 >= 0.0, u1 = s1 >= 0.0, u2 = s2 >= 0.0;
  const bool a0 = u0 && !u1, a1 = !a0 && u1 && !u2;   // q0's edge is p1 p2, p2 p3, else p3 p1
  const bool b0 = !u0 && u1, b1 = !b0 && !u1 && u2;   // q1's edge likewise
  q0 = plane_point(a0 ? x0 : (a1 ? x1 : x2), a0 ? y0 : (a1 ? y1 : y2), a0 ? z0 : (a1 ? z1 : z2), a0 ? s0 : (a1 ? s1 : s2),
                   a0 ? x1 : (a1 ? x2 : x0), a0 ? y1 : (a1 ? y2 : y0), a0 ? z1 : (a1 ? z2 : z0), a0 ? s1 : (a1 ? s2 : s0));
  q1 = plane_point(b0 ? x0 : (b1 ? x1 : x2), b0 ? y0 : (b1 ? y1 : y2), b0 ? z0 : (b1 ? z1 : z2), b0 ? s0 : (b1 ? s1 : s2),
                   b0 ? x1 : (b1 ? x2 : x0), b0 ? y1 : (b1 ? y2 : y0), b0 ? z1 : (b1 ? z2 : z0), b0 ? s1 : (b1 ? s2 : s0));
}

// ---- box-overlap queries (include/ezrt_box_overlap.h, where the definition is the contract): H1 .. H3 of one triangle against a
// LIVE box (the caller has checked the box), in the header's order.  An edge axis has a[j] = 0: its term a[j] * d is a zero (d is
// finite), and adding a zero changes at most the sign of a zero sum, which no comparison sees -- so those terms are left out and
// bmin, bmax and t are sums of two products.  Only the live state of one edge is held at a time: the three edges are one loop that
// is not unrolled, with (A, B, C) moved from one edge to the next between its rounds.
struct BoxInterval {
  double mn, mx;
};
// t_c of bmin and of bmax for one component: a * d(lo, A) and a * d(hi, A), given to bmin and bmax by the sign of a
EZD BoxInterval box_term(double a, double dl, double dh) {
  const double pl = a * dl, ph = a * dh;
  const bool up = a >= 0.0;
  return BoxInterval{up ? pl : ph, up ? ph : pl};
}
// does e x (box axis j) separate?  (u, w) = ((j + 1) % 3, (j + 2) % 3): a[u] = -e[w], a[w] = e[u]; q = C - A
EZD bool box_edge_axis_separates(double eu, double ew, double dlu, double dhu, double dlw, double dhw, double qu, double qw) {
  const double au = -ew, aw = eu;
  const BoxInterval tu = box_term(au, dlu, dhu), tw = box_term(aw, dlw, dhw);
  const double bmin = tu.mn + tw.mn, bmax = tu.mx + tw.mx;
  const double t = au * qu + aw * qw;
  return bmin > (t > 0.0 ? t : 0.0) || bmax < (t < 0.0 ? t : 0.0);
}
// a live box: six finite numbers and lo <= hi on every axis (false for a NaN); a box that is not live overlaps nothing
EZD bool box_live(f3 lo, f3 hi) {
  const float inf = __builtin_inff();
  return ez_abs(lo.x) < inf && ez_abs(lo.y) < inf && ez_abs(lo.z) < inf && ez_abs(hi.x) < inf && ez_abs(hi.y) < inf && ez_abs(hi.z) < inf &&
         lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
}
EZD bool box_overlaps(const float4* __restrict__ tg, f3 lo, f3 hi) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  f3 a = mk(ga.x, ga.y, ga.z), b = mk(gb.x, gb.y, gb.z), c = mk(gc.x, gc.y, gc.z);
  if (!((a.x <= hi.x || b.x <= hi.x || c.x <= hi.x) && (a.x >= lo.x || b.x >= lo.x || c.x >= lo.x))) return false;   // H1
  if (!((a.y <= hi.y || b.y <= hi.y || c.y <= hi.y) && (a.y >= lo.y || b.y >= lo.y || c.y >= lo.y))) return false;
  if (!((a.z <= hi.z || b.z <= hi.z || c.z <= hi.z) && (a.z >= lo.z || b.z >= lo.z || c.z >= lo.z))) return false;
  const float inf = __builtin_inff();
  if (!(ez_abs(a.x) < inf && ez_abs(a.y) < inf && ez_abs(a.z) < inf && ez_abs(b.x) < inf && ez_abs(b.y) < inf && ez_abs(b.z) < inf &&
        ez_abs(c.x) < inf && ez_abs(c.y) < inf && ez_abs(c.z) < inf))
    return false; // a non-finite vertex never overlaps
  auto cswap = [](f3& x, f3& y) {
    if (y.x < x.x || (y.x == x.x && (y.y < x.y || (y.y == x.y && y.z < x.z)))) { // less(y, x)
      const f3 h = x;
      x = y, y = h;
    }
  };
  cswap(a, b);
  cswap(b, c);
  cswap(a, b);
  // fp64 from here: (v0 v1 v2) = (a b c)
  {
    const double e1x = (double)b.x - (double)a.x, e1y = (double)b.y - (double)a.y, e1z = (double)b.z - (double)a.z;
    const double e2x = (double)c.x - (double)a.x, e2y = (double)c.y - (double)a.y, e2z = (double)c.z - (double)a.z;
    const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
    const BoxInterval t0 = box_term(Nx, (double)lo.x - (double)a.x, (double)hi.x - (double)a.x);
    const BoxInterval t1 = box_term(Ny, (double)lo.y - (double)a.y, (double)hi.y - (double)a.y);
    const BoxInterval t2 = box_term(Nz, (double)lo.z - (double)a.z, (double)hi.z - (double)a.z);
    if (!((t0.mn + t1.mn) + t2.mn <= 0.0 && (t0.mx + t1.mx) + t2.mx >= 0.0)) return false;                              // H2
  }
  // H3: (A, B; C) = (v0, v1; v2), then (v1, v2; v0), then (v0, v2; v1)
  f3 A = a, B = b, C = c;
#pragma unroll 1
  for (int edge = 0; edge < 3; edge++) {
    const double ex = (double)B.x - (double)A.x, ey = (double)B.y - (double)A.y, ez = (double)B.z - (double)A.z;
    const double qx = (double)C.x - (double)A.x, qy = (double)C.y - (double)A.y, qz = (double)C.z - (double)A.z;
    const double lx = (double)lo.x - (double)A.x, ly = (double)lo.y - (double)A.y, lz = (double)lo.z - (double)A.z;
    const double hx = (double)hi.x - (double)A.x, hy = (double)hi.y - (double)A.y, hz = (double)hi.z - (double)A.z;
    if (box_edge_axis_separates(ey, ez, ly, hy, lz, hz, qy, qz)) return false; // j = 0: (u, w) = (y, z)
    if (box_edge_axis_separates(ez, ex, lz, hz, lx, hx, qz, qx)) return false; // j = 1: (z, x)
    if (box_edge_axis_separates(ex, ey, lx, hx, ly, hy, qx, qy)) return false; // j = 2: (x, y)
    const f3 h = A; // (v0, v1; v2) -> (v1, v2; v0): rotate;  (v1, v2; v0) -> (v0, v2; v1): exchange A and C
    if (edge == 0) A = B, B = C, C = h;
    else A = C, C = h;
  }
  return true;
}

// ---- oriented-box queries (include/ezrt_obb_overlap.h, where the definition is the contract): the per-box numbers (obb_query: n_j,
// r_j and the hull, once per box), the two gates of a walk (obb_hull_gate, obb_face_gate) and H0 .. H3 of one triangle against a LIVE
// box (obb_overlaps), in the header's order.  H0 is asked in fp32 against the hull rounded inward -- the same answer as the fp64
// comparison for every fp32 coordinate, a NaN or an infinity included.  The axes are kept as the caller's fp32 numbers and converted
// where they are used (exact, and 9 registers instead of 18); only one edge's fp64 state is live at a time, as in box_overlaps: the
// three edges are one loop that is not unrolled, with (A, B, C) moved from one edge to the next between its rounds.
struct d3 {
  double x, y, z;
};
EZD d3 obb_up(f3 u) { return d3{(double)u.x, (double)u.y, (double)u.z}; }
EZD d3 obb_d(f3 x, f3 y) { return d3{(double)x.x - (double)y.x, (double)x.y - (double)y.y, (double)x.z - (double)y.z}; }
EZD double obb_dot(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
EZD d3 obb_cross(d3 a, d3 b) { return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// x rounded to fp32 toward minus infinity / toward plus infinity (x finite; a result past the largest float is that float's)
EZD float obb_round_down(double x) {
  const float f = (float)x;
  if (!((double)f > x)) return f;
  const uint32_t b = __builtin_bit_cast(uint32_t, f);
  return __builtin_bit_cast(float, f > 0.0f ? b - 1u : (f < 0.0f ? b + 1u : 0x80000001u));
}
EZD float obb_round_up(double x) { return -obb_round_down(-x); }
struct ObbQuery {
  f3 c, u0, u1, u2; // the caller's twelve numbers
  f3 lo, hi;        // the hull rounded inward to fp32: the first gate of the walk, and H0
  d3 n0, n1, n2;    // the face directions
  double r0, r1, r2;
};
// the box as the kernels hold it; false when it is not live (q is then not to be used)
EZD bool obb_query(f3 c, f3 u0, f3 u1, f3 u2, ObbQuery& q) {
  const float inf = __builtin_inff();
  if (!(ez_abs(c.x) < inf && ez_abs(c.y) < inf && ez_abs(c.z) < inf && ez_abs(u0.x) < inf && ez_abs(u0.y) < inf && ez_abs(u0.z) < inf &&
        ez_abs(u1.x) < inf && ez_abs(u1.y) < inf && ez_abs(u1.z) < inf && ez_abs(u2.x) < inf && ez_abs(u2.y) < inf && ez_abs(u2.z) < inf))
    return false;
  q.c = c, q.u0 = u0, q.u1 = u1, q.u2 = u2;
  const d3 U0 = obb_up(u0), U1 = obb_up(u1), U2 = obb_up(u2);
  q.n0 = obb_cross(U1, U2), q.n1 = obb_cross(U2, U0), q.n2 = obb_cross(U0, U1);
  q.r0 = __builtin_fabs(obb_dot(q.n0, U0)), q.r1 = __builtin_fabs(obb_dot(q.n1, U1)), q.r2 = __builtin_fabs(obb_dot(q.n2, U2));
  const double hx = (__builtin_fabs(U0.x) + __builtin_fabs(U1.x)) + __builtin_fabs(U2.x);
  const double hy = (__builtin_fabs(U0.y) + __builtin_fabs(U1.y)) + __builtin_fabs(U2.y);
  const double hz = (__builtin_fabs(U0.z) + __builtin_fabs(U1.z)) + __builtin_fabs(U2.z);
  q.lo = mk(obb_round_up((double)c.x - hx), obb_round_up((double)c.y - hy), obb_round_up((double)c.z - hz));
  q.hi = mk(obb_round_down((double)c.x + hx), obb_round_down((double)c.y + hy), obb_round_down((double)c.z + hz));
  return q.r0 > 0.0 && q.r1 > 0.0 && q.r2 > 0.0;
}
// the first gate of a slot's box [lo, hi]: H0 on the box.  An unused slot (an all-NaN box) fails it.
EZD bool obb_hull_gate(const ObbQuery& q, f3 lo, f3 hi) {
  return lo.x <= q.hi.x && hi.x >= q.lo.x && lo.y <= q.hi.y && hi.y >= q.lo.y && lo.z <= q.hi.z && hi.z >= q.lo.z;
}
// one face direction against the box [c + dl, c + dh] (dl = d(lo, c), dh = d(hi, c)): p_j at the corner chosen per component by the
// sign of n[c], by the rule's own expression.  pmin <= p_j(v) <= pmax on the bits for every fp32 v in the box: no margin.
EZD bool obb_face_misses(d3 n, double r, d3 dl, d3 dh) {
  const double lx = n.x * dl.x, hx = n.x * dh.x, ly = n.y * dl.y, hy = n.y * dh.y, lz = n.z * dl.z, hz = n.z * dh.z;
  const bool ux = n.x >= 0.0, uy = n.y >= 0.0, uz = n.z >= 0.0;
  const double pmin = ((ux ? lx : hx) + (uy ? ly : hy)) + (uz ? lz : hz);
  const double pmax = ((ux ? hx : lx) + (uy ? hy : ly)) + (uz ? hz : lz);
  return pmin > r || pmax < -r; // (false for a NaN: such a box is not skipped)
}
// the second gate, asked only behind the first: no face direction has the whole box on one side
EZD bool obb_face_gate(const ObbQuery& q, f3 lo, f3 hi) {
  const d3 dl = obb_d(lo, q.c), dh = obb_d(hi, q.c);
  return !(obb_face_misses(q.n0, q.r0, dl, dh) || obb_face_misses(q.n1, q.r1, dl, dh) || obb_face_misses(q.n2, q.r2, dl, dh));
}
// H1 for one j: some vertex has p <= r and some vertex has p >= -r
EZD bool obb_face_holds(d3 n, double r, d3 da, d3 db, d3 dc) {
  const double pa = obb_dot(n, da), pb = obb_dot(n, db), pc = obb_dot(n, dc);
  return (pa <= r || pb <= r || pc <= r) && (pa >= -r || pb >= -r || pc >= -r);
}
// does cross(U_j, e) separate?  q = d(C, A), g = d(c, A); (Uv, Uw) = (U_{j+1}, U_{j+2})
EZD bool obb_edge_axis_separates(f3 uj, f3 uv, f3 uw, d3 e, d3 q, d3 g) {
  const d3 a = obb_cross(obb_up(uj), e);
  const double t = obb_dot(a, q), s = obb_dot(a, g);
  const double R = __builtin_fabs(obb_dot(a, obb_up(uv))) + __builtin_fabs(obb_dot(a, obb_up(uw)));
  return s - R > (t > 0.0 ? t : 0.0) || s + R < (t < 0.0 ? t : 0.0);
}
EZD bool obb_overlaps(const float4* __restrict__ tg, const ObbQuery& q) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  f3 a = mk(ga.x, ga.y, ga.z), b = mk(gb.x, gb.y, gb.z), c = mk(gc.x, gc.y, gc.z);
  if (!((a.x <= q.hi.x || b.x <= q.hi.x || c.x <= q.hi.x) && (a.x >= q.lo.x || b.x >= q.lo.x || c.x >= q.lo.x))) return false; // H0
  if (!((a.y <= q.hi.y || b.y <= q.hi.y || c.y <= q.hi.y) && (a.y >= q.lo.y || b.y >= q.lo.y || c.y >= q.lo.y))) return false;
  if (!((a.z <= q.hi.z || b.z <= q.hi.z || c.z <= q.hi.z) && (a.z >= q.lo.z || b.z >= q.lo.z || c.z >= q.lo.z))) return false;
  const float inf = __builtin_inff();
  if (!(ez_abs(a.x) < inf && ez_abs(a.y) < inf && ez_abs(a.z) < inf && ez_abs(b.x) < inf && ez_abs(b.y) < inf && ez_abs(b.z) < inf &&
        ez_abs(c.x) < inf && ez_abs(c.y) < inf && ez_abs(c.z) < inf))
    return false; // a non-finite vertex never overlaps
  {
    const d3 da = obb_d(a, q.c), db = obb_d(b, q.c), dc = obb_d(c, q.c);
    if (!obb_face_holds(q.n0, q.r0, da, db, dc)) return false;                                                          // H1
    if (!obb_face_holds(q.n1, q.r1, da, db, dc)) return false;
    if (!obb_face_holds(q.n2, q.r2, da, db, dc)) return false;
  }
  auto cswap = [](f3& x, f3& y) {
    if (y.x < x.x || (y.x == x.x && (y.y < x.y || (y.y == x.y && y.z < x.z)))) { // less(y, x)
      const f3 h = x;
      x = y, y = h;
    }
  };
  cswap(a, b);
  cswap(b, c);
  cswap(a, b);
  // (v0 v1 v2) = (a b c)
  {
    const d3 N = obb_cross(obb_d(b, a), obb_d(c, a));
    const double s = obb_dot(N, obb_d(q.c, a));
    const double R = (__builtin_fabs(obb_dot(N, obb_up(q.u0))) + __builtin_fabs(obb_dot(N, obb_up(q.u1)))) + __builtin_fabs(obb_dot(N, obb_up(q.u2)));
    if (!(__builtin_fabs(s) <= R)) return false;                                                                         // H2
  }
  // H3: (A, B; C) = (v0, v1; v2), then (v1, v2; v0), then (v0, v2; v1)
  f3 A = a, B = b, C = c;
#pragma unroll 1
  for (int edge = 0; edge < 3; edge++) {
    const d3 e = obb_d(B, A), qq = obb_d(C, A), g = obb_d(q.c, A);
    if (obb_edge_axis_separates(q.u0, q.u1, q.u2, e, qq, g)) return false;
    if (obb_edge_axis_separates(q.u1, q.u2, q.u0, e, qq, g)) return false;
    if (obb_edge_axis_separates(q.u2, q.u0, q.u1, e, qq, g)) return false;
    const f3 h = A; // (v0, v1; v2) -> (v1, v2; v0): rotate;  (v1, v2; v0) -> (v0, v2; v1): exchange A and C
    if (edge == 0) A = B, B = C, C = h;
    else A = C, C = h;
  }
  return true;
}

// ---- triangle-overlap queries (include/ezrt_tri_overlap.h, where the definition is the contract): liveness, T1 and T2 of one scene
// triangle against a LIVE query triangle (the caller has checked it with tri_live), in the header's order.  A direction g x axis_j
// has x[j] = 0: its term x[j] * D[j] is a zero (D is finite), and adding a zero changes at most the sign of a zero sum, which no
// comparison sees -- so those projections are sums of two products.  Only the fp64 state of one direction is held at a time: the
// loops over edges are not unrolled, an edge's end points are picked from the sorted vertices by its index, and every difference is
// taken from the fp32 values where it is used.
struct TriSorted {
  f3 v0, v1, v2; // v0 <= v1 <= v2 by value
};
struct TriQuery {
  TriSorted t;
  f3 lo, hi; // its bounding box: the gate of T1 and of the walk
};
EZD bool tri_less(f3 x, f3 y) { return x.x < y.x || (x.x == y.x && (x.y < y.y || (x.y == y.y && x.z < y.z))); }
EZD bool tri_same(f3 x, f3 y) { return x.x == y.x && x.y == y.y && x.z == y.z; }
// a live triangle: nine finite numbers and, of the sorted vertices, N != (0, 0, 0); `t` is the sorted triangle when it is live
EZD bool tri_live(f3 a, f3 b, f3 c, TriSorted& t) {
  const float inf = __builtin_inff();
  if (!(ez_abs(a.x) < inf && ez_abs(a.y) < inf && ez_abs(a.z) < inf && ez_abs(b.x) < inf && ez_abs(b.y) < inf && ez_abs(b.z) < inf &&
        ez_abs(c.x) < inf && ez_abs(c.y) < inf && ez_abs(c.z) < inf))
    return false;
  auto cswap = [](f3& x, f3& y) {
    if (tri_less(y, x)) {
      const f3 h = x;
      x = y, y = h;
    }
  };
  cswap(a, b);
  cswap(b, c);
  cswap(a, b);
  t.v0 = a, t.v1 = b, t.v2 = c;
  const double e1x = (double)b.x - (double)a.x, e1y = (double)b.y - (double)a.y, e1z = (double)b.z - (double)a.z;
  const double e2x = (double)c.x - (double)a.x, e2y = (double)c.y - (double)a.y, e2z = (double)c.z - (double)a.z;
  const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
  return Nx != 0.0 || Ny != 0.0 || Nz != 0.0;
}
// the query triangle p1 p2 p3 as the kernels hold it; false when it is not live (q is then not to be used)
EZD bool tri_query(f3 p1, f3 p2, f3 p3, TriQuery& q) {
  if (!tri_live(p1, p2, p3, q.t)) return false;
  const f3 a = q.t.v0, b = q.t.v1, c = q.t.v2;
  q.lo = mk(a.x, ez_min(ez_min(a.y, b.y), c.y), ez_min(ez_min(a.z, b.z), c.z)); // (sorted by x first)
  q.hi = mk(c.x, ez_max(ez_max(a.y, b.y), c.y), ez_max(ez_max(a.z, b.z), c.z));
  return true;
}
// edge i of a sorted triangle: E0 = (v0, v1), E1 = (v1, v2), E2 = (v0, v2)
EZD f3 tri_edge_from(const TriSorted& t, int i) { return i == 1 ? t.v1 : t.v0; }
EZD f3 tri_edge_to(const TriSorted& t, int i) { return i == 0 ? t.v1 : t.v2; }
// max(0, p1, p2) < min(p3, p4, p5) || max(p3, p4, p5) < min(0, p1, p2)
EZD bool tri_intervals_apart(double p1, double p2, double p3, double p4, double p5) {
  double amax = p1 > 0.0 ? p1 : 0.0, amin = p1 < 0.0 ? p1 : 0.0;
  amax = p2 > amax ? p2 : amax, amin = p2 < amin ? p2 : amin;
  double bmax = p4 > p3 ? p4 : p3, bmin = p4 < p3 ? p4 : p3;
  bmax = p5 > bmax ? p5 : bmax, bmin = p5 < bmin ? p5 : bmin;
  return amax < bmin || bmax < amin;
}
// does the direction x separate A and B?  p(x, D) = (x0*D[0] + x1*D[1]) + x2*D[2], D relative to a0
EZD bool tri_axis_separates(double x0, double x1, double x2, const TriSorted& A, const TriSorted& B) {
  const f3 o = A.v0;
  auto p = [&](f3 X) { return (x0 * ((double)X.x - (double)o.x) + x1 * ((double)X.y - (double)o.y)) + x2 * ((double)X.z - (double)o.z); };
  return tri_intervals_apart(p(A.v1), p(A.v2), p(B.v0), p(B.v1), p(B.v2));
}
// does g x axis_j separate, for the edge g = (from, to) and all three j?  (u, w) = ((j + 1) % 3, (j + 2) % 3): x[u] = -g[w], x[w] = g[u]
EZD bool tri_edge_axes_separate(f3 from, f3 to, const TriSorted& A, const TriSorted& B) {
  const f3 o = A.v0;
  const double gx = (double)to.x - (double)from.x, gy = (double)to.y - (double)from.y, gz = (double)to.z - (double)from.z;
  auto px = [&](f3 X) { return -gz * ((double)X.y - (double)o.y) + gy * ((double)X.z - (double)o.z); }; // j = 0: (u, w) = (y, z)
  if (tri_intervals_apart(px(A.v1), px(A.v2), px(B.v0), px(B.v1), px(B.v2))) return true;
  auto py = [&](f3 X) { return gz * ((double)X.x - (double)o.x) + -gx * ((double)X.z - (double)o.z); }; // j = 1: (z, x); x0 = g[z], x2 = -g[x]
  if (tri_intervals_apart(py(A.v1), py(A.v2), py(B.v0), py(B.v1), py(B.v2))) return true;
  auto pz = [&](f3 X) { return -gy * ((double)X.x - (double)o.x) + gx * ((double)X.y - (double)o.y); }; // j = 2: (x, y)
  return tri_intervals_apart(pz(A.v1), pz(A.v2), pz(B.v0), pz(B.v1), pz(B.v2));
}
EZD bool tri_overlaps(const float4* __restrict__ tg, const TriQuery& q) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  const f3 a = mk(ga.x, ga.y, ga.z), b = mk(gb.x, gb.y, gb.z), c = mk(gc.x, gc.y, gc.z);
  // T1: q.lo is the least and q.hi the greatest coordinate of the query's vertices (a comparison with a NaN is false)
  if (!((q.lo.x <= a.x || q.lo.x <= b.x || q.lo.x <= c.x) && (a.x <= q.hi.x || b.x <= q.hi.x || c.x <= q.hi.x))) return false;
  if (!((q.lo.y <= a.y || q.lo.y <= b.y || q.lo.y <= c.y) && (a.y <= q.hi.y || b.y <= q.hi.y || c.y <= q.hi.y))) return false;
  if (!((q.lo.z <= a.z || q.lo.z <= b.z || q.lo.z <= c.z) && (a.z <= q.hi.z || b.z <= q.hi.z || c.z <= q.hi.z))) return false;
  TriSorted s;
  if (!tri_live(a, b, c, s)) return false;
  // (A, B): the two triangles in the order of their values
  const bool scene_first = tri_less(s.v0, q.t.v0) ||
                           (tri_same(s.v0, q.t.v0) && (tri_less(s.v1, q.t.v1) || (tri_same(s.v1, q.t.v1) && tri_less(s.v2, q.t.v2))));
  const TriSorted A = scene_first ? s : q.t, B = scene_first ? q.t : s;
  // T2: the two normals
#pragma unroll 1
  for (int side = 0; side < 2; side++) {
    const TriSorted t = side ? B : A;
    const double e1x = (double)t.v1.x - (double)t.v0.x, e1y = (double)t.v1.y - (double)t.v0.y, e1z = (double)t.v1.z - (double)t.v0.z;
    const double e2x = (double)t.v2.x - (double)t.v0.x, e2y = (double)t.v2.y - (double)t.v0.y, e2z = (double)t.v2.z - (double)t.v0.z;
    if (tri_axis_separates(e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x, A, B)) return false;
  }
  // ... g x axis_j for the edges of A, then of B
#pragma unroll 1
  for (int g = 0; g < 6; g++) {
    const TriSorted t = g < 3 ? A : B;
    const int i = g < 3 ? g : g - 3;
    if (tri_edge_axes_separate(tri_edge_from(t, i), tri_edge_to(t, i), A, B)) return false;
  }
  // ... e_i x f_j
#pragma unroll 1
  for (int ij = 0; ij < 9; ij++) {
    const int i = ij / 3, j = ij - 3 * i;
    const f3 ea = tri_edge_from(A, i), eb = tri_edge_to(A, i), fa = tri_edge_from(B, j), fb = tri_edge_to(B, j);
    const double ex = (double)eb.x - (double)ea.x, ey = (double)eb.y - (double)ea.y, ez = (double)eb.z - (double)ea.z;
    const double fx = (double)fb.x - (double)fa.x, fy = (double)fb.y - (double)fa.y, fz = (double)fb.z - (double)fa.z;
    if (tri_axis_separates(ey * fz - ez * fy, ez * fx - ex * fz, ex * fy - ey * fx, A, B)) return false;
  }
  return true;
}

// ---- self-overlap queries (include/ezrt_self_overlap.h, where the definition is the contract): crosses(I, J) of one scene triangle
// against a LIVE triangle of the scene held as a TriQuery (the caller keeps the triangle's own id out), in the header's order: the
// number s of vertices shared by value, then tri_overlaps, the two seg_meets, the fold rule or true.  As in tri_overlaps only the
// fp64 state of one direction is held at a time, the loops are not unrolled and every difference is taken where it is used; the
// projections of a direction g x axis_j are sums of two products, by the argument above.
// max(0, p1, p2) < min(p3, p4) || max(p3, p4) < min(0, p1, p2)
EZD bool seg_intervals_apart(double p1, double p2, double p3, double p4) {
  double tmax = p1 > 0.0 ? p1 : 0.0, tmin = p1 < 0.0 ? p1 : 0.0;
  tmax = p2 > tmax ? p2 : tmax, tmin = p2 < tmin ? p2 : tmin;
  const double smax = p4 > p3 ? p4 : p3, smin = p4 < p3 ? p4 : p3;
  return tmax < smin || smax < tmin;
}
// does the direction x separate the segment a b from T?  p(x, D), D relative to t0
EZD bool seg_axis_separates(double x0, double x1, double x2, f3 a, f3 b, const TriSorted& T) {
  const f3 o = T.v0;
  auto p = [&](f3 X) { return (x0 * ((double)X.x - (double)o.x) + x1 * ((double)X.y - (double)o.y)) + x2 * ((double)X.z - (double)o.z); };
  return seg_intervals_apart(p(T.v1), p(T.v2), p(a), p(b));
}
// does g x axis_j separate, for g = (from, to) and all three j?  (as tri_edge_axes_separate)
EZD bool seg_edge_axes_separate(f3 from, f3 to, f3 a, f3 b, const TriSorted& T) {
  const f3 o = T.v0;
  const double gx = (double)to.x - (double)from.x, gy = (double)to.y - (double)from.y, gz = (double)to.z - (double)from.z;
  auto px = [&](f3 X) { return -gz * ((double)X.y - (double)o.y) + gy * ((double)X.z - (double)o.z); };
  if (seg_intervals_apart(px(T.v1), px(T.v2), px(a), px(b))) return true;
  auto py = [&](f3 X) { return gz * ((double)X.x - (double)o.x) + -gx * ((double)X.z - (double)o.z); };
  if (seg_intervals_apart(py(T.v1), py(T.v2), py(a), py(b))) return true;
  auto pz = [&](f3 X) { return -gy * ((double)X.x - (double)o.x) + gx * ((double)X.y - (double)o.y); };
  return seg_intervals_apart(pz(T.v1), pz(T.v2), pz(a), pz(b));
}
// the closed segment a b, (a, b) in the order of their values, against the closed live triangle T: none of the 16 directions separates
EZD bool seg_meets(f3 a, f3 b, const TriSorted& T) {
  {
    const double e1x = (double)T.v1.x - (double)T.v0.x, e1y = (double)T.v1.y - (double)T.v0.y, e1z = (double)T.v1.z - (double)T.v0.z;
    const double e2x = (double)T.v2.x - (double)T.v0.x, e2y = (double)T.v2.y - (double)T.v0.y, e2z = (double)T.v2.z - (double)T.v0.z;
    if (seg_axis_separates(e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x, a, b, T)) return false;
  }
  // ... g x axis_j for the segment, then for the edges of T
#pragma unroll 1
  for (int g = 0; g < 4; g++) {
    const f3 from = g == 0 ? a : tri_edge_from(T, g - 1), to = g == 0 ? b : tri_edge_to(T, g - 1);
    if (seg_edge_axes_separate(from, to, a, b, T)) return false;
  }
  // ... g_0 x f_j
#pragma unroll 1
  for (int j = 0; j < 3; j++) {
    const f3 fa = tri_edge_from(T, j), fb = tri_edge_to(T, j);
    const double dx = (double)b.x - (double)a.x, dy = (double)b.y - (double)a.y, dz = (double)b.z - (double)a.z;
    const double fx = (double)fb.x - (double)fa.x, fy = (double)fb.y - (double)fa.y, fz = (double)fb.z - (double)fa.z;
    if (seg_axis_separates(dy * fz - dz * fy, dz * fx - dx * fz, dx * fy - dy * fx, a, b, T)) return false;
  }
  return true;
}
// one of two vertices or triangles, chosen value by value (selects, never an address)
EZD f3 tri_pick(bool c, f3 x, f3 y) { return mk(c ? x.x : y.x, c ? x.y : y.y, c ? x.z : y.z); }
EZD TriSorted tri_pick(bool c, const TriSorted& x, const TriSorted& y) {
  TriSorted r;
  r.v0 = tri_pick(c, x.v0, y.v0), r.v1 = tri_pick(c, x.v1, y.v1), r.v2 = tri_pick(c, x.v2, y.v2);
  return r;
}
// vertex i of a sorted triangle, and the two others in the order of their values
EZD f3 tri_vertex(const TriSorted& t, int i) { return tri_pick(i == 0, t.v0, tri_pick(i == 1, t.v1, t.v2)); }
EZD f3 tri_rest_lo(const TriSorted& t, int i) { return tri_pick(i == 0, t.v1, t.v0); }
EZD f3 tri_rest_hi(const TriSorted& t, int i) { return tri_pick(i == 2, t.v1, t.v2); }
EZD bool tri_holds(const TriSorted& t, f3 x) { return tri_same(x, t.v0) || tri_same(x, t.v1) || tri_same(x, t.v2); }
EZD bool self_crosses(const float4* __restrict__ tg, const TriQuery& q) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  const f3 a = mk(ga.x, ga.y, ga.z), b = mk(gb.x, gb.y, gb.z), c = mk(gc.x, gc.y, gc.z);
  // s, on the vertices as they are stored: a NaN equals nothing, and a triangle with a repeated vertex is not live
  const int s = (tri_holds(q.t, a) ? 1 : 0) + (tri_holds(q.t, b) ? 1 : 0) + (tri_holds(q.t, c) ? 1 : 0);
  if (s == 0) return tri_overlaps(tg, q);
  TriSorted t;
  if (!tri_live(a, b, c, t)) return false; // (T1 holds: the shared value is in both bounding boxes)
  if (s == 3) return true;
  if (s == 1) {
    // the place of the shared vertex in each sorted triangle; each triangle's opposite edge against the other triangle
    const int iq = tri_holds(t, q.t.v0) ? 0 : tri_holds(t, q.t.v1) ? 1 : 2;
    const int it = tri_holds(q.t, t.v0) ? 0 : tri_holds(q.t, t.v1) ? 1 : 2;
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
      const TriSorted S = tri_pick(side != 0, t, q.t), T = tri_pick(side != 0, q.t, t);
      const int i = side ? it : iq;
      if (seg_meets(tri_rest_lo(S, i), tri_rest_hi(S, i), T)) return true;
    }
    return false;
  }
  // s == 2: the place of the apex in each sorted triangle, (A, B) the two in the order of their values
  const int iq = !tri_holds(t, q.t.v0) ? 0 : !tri_holds(t, q.t.v1) ? 1 : 2;
  const int it = !tri_holds(q.t, t.v0) ? 0 : !tri_holds(q.t, t.v1) ? 1 : 2;
  const bool scene_first = tri_less(t.v0, q.t.v0) ||
                           (tri_same(t.v0, q.t.v0) && (tri_less(t.v1, q.t.v1) || (tri_same(t.v1, q.t.v1) && tri_less(t.v2, q.t.v2))));
  const TriSorted A = tri_pick(scene_first, t, q.t);
  const int ia = scene_first ? it : iq;
  const f3 u = tri_rest_lo(A, ia), v = tri_rest_hi(A, ia), pa = tri_vertex(A, ia), pb = tri_pick(scene_first, tri_vertex(q.t, iq), tri_vertex(t, it));
  const double ex = (double)v.x - (double)u.x, ey = (double)v.y - (double)u.y, ez = (double)v.z - (double)u.z;
  const double ax = (double)pa.x - (double)u.x, ay = (double)pa.y - (double)u.y, az = (double)pa.z - (double)u.z;
  const double bx = (double)pb.x - (double)u.x, by = (double)pb.y - (double)u.y, bz = (double)pb.z - (double)u.z;
  const double Xax = ey * az - ez * ay, Xay = ez * ax - ex * az, Xaz = ex * ay - ey * ax;
  if (!((Xax * bx + Xay * by) + Xaz * bz == 0.0)) return false; // coplanar
  const double Xbx = ey * bz - ez * by, Xby = ez * bx - ex * bz, Xbz = ex * by - ey * bx;
  return (Xax > 0.0 && Xbx > 0.0) || (Xax < 0.0 && Xbx < 0.0) || (Xay > 0.0 && Xby > 0.0) || (Xay < 0.0 && Xby < 0.0) ||
         (Xaz > 0.0 && Xbz > 0.0) || (Xaz < 0.0 && Xbz < 0.0); // same_side
}

// hitBVH: P5/fsh:254-306 + hitArray 238-251.  Unpruned, near-first, ties go
// right-first, strict < keeps the first-found hit -- identical visit order per
// ray.  The traversal stack lives in LDS: `stack` points at this lane's column
// (stride = STRIDE ints) so bank = lane % 32 and the two half-waves never
// conflict.  Only {t, triangle} are carried; everything else is a pure function
// of the winner.
template <bool FULLCTR, int STRIDE>
EZD void hit_bvh(const DevScene& sc, f3 S, f3 d, int* __restrict__ stack, int32_t& best_tri, float& best_t,
                 Counters& ctr) {
  ctr.rays++;
  best_tri = -1;
  best_t = INF;
  f3 inv = mk(ez_rcp(d.x), ez_rcp(d.y), ez_rcp(d.z));
  int sp = 0;
  uint32_t ref = sc.root_ref;
  for (;;) {
    if (FULLCTR) ctr.pops++;
    if (ref & LEAF_BIT) {
      int first = (int)(ref & 0x00ffffffu);
      int n = (int)((ref >> 24) & 0x7fu) + 1;
      float leaf_best = INF; // only for the M counter (hitArray's local res)
      for (int i = first; i < first + n; i++) {
        float t;
        bool hit = hit_triangle_t(sc.tri_geom + (size_t)i * 3, S, d, t);
        if (FULLCTR) {
          ctr.tris++;
          if (hit && t < leaf_best) {
            leaf_best = t;
            ctr.mats++;
          }
        }
        if (hit && t < best_t) {
          best_t = t;
          best_tri = i;
        }
      }
    } else {
      if (FULLCTR) ctr.inner++;
      const float4* r = sc.inner + (size_t)ref * 4;
      float4 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3];
      float d1 = hit_aabb(S, inv, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y));
      float d2 = hit_aabb(S, inv, mk(q1.z, q1.w, q2.x), mk(q2.y, q2.z, q2.w));
      uint32_t left = __float_as_uint(q3.x), right = __float_as_uint(q3.y);
      if (d1 > 0.0f && d2 > 0.0f) {
        if (d1 < d2) { // left first: push right, continue with left
          stack[sp * STRIDE] = (int)right;
          sp++;
          ref = left;
        } else {
          stack[sp * STRIDE] = (int)left;
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
    ref = (uint32_t)stack[sp * STRIDE];
  }
}

// ---- sphere-cast queries (include/ezrt_sphere_cast.h, where the definition is the contract): a sphere of radius r whose centre
// moves along o + d t, against one scene triangle.  sphere_cast_live is the query's liveness, sphere_cast_slab the gate -- the slab
// test of the ray against a box inflated by r, which is also the walk's bound of a node box (sphere_cast_box) --, sphere_cast_pair
// the seven sub-candidates in the header's order (face, edges ab bc ca, vertices a b c), the first smallest finite t, clamped up to
// the gate's tnear.  The edge and vertex loops are not unrolled and pick their vertices from the registers by index, as
// tri_distance_pair does: one sub-candidate's state is held at a time.
struct SphereRay {
  f3 o, d, inv; // inv = 1 / d per axis (used where d != 0 alone)
  float r, rr, dd; // rr = r * r, dd = dot(d, d)
};
EZD bool sphere_cast_live(f3 o, f3 d, float r, SphereRay& q) {
  const float inf = __builtin_inff();
  q.o = o, q.d = d, q.r = r;
  q.rr = r * r;
  q.dd = dot(d, d);
  q.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  return ez_abs(o.x) < inf && ez_abs(o.y) < inf && ez_abs(o.z) < inf && ez_abs(d.x) < inf && ez_abs(d.y) < inf && ez_abs(d.z) < inf &&
         r >= 0.0f && r < inf && q.dd > 0.0f && q.dd < inf && (d.x == 0.0f || ez_abs(q.inv.x) < inf) &&
         (d.y == 0.0f || ez_abs(q.inv.y) < inf) && (d.z == 0.0f || ez_abs(q.inv.z) < inf);
}
// one axis of the slab test: false when a flat axis (d == 0 or -0) lies outside [lo - r, hi + r]; a NaN bound constrains nothing
EZD bool sphere_cast_axis(float o, float d, float inv, float r, float lo, float hi, float& tn, float& tf) {
  const float L = lo - r, H = hi + r;
  if (d == 0.0f) return !(o < L || o > H);
  const float x = (L - o) * inv, y = (H - o) * inv;
  tn = ez_max(tn, d < 0.0f ? y : x);
  tf = ez_min(tf, d < 0.0f ? x : y);
  return true;
}
// the gate: tnear = max(0, nears), tfar = min(+inf, fars); true when no flat axis fails and tnear <= tfar.  For a box that holds
// another, tnear is no larger and tfar no smaller ON THE BITS, and it passes whenever the inner one does (ezrt_point_queries.h:
// sphere_cast_kernel).
EZD bool sphere_cast_slab(const SphereRay& q, f3 lo, f3 hi, float& tnear) {
  float tn = 0.0f, tf = __builtin_inff();
  const bool x = sphere_cast_axis(q.o.x, q.d.x, q.inv.x, q.r, lo.x, hi.x, tn, tf);
  const bool y = sphere_cast_axis(q.o.y, q.d.y, q.inv.y, q.r, lo.y, hi.y, tn, tf);
  const bool z = sphere_cast_axis(q.o.z, q.d.z, q.inv.z, q.r, lo.z, hi.z, tn, tf);
  tnear = tn;
  return x && y && z && tn <= tf;
}
// ... as the lower bound of the t of every pair below a box: tnear, +inf where the gate fails
EZD float sphere_cast_box(const SphereRay& q, f3 lo, f3 hi) {
  float tn;
  return sphere_cast_slab(q, lo, hi, tn) ? tn : __builtin_inff();
}
EZD f3 sphere_into_box(f3 x, f3 lo, f3 hi) {
  return mk(x.x < lo.x ? lo.x : (x.x > hi.x ? hi.x : x.x), x.y < lo.y ? lo.y : (x.y > hi.y ? hi.y : x.y),
            x.z < lo.z ? lo.z : (x.z > hi.z ? hi.z : x.z));
}
EZD f3 sphere_corner(int i, f3 a, f3 b, f3 c) {
  return mk(i == 0 ? a.x : (i == 1 ? b.x : c.x), i == 0 ? a.y : (i == 1 ? b.y : c.y), i == 0 ? a.z : (i == 1 ? b.z : c.z));
}
// the first time A t^2 + 2 B t + C reaches 0 for a centre that approaches (B < 0) from outside (C > 0), in the form without
// cancellation; 0 where the feature already holds the centre (C <= 0); NaN -- skipped by the caller -- otherwise.  disc is the
// caller's B^2 - A C in Lagrange's form, A r^2 - |m x d|^2, which does not cancel for a thin sphere far away
EZD float sphere_root(float B, float C, float disc) {
  if (C <= 0.0f) return 0.0f;
  return (B < 0.0f && disc >= 0.0f) ? C / (__builtin_sqrtf(disc) - B) : __builtin_nanf("");
}
// The pair rule.  False: the triangle is not live, the gate fails, tnear > limit (such a pair's t exceeds limit: the caller's running
// best, +inf for none) or no sub-candidate has a finite t.  Else t = max(smallest valid t, tnear), `point` the contact point on the
// triangle and `sub` the sub-candidate that supplied it (0 face, 1 2 3 edges, 4 5 6 vertices).
EZD bool sphere_cast_pair(const float4* __restrict__ tg, const SphereRay& q, float limit, float& t, f3& point, int& sub, float& tnear) {
  const float inf = __builtin_inff();
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  const f3 a = mk(ga.x, ga.y, ga.z), b = mk(gb.x, gb.y, gb.z), c = mk(gc.x, gc.y, gc.z);
  if (!(ez_abs(a.x) < inf && ez_abs(a.y) < inf && ez_abs(a.z) < inf && ez_abs(b.x) < inf && ez_abs(b.y) < inf && ez_abs(b.z) < inf &&
        ez_abs(c.x) < inf && ez_abs(c.y) < inf && ez_abs(c.z) < inf))
    return false;
  const f3 lo = mk(ez_min(ez_min(a.x, b.x), c.x), ez_min(ez_min(a.y, b.y), c.y), ez_min(ez_min(a.z, b.z), c.z));
  const f3 hi = mk(ez_max(ez_max(a.x, b.x), c.x), ez_max(ez_max(a.y, b.y), c.y), ez_max(ez_max(a.z, b.z), c.z));
  if (!sphere_cast_slab(q, lo, hi, tnear) || tnear > limit) return false;
  float best = inf;
  auto take = [&](float tt, f3 x, int which) {
    if (tt < best) best = tt, point = x, sub = which; // (false for a NaN or infinite tt; the first wins on equality)
  };
  { // the face: the unnormalised normal flipped to o's side; valid when the centre approaches the plane and the foot is in the triangle
    const f3 ab = b - a, ac = c - a, m = q.o - a;
    const f3 n0 = cross(ab, ac);
    const float h0 = dot(n0, m);
    const bool flip = h0 < 0.0f;
    const f3 n = flip ? -n0 : n0;
    const float h = flip ? -h0 : h0;
    const float nd = dot(n, q.d);
    if (nd < 0.0f) {
      const float len = __builtin_sqrtf(dot(n, n));
      const float g = h - q.r * len;
      const float tt = g <= 0.0f ? 0.0f : g / (-nd);
      const f3 x = (q.o + q.d * tt) - n * (q.r / len);
      const float e0 = dot(cross(ab, x - a), n0), e1 = dot(cross(c - b, x - b), n0), e2 = dot(cross(a - c, x - c), n0);
      if (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) take(tt, sphere_into_box(x, lo, hi), 0);
    }
  }
#pragma unroll 1
  for (int j = 0; j < 3; j++) { // the edges (a, b) (b, c) (c, a): the cylinder of radius r about the edge, in the plane across it
    const f3 u = sphere_corner(j, a, b, c), v = sphere_corner(j, b, c, a);
    const f3 e = v - u, m = q.o - u;
    const float ee = dot(e, e);
    const float sd = dot(e, q.d) / ee, sm = dot(e, m) / ee;
    const f3 dp = q.d - e * sd, mp = m - e * sm;
    const f3 x = cross(mp, dp);
    const float tt = sphere_root(dot(mp, dp), dot(mp, mp) - q.rr, dot(dp, dp) * q.rr - dot(x, x));
    const float s = sm + sd * tt;
    const f3 elo = mk(ez_min(u.x, v.x), ez_min(u.y, v.y), ez_min(u.z, v.z)), ehi = mk(ez_max(u.x, v.x), ez_max(u.y, v.y), ez_max(u.z, v.z));
    if (s >= 0.0f && s <= 1.0f) take(tt, sphere_into_box(u + e * s, elo, ehi), 1 + j);
  }
#pragma unroll 1
  for (int j = 0; j < 3; j++) { // the vertices a b c: the sphere of radius r about the vertex
    const f3 p = sphere_corner(j, a, b, c);
    const f3 m = q.o - p;
    const f3 x = cross(m, q.d);
    take(sphere_root(dot(m, q.d), dot(m, m) - q.rr, q.dd * q.rr - dot(x, x)), p, 4 + j);
  }
  if (!(best < inf)) return false;
  t = ez_max(best, tnear);
  return t < inf;
}
// The running answer of one query.  `t` starts as t_max (tri = -1) and is the radius of the walk from the first step on; the smallest
// t wins and, among equal t, the smallest index -- whatever the order in which the triangles are met.
struct SphereBest {
  float t;
  int32_t tri;
  f3 point;
  bool touching;
};
EZD void sphere_cast_candidate(SphereBest& r, const float4* __restrict__ tri_geom, int32_t k, const SphereRay& q) {
  float t, tnear;
  f3 x;
  int sub;
  if (!sphere_cast_pair(tri_geom + (size_t)k * 3, q, r.t, t, x, sub, tnear)) return;
  if (t < r.t || (t == r.t && (r.tri < 0 || k < r.tri))) r.t = t, r.tri = k, r.point = x;
}
// the pair for a caller who holds it: touching where closest_point_triangle's dist2 <= r * r, else the swept pair; tri stays -1 for a miss
EZD void sphere_cast_at(SphereBest& r, const float4* __restrict__ tri_geom, int32_t k, const SphereRay& q) {
  f3 x;
  float v, w;
  const float d2 = closest_point_triangle(tri_geom + (size_t)k * 3, q.o, x, v, w);
  if (d2 < __builtin_inff() && d2 <= q.rr) { // closest_point_candidate's test with B = r * r (false for a NaN d2)
    r.t = 0.0f, r.tri = k, r.point = x, r.touching = true;
    return;
  }
  sphere_cast_candidate(r, tri_geom, k, q);
}

// ---- triangle-distance queries (include/ezrt_tri_distance.h, where the definition is the contract): the pair rule of one scene
// triangle against a LIVE query triangle -- q from tri_query, p1 p2 p3 its vertices as the caller gave them.  The 15 sub-candidates in
// the header's order (vertices of Q against the triangle, its vertices against Q, the nine edge pairs with Q's edge outer), the first
// smallest finite d2 wins and supplies (x, y); then the crossing step.  False: the pair is no candidate (the triangle is not live, or
// no d2 is finite).  The loops are not unrolled and a vertex or an edge is picked from the registers by its index, as in
// tri_overlaps: one sub-candidate's state is held at a time.
EZD f3 tri_corner(int i, f3 a, f3 b, f3 c) { return mk(i == 0 ? a.x : (i == 1 ? b.x : c.x), i == 0 ? a.y : (i == 1 ? b.y : c.y), i == 0 ? a.z : (i == 1 ? b.z : c.z)); }
EZD bool tri_distance_pair(const float4* __restrict__ tg, const TriQuery& q, f3 p1, f3 p2, f3 p3, float& dist2, f3& x, f3& y, bool& crosses) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  const f3 a = mk(ga.x, ga.y, ga.z), b = mk(gb.x, gb.y, gb.z), c = mk(gc.x, gc.y, gc.z);
  TriSorted s;
  if (!tri_live(a, b, c, s)) return false;
  const float inf = __builtin_inff();
  float best = inf;
  bool found = false;
  auto take = [&](float d2, f3 cx, f3 cy) {
    if (d2 < inf && (!found || d2 < best)) best = d2, x = cx, y = cy, found = true; // (false for a NaN d2; the first wins on equality)
  };
#pragma unroll 1
  for (int i = 0; i < 6; i++) {
    const bool scene = i >= 3; // the vertices of Q against the triangle, then the triangle's against Q
    const int j = scene ? i - 3 : i;
    const f3 p = tri_corner(j, scene ? a : p1, scene ? b : p2, scene ? c : p3);
    f3 qq;
    float v, w;
    const float d2 = closest_point_abc(scene ? p1 : a, scene ? p2 : b, scene ? p3 : c, p, qq, v, w);
    take(d2, scene ? qq : p, scene ? p : qq);
  }
#pragma unroll 1
  for (int ij = 0; ij < 9; ij++) {
    const int i = ij / 3, j = ij - 3 * i;
    f3 cx, cy;
    const float d2 = segment_segment_closest(tri_corner(i, p1, p2, p3), tri_corner(i, p2, p3, p1), tri_corner(j, a, b, c), tri_corner(j, b, c, a), cx, cy);
    take(d2, cx, cy);
  }
  if (!found) return false;
  crosses = tri_overlaps(tg, q);
  dist2 = crosses ? 0.0f : best;
  return true;
}
// The running answer of one query triangle, as ClosestBest is a point's: `best` starts as the bound B (tri = -1) and is the pruning
// radius of the walk from the first step on.  The smallest dist2 wins; among equal dist2 a pair that crosses comes before one that
// does not (possible at dist2 = 0 alone: a sub-candidate of a pair that is apart by less than fp32 resolves may round to 0), then the
// smallest index -- whatever the order in which the triangles are met.
struct TriDistanceBest {
  float best;
  int32_t tri;
  f3 x, y;
  bool crosses;
};
EZD void tri_distance_candidate(TriDistanceBest& r, const float4* __restrict__ tri_geom, int32_t k, const TriQuery& q, f3 p1, f3 p2, f3 p3) {
  f3 x, y;
  float d2;
  bool crosses;
  if (!tri_distance_pair(tri_geom + (size_t)k * 3, q, p1, p2, p3, d2, x, y, crosses)) return;
  if (d2 < r.best || (d2 == r.best && (r.tri < 0 || (crosses && !r.crosses) || (crosses == r.crosses && k < r.tri))))
    r.best = d2, r.tri = k, r.x = x, r.y = y, r.crosses = crosses;
}

// ---- segment queries (include/ezrt_segment.h, where the definition is the contract): the pair rule of one scene triangle against a
// LIVE query segment [a, b] (six finite numbers; a == b is a point) -- (lo, hi) are a and b in the order of their values, as
// seg_meets takes them.  The five sub-candidates in the header's order (a, then b, against the triangle by closest_point_abc; the
// segment as the FIRST argument of segment_segment_closest against the edges (p, q), (q, r), (r, p)), the first smallest finite d2
// wins and supplies (x, y); then the crossing step: T1 on the two fp32 bounding boxes, and seg_meets as it stands.  False: the pair
// is no candidate (the triangle is not live, or no d2 is finite).  The two loops are not unrolled and a vertex is picked from the
// registers by its index, as in tri_distance_pair: one sub-candidate's state is held at a time.
EZD bool segment_pair(const float4* __restrict__ tg, f3 a, f3 b, f3 lo, f3 hi, float& dist2, f3& x, f3& y, bool& crosses) {
  const float4 gp = tg[0], gq = tg[1], gr = tg[2];
  const f3 p = mk(gp.x, gp.y, gp.z), q = mk(gq.x, gq.y, gq.z), r = mk(gr.x, gr.y, gr.z);
  TriSorted s;
  if (!tri_live(p, q, r, s)) return false;
  const float inf = __builtin_inff();
  float best = inf;
  bool found = false;
  auto take = [&](float d2, f3 cx, f3 cy) {
    if (d2 < inf && (!found || d2 < best)) best = d2, x = cx, y = cy, found = true; // (false for a NaN d2; the first wins on equality)
  };
#pragma unroll 1
  for (int i = 0; i < 2; i++) {
    const f3 e = tri_pick(i == 0, a, b);
    f3 qq;
    float v, w;
    const float d2 = closest_point_abc(p, q, r, e, qq, v, w);
    take(d2, e, qq);
  }
#pragma unroll 1
  for (int j = 0; j < 3; j++) {
    f3 cx, cy;
    const float d2 = segment_segment_closest(a, b, tri_corner(j, p, q, r), tri_corner(j, q, r, p), cx, cy);
    take(d2, cx, cy);
  }
  if (!found) return false;
  // T1: the segment's bounding box against the triangle's, closed, on all three axes (every number is finite here)
  const bool t1 = ez_min(a.x, b.x) <= ez_max(ez_max(p.x, q.x), r.x) && ez_min(ez_min(p.x, q.x), r.x) <= ez_max(a.x, b.x) &&
                  ez_min(a.y, b.y) <= ez_max(ez_max(p.y, q.y), r.y) && ez_min(ez_min(p.y, q.y), r.y) <= ez_max(a.y, b.y) &&
                  ez_min(a.z, b.z) <= ez_max(ez_max(p.z, q.z), r.z) && ez_min(ez_min(p.z, q.z), r.z) <= ez_max(a.z, b.z);
  crosses = t1 && seg_meets(lo, hi, s);
  dist2 = crosses ? 0.0f : best;
  return true;
}
// a query segment as the kernels hold it; false when it is not live (one of its six numbers is not finite)
struct SegQuery {
  f3 a, b;     // the end points as the caller gave them
  f3 lo, hi;   // ... in the order of their values (seg_meets)
  f3 qlo, qhi; // the segment's fp32 bounding box: the walk's bound and the pair gate
};
EZD bool segment_query(f3 a, f3 b, SegQuery& s) {
  const float inf = __builtin_inff();
  if (!(ez_abs(a.x) < inf && ez_abs(a.y) < inf && ez_abs(a.z) < inf && ez_abs(b.x) < inf && ez_abs(b.y) < inf && ez_abs(b.z) < inf)) return false;
  const bool swap = tri_less(b, a);
  s.a = a, s.b = b;
  s.lo = tri_pick(swap, b, a), s.hi = tri_pick(swap, a, b);
  s.qlo = mk(ez_min(a.x, b.x), ez_min(a.y, b.y), ez_min(a.z, b.z));
  s.qhi = mk(ez_max(a.x, b.x), ez_max(a.y, b.y), ez_max(a.z, b.z));
  return true;
}
// tri_distance_box of the query's bounding box against triangle k's OWN bounding box: the pair gate of both segment kernels (a NaN
// vertex gives a NaN lb, which fails every comparison and goes on to segment_pair, where the triangle is found not live)
EZD float segment_gate(const float4* __restrict__ tg, const SegQuery& s) {
  const float4 ga = tg[0], gb = tg[1], gc = tg[2];
  const f3 lo = mk(ez_min(ez_min(ga.x, gb.x), gc.x), ez_min(ez_min(ga.y, gb.y), gc.y), ez_min(ez_min(ga.z, gb.z), gc.z));
  const f3 hi = mk(ez_max(ez_max(ga.x, gb.x), gc.x), ez_max(ez_max(ga.y, gb.y), gc.y), ez_max(ez_max(ga.z, gb.z), gc.z));
  return tri_distance_box(s.qlo, s.qhi, lo, hi);
}
// the running answer is TriDistanceBest, with its order: the smallest dist2, a crossing pair first, then the smallest index
EZD void segment_candidate(TriDistanceBest& r, const float4* __restrict__ tri_geom, int32_t k, const SegQuery& s) {
  f3 x, y;
  float d2;
  bool crosses;
  if (!segment_pair(tri_geom + (size_t)k * 3, s.a, s.b, s.lo, s.hi, d2, x, y, crosses)) return;
  if (d2 < r.best || (d2 == r.best && (r.tri < 0 || (crosses && !r.crosses) || (crosses == r.crosses && k < r.tri))))
    r.best = d2, r.tri = k, r.x = x, r.y = y, r.crosses = crosses;
}

// ---------------------------------------------------------------------------
// Winner reconstruction: the rest of hitTriangle (P5/fsh:172-178, 199-214) and
// getMaterial (P5/fsh:110-135), evaluated once per ray for the closest hit.
struct Mat {
  f3 emissive, baseColor;
  float subsurface, metallic, specular, specularTint, roughness, anisotropic;
  float sheen, sheenTint, clearcoat, clearcoatGloss;
  // Sub-expressions of BRDF_Evaluate / SampleBRDF / BRDF_Pdf that depend on the material alone (P5/fsh:446-451, 468,
  // 486, 636-637, 727-728), evaluated ONCE per distinct material by mat_derive -- the same fp32 operations in the same
  // order, on the host at ezrt_scene_create (contraction off, ez_log from the shared header: bit-identical to the
  // device, tests/test_gpu_parity.py) -- instead of once per shaded hit: three divisions, a logarithm, seven mixes
  f3 Cspec0, Csheen;
  float alpha_gtr2;   // max(0.001, sqr(roughness))
  float alpha_gtr1;   // mix(0.1, 0.001, clearcoatGloss)
  float gtr1_a2m1;    // a2 - 1,         a2 = alpha_gtr1^2      (GTR1, P5/fsh:410-415)
  float gtr1_pilog;   // PI * log(a2)
};
struct Hit {
  f3 P, N, viewDir;
  Mat m;
};

EZD f3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }
EZD void st3(float* p, f3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }

__host__ __device__ inline void mat_derive(Mat& m) {
  const float Cdlum = 0.3f * m.baseColor.x + 0.6f * m.baseColor.y + 0.1f * m.baseColor.z;
  const float tx = (Cdlum > 0.0f) ? m.baseColor.x / Cdlum : 1.0f, ty = (Cdlum > 0.0f) ? m.baseColor.y / Cdlum : 1.0f,
              tz = (Cdlum > 0.0f) ? m.baseColor.z / Cdlum : 1.0f;                                  // Ctint
  const float sx = ez_mix(1.0f, tx, m.specularTint) * m.specular, sy = ez_mix(1.0f, ty, m.specularTint) * m.specular,
              sz = ez_mix(1.0f, tz, m.specularTint) * m.specular;                                  // Cspec
  m.Cspec0 = f3{ez_mix(sx * 0.08f, m.baseColor.x, m.metallic), ez_mix(sy * 0.08f, m.baseColor.y, m.metallic),
                ez_mix(sz * 0.08f, m.baseColor.z, m.metallic)};
  m.Csheen = f3{ez_mix(1.0f, tx, m.sheenTint), ez_mix(1.0f, ty, m.sheenTint), ez_mix(1.0f, tz, m.sheenTint)};
  m.alpha_gtr2 = ez_max(0.001f, m.roughness * m.roughness);
  m.alpha_gtr1 = ez_mix(0.1f, 0.001f, m.clearcoatGloss);
  const float a2 = m.alpha_gtr1 * m.alpha_gtr1;
  m.gtr1_a2m1 = a2 - 1.0f;
  m.gtr1_pilog = EZ_PI * ez_log(a2);
}

// A material's row of DevScene::mat_table: its 18 floats as the reference stores them (texels 6-11 of a triangle record,
// `m18`) followed by what mat_derive makes of them.  ezrt_scene_create packs one row per distinct material through
// mat_pack_row and shade_point reads it back through mat_unpack_row; the function-level audit (ezrt_debug_fn) sends its
// operand materials down the same two functions.
constexpr int MAT_ROW_FLOAT4 = 7;
// the reference's 18 material floats -> Mat, constants derived (m18[16], m18[17] = IOR, transmission: read by no shader)
__host__ __device__ inline void mat_from18(Mat& m, const float* m18) {
  m.emissive = f3{m18[0], m18[1], m18[2]};
  m.baseColor = f3{m18[3], m18[4], m18[5]};
  m.subsurface = m18[6];
  m.metallic = m18[7];
  m.specular = m18[8];
  m.specularTint = m18[9];
  m.roughness = m18[10];
  m.anisotropic = m18[11];
  m.sheen = m18[12];
  m.sheenTint = m18[13];
  m.clearcoat = m18[14];
  m.clearcoatGloss = m18[15];
  mat_derive(m);
}
inline void mat_pack_row(const float* m18, float4* row) {
  Mat m;
  mat_from18(m, m18);
  row[0] = make_float4(m18[0], m18[1], m18[2], m18[3]);
  row[1] = make_float4(m18[4], m18[5], m18[6], m18[7]);
  row[2] = make_float4(m18[8], m18[9], m18[10], m18[11]);
  row[3] = make_float4(m18[12], m18[13], m18[14], m18[15]);
  row[4] = make_float4(m18[16], m18[17], m.Cspec0.x, m.Cspec0.y);
  row[5] = make_float4(m.Cspec0.z, m.Csheen.x, m.Csheen.y, m.Csheen.z);
  row[6] = make_float4(m.alpha_gtr2, m.alpha_gtr1, m.gtr1_a2m1, m.gtr1_pilog);
}
EZD void mat_unpack_row(Mat& m, float4 m0, float4 m1, float4 m2, float4 m3, float4 m4, float4 m5, float4 m6) {
  m.emissive = mk(m0.x, m0.y, m0.z);
  m.baseColor = mk(m0.w, m1.x, m1.y);
  m.subsurface = m1.z;
  m.metallic = m1.w;
  m.specular = m2.x;
  m.specularTint = m2.y;
  m.roughness = m2.z;
  m.anisotropic = m2.w;
  m.sheen = m3.x;
  m.sheenTint = m3.y;
  m.clearcoat = m3.z;
  m.clearcoatGloss = m3.w;
  // (m4.x, m4.y = IOR, transmission: carried by the reference, read by no shader)
  m.Cspec0 = mk(m4.z, m4.w, m5.x);
  m.Csheen = mk(m5.y, m5.z, m5.w);
  m.alpha_gtr2 = m6.x;
  m.alpha_gtr1 = m6.y;
  m.gtr1_a2m1 = m6.z;
  m.gtr1_pilog = m6.w;
}

// What a winning hit reads besides the 48-byte tri_geom record: 64 B per triangle, four aligned 16-byte loads
// (the reference record's texels 3-11 were seven, P5/fsh:110-135, 199-214):
//   (n1.xyz, n2.x) (n2.yz, n3.xy) (n3.z, bits(material index), -, -) (alpha and beta denominators of the smooth-normal
//   interpolation, P5/fsh:206-207 form and P3/fsh:273-274 form: functions of the triangle alone)
constexpr int SHADE_REC_FLOAT4 = 4, MAT_REC_FLOAT4 = MAT_ROW_FLOAT4;
struct ShadeDen { float a5, b5, a34, b34; };
__host__ __device__ inline ShadeDen shade_denominators(f3 p1, f3 p2, f3 p3) {
  ShadeDen d;
  d.a5 = -(p1.x - p2.x) * (p3.y - p2.y) + (p1.y - p2.y) * (p3.x - p2.x) + 1e-7f;
  d.b5 = -(p2.x - p3.x) * (p1.y - p3.y) + (p2.y - p3.y) * (p1.x - p3.x) + 1e-7f;
  d.a34 = -(p1.x - p2.x - 0.00005f) * (p3.y - p2.y + 0.00005f) + (p1.y - p2.y + 0.00005f) * (p3.x - p2.x + 0.00005f);
  d.b34 = -(p2.x - p3.x - 0.00005f) * (p1.y - p3.y + 0.00005f) + (p2.y - p3.y + 0.00005f) * (p1.x - p3.x + 0.00005f);
  return d;
}

// The surface attributes of a winning hit: hitTriangle's isInside, hitPoint and smooth normal (P5/fsh:172-178, 199-214) for
// triangle `tri` at distance t along the ray (S, d) as given.  Reads the two per-triangle records (tri_geom, tri_shade: seven 16-byte
// loads), not the material table.  shade_point (every shaded hit of a render) and query_surface_kernel (ezrt_surface.h) both run it,
// so a query's attributes are the render's on the bits.  P5TRI: the P5/fsh:206-207 form of the smooth-normal interpolation (+1e-7
// denominators), else P3/fsh:273-274 = P4/fsh:196-197 (the +-0.00005 form).  N_out = the smooth normal, normalised, negated when
// inside (N = the geometric normal, tri_geom's .w).  on_record(r2) is called once the shade record is loaded (r2.y = bits of the
// material index): shade_point issues its material loads there, ahead of the arithmetic, in the order they always had -- the
// render's kernels compile to the same instructions as before this helper existed.
template <bool P5TRI, class OnRecord>
EZD void surface_point(const float4* tri_geom, const float4* tri_shade, int32_t tri, float t, f3 S, f3 d, f3& P_out, f3& N_out,
                       bool& inside_out, OnRecord&& on_record) {
  const float4* g = tri_geom + (size_t)tri * 3;
  float4 a = g[0], b = g[1], c = g[2];
  f3 p1 = mk(a.x, a.y, a.z), p2 = mk(b.x, b.y, b.z), p3 = mk(c.x, c.y, c.z);
  f3 N = mk(a.w, b.w, c.w);
  bool inside = dot(N, d) > 0.0f;
  f3 P = S + d * t;
  const float4* rq = tri_shade + (size_t)tri * SHADE_REC_FLOAT4;
  const float4 r0 = rq[0], r1 = rq[1], r2 = rq[2], r3 = rq[3];
  f3 n1 = mk(r0.x, r0.y, r0.z), n2 = mk(r0.w, r1.x, r1.y), n3 = mk(r1.z, r1.w, r2.x);
  on_record(r2);
  float alpha, beta;
  if (P5TRI) { // P5/fsh:206-207
    alpha = (-(P.x - p2.x) * (p3.y - p2.y) + (P.y - p2.y) * (p3.x - p2.x)) / r3.x;
    beta = (-(P.x - p3.x) * (p1.y - p3.y) + (P.y - p3.y) * (p1.x - p3.x)) / r3.y;
  } else { // P3/fsh:273-274, P4/fsh:196-197
    alpha = (-(P.x - p2.x) * (p3.y - p2.y) + (P.y - p2.y) * (p3.x - p2.x)) / r3.z;
    beta = (-(P.x - p3.x) * (p1.y - p3.y) + (P.y - p3.y) * (p1.x - p3.x)) / r3.w;
  }
  float gama = 1.0f - alpha - beta;
  f3 Ns = normalize(n1 * alpha + n2 * beta + n3 * gama);
  P_out = P;
  N_out = inside ? -Ns : Ns;
  inside_out = inside;
}

template <bool P5TRI>
EZD void shade_point(const DevScene& sc, int32_t tri, float t, f3 S, f3 d, Hit& h) {
  float4 m0, m1, m2, m3, m4, m5, m6;
  bool inside;
  surface_point<P5TRI>(sc.tri_geom, sc.tri_shade, tri, t, S, d, h.P, h.N, inside, [&](float4 r2) {
    const float4* mq = sc.mat_table + (size_t)__float_as_uint(r2.y) * MAT_REC_FLOAT4;
    m0 = mq[0], m1 = mq[1], m2 = mq[2], m3 = mq[3], m4 = mq[4], m5 = mq[5], m6 = mq[6];
  });
  h.viewDir = d;
  mat_unpack_row(h.m, m0, m1, m2, m3, m4, m5, m6);
}

// ---------------------------------------------------------------------------
// textures.  Defined (reference leaves it to the driver): texel-centre
// sampling, clamp-to-edge, NEAREST = floor(u*W), BILINEAR = GL formula in fp32
// with x-lerp then y-lerp.  NaN coordinates read texel 0.
EZD float sane01(float u) {
  if (!(u == u)) return 0.0f;
  return ez_clamp(u, 0.0f, 1.0f);
}
EZD f3 tex_fetch(const float4* __restrict__ img, int W, int H, int filter, float u, float v) {
  u = sane01(u);
  v = sane01(v);
  if (filter == EZRT_FILTER_NEAREST) {
    int ix = (int)ez_floor(u * (float)W), iy = (int)ez_floor(v * (float)H);
    if (ix > W - 1) ix = W - 1;
    if (iy > H - 1) iy = H - 1;
    float4 p = img[(size_t)iy * W + ix];
    return mk(p.x, p.y, p.z);
  }
  float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
  float x0 = ez_floor(x), y0 = ez_floor(y);
  float fx = x - x0, fy = y - y0;
  int ix0 = (int)x0, iy0 = (int)y0, ix1 = ix0 + 1, iy1 = iy0 + 1;
  if (ix0 < 0) ix0 = 0;
  if (iy0 < 0) iy0 = 0;
  if (ix1 > W - 1) ix1 = W - 1;
  if (iy1 > H - 1) iy1 = H - 1;
  float4 p00 = img[(size_t)iy0 * W + ix0], p10 = img[(size_t)iy0 * W + ix1];
  float4 p01 = img[(size_t)iy1 * W + ix0], p11 = img[(size_t)iy1 * W + ix1];
  f3 top = mix3(mk(p00.x, p00.y, p00.z), mk(p10.x, p10.y, p10.z), fx);
  f3 bot = mix3(mk(p01.x, p01.y, p01.z), mk(p11.x, p11.y, p11.z), fx);
  return mix3(top, bot, fy);
}

// The environment map through its RGBE form when it has one (DevScene::hdr_rgbe): 4 bytes per texel instead of 16, so
// a 1024x512 map is 2 MB and stays in every XCD's L2 (the float4 map is 8 MB and the bounce rays' lookups are random).
// Decoding reproduces HDRLoader's convertComponent exactly: (m / 256) * 2^(E - 128) = ldexp(m, E - 136), exact in fp32
// down to the subnormals.
EZD f3 rgbe_texel(uint32_t p) {
  const int e = (int)(p >> 24) - 136;
  return mk(__builtin_amdgcn_ldexpf((float)(p & 255u), e), __builtin_amdgcn_ldexpf((float)((p >> 8) & 255u), e),
            __builtin_amdgcn_ldexpf((float)((p >> 16) & 255u), e));
}
EZD f3 tex_fetch_rgbe(const uint32_t* __restrict__ img, const uint2* __restrict__ pairs, int W, int H, int filter, float u, float v) {
  u = sane01(u);
  v = sane01(v);
  if (filter == EZRT_FILTER_NEAREST) {
    int ix = (int)ez_floor(u * (float)W), iy = (int)ez_floor(v * (float)H);
    if (ix > W - 1) ix = W - 1;
    if (iy > H - 1) iy = H - 1;
    return rgbe_texel(img[(size_t)iy * W + ix]);
  }
  float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
  float x0 = ez_floor(x), y0 = ez_floor(y);
  float fx = x - x0, fy = y - y0;
  int ix0 = (int)x0, iy0 = (int)y0, ix1 = ix0 + 1, iy1 = iy0 + 1;
  if (ix0 < 0) ix0 = 0;
  if (iy0 < 0) iy0 = 0;
  if (ix1 > W - 1) ix1 = W - 1;
  if (iy1 > H - 1) iy1 = H - 1;
  // The two texels of a row are neighbours (or, at the map's left / right edge, the same texel): ONE 8-byte load per row
  // from the pair (bx, bx + 1) that contains them -- the bounce rays' lookups are scattered, so the stage is bound by
  // the number of load requests, not by bytes.  (4-byte aligned: the struct says so.)
  struct __attribute__((packed, aligned(4))) TexelPair {
    uint32_t a, b;
  };
  uint32_t q00, q10, q01, q11;
  if (pairs) {
    // The row-pair plane (DevScene::hdr_pairs): entry row j = (int)y0 + 1 holds the texels of rows (iy0, iy1) as clamped above, the
    // map's top and bottom edges included (j = 0: rows (0, 0); j = H: rows (H - 1, H - 1)), so the footprint's two rows are one
    // request to one line instead of two to two.  (8-byte aligned: the struct says so.)
    struct __attribute__((packed, aligned(8))) PairPair {
      uint32_t a_top, a_bot, b_top, b_bot; // entries bx and bx + 1
    };
    const int bx = ix0 < W - 2 ? ix0 : W - 2;
    const PairPair r = *reinterpret_cast<const PairPair*>(pairs + (size_t)((int)y0 + 1) * W + bx);
    q00 = ix0 == bx ? r.a_top : r.b_top;
    q10 = ix1 == bx ? r.a_top : r.b_top;
    q01 = ix0 == bx ? r.a_bot : r.b_bot;
    q11 = ix1 == bx ? r.a_bot : r.b_bot;
  } else if (W >= 2) {
    int bx = ix0 < W - 2 ? ix0 : W - 2;
    const TexelPair r0 = *reinterpret_cast<const TexelPair*>(img + (size_t)iy0 * W + bx);
    const TexelPair r1 = *reinterpret_cast<const TexelPair*>(img + (size_t)iy1 * W + bx);
    q00 = ix0 == bx ? r0.a : r0.b;
    q10 = ix1 == bx ? r0.a : r0.b;
    q01 = ix0 == bx ? r1.a : r1.b;
    q11 = ix1 == bx ? r1.a : r1.b;
  } else {
    q00 = img[(size_t)iy0 * W + ix0], q10 = img[(size_t)iy0 * W + ix1];
    q01 = img[(size_t)iy1 * W + ix0], q11 = img[(size_t)iy1 * W + ix1];
  }
  f3 top = mix3(rgbe_texel(q00), rgbe_texel(q10), fx);
  f3 bot = mix3(rgbe_texel(q01), rgbe_texel(q11), fx);
  return mix3(top, bot, fy);
}

// Bilinear lookups in the two planes of the env cache (DevScene::cache_xy, cache_pdf): tex_fetch's arithmetic on the
// components the caller uses, with a row's two texels -- neighbours, or the same texel at the map's edge -- taken from
// the pair (bx, bx + 1) with one load.  W >= 2.
EZD void bilinear_taps(int W, int H, float u, float v, int& ix0, int& ix1, int& iy0, int& iy1, float& fx, float& fy) {
  float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
  float x0 = ez_floor(x), y0 = ez_floor(y);
  fx = x - x0;
  fy = y - y0;
  ix0 = (int)x0, iy0 = (int)y0, ix1 = ix0 + 1, iy1 = iy0 + 1;
  if (ix0 < 0) ix0 = 0;
  if (iy0 < 0) iy0 = 0;
  if (ix1 > W - 1) ix1 = W - 1;
  if (iy1 > H - 1) iy1 = H - 1;
}
EZD float tex_fetch_pdf(const float* __restrict__ img, int W, int H, float u, float v) {
  struct __attribute__((packed, aligned(4))) Pair {
    float a, b;
  };
  int ix0, ix1, iy0, iy1;
  float fx, fy;
  bilinear_taps(W, H, sane01(u), sane01(v), ix0, ix1, iy0, iy1, fx, fy);
  const int bx = ix0 < W - 2 ? ix0 : W - 2;
  const Pair r0 = *reinterpret_cast<const Pair*>(img + (size_t)iy0 * W + bx);
  const Pair r1 = *reinterpret_cast<const Pair*>(img + (size_t)iy1 * W + bx);
  const float p00 = ix0 == bx ? r0.a : r0.b, p10 = ix1 == bx ? r0.a : r0.b;
  const float p01 = ix0 == bx ? r1.a : r1.b, p11 = ix1 == bx ? r1.a : r1.b;
  return ez_mix(ez_mix(p00, p10, fx), ez_mix(p01, p11, fx), fy);
}
EZD void tex_fetch_xy(const float2* __restrict__ img, int W, int H, float u, float v, float& cx, float& cy) {
  struct __attribute__((aligned(8))) Pair {
    float2 a, b;
  };
  int ix0, ix1, iy0, iy1;
  float fx, fy;
  bilinear_taps(W, H, sane01(u), sane01(v), ix0, ix1, iy0, iy1, fx, fy);
  const int bx = ix0 < W - 2 ? ix0 : W - 2;
  const Pair r0 = *reinterpret_cast<const Pair*>(img + (size_t)iy0 * W + bx);
  const Pair r1 = *reinterpret_cast<const Pair*>(img + (size_t)iy1 * W + bx);
  const float2 p00 = ix0 == bx ? r0.a : r0.b, p10 = ix1 == bx ? r0.a : r0.b;
  const float2 p01 = ix0 == bx ? r1.a : r1.b, p11 = ix1 == bx ? r1.a : r1.b;
  cx = ez_mix(ez_mix(p00.x, p10.x, fx), ez_mix(p01.x, p11.x, fx), fy);
  cy = ez_mix(ez_mix(p00.y, p10.y, fx), ez_mix(p01.y, p11.y, fx), fy);
}

// toSphericalCoord: P5/fsh:684-690
EZD void to_spherical(f3 v, float& u, float& w) {
  u = ez_atan2(v.z, v.x);
  w = ez_asin(v.y);
  u = u / (2.0f * PI);
  w = w / PI;
  u = u + 0.5f;
  w = w + 0.5f;
  w = 1.0f - w;
}
// hdrColor: P5/fsh:693-697 (P3 clamp: P3/fsh:151-156)
template <bool FULLCTR>
EZD f3 hdr_color(const DevScene& sc, f3 L, float env_clamp, Counters& ctr) {
  if (FULLCTR) ctr.envmap++;
  if (!sc.hdr) return mk(0, 0, 0);
  float u, v;
  to_spherical(normalize(L), u, v);
  f3 c = sc.hdr_rgbe ? tex_fetch_rgbe(sc.hdr_rgbe, sc.hdr_pairs, sc.env_w, sc.env_h, sc.env_filter, u, v)
                     : tex_fetch(sc.hdr, sc.env_w, sc.env_h, sc.env_filter, u, v);
  if (env_clamp > 0.0f) c = mk(ez_min(c.x, env_clamp), ez_min(c.y, env_clamp), ez_min(c.z, env_clamp));
  return c;
}
// SampleHdr: P5/fsh:667-679
template <bool FULLCTR>
EZD f3 sample_hdr(const DevScene& sc, float xi1, float xi2, Counters& ctr) {
  if (FULLCTR) ctr.envcache++;
  f3 c;
  if (sc.cache_xy && sc.env_filter == EZRT_FILTER_BILINEAR) {
    c.z = 0.0f;
    tex_fetch_xy(sc.cache_xy, sc.env_w, sc.env_h, xi1, xi2, c.x, c.y);
  } else {
    c = tex_fetch(sc.cache, sc.env_w, sc.env_h, sc.env_filter, xi1, xi2);
  }
  float x = c.x, y = 1.0f - c.y;
  float phi = 2.0f * PI * (x - 0.5f);
  float theta = PI * (y - 0.5f);
  float st, ct, sp, cp;
  ez_sincos(theta, &st, &ct);
  ez_sincos(phi, &sp, &cp);
  return mk(ct * cp, st, ct * sp);
}
// hdrPdf: P5/fsh:701-712
template <bool FULLCTR>
EZD float hdr_pdf(const DevScene& sc, f3 L, Counters& ctr) {
  if (FULLCTR) ctr.envcache++;
  float u, v;
  to_spherical(normalize(L), u, v);
  float pdf = (sc.cache_pdf && sc.env_filter == EZRT_FILTER_BILINEAR) ? tex_fetch_pdf(sc.cache_pdf, sc.env_w, sc.env_h, u, v)
                                                                     : tex_fetch(sc.cache, sc.env_w, sc.env_h, sc.env_filter, u, v).z;
  float theta = PI * (0.5f - v);
  float sin_theta = ez_max(ez_sin(theta), 1e-10f);
  int res = sc.env_w;
  float p_convert = (float)(res * res / 2) / (2.0f * PI * PI * sin_theta);
  return pdf * p_convert;
}

// hdrColor(L) and hdrPdf(L) of the SAME direction (P5/fsh:829-830, 873-874): both start with
// toSphericalCoord(normalize(L)) -- a software atan2 and asin, ~170 instructions -- evaluated once here; the same
// operations on the same operands, so the same bits as the two separate calls (the compiler does not merge them).
template <bool FULLCTR>
EZD void hdr_color_pdf(const DevScene& sc, f3 L, float env_clamp, Counters& ctr, f3& color, float& pdf_light) {
  if (FULLCTR) {
    ctr.envmap++;
    ctr.envcache++;
  }
  float u, v;
  to_spherical(normalize(L), u, v);
  if (!sc.hdr) {
    color = mk(0, 0, 0);
  } else {
    f3 c = sc.hdr_rgbe ? tex_fetch_rgbe(sc.hdr_rgbe, sc.hdr_pairs, sc.env_w, sc.env_h, sc.env_filter, u, v)
                       : tex_fetch(sc.hdr, sc.env_w, sc.env_h, sc.env_filter, u, v);
    if (env_clamp > 0.0f) c = mk(ez_min(c.x, env_clamp), ez_min(c.y, env_clamp), ez_min(c.z, env_clamp));
    color = c;
  }
  float pdf = (sc.cache_pdf && sc.env_filter == EZRT_FILTER_BILINEAR) ? tex_fetch_pdf(sc.cache_pdf, sc.env_w, sc.env_h, u, v)
                                                                     : tex_fetch(sc.cache, sc.env_w, sc.env_h, sc.env_filter, u, v).z;
  float theta = PI * (0.5f - v);
  float sin_theta = ez_max(ez_sin(theta), 1e-10f);
  int res = sc.env_w;
  float p_convert = (float)(res * res / 2) / (2.0f * PI * PI * sin_theta);
  pdf_light = pdf * p_convert;
}

// ---------------------------------------------------------------------------
// Disney principled BRDF: P5/fsh:400-549 (isotropic), P4/fsh:375-473 (anisotropic)
EZD float schlick(float u) {
  float m = ez_clamp(1.0f - u, 0.0f, 1.0f);
  float m2 = m * m;
  return m2 * m2 * m;
}
EZD float gtr1(float NdotH, float a) {
  if (a >= 1.0f) return 1.0f / PI;
  float a2 = a * a;
  float t = 1.0f + (a2 - 1.0f) * NdotH * NdotH;
  return (a2 - 1.0f) / (PI * ez_log(a2) * t);
}
// the same with the material's precomputed a2 - 1 and PI * log(a2) (Mat)
EZD float gtr1_m(float NdotH, const Mat& m) {
  if (m.alpha_gtr1 >= 1.0f) return 1.0f / PI;
  float t = 1.0f + m.gtr1_a2m1 * NdotH * NdotH;
  return m.gtr1_a2m1 / (m.gtr1_pilog * t);
}
EZD float gtr2(float NdotH, float a) {
  float a2 = a * a;
  float t = 1.0f + (a2 - 1.0f) * NdotH * NdotH;
  return a2 / (PI * t * t);
}
EZD float gtr2_aniso(float NdotH, float HdotX, float HdotY, float ax, float ay) {
  return 1.0f / (PI * ax * ay * sqr(sqr(HdotX / ax) + sqr(HdotY / ay) + NdotH * NdotH));
}
EZD float smith_ggx(float NdotV, float alphaG) {
  float a = alphaG * alphaG;
  float b = NdotV * NdotV;
  return 1.0f / (NdotV + __builtin_sqrtf(a + b - a * b));
}
EZD float smith_ggx_aniso(float NdotV, float VdotX, float VdotY, float ax, float ay) {
  return 1.0f / (NdotV + __builtin_sqrtf(sqr(VdotX * ax) + sqr(VdotY * ay) + sqr(NdotV)));
}

template <bool ANISO>
EZD f3 brdf_evaluate(f3 V, f3 N, f3 L, f3 X, f3 Y, const Mat& m) {
  float NdotL = dot(N, L), NdotV = dot(N, V);
  if (NdotL < 0.0f || NdotV < 0.0f) return mk(0, 0, 0);
  f3 H = normalize(L + V);
  float NdotH = dot(N, H), LdotH = dot(L, H);

  // Cdlum, Ctint, Cspec, Cspec0, Csheen (P5/fsh:446-451): functions of the material alone -> Mat (mat_derive)
  const f3 Cdlin = m.baseColor, one = mk(1, 1, 1), Cspec0 = m.Cspec0, Csheen = m.Csheen;

  float Fd90 = 0.5f + 2.0f * LdotH * LdotH * m.roughness;
  float FL = schlick(NdotL), FV = schlick(NdotV);
  float Fd = ez_mix(1.0f, Fd90, FL) * ez_mix(1.0f, Fd90, FV);

  float Fss90 = LdotH * LdotH * m.roughness;
  float Fss = ez_mix(1.0f, Fss90, FL) * ez_mix(1.0f, Fss90, FV);
  float ss = 1.25f * (Fss * (1.0f / (NdotL + NdotV) - 0.5f) + 0.5f);

  float Ds, Gs;
  float FH = schlick(LdotH);
  f3 Fs = mix3(Cspec0, one, FH);
  if (!ANISO) {
    Ds = gtr2(NdotH, m.alpha_gtr2);
    Gs = smith_ggx(NdotL, m.roughness);
    Gs *= smith_ggx(NdotV, m.roughness);
  } else {
    float aspect = __builtin_sqrtf(1.0f - m.anisotropic * 0.9f);
    float ax = ez_max(0.001f, sqr(m.roughness) / aspect);
    float ay = ez_max(0.001f, sqr(m.roughness) * aspect);
    Ds = gtr2_aniso(NdotH, dot(H, X), dot(H, Y), ax, ay);
    Gs = smith_ggx_aniso(NdotL, dot(L, X), dot(L, Y), ax, ay);
    Gs *= smith_ggx_aniso(NdotV, dot(V, X), dot(V, Y), ax, ay);
  }
  float Dr = gtr1_m(NdotH, m);
  float Fr = ez_mix(0.04f, 1.0f, FH);
  float Gr = smith_ggx(NdotL, 0.25f) * smith_ggx(NdotV, 0.25f);

  f3 Fsheen = Csheen * (FH * m.sheen);
  f3 diffuse = Cdlin * ((1.0f / PI) * ez_mix(Fd, ss, m.subsurface)) + Fsheen;
  f3 specular = (Fs * Gs) * Ds;
  float cc = 0.25f * Gr * Fr * Dr * m.clearcoat;
  return (diffuse * (1.0f - m.metallic) + specular) + mk(cc, cc, cc);
}

// getTangent: P5/fsh:553-558
EZD void get_tangent(f3 N, f3& tangent, f3& bitangent) {
  f3 helper = mk(1, 0, 0);
  if (ez_abs(N.x) > 0.999f) helper = mk(0, 0, 1);
  bitangent = normalize(cross(N, helper));
  tangent = normalize(cross(N, bitangent));
}
// toNormalHemisphere: P5/fsh:561-567
EZD f3 to_normal_hemisphere(f3 v, f3 N) {
  f3 helper = mk(1, 0, 0);
  if (ez_abs(N.x) > 0.999f) helper = mk(0, 0, 1);
  f3 tangent = normalize(cross(N, helper));
  f3 bitangent = normalize(cross(N, tangent));
  return (tangent * v.x + bitangent * v.y) + N * v.z;
}
// SampleHemisphere: P5/fsh:570-576
EZD f3 sample_hemisphere(float xi1, float xi2) {
  float z = xi1;
  float r = ez_max(0.0f, __builtin_sqrtf(1.0f - z * z));
  float phi = 2.0f * PI * xi2;
  float s, c;
  ez_sincos(phi, &s, &c);
  return mk(r * c, r * s, z);
}
// SampleCosineHemisphere: P5/fsh:579-590
EZD f3 sample_cosine_hemisphere(float xi1, float xi2, f3 N) {
  float r = __builtin_sqrtf(xi1);
  float theta = xi2 * 2.0f * PI;
  float s, c;
  ez_sincos(theta, &s, &c);
  float x = r * c, y = r * s;
  float z = __builtin_sqrtf(1.0f - x * x - y * y);
  return to_normal_hemisphere(mk(x, y, z), N);
}
// SampleGTR2 / SampleGTR1: P5/fsh:593-630
EZD f3 sample_gtr(float xi1, f3 V, f3 N, float cos_theta_h) {
  float phi_h = 2.0f * PI * xi1;
  float sin_phi_h, cos_phi_h;
  ez_sincos(phi_h, &sin_phi_h, &cos_phi_h);
  float sin_theta_h = __builtin_sqrtf(ez_max(0.0f, 1.0f - cos_theta_h * cos_theta_h));
  f3 H = mk(sin_theta_h * cos_phi_h, sin_theta_h * sin_phi_h, cos_theta_h);
  H = to_normal_hemisphere(H, N);
  return reflect(-V, H);
}
// SampleBRDF: P5/fsh:633-664
EZD f3 sample_brdf(float xi1, float xi2, float xi3, f3 V, f3 N, const Mat& m) {
  const float alpha_GTR1 = m.alpha_gtr1, alpha_GTR2 = m.alpha_gtr2;
  float r_diffuse = 1.0f - m.metallic;
  float r_specular = 1.0f;
  float r_clearcoat = 0.25f * m.clearcoat;
  float r_sum = r_diffuse + r_specular + r_clearcoat;
  float p_diffuse = r_diffuse / r_sum;
  float p_specular = r_specular / r_sum;
  float rd = xi3;
  if (rd <= p_diffuse) return sample_cosine_hemisphere(xi1, xi2, N);
  if (p_diffuse < rd && rd <= p_diffuse + p_specular) {
    float c = __builtin_sqrtf((1.0f - xi2) / (1.0f + (alpha_GTR2 * alpha_GTR2 - 1.0f) * xi2));
    return sample_gtr(xi1, V, N, c);
  }
  if (p_diffuse + p_specular < rd) {
    float c = __builtin_sqrtf((1.0f - ez_pow(alpha_GTR1 * alpha_GTR1, 1.0f - xi2)) / (1.0f - alpha_GTR1 * alpha_GTR1));
    return sample_gtr(xi1, V, N, c);
  }
  return mk(0, 1, 0);
}
// BRDF_Pdf: P5/fsh:715-752
EZD float brdf_pdf(f3 V, f3 N, f3 L, const Mat& m) {
  float NdotL = dot(N, L), NdotV = dot(N, V);
  if (NdotL < 0.0f || NdotV < 0.0f) return 0.0f;
  f3 H = normalize(L + V);
  float NdotH = dot(N, H), LdotH = dot(L, H);
  float Ds = gtr2(NdotH, m.alpha_gtr2);
  float Dr = gtr1_m(NdotH, m);
  float pdf_diffuse = NdotL / PI;
  float pdf_specular = Ds * NdotH / (4.0f * LdotH);
  float pdf_clearcoat = Dr * NdotH / (4.0f * LdotH);
  float r_diffuse = 1.0f - m.metallic;
  float r_specular = 1.0f;
  float r_clearcoat = 0.25f * m.clearcoat;
  float r_sum = r_diffuse + r_specular + r_clearcoat;
  float p_diffuse = r_diffuse / r_sum;
  float p_specular = r_specular / r_sum;
  float p_clearcoat = r_clearcoat / r_sum;
  float pdf = p_diffuse * pdf_diffuse + p_specular * pdf_specular + p_clearcoat * pdf_clearcoat;
  return ez_max(1e-10f, pdf);
}
EZD float mis_mix_weight(float a, float b) { // P5/fsh:754-757
  float t = a * a;
  return t / (b * b + t);
}

// ---- SURVEY 8(f4), integrator 52: the anisotropic specular lobe (P4/fsh:440-449; commented out in P5/fsh:472-483)
// importance-sampled and priced.  Not in the reference: include/ezrt.h (EZRT_INTEGRATOR_P5_MIS_ANISO) names the
// specification (sample_gtr2_aniso, sample_brdf_aniso, brdf_pdf_aniso); these are the same operations in the same order.
EZD void aniso_alphas(const Mat& m, float& ax, float& ay) { // P4/fsh:441-443
  float aspect = __builtin_sqrtf(1.0f - m.anisotropic * 0.9f);
  ax = ez_max(0.001f, sqr(m.roughness) / aspect);
  ay = ez_max(0.001f, sqr(m.roughness) * aspect);
}
EZD f3 sample_gtr2_aniso(float xi1, float xi2, f3 V, f3 N, f3 X, f3 Y, float ax, float ay) {
  float phi_h = 2.0f * PI * xi1;
  float sin_phi_h, cos_phi_h;
  ez_sincos(phi_h, &sin_phi_h, &cos_phi_h);
  float k = __builtin_sqrtf(xi2 / ez_max(1e-7f, 1.0f - xi2));
  f3 H = (X * (k * ax * cos_phi_h) + Y * (k * ay * sin_phi_h)) + N;
  H = normalize(H);
  return reflect(-V, H);
}
EZD f3 sample_brdf_aniso(float xi1, float xi2, float xi3, f3 V, f3 N, f3 X, f3 Y, const Mat& m) {
  const float alpha_GTR1 = m.alpha_gtr1;
  float ax, ay;
  aniso_alphas(m, ax, ay);
  float r_diffuse = 1.0f - m.metallic;
  float r_specular = 1.0f;
  float r_clearcoat = 0.25f * m.clearcoat;
  float r_sum = r_diffuse + r_specular + r_clearcoat;
  float p_diffuse = r_diffuse / r_sum;
  float p_specular = r_specular / r_sum;
  float rd = xi3;
  if (rd <= p_diffuse) return sample_cosine_hemisphere(xi1, xi2, N);
  if (p_diffuse < rd && rd <= p_diffuse + p_specular) return sample_gtr2_aniso(xi1, xi2, V, N, X, Y, ax, ay);
  if (p_diffuse + p_specular < rd) {
    float c = __builtin_sqrtf((1.0f - ez_pow(alpha_GTR1 * alpha_GTR1, 1.0f - xi2)) / (1.0f - alpha_GTR1 * alpha_GTR1));
    return sample_gtr(xi1, V, N, c);
  }
  return mk(0, 1, 0);
}
EZD float brdf_pdf_aniso(f3 V, f3 N, f3 L, f3 X, f3 Y, const Mat& m) {
  float NdotL = dot(N, L), NdotV = dot(N, V);
  if (NdotL < 0.0f || NdotV < 0.0f) return 0.0f;
  f3 H = normalize(L + V);
  float NdotH = dot(N, H), LdotH = dot(L, H);
  float ax, ay;
  aniso_alphas(m, ax, ay);
  float Ds = gtr2_aniso(NdotH, dot(H, X), dot(H, Y), ax, ay);
  float Dr = gtr1_m(NdotH, m);
  float pdf_diffuse = NdotL / PI;
  float pdf_specular = Ds * NdotH / (4.0f * LdotH);
  float pdf_clearcoat = Dr * NdotH / (4.0f * LdotH);
  float r_diffuse = 1.0f - m.metallic;
  float r_specular = 1.0f;
  float r_clearcoat = 0.25f * m.clearcoat;
  float r_sum = r_diffuse + r_specular + r_clearcoat;
  float p_diffuse = r_diffuse / r_sum;
  float p_specular = r_specular / r_sum;
  float p_clearcoat = r_clearcoat / r_sum;
  float pdf = p_diffuse * pdf_diffuse + p_specular * pdf_specular + p_clearcoat * pdf_clearcoat;
  return ez_max(1e-10f, pdf);
}

// BRDF_Evaluate(V, N, L) and BRDF_Pdf(V, N, L) of the SAME direction (P5/fsh:832-833, 858-859): both start with
// H = normalize(L + V), N.H, L.H and both evaluate GTR2 / GTR1 of that half vector -- once here.  The same operations
// on the same operands as brdf_evaluate<ANISO> followed by brdf_pdf (ANISO: brdf_pdf_aniso), hence the same bits; the
// compiler does not merge the two calls (a normalisation, two divisions and the GTR terms per pair).
template <bool ANISO>
EZD void brdf_evaluate_pdf(f3 V, f3 N, f3 L, f3 X, f3 Y, const Mat& m, f3& f_r, float& pdf_out) {
  float NdotL = dot(N, L), NdotV = dot(N, V);
  if (NdotL < 0.0f || NdotV < 0.0f) {
    f_r = mk(0, 0, 0);
    pdf_out = 0.0f;
    return;
  }
  f3 H = normalize(L + V);
  float NdotH = dot(N, H), LdotH = dot(L, H);
  const f3 Cdlin = m.baseColor, one = mk(1, 1, 1), Cspec0 = m.Cspec0, Csheen = m.Csheen;

  float Fd90 = 0.5f + 2.0f * LdotH * LdotH * m.roughness;
  float FL = schlick(NdotL), FV = schlick(NdotV);
  float Fd = ez_mix(1.0f, Fd90, FL) * ez_mix(1.0f, Fd90, FV);

  float Fss90 = LdotH * LdotH * m.roughness;
  float Fss = ez_mix(1.0f, Fss90, FL) * ez_mix(1.0f, Fss90, FV);
  float ss = 1.25f * (Fss * (1.0f / (NdotL + NdotV) - 0.5f) + 0.5f);

  float Ds, Gs;
  float FH = schlick(LdotH);
  f3 Fs = mix3(Cspec0, one, FH);
  if (!ANISO) {
    Ds = gtr2(NdotH, m.alpha_gtr2);
    Gs = smith_ggx(NdotL, m.roughness);
    Gs *= smith_ggx(NdotV, m.roughness);
  } else {
    float aspect = __builtin_sqrtf(1.0f - m.anisotropic * 0.9f);
    float ax = ez_max(0.001f, sqr(m.roughness) / aspect);
    float ay = ez_max(0.001f, sqr(m.roughness) * aspect);
    Ds = gtr2_aniso(NdotH, dot(H, X), dot(H, Y), ax, ay);
    Gs = smith_ggx_aniso(NdotL, dot(L, X), dot(L, Y), ax, ay);
    Gs *= smith_ggx_aniso(NdotV, dot(V, X), dot(V, Y), ax, ay);
  }
  float Dr = gtr1_m(NdotH, m);
  float Fr = ez_mix(0.04f, 1.0f, FH);
  float Gr = smith_ggx(NdotL, 0.25f) * smith_ggx(NdotV, 0.25f);

  f3 Fsheen = Csheen * (FH * m.sheen);
  f3 diffuse = Cdlin * ((1.0f / PI) * ez_mix(Fd, ss, m.subsurface)) + Fsheen;
  f3 specular = (Fs * Gs) * Ds;
  float cc = 0.25f * Gr * Fr * Dr * m.clearcoat;
  f_r = (diffuse * (1.0f - m.metallic) + specular) + mk(cc, cc, cc);

  // BRDF_Pdf: P5/fsh:729-751 on the same H, Ds, Dr
  float pdf_diffuse = NdotL / PI;
  float pdf_specular = Ds * NdotH / (4.0f * LdotH);
  float pdf_clearcoat = Dr * NdotH / (4.0f * LdotH);
  float r_diffuse = 1.0f - m.metallic;
  float r_specular = 1.0f;
  float r_clearcoat = 0.25f * m.clearcoat;
  float r_sum = r_diffuse + r_specular + r_clearcoat;
  float p_diffuse = r_diffuse / r_sum;
  float p_specular = r_specular / r_sum;
  float p_clearcoat = r_clearcoat / r_sum;
  float pdf = p_diffuse * pdf_diffuse + p_specular * pdf_specular + p_clearcoat * pdf_clearcoat;
  pdf_out = ez_max(1e-10f, pdf);
}

} // namespace ezd
