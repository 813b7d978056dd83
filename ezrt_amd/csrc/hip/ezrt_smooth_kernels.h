// ezrt_smooth_kernels.h -- the kernels of the mesh smoothing (include/ezrt_smooth.h, rules U1 to U9): many umbrella steps over the
// stars of a weld in one stream-ordered call.  Included by ezrt_mesh.hip, after ezrt_iso_kernels.h (it uses ezi::tri_normal, the N1
// of ezrt_vertices.h, and the tiled prefix sum of ezrt_scan_kernels.h through its host).
//
//   smooth_plan_kernel      U2, U4: one lane per corner; the lane that is the FIRST corner of its vertex's star walks the star once and
//                           leaves the verdict in state[c]; every lane copies its position into both buffers; a workgroup counts its
//                           moving vertices into counts[block]
//   smooth_terms_kernel     U3, U9: one lane per index i -- as a corner it counts itself under its rule, as a position of `star` it
//                           resolves the two terms of star[i] to slots, as a moving vertex it takes its rank and writes its record
//   smooth_step_kernel      U5 .. U7, global route: one launch per step, one lane per moving vertex
//   smooth_steps_lds_kernel the same, LDS route: ONE workgroup, both buffers in LDS, every step in one launch
//   smooth_fill_kernel      U1, U8: a workgroup per tile of consecutive rows; STAGED or per lane
//
// Slots.  The state x_j(v) of an ACTIVE vertex lives in slot f, the first corner of its star; every other corner's pos_j is its own
// stored position and lives in slot c.  f is a corner of v and of no other vertex, so the two kinds cannot collide.  Both buffers
// start as a copy of the stored positions, a step writes the slots of the moving vertices only, and everything else stays what it was:
// U3 for free.  A term is 31 bits of slot and bit 31: set when the half-edge it came over has edge_class 1.  The SMOOTH sum masks the
// bit, the BORDER sum takes the terms that carry it; U4 counted two of them.  Terms are indexed by the position in `star`, not by the
// vertex: they are a function of star[i] alone, so arrays whose ranges overlap still give every vertex what U6 says.
//
// Bounds (U2).  The weld and topology arrays are the caller's and are NOT trusted: every index read from them is checked against
// 3 n_rows before it is used, star_offsets[v + 1] is read for v < 3 n_rows only, rows of tri36 are read at ids below n_rows only.
// What the steps and the fill read from `work` this call wrote from checked values: a record's f, lo and hi passed U2 in the plan, a
// term read at a position of an ACTIVE vertex's range is a slot below 3 n_rows, and the number of records is clamped to 3 n_rows.
// The only loops not bounded by a constant are the walk of a star, at most 3 n_rows steps, the steps of the LDS route, and a
// workgroup's stride over tiles or records.  No floating-point atomics; no grid-wide barrier, no workgroup waits for another; the
// buffers cross launch boundaries.
#pragma once

#include "ezrt_lds_budget.h"

constexpr int SM_BLOCK = 256;                  // lanes of a workgroup; corners of an entry of counts
constexpr int SM_FILL_TILE = 64;               // rows of a fill tile: 576 float4s, 9 KiB of LDS
constexpr unsigned SM_GRID_MAX = 2048;         // workgroups of the strided launches: 8 per CU
constexpr int SM_LDS_BLOCK = 512;              // lanes of the LDS route's one workgroup
// the LDS route keeps both buffers, 2 * 3 * 12 B per row, under the static cap of a launch with a granule's slack, in whole waves of rows
constexpr int SM_TILE_MAX = (int)((ezi::LDS_PER_LAUNCH - ezi::LDS_PER_LAUNCH / 16) / 72 / 64 * 64);
static_assert(SM_TILE_MAX >= 64 && (size_t)SM_TILE_MAX * 72 <= ezi::LDS_PER_LAUNCH, "the LDS route's buffers must fit a launch");
constexpr uint32_t SM_KEPT = 0u, SM_SMOOTH = 1u, SM_BORDER = 2u, SM_ACTIVE = 4u; // state: the rule in bits 0-1, ACTIVE in bit 2
constexpr uint32_t SM_BIT = 0x80000000u;       // of a term: over a BOUNDARY half-edge; of a record's f: a BORDER vertex

struct SmoothArgs {
  const float* tri36;
  int32_t n_rows;
  int32_t steps;
  int32_t flags;
  float lambda, mu;
  const uint8_t* edge_class;
  const int32_t* vertex;
  const int32_t* star_offsets;
  const int32_t* star;
  const uint8_t* vert_flags;
  float* out;
  unsigned long long* summary;
  // work
  long long* counts; // moving vertices per SM_BLOCK corners, then their prefix sum; the total behind them
  long long* tiles;  // of the tiled scan
  float* pos[2];     // 3 floats per slot
  uint32_t* term;    // two per position of star
  uint32_t* rec;     // three per moving vertex: f (bit 31: BORDER), lo, hi
  uint8_t* state;    // per corner; nonzero at first corners only
};

// U2 (S4): the star of corner c's vertex, when the arrays are usable that far (the star's entries are checked by the walk)
__device__ inline bool smooth_range(const SmoothArgs& a, uint32_t H, uint32_t c, int32_t& v, int32_t& lo, int32_t& hi) {
  v = a.vertex[c];
  if (v < 0 || (uint32_t)v >= H) return false;
  lo = a.star_offsets[v], hi = a.star_offsets[v + 1];
  return lo >= 0 && lo < hi && (uint32_t)hi <= H;
}
// U3, U8: the slot of corner c and the rule it is under -- f and its vertex's rule when the vertex is ACTIVE, else c and KEPT
__device__ inline uint32_t smooth_slot(const SmoothArgs& a, uint32_t H, uint32_t c, uint32_t& rule) {
  rule = SM_KEPT;
  int32_t v, lo, hi;
  if (!smooth_range(a, H, c, v, lo, hi)) return c;
  const int32_t f = a.star[lo];
  if (f < 0 || (uint32_t)f >= H || a.vertex[f] != v) return c;
  const uint32_t s = a.state[f]; // lane f of the plan wrote it, from this vertex's star
  if (!(s & SM_ACTIVE)) return c;
  rule = s & 3u;
  return (uint32_t)f;
}

// U2, U4: the verdict of every vertex at the first corner of its star, 0 at every other corner; both buffers; the workgroup's count
__global__ __launch_bounds__(SM_BLOCK) void smooth_plan_kernel(SmoothArgs a) {
  const uint32_t H = 3u * (uint32_t)a.n_rows;
  const uint64_t c64 = (uint64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
  uint32_t s = 0u;
  if (c64 < H) {
    const uint32_t c = (uint32_t)c64, t = c / 3u, k = c - 3u * t;
    const float* p = a.tri36 + (size_t)t * 36 + 3u * k;
    const float x = p[0], y = p[1], z = p[2];
    float *q0 = a.pos[0] + 3u * (size_t)c, *q1 = a.pos[1] + 3u * (size_t)c;
    q0[0] = x, q0[1] = y, q0[2] = z, q1[0] = x, q1[1] = y, q1[2] = z;
    int32_t v, lo, hi;
    if (smooth_range(a, H, c, v, lo, hi) && a.star[lo] == (int32_t)c) {
      const uint32_t fl = a.vert_flags[v];
      const bool border = fl == 1u && !(a.flags & EZRT_SMOOTH_PIN_BORDER);
      bool usable = true;
      uint32_t r = 0u;
      for (int32_t j = lo; j < hi; j++) { // at most 3 n_rows steps
        const int32_t o = a.star[j];
        if (o < 0 || (uint32_t)o >= H) {
          usable = false;
          break;
        }
        if (border) { // the half-edge that leaves the corner is o, the one that enters it 3 t + kb
          const uint32_t to = (uint32_t)o / 3u, ko = (uint32_t)o - 3u * to, kb = ko == 0u ? 2u : ko - 1u;
          r += (a.edge_class[o] == 1u) + (a.edge_class[3u * to + kb] == 1u);
        }
      }
      if (usable) s = SM_ACTIVE | (fl == 0u ? SM_SMOOTH : (border && r == 2u ? SM_BORDER : SM_KEPT));
    }
    a.state[c] = (uint8_t)s;
  }
  const int moving = __syncthreads_count((s & 3u) != 0u);
  if (threadIdx.x == 0) a.counts[blockIdx.x] = moving;
}

// U3, U9: terms, records and the summary; counts holds the exclusive prefix sum of the plan's counts
__global__ __launch_bounds__(SM_BLOCK) void smooth_terms_kernel(SmoothArgs a) {
  __shared__ uint32_t red[(SM_BLOCK / 64) * 4];
  __shared__ uint32_t wave_moving[SM_BLOCK / 64];
  const uint32_t H = 3u * (uint32_t)a.n_rows;
  const uint64_t i64 = (uint64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t cnt[4] = {0u, 0u, 0u, 0u}; // summary[1 .. 4]
  uint32_t s = 0u;
  if (i64 < H) {
    const uint32_t i = (uint32_t)i64;
    uint32_t rule;
    smooth_slot(a, H, i, rule);
    cnt[0] = rule == SM_SMOOTH, cnt[1] = rule == SM_BORDER, cnt[2] = rule == SM_KEPT;
    s = a.state[i];
    cnt[3] = (s & SM_ACTIVE) != 0u;
    const int32_t o = a.star[i];
    uint32_t ta = 0u, tb = 0u; // of an entry that is out of range: never read, its vertex is not ACTIVE
    if (o >= 0 && (uint32_t)o < H) {
      const uint32_t t = (uint32_t)o / 3u, k = (uint32_t)o - 3u * t, ka = k == 2u ? 0u : k + 1u, kb = ka == 2u ? 0u : ka + 1u;
      uint32_t unused;
      ta = smooth_slot(a, H, 3u * t + ka, unused) | (a.edge_class[o] == 1u ? SM_BIT : 0u);
      tb = smooth_slot(a, H, 3u * t + kb, unused) | (a.edge_class[3u * t + kb] == 1u ? SM_BIT : 0u);
    }
    a.term[2u * (size_t)i] = ta, a.term[2u * (size_t)i + 1u] = tb;
  }
  // the rank of a moving vertex: the workgroup's offset, the waves before this one, the lanes before this one
  const bool moving = (s & 3u) != 0u;
  const unsigned long long ballot = __ballot(moving);
  if (lane == 0u) wave_moving[wave] = (uint32_t)__popcll(ballot);
#pragma unroll
  for (int f = 0; f < 4; f++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt[f] += __shfl_xor(cnt[f], o);
    if (lane == 0u) red[wave * 4 + f] = cnt[f];
  }
  __syncthreads();
  if (moving) {
    unsigned long long rank = (unsigned long long)a.counts[blockIdx.x] + (unsigned long long)__popcll(ballot & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; w++) rank += wave_moving[w];
    if (rank < H) { // (it is: at most one record per corner)
      const uint32_t i = (uint32_t)i64;
      int32_t v, lo, hi;
      smooth_range(a, H, i, v, lo, hi); // the plan's lane passed it, on the same arrays
      uint32_t* r = a.rec + 3u * (size_t)rank;
      r[0] = i | ((s & 3u) == SM_BORDER ? SM_BIT : 0u), r[1] = (uint32_t)lo, r[2] = (uint32_t)hi;
    }
  }
  if (threadIdx.x < 4) {
    unsigned long long x = 0ull;
#pragma unroll
    for (int w = 0; w < SM_BLOCK / 64; w++) x += red[w * 4 + threadIdx.x];
    if (x) atomicAdd(&a.summary[1 + threadIdx.x], x);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    atomicAdd(&a.summary[0], (unsigned long long)a.n_rows);
    atomicAdd(&a.summary[5], (unsigned long long)a.steps);
    atomicAdd(&a.summary[6], (unsigned long long)a.flags);
  }
}

// the records of this call: the scan's total, never more than one per corner
__device__ inline uint32_t smooth_moving(const SmoothArgs& a, uint32_t H) {
  const long long m = a.counts[((uint64_t)H + SM_BLOCK - 1) / SM_BLOCK];
  return m < 0 ? 0u : (m > (long long)H ? H : (uint32_t)m);
}
// U5 .. U7: record i's vertex from src to dst with weight w.  One lane; k sequential gathers of two slots.
__device__ inline void smooth_vertex_step(const SmoothArgs& a, uint32_t i, const float* src, float* dst, float w) {
  const uint32_t* r = a.rec + 3u * (size_t)i;
  const uint32_t fb = r[0], f = fb & ~SM_BIT, lo = r[1], hi = r[2];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, mx, my, mz; // from +0
  if (!(fb & SM_BIT)) { // U6
    for (uint32_t j = lo; j < hi; j++) {
      const uint2 tm = *(const uint2*)(a.term + 2u * (size_t)j);
      const float *pa = src + 3u * (size_t)(tm.x & ~SM_BIT), *pb = src + 3u * (size_t)(tm.y & ~SM_BIT);
      sx = sx + (pa[0] + pb[0]), sy = sy + (pa[1] + pb[1]), sz = sz + (pa[2] + pb[2]); // the inner sum first
    }
    const float d = (float)(2u * (hi - lo));
    mx = sx / d, my = sy / d, mz = sz / d;
  } else { // U7: the two terms that came over a BOUNDARY half-edge, in the walk's order
    for (uint32_t j = lo; j < hi; j++) {
      const uint2 tm = *(const uint2*)(a.term + 2u * (size_t)j);
      if (tm.x & SM_BIT) {
        const float* p = src + 3u * (size_t)(tm.x & ~SM_BIT);
        sx = sx + p[0], sy = sy + p[1], sz = sz + p[2];
      }
      if (tm.y & SM_BIT) {
        const float* p = src + 3u * (size_t)(tm.y & ~SM_BIT);
        sx = sx + p[0], sy = sy + p[1], sz = sz + p[2];
      }
    }
    mx = sx * 0.5f, my = sy * 0.5f, mz = sz * 0.5f;
  }
  const float* x = src + 3u * (size_t)f;
  float* y = dst + 3u * (size_t)f;
  const float x0 = x[0], x1 = x[1], x2 = x[2];
  y[0] = x0 + w * (mx - x0), y[1] = x1 + w * (my - x1), y[2] = x2 + w * (mz - x2);
}

// the global route: step j reads buffer j & 1 and writes the other
__global__ __launch_bounds__(SM_BLOCK) void smooth_step_kernel(SmoothArgs a, int32_t j) {
  const uint32_t H = 3u * (uint32_t)a.n_rows, M = smooth_moving(a, H);
  const float w = (j & 1) ? a.mu : a.lambda;
  const float* src = a.pos[j & 1];
  float* dst = a.pos[(j + 1) & 1];
  for (uint64_t i = (uint64_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < M; i += (uint64_t)gridDim.x * SM_BLOCK) // at most M rounds
    smooth_vertex_step(a, (uint32_t)i, src, dst, w);
}

// the LDS route: n_rows <= SM_TILE_MAX, ONE workgroup.  Both buffers in LDS, a workgroup barrier between steps, and the final
// buffer -- every slot of it -- back to pos[steps & 1], where the fill reads it on either route.
__global__ __launch_bounds__(SM_LDS_BLOCK) void smooth_steps_lds_kernel(SmoothArgs a) {
  __shared__ float buf[2][SM_TILE_MAX * 9];
  const uint32_t H = 3u * (uint32_t)a.n_rows, M = smooth_moving(a, H);
  if (H > (uint32_t)SM_TILE_MAX * 3u) return; // (the host chose this route: it is not)
  for (uint32_t i = threadIdx.x; i < 3u * H; i += SM_LDS_BLOCK) {
    const float x = a.pos[0][i];
    buf[0][i] = x, buf[1][i] = x;
  }
  __syncthreads();
  for (int32_t j = 0; j < a.steps; j++) { // at most EZRT_SMOOTH_STEPS_MAX rounds
    const float w = (j & 1) ? a.mu : a.lambda;
    for (uint32_t i = threadIdx.x; i < M; i += SM_LDS_BLOCK) smooth_vertex_step(a, i, buf[j & 1], buf[(j + 1) & 1], w);
    __syncthreads();
  }
  float* dst = a.pos[a.steps & 1];
  const float* fin = buf[a.steps & 1];
  for (uint32_t i = threadIdx.x; i < 3u * H; i += SM_LDS_BLOCK) dst[i] = fin[i];
}

// U1, U8: the position of corner c of the output, whose own stored position is p
__device__ inline void smooth_corner(const SmoothArgs& a, uint32_t H, const float* fin, uint32_t c, const float* p, float P[3]) {
  uint32_t rule;
  const uint32_t f = smooth_slot(a, H, c, rule);
  if (rule == SM_KEPT) {
    P[0] = p[0], P[1] = p[1], P[2] = p[2]; // its own bits
  } else {
    const float* x = fin + 3u * (size_t)f;
    P[0] = x[0], P[1] = x[1], P[2] = x[2];
  }
}

// The fill.  STAGED: a workgroup takes tiles of SM_FILL_TILE rows, blockIdx.x, blockIdx.x + gridDim.x, ...; the lanes load the tile's
// float4s into LDS (with out == tri36 the tile is read whole before any of it is written), one lane per corner replaces the
// position, one lane per row computes N1, and the lanes store the tile's float4s at consecutive addresses.  Per lane: every lane
// reads its own row's positions into registers and writes the row float by float, to the same bits.
template <bool STAGED>
__global__ __launch_bounds__(SM_BLOCK) void smooth_fill_kernel(SmoothArgs a) {
  const uint32_t H = 3u * (uint32_t)a.n_rows;
  const float* fin = a.pos[a.steps & 1];
  if constexpr (STAGED) {
    __shared__ float4 rec4[SM_FILL_TILE * 9];
    float* rec = (float*)rec4;
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = ((uint64_t)a.n_rows + SM_FILL_TILE - 1) / SM_FILL_TILE;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // at most `tiles` rounds
      const uint64_t base = tile * SM_FILL_TILE;
      const uint32_t rows = (uint32_t)std::min<uint64_t>((uint64_t)a.n_rows - base, (uint64_t)SM_FILL_TILE);
      const float4* in4 = (const float4*)a.tri36 + base * 9; // 16-byte aligned: the host chose this instance
      float4* out4 = (float4*)a.out + base * 9;
      for (uint32_t i = tid; i < rows * 9u; i += SM_BLOCK) rec4[i] = in4[i];
      __syncthreads();
      if (tid < rows * 3u) { // one lane per corner
        const uint32_t r = tid / 3u, k = tid - 3u * r;
        float* p = rec + r * 36u + 3u * k;
        float P[3];
        smooth_corner(a, H, fin, 3u * ((uint32_t)base + r) + k, p, P);
        p[0] = P[0], p[1] = P[1], p[2] = P[2];
      }
      __syncthreads();
      if (tid < rows) { // one lane per row
        float* own = rec + tid * 36u;
        float nx, ny, nz;
        ezi::tri_normal(own, nx, ny, nz);
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) own[9u + 3u * k] = nx, own[10u + 3u * k] = ny, own[11u + 3u * k] = nz;
      }
      __syncthreads();
      for (uint32_t i = tid; i < rows * 9u; i += SM_BLOCK) out4[i] = rec4[i];
      __syncthreads(); // the records are the next tile's
    }
  } else {
    const uint64_t t64 = (uint64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (t64 < (uint64_t)a.n_rows) {
      const uint32_t t = (uint32_t)t64;
      const float* own = a.tri36 + (size_t)t * 36;
      float p[9], q[9];
#pragma unroll
      for (uint32_t i = 0; i < 9u; i++) p[i] = own[i]; // with out == tri36: the positions are read before any is written
#pragma unroll
      for (uint32_t k = 0; k < 3u; k++) smooth_corner(a, H, fin, 3u * t + k, p + 3u * k, q + 3u * k);
      float nx, ny, nz;
      ezi::tri_normal(q, nx, ny, nz);
      float* o = a.out + (size_t)t * 36;
#pragma unroll
      for (uint32_t i = 0; i < 9u; i++) o[i] = q[i];
#pragma unroll
      for (uint32_t k = 0; k < 3u; k++) o[9u + 3u * k] = nx, o[10u + 3u * k] = ny, o[11u + 3u * k] = nz;
#pragma unroll
      for (uint32_t i = 18; i < 36u; i++) o[i] = own[i]; // U1: the source row's material on the bits (in place: itself)
    }
  }
}
