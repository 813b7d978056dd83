// ezrt_iso_kernels.h -- the kernels of the isosurface extraction (include/ezrt_isosurface.h, rules G1 to G9): marching tetrahedra on the
// Kuhn split of every cell of the caller's grid of values, as triangle rows.  Included by ezrt_mesh.hip, after
// ezrt_decimate_kernels.h (it uses ezi::tri_normal, the N1 of ezrt_vertices.h; the prefix sum between the two kernels is scan_tiled
// of ezrt_scan_kernels.h, launched by the host).
//
//   iso_count_kernel    G3, G5, G8: a workgroup per block of ISO_BLOCK cells, one lane per cell; the block's count into offsets[b], the
//                       terms of the summary reduced over the wave
//   iso_fill_kernel     G5 .. G9: a workgroup per block; STAGED or per lane
//
// A cell's eight values stay in registers and nothing is indexed by a run-time value: a tet's corners come out of two packed
// constants (iso_c1, iso_c2), a corner's value out of a chain of selects (iso_pick), and a piece's edges out of the mask's bits.  The
// winding of a piece is G5's table, two words of 14 bits.
//
// The STAGED fill.  A lane that writes its own rows of 144 B issues accesses that its neighbours cannot merge, and a block holds up
// to 12 * ISO_BLOCK rows, which do not fit the LDS.  So the block's rows are built in at most ISO_ROUNDS rounds of ISO_BLOCK rows:
// in a round every lane whose rows reach into it puts floats 0-17 of those rows into LDS (floats 18-35, the material, were put
// there once), and then the lanes are laid over the round's float4s -- 16 B per lane at consecutive addresses, since the rows of a
// block are consecutive (G8).  That route needs out 16-byte aligned (a row is nine float4s, so then every row is); otherwise, and in
// the measurement variant EZRT_ISO_PER_LANE, the host launches the per-lane instance, in which every lane writes its own rows float
// by float.  Both build a row by iso_row, so they give the same bits.
//
// Bounds (G9).  offsets is the caller's and is NOT trusted: a block is written only when 0 <= offsets[b], offsets[b] + c <= capacity
// and offsets[b + 1] - offsets[b] == c with c recomputed here, so every row index written is below capacity and a block is written
// whole or not at all.  values is read at vertices of cells below n_cells only, offsets at b and b + 1 with b < n_blocks.  Every
// loop is bounded by a constant: six tets, two pieces, ISO_ROUNDS rounds, nine float4s per lane and round.
#pragma once

constexpr int ISO_BLOCK = EZRT_ISO_BLOCK;          // lanes of a workgroup, and cells of a block
constexpr int ISO_ROUND = 256;                     // rows of a staging round: 36 KiB, below a quarter of the CU's LDS
constexpr int ISO_ROUNDS = 12 * ISO_BLOCK / ISO_ROUND; // a cell emits at most 12 rows
static_assert(ISO_ROUND == ISO_BLOCK, "the material is put into LDS one row per lane");

struct IsoGrid {
  double ox, oy, oz, hx, hy, hz; // G2 is computed in double
  float iso;
  bool live; // G1
};
__device__ inline void iso_grid_load(const float* __restrict__ grid8, IsoGrid& G) {
  const float inf = __builtin_inff();
  const float ox = grid8[0], oy = grid8[1], oz = grid8[2], hx = grid8[3], hy = grid8[4], hz = grid8[5], iso = grid8[6];
  G.ox = (double)ox, G.oy = (double)oy, G.oz = (double)oz, G.hx = (double)hx, G.hy = (double)hy, G.hz = (double)hz, G.iso = iso;
  G.live = ez_abs(ox) < inf && ez_abs(oy) < inf && ez_abs(oz) < inf && ez_abs(hx) < inf && ez_abs(hy) < inf && ez_abs(hz) < inf &&
           ez_abs(iso) < inf && hx > 0.0f && hy > 0.0f && hz > 0.0f;
}

// a cell: its low corner, its eight values (corner dx + 2 dy + 4 dz), the byte of the INSIDE corners, and what it emits
struct IsoCell {
  uint32_t i, j, k;
  float f[8];
  uint32_t byte;
  uint32_t count; // G5: 0 .. 12
  bool finite;    // G3
};
// G4: corners T1 and T2 of tet t (T0 is corner 0 and T3 corner 7), a nibble each: 1 1 2 2 4 4 and 3 5 3 6 5 6
__device__ inline uint32_t iso_c1(uint32_t t) { return (0x442211u >> (4u * t)) & 7u; }
__device__ inline uint32_t iso_c2(uint32_t t) { return (0x656353u >> (4u * t)) & 7u; }
// the mask of the INSIDE vertices of tet t, T0 the low bit
__device__ inline uint32_t iso_tet_mask(uint32_t byte, uint32_t t) {
  return (byte & 1u) | (((byte >> iso_c1(t)) & 1u) << 1) | (((byte >> iso_c2(t)) & 1u) << 2) | (((byte >> 7) & 1u) << 3);
}
// G5: {0, 1, 2, 1, 0}[popcount]
__device__ inline uint32_t iso_tet_count(uint32_t mask) {
  const uint32_t p = (uint32_t)__popc(mask);
  return p == 2u ? 2u : (p & 1u);
}
// G3, G5 of cell c < n_cells: eight loads
__device__ inline void iso_classify(const float* __restrict__ values, int nx, int ny, const IsoGrid& G, uint32_t c, IsoCell& C) {
  const uint32_t cx = (uint32_t)nx - 1u, cy = (uint32_t)ny - 1u, r = c / cx;
  C.i = c - r * cx, C.k = r / cy, C.j = r - C.k * cy;
  const size_t sx = (size_t)nx, sxy = sx * (size_t)ny, base = (size_t)C.k * sxy + (size_t)C.j * sx + C.i;
  const float inf = __builtin_inff();
  bool fin = true;
  uint32_t byte = 0u;
#pragma unroll
  for (int n = 0; n < 8; n++) {
    const float f = values[base + (n & 1) + ((n >> 1) & 1) * sx + (n >> 2) * sxy];
    C.f[n] = f;
    fin = fin && ez_abs(f) < inf;
    byte |= (f < G.iso ? 1u : 0u) << n;
  }
  uint32_t count = 0u;
#pragma unroll
  for (uint32_t t = 0; t < 6u; t++) count += iso_tet_count(iso_tet_mask(byte, t));
  C.byte = byte, C.finite = fin, C.count = fin && G.live ? count : 0u;
}

// (the eight values by value: handed a pointer, the compiler turns the selects into a load at a run-time index and the cell into scratch)
__device__ inline float iso_pick(float f0, float f1, float f2, float f3, float f4, float f5, float f6, float f7, uint32_t c) {
  const float lo = c & 2u ? (c & 1u ? f3 : f2) : (c & 1u ? f1 : f0), hi = c & 2u ? (c & 1u ? f7 : f6) : (c & 1u ? f5 : f4);
  return c & 4u ? hi : lo;
}
__device__ inline float iso_value(const IsoCell& C, uint32_t c) { return iso_pick(C.f[0], C.f[1], C.f[2], C.f[3], C.f[4], C.f[5], C.f[6], C.f[7], c); }
__device__ inline uint32_t iso_corner(uint32_t t, uint32_t l) { return l == 0u ? 0u : (l == 1u ? iso_c1(t) : (l == 2u ? iso_c2(t) : 7u)); }
// G6: the point on the edge of tet t between its local vertices la < lb
__device__ inline void iso_point(const IsoGrid& G, const IsoCell& C, uint32_t t, uint32_t la, uint32_t lb, float* P) {
  const uint32_t ca = iso_corner(t, la), cb = iso_corner(t, lb);
  const double fA = (double)iso_value(C, ca), fB = (double)iso_value(C, cb);
  const double s = ((double)G.iso - fA) / (fB - fA);
  const double ax = G.ox + (double)(C.i + (ca & 1u)) * G.hx, bx = G.ox + (double)(C.i + (cb & 1u)) * G.hx;
  const double ay = G.oy + (double)(C.j + ((ca >> 1) & 1u)) * G.hy, by = G.oy + (double)(C.j + ((cb >> 1) & 1u)) * G.hy;
  const double az = G.oz + (double)(C.k + (ca >> 2)) * G.hz, bz = G.oz + (double)(C.k + (cb >> 2)) * G.hz;
  const double dx = bx - ax, dy = by - ay, dz = bz - az;
  P[0] = (float)(ax + s * dx), P[1] = (float)(ay + s * dy), P[2] = (float)(az + s * dz);
}
// G5, G7: floats 0-17 of piece p of tet t, whose mask has one, two or three bits
__device__ inline void iso_row(const IsoGrid& G, const IsoCell& C, uint32_t t, uint32_t mask, uint32_t p, float row[18]) {
  const uint32_t pc = (uint32_t)__popc(mask), other = ~mask & 15u;
  uint32_t x0, y0, x1, y1, x2, y2; // the three edges, as written
  if (pc != 2u) {                  // the lone vertex against the other three in ascending order
    const uint32_t lone = (uint32_t)__ffs(pc == 1u ? mask : other) - 1u;
    x0 = lone, x1 = lone, x2 = lone;
    y0 = lone == 0u ? 1u : 0u, y1 = lone <= 1u ? 2u : 1u, y2 = lone == 3u ? 2u : 3u;
  } else {
    const uint32_t a = (uint32_t)__ffs(mask) - 1u, b = 31u - (uint32_t)__clz(mask), c = (uint32_t)__ffs(other) - 1u, d = 31u - (uint32_t)__clz(other);
    x0 = a, y0 = c;
    x1 = p == 0u ? a : b, y1 = d;
    x2 = b, y2 = p == 0u ? d : c;
  }
  // the winding: exchanged masks 2 5 8 10 11 14 for the even permutations (tets 0, 3, 4), the other eight for the odd ones
  const uint32_t table = (0x19u >> t) & 1u ? 0x4D24u : 0x32DAu;
  if ((table >> mask) & 1u) {
    const uint32_t tx = x1, ty = y1;
    x1 = x2, y1 = y2, x2 = tx, y2 = ty;
  }
  iso_point(G, C, t, x0 < y0 ? x0 : y0, x0 < y0 ? y0 : x0, row);
  iso_point(G, C, t, x1 < y1 ? x1 : y1, x1 < y1 ? y1 : x1, row + 3);
  iso_point(G, C, t, x2 < y2 ? x2 : y2, x2 < y2 ? y2 : x2, row + 6);
  ezi::tri_normal(row, row[9], row[10], row[11]); // N1 of the OUTPUT positions
#pragma unroll
  for (int n = 0; n < 3; n++) row[12 + n] = row[9 + n], row[15 + n] = row[9 + n];
}

// G3, G5, G8.  The four terms of the summary are at most 768 and 64 per wave: they travel as 10-bit fields of one word.
__global__ __launch_bounds__(ISO_BLOCK) void iso_count_kernel(const float* values, int nx, int ny, uint32_t n_cells, const float* grid8,
                                                              long long* offsets, unsigned long long* summary) {
  __shared__ uint32_t part[ISO_BLOCK / 64];
  IsoGrid G;
  iso_grid_load(grid8, G);
  const uint64_t c = (uint64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
  unsigned long long term = 0ull;
  if (c < (uint64_t)n_cells) {
    IsoCell C;
    iso_classify(values, nx, ny, G, (uint32_t)c, C);
    const int field = !C.finite ? 3 : (C.count ? 1 : 2);
    term = (unsigned long long)C.count | (1ull << (10 * field));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
  if ((threadIdx.x & 63) == 0) { // one int64 atomic per wave and term
    part[threadIdx.x >> 6] = (uint32_t)(term & 1023ull);
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const unsigned long long x = (term >> (10 * f)) & 1023ull;
      if (x) atomicAdd(&summary[f], x);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0u;
#pragma unroll
    for (int w = 0; w < ISO_BLOCK / 64; w++) sum += part[w];
    offsets[blockIdx.x] = (long long)sum;
    if (sum) atomicAdd(&summary[4], 1ull);
    if (blockIdx.x == 0) {
      atomicAdd(&summary[5], (unsigned long long)n_cells);
      if (G.live) atomicAdd(&summary[6], 1ull);
    }
  }
}

struct IsoFillArgs {
  const float* values;
  int32_t nx, ny;
  uint32_t n_cells;
  const float* grid8;
  const float* material18;
  const long long* offsets;
  long long capacity;
  float* out;
  int32_t* cell; // or nullptr
};

template <bool STAGED>
__global__ __launch_bounds__(ISO_BLOCK) void iso_fill_kernel(IsoFillArgs a) {
  __shared__ uint32_t sums[ISO_BLOCK];
  __shared__ __attribute__((aligned(16))) float stage[STAGED ? ISO_ROUND * 36 : 4];
  const uint32_t t = threadIdx.x;
  const long long o = a.offsets[blockIdx.x], o1 = a.offsets[blockIdx.x + 1];
  if (o1 == o) return; // G9: the block has nothing, or is not written; no value is read
  IsoGrid G;
  iso_grid_load(a.grid8, G);
  const uint64_t c = (uint64_t)blockIdx.x * ISO_BLOCK + t;
  IsoCell C;
  C.count = 0u, C.byte = 0u;
  if (c < (uint64_t)a.n_cells) iso_classify(a.values, a.nx, a.ny, G, (uint32_t)c, C);
  sums[t] = C.count;
  __syncthreads();
#pragma unroll
  for (uint32_t s = 1; s < (uint32_t)ISO_BLOCK; s <<= 1) {
    const uint32_t add = t >= s ? sums[t - s] : 0u;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  const uint32_t total = sums[ISO_BLOCK - 1], first = sums[t] - C.count; // the block's count and this cell's first row in it
  if (!(total > 0u && o >= 0 && o <= a.capacity - (long long)total && o1 >= o && o1 - o == (long long)total)) return; // G9
  if (STAGED) {
#pragma unroll
    for (int n = 0; n < 18; n++) stage[t * 36u + 18u + n] = a.material18[n];
  }
#pragma unroll 1
  for (uint32_t round = 0; round < (uint32_t)(STAGED ? ISO_ROUNDS : 1); round++) {
    const uint32_t lo = STAGED ? round * ISO_ROUND : 0u, hi = STAGED ? (lo + ISO_ROUND < total ? lo + ISO_ROUND : total) : total;
    if (lo >= total) break; // the same for every lane
    if (C.count > 0u && first < hi && first + C.count > lo) { // (a cell that takes no part has a byte and no count)
      uint32_t r = first; // the row of the next piece, in the block
#pragma unroll 1
      for (uint32_t tet = 0; tet < 6u; tet++) {
        const uint32_t mask = iso_tet_mask(C.byte, tet), n = iso_tet_count(mask);
#pragma unroll 1
        for (uint32_t p = 0; p < 2u; p++) {
          if (p >= n) continue;
          if (r >= lo && r < hi) {
            float row[18];
            iso_row(G, C, tet, mask, p, row);
            if (STAGED) {
              float* d = stage + (r - lo) * 36u;
#pragma unroll
              for (int n2 = 0; n2 < 18; n2++) d[n2] = row[n2];
            } else {
              float* d = a.out + (size_t)(o + r) * 36;
#pragma unroll
              for (int n2 = 0; n2 < 18; n2++) d[n2] = row[n2];
#pragma unroll
              for (int n2 = 0; n2 < 18; n2++) d[18 + n2] = a.material18[n2]; // G7: on the bits
            }
            if (a.cell) a.cell[o + r] = (int32_t)c;
          }
          r++;
        }
      }
    }
    if (STAGED) {
      __syncthreads();
      const float4* in4 = (const float4*)stage;
      float4* out4 = (float4*)(a.out + (size_t)(o + lo) * 36); // 16-byte aligned: the host chose this instance
      const uint32_t n4 = (hi - lo) * 9u;
#pragma unroll
      for (int j = 0; j < 9; j++) {
        const uint32_t f = (uint32_t)j * ISO_BLOCK + t;
        if (f < n4) out4[f] = in4[f];
      }
      __syncthreads();
    }
  }
}
