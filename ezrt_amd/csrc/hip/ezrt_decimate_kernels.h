// ezrt_decimate_kernels.h -- the kernels of the decimation (include/ezrt_decimate.h, rules D1 to D10): the caller's rows with their
// vertices clustered on a uniform grid.  Included by ezrt_mesh.hip, after ezrt_subdiv_kernels.h (it uses loops_hash, topo_bits and
// ezi::tri_normal; the two prefix sums are scan_tiled of ezrt_scan_kernels.h, launched by the host).
//
//   dec_init_kernel      the two tables, the accumulators and the summary, whatever `work` held
//   dec_insert_kernel    D2, D3, D4, D5: one lane per corner; THE HOT KERNEL.  A run of neighbouring lanes with the same cell claims or
//                        finds the cell's slot once (64-bit atomicCAS) and adds its sums, its count, its lowest corner and its D5 words
//                        with one set of integer atomics
//   dec_flag_kernel      D3: one lane per corner; 1 where the corner is the lowest of its cell (the prefix sum numbers the cells)
//   dec_cells_kernel     D3, D4, D5: one lane per corner; cell; the lowest corner of a cell writes cell_corner and cell_point
//   dec_classify_kernel  D6, D7: one lane per row; a survivor claims or finds the slot of its unordered triple; atomicMin leaves the
//                        lowest row
//   dec_keep_kernel      D6, D7, D9: one lane per row; the keep flag into offsets (the prefix sum follows), the summary
//   dec_fill_kernel      D8, D10: a workgroup per tile of DC_BLOCK consecutive rows; STAGED or per lane
//
// The discipline is that of ezrt_topology_kernels.h.  INSIDE a launch, a word that one workgroup writes and another reads is touched
// by agent-scope atomics ONLY: key (atomicCAS), sum and cnt (atomicAdd), low, mn (atomicMin), mx (atomicMax) in the insert, which
// nobody reads in the launch that writes them; rep2 (atomicCAS, atomicMin) in the classify.  EVERYTHING ELSE crosses a launch
// boundary on one stream: slot, slot2, ids, and the outputs cell and offsets, which later launches of the same call read back with
// plain loads.  cell[c] doubles as the liveness of corner c between the launches (the insert stores -1 or 0, the cells launch the
// number); the classify reads the cells of ANOTHER row, one launch after they were written.  No floating-point atomics: a cell's
// sums are int64 and exact, so nothing depends on the order of arrival.
//
// The run.  On a coarse grid most neighbouring corners share a cell, and 64 lanes adding to one slot are 64 atomics in a row on one
// address.  A lane is the HEAD of a run when its key differs from the lane before it; the three fractions and a word of counts (the
// corners, and per axis the corners whose M1 key differs from the head's) go through a segmented inclusive scan of six shuffle steps,
// and the LAST lane of the run holds the run's totals and issues the atomics.  The lowest corner of a run is its head's.  D5 needs
// only "are all keys of the cell equal": a uniform run lowers mn and raises mx with its key, any other run sets them to 0 and ~0, and
// the axis is kept when mn == mx in the end.
//
// Bounds.  Every probe loop runs at most T (T2) times; the tables are at most half full (3 n_rows cells in T >= 6 n_rows slots, n_rows
// triples in T2 >= 2 n_rows).  Every index read back from `work` is checked against its array before it is used.  The fill trusts
// neither cell nor offsets (D10): a row is written only when its three cells are in 0 .. 3 n_rows - 1 -- cell_point has that many
// points -- and 0 <= offsets[t], offsets[t] + 1 <= capacity, offsets[t + 1] - offsets[t] == 1, so every row index written is below
// capacity and a row is written whole or not at all.  tri36, cell and offsets are read at rows below n_rows only.
#pragma once

constexpr int DC_BLOCK = 256;            // lanes of a workgroup, and rows of a fill tile
constexpr unsigned long long DC_EMPTY = ~0ull; // an empty slot: a key has 63 bits
constexpr uint32_t DC_NONE = 0xFFFFFFFFu;

// D1
struct DecGrid {
  double o[3], h;
  bool live;
};
__device__ inline void dec_grid_load(const float* __restrict__ g, DecGrid& G) {
  const float inf = __builtin_inff();
  const float a = g[0], b = g[1], c = g[2], h = g[3];
  G.o[0] = (double)a, G.o[1] = (double)b, G.o[2] = (double)c, G.h = (double)h;
  G.live = ez_abs(a) < inf && ez_abs(b) < inf && ez_abs(c) < inf && h > 0.0f && h < inf;
}
// D2: U of one coordinate; false when it is out of range (a NaN and an infinity are: every comparison with them fails or overflows)
__device__ inline bool dec_fixed(float x, double o, double h, long long& U) {
  const double u = ((double)x - o) / h;
  const double w = u * 16777216.0;
  const bool ok = w >= -0x1p44 && w < 0x1p44;
  U = ok ? (long long)__builtin_floor(w) : 0ll;
  return ok;
}
// D2: does the row take part, and U of its corner k
__device__ inline bool dec_corner(const float* __restrict__ row, uint32_t k, const DecGrid& G, long long U[3]) {
  bool ok = G.live;
  U[0] = U[1] = U[2] = 0;
#pragma unroll
  for (uint32_t m = 0; m < 3u; m++) {
#pragma unroll
    for (uint32_t ax = 0; ax < 3u; ax++) {
      long long u;
      ok = dec_fixed(row[3u * m + ax], G.o[ax], G.h, u) && ok;
      U[ax] = m == k ? u : U[ax];
    }
  }
  return ok;
}

// The cell table is twelve ARRAYS over the slots, not an array of 64-byte records.  The record was tried (profiles/r36): with one
// vertex per cell the count fell from 2.18 to 1.97 ms per 10^6 rows, but on a coarse grid, which is what the call is for, it rose from
// 0.47 to 0.71 ms (the Bunny scene, 729 cells): the eleven atomics of every run then queue on ONE line of one channel, where the
// arrays spread them over eleven.
struct DecArgs {
  const float* tri36;
  int32_t n_rows;
  const float* grid4;
  int32_t flags;
  uint64_t T, T2;           // slots of the two tables, powers of two, at most 2^32
  // work
  long long* ids;           // 3 n_rows + 1: 1 at the lowest corner of a cell, then its exclusive prefix sum; [3 n_rows] = n_cells
  long long* tiles;         // ceil(3 n_rows / SCAN_TILE) + 1: the sums of a scan's tiles
  unsigned long long* key;  // T: the cell of the slot, three 21-bit indices; DC_EMPTY
  unsigned long long* sum;  // 3 T, axis by axis: the sum of the fractions q
  uint32_t* cnt;            // T: the corners of the cell
  int32_t* low;             // T: its lowest corner
  uint32_t *mn, *mx;        // 3 T each, axis by axis: D5
  uint32_t* slot;           // 3 n_rows
  int32_t* rep2;            // T2: a survivor with the slot's triple of cells, in the end the lowest; -1 empty
  uint32_t* slot2;          // n_rows
  // outputs
  int32_t *cell, *cell_corner;
  float* cell_point;
  long long* offsets;
  unsigned long long* summary;
};

// x of all lanes of the workgroup added to *dst with ONE atomic (every lane of the workgroup calls it; `red` is free again behind it)
__device__ inline void dec_block_add(uint32_t x, unsigned long long* dst, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int w = 0; w < DC_BLOCK / 64; w++) s += red[w];
    if (s) atomicAdd(dst, s);
  }
}

__global__ __launch_bounds__(DC_BLOCK) void dec_init_kernel(DecArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * DC_BLOCK, i0 = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
  for (uint64_t i = i0; i < a.T; i += stride) a.key[i] = DC_EMPTY, a.cnt[i] = 0u, a.low[i] = INT32_MAX;
  for (uint64_t i = i0; i < 3 * a.T; i += stride) a.sum[i] = 0ull, a.mn[i] = 0xFFFFFFFFu, a.mx[i] = 0u;
  for (uint64_t i = i0; i < a.T2; i += stride) a.rep2[i] = -1;
  if (i0 < 8) a.summary[i0] = 0ull;
}

__global__ __launch_bounds__(DC_BLOCK) void dec_insert_kernel(DecArgs a) {
  DecGrid G;
  dec_grid_load(a.grid4, G);
  const uint64_t H = 3ull * (uint64_t)a.n_rows, stride = (uint64_t)gridDim.x * DC_BLOCK;
  const uint64_t rounds = (H + stride - 1) / stride; // every lane of a wave runs the same number of rounds: the shuffles are uniform
  const uint32_t mask = (uint32_t)(a.T - 1), lane = threadIdx.x & 63u;
  const unsigned long long upto = ~0ull >> (63u - lane); // the lanes 0 .. lane
  uint64_t c = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, c += stride) {
    unsigned long long key = DC_EMPTY;
    uint32_t s0 = 0u, s1 = 0u, s2 = 0u, k0 = 0u, k1 = 0u, k2 = 0u;
    bool part = false;
    if (c < H) {
      const uint64_t t = c / 3;
      const uint32_t k = (uint32_t)(c - 3 * t);
      const float* row = a.tri36 + (size_t)t * 36;
      long long U[3];
      part = dec_corner(row, k, G, U);
      if (part) {
        key = (unsigned long long)((U[0] >> 24) + 1048576ll) | (unsigned long long)((U[1] >> 24) + 1048576ll) << 21 |
              (unsigned long long)((U[2] >> 24) + 1048576ll) << 42;
        s0 = (uint32_t)(U[0] & 0xFFFFFFll), s1 = (uint32_t)(U[1] & 0xFFFFFFll), s2 = (uint32_t)(U[2] & 0xFFFFFFll);
        k0 = topo_bits(row[3u * k]), k1 = topo_bits(row[3u * k + 1u]), k2 = topo_bits(row[3u * k + 2u]);
      }
    }
    // the runs of the wave: a lane that takes no part has the key DC_EMPTY and its run does nothing
    const unsigned long long before = __shfl_up(key, 1);
    const unsigned long long heads = __ballot(lane == 0u || before != key);
    const uint32_t head = 63u - (uint32_t)__builtin_clzll(heads & upto); // lane 0 is a head: never 0 bits
    const unsigned long long above = heads & ~upto;
    const uint32_t tail = above ? (uint32_t)__builtin_ctzll(above) - 1u : 63u;
    const uint32_t h0 = (uint32_t)__shfl((int)k0, (int)head), h1 = (uint32_t)__shfl((int)k1, (int)head), h2 = (uint32_t)__shfl((int)k2, (int)head);
    // the corners (bits 0-7) and the corners whose key differs from the head's, per axis (bits 8-15, 16-23, 24-31): at most 64 each
    uint32_t w = 1u | (k0 != h0 ? 1u << 8 : 0u) | (k1 != h1 ? 1u << 16 : 0u) | (k2 != h2 ? 1u << 24 : 0u);
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
      const uint32_t t0 = (uint32_t)__shfl_up((int)s0, o), t1 = (uint32_t)__shfl_up((int)s1, o), t2 = (uint32_t)__shfl_up((int)s2, o);
      const uint32_t tw = (uint32_t)__shfl_up((int)w, o);
      if (lane >= head + o) s0 += t0, s1 += t1, s2 += t2, w += tw; // 64 fractions below 2^24: below 2^30
    }
    uint32_t p = 0u;
    bool found = false;
    if (part && lane == tail) {
      p = loops_hash((uint32_t)key, (uint32_t)(key >> 32), 0x9E3779B9u) & mask;
      for (uint64_t probe = 0; probe < a.T && !found; probe++) {
        const unsigned long long old = atomicCAS(&a.key[p], DC_EMPTY, key);
        found = old == DC_EMPTY || old == key;
        if (!found) p = (p + 1u) & mask;
      }
      if (found) {
        atomicAdd(&a.sum[p], (unsigned long long)s0);
        atomicAdd(&a.sum[a.T + p], (unsigned long long)s1);
        atomicAdd(&a.sum[2 * a.T + p], (unsigned long long)s2);
        atomicAdd(&a.cnt[p], w & 255u);
        atomicMin(&a.low[p], (int32_t)(c - (uint64_t)(lane - head)));
        const bool u0 = ((w >> 8) & 255u) == 0u, u1 = ((w >> 16) & 255u) == 0u, u2 = (w >> 24) == 0u;
        atomicMin(&a.mn[p], u0 ? h0 : 0u), atomicMax(&a.mx[p], u0 ? h0 : 0xFFFFFFFFu);
        atomicMin(&a.mn[a.T + p], u1 ? h1 : 0u), atomicMax(&a.mx[a.T + p], u1 ? h1 : 0xFFFFFFFFu);
        atomicMin(&a.mn[2 * a.T + p], u2 ? h2 : 0u), atomicMax(&a.mx[2 * a.T + p], u2 ? h2 : 0xFFFFFFFFu);
      }
    }
    const uint32_t ps = (uint32_t)__shfl((int)p, (int)tail);
    const bool fs = __shfl((int)found, (int)tail) != 0;
    // one exit: a corner that takes no part -- or that found no slot, which cannot happen in a table at most half full -- is -1
    if (c < H) {
      a.slot[c] = part && fs ? ps : 0u;
      a.cell[c] = part && fs ? 0 : -1;
    }
  }
}

// every word read from here on was written by an earlier launch
__global__ __launch_bounds__(DC_BLOCK) void dec_flag_kernel(DecArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_rows, stride = (uint64_t)gridDim.x * DC_BLOCK;
  for (uint64_t c = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x; c < H; c += stride) {
    const uint32_t s = a.slot[c];
    a.ids[c] = a.cell[c] >= 0 && (uint64_t)s < a.T && a.low[s] == (int32_t)c ? 1 : 0;
  }
}

// D4, D5: component `ax` of the point of the cell in slot s
__device__ inline float dec_point(const DecArgs& a, const DecGrid& G, uint32_t s, uint32_t ax, bool& kept) {
  const long long i = (long long)((a.key[s] >> (21u * ax)) & 0x1FFFFFull) - 1048576ll;
  const double m = (double)(long long)a.sum[ax * a.T + s] / (double)a.cnt[s];
  const double f = m * 0x1p-24;
  const double g = (double)i + f;
  const double x = G.o[ax] + g * G.h;
  const uint32_t lo = a.mn[ax * a.T + s], hi = a.mx[ax * a.T + s];
  kept = lo == hi;
  return kept ? __uint_as_float(lo) : (float)x;
}
__global__ __launch_bounds__(DC_BLOCK) void dec_cells_kernel(DecArgs a) {
  __shared__ uint32_t red[DC_BLOCK / 64];
  DecGrid G;
  dec_grid_load(a.grid4, G);
  const uint64_t H = 3ull * (uint64_t)a.n_rows, stride = (uint64_t)gridDim.x * DC_BLOCK;
  const uint64_t rounds = (H + stride - 1) / stride;
  uint64_t c = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
  uint32_t all_kept = 0u;
  for (uint64_t r = 0; r < rounds; r++, c += stride) {
    if (c >= H || a.cell[c] < 0) continue;
    const uint32_t s = a.slot[c];
    const int32_t lowest = (uint64_t)s < a.T ? a.low[s] : -1;
    const long long v = lowest >= 0 && (uint64_t)lowest < H ? a.ids[lowest] : -1;
    const bool ok = v >= 0 && (uint64_t)v < H;
    a.cell[c] = ok ? (int32_t)v : -1;
    if (!ok || (uint64_t)lowest != c) continue;
    a.cell_corner[v] = (int32_t)c;
    bool k0, k1, k2;
    float* pt = a.cell_point + 3 * (size_t)v;
    pt[0] = dec_point(a, G, s, 0u, k0), pt[1] = dec_point(a, G, s, 1u, k1), pt[2] = dec_point(a, G, s, 2u, k2);
    all_kept += k0 && k1 && k2 ? 1u : 0u;
  }
  dec_block_add(all_kept, &a.summary[5], red);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.summary[4] = (unsigned long long)a.ids[H];
}

// D6: the three cells of row t; 0 takes no part, 1 collapsed, 2 survives (c is then sorted ascending)
__device__ inline uint32_t dec_row(const int32_t* __restrict__ cell, uint64_t t, int32_t c[3]) {
  int32_t x = cell[3 * t], y = cell[3 * t + 1], z = cell[3 * t + 2];
  if (x < 0 || y < 0 || z < 0) return 0u;
  if (x == y || y == z || x == z) return 1u;
  int32_t s;
  if (x > y) s = x, x = y, y = s;
  if (y > z) s = y, y = z, z = s;
  if (x > y) s = x, x = y, y = s;
  c[0] = x, c[1] = y, c[2] = z;
  return 2u;
}
// D7.  rep2[p] is claimed by atomicCAS and afterwards only ever replaced, by atomicMin, with another row of the SAME triple: whoever
// reads it, at any time, reads a row that carries the slot's triple.
__global__ __launch_bounds__(DC_BLOCK) void dec_classify_kernel(DecArgs a) {
  const uint64_t N = (uint64_t)a.n_rows, stride = (uint64_t)gridDim.x * DC_BLOCK;
  const uint32_t mask = (uint32_t)(a.T2 - 1);
  for (uint64_t t = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x; t < N; t += stride) {
    int32_t c[3];
    uint32_t mine = DC_NONE;
    if (dec_row(a.cell, t, c) == 2u) {
      uint32_t p = loops_hash((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2]) & mask;
      bool found = false;
      for (uint64_t probe = 0; probe < a.T2 && !found; probe++) {
        const int32_t old = atomicCAS(&a.rep2[p], -1, (int32_t)t);
        if (old == -1) found = true;
        else if (old >= 0 && (uint64_t)old < N) {
          int32_t d[3];
          found = dec_row(a.cell, (uint64_t)old, d) == 2u && d[0] == c[0] && d[1] == c[1] && d[2] == c[2];
        }
        if (!found) p = (p + 1u) & mask;
      }
      if (found) {
        atomicMin(&a.rep2[p], (int32_t)t);
        mine = p;
      }
    }
    a.slot2[t] = mine;
  }
}
// D6, D7, D9: the keep flags and the summary; one workgroup per DC_BLOCK rows
__global__ __launch_bounds__(DC_BLOCK) void dec_keep_kernel(DecArgs a) {
  __shared__ uint32_t red[DC_BLOCK / 64];
  const uint64_t t = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
  uint32_t kind = 4u; // 0 kept, 1 collapsed, 2 duplicate, 3 takes no part
  if (t < (uint64_t)a.n_rows) {
    int32_t c[3];
    const uint32_t w = dec_row(a.cell, t, c);
    kind = w == 0u ? 3u : (w == 1u ? 1u : 0u);
    if (kind == 0u && (a.flags & EZRT_DECIMATE_DEDUP)) {
      const uint32_t s = a.slot2[t];
      if ((uint64_t)s < a.T2 && a.rep2[s] != (int32_t)t) kind = 2u;
    }
    a.offsets[t] = kind == 0u ? 1 : 0;
  }
#pragma unroll
  for (uint32_t f = 0; f < 4u; f++) dec_block_add(kind == f ? 1u : 0u, &a.summary[f], red);
  if (t == 0) {
    DecGrid G;
    dec_grid_load(a.grid4, G);
    a.summary[6] = (unsigned long long)a.flags;
    a.summary[7] = G.live ? 1ull : 0ull;
  }
}

struct DecFillArgs {
  const float* tri36;
  int32_t n_rows;
  const int32_t* cell;
  const float* cell_point;
  const long long* offsets;
  long long capacity;
  float* out;
  int32_t* src; // or nullptr
};
// D10: the output row of row t, or -1; pn gets the nine positions and the face normal of the OUTPUT row (D8)
__device__ inline long long dec_dest(const DecFillArgs& a, uint64_t t, float pn[12]) {
  const int64_t H = 3ll * a.n_rows;
  const int32_t x = a.cell[3 * t], y = a.cell[3 * t + 1], z = a.cell[3 * t + 2];
  if (x < 0 || x >= H || y < 0 || y >= H || z < 0 || z >= H || x == y || y == z || x == z) return -1;
  const long long o = a.offsets[t], o1 = a.offsets[t + 1];
  if (!(o >= 0 && o <= a.capacity - 1 && o1 >= o && o1 - o == 1)) return -1;
  const float *p0 = a.cell_point + 3 * (size_t)x, *p1 = a.cell_point + 3 * (size_t)y, *p2 = a.cell_point + 3 * (size_t)z;
#pragma unroll
  for (int i = 0; i < 3; i++) pn[i] = p0[i], pn[3 + i] = p1[i], pn[6 + i] = p2[i];
  ezi::tri_normal(pn, pn[9], pn[10], pn[11]);
  return o;
}

template <bool STAGED>
__global__ __launch_bounds__(DC_BLOCK) void dec_fill_kernel(DecFillArgs a) {
  __shared__ long long at_s[STAGED ? DC_BLOCK : 1];   // the destination of a row, or -1
  __shared__ float pn_s[STAGED ? DC_BLOCK * 12 : 1];  // its positions and its normal
  const uint64_t base = (uint64_t)blockIdx.x * DC_BLOCK, t = base + threadIdx.x;
  float pn[12];
  long long at = -1;
  if (t < (uint64_t)a.n_rows) at = dec_dest(a, t, pn);
  if (at >= 0 && a.src) a.src[at] = (int32_t)t;
  if (STAGED) {
    at_s[threadIdx.x] = at;
    if (at >= 0) {
#pragma unroll
      for (int i = 0; i < 12; i++) pn_s[threadIdx.x * 12 + i] = pn[i];
    }
    __syncthreads();
    const float4* in4 = (const float4*)a.tri36 + base * 9; // 16-byte aligned: the host chose this instance
    float4* out4 = (float4*)a.out;
#pragma unroll
    for (int j = 0; j < 9; j++) {
      const uint32_t f = (uint32_t)j * DC_BLOCK + threadIdx.x, r = f / 9u, part = f - 9u * r;
      const long long d = at_s[r]; // -1 for every row at and beyond n_rows: nothing is read there
      if (d < 0) continue;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (part >= 4u) v = in4[f]; // floats 16 .. 35 of the source row; 16 and 17 are replaced below
      if (part < 5u) {
        const float* b = pn_s + r * 12u;
        const uint32_t i = 4u * part; // floats i .. i + 3: a position below 9, else component (i - 9) % 3 of the normal
        const float e0 = b[i < 9u ? i : 9u + (i - 9u) % 3u], e1 = b[i + 1u < 9u ? i + 1u : 9u + (i - 8u) % 3u];
        v.x = e0, v.y = e1;
        if (part < 4u) v.z = b[i + 2u < 9u ? i + 2u : 9u + (i - 7u) % 3u], v.w = b[i + 3u < 9u ? i + 3u : 9u + (i - 6u) % 3u];
      }
      out4[(size_t)d * 9 + part] = v;
    }
  } else if (at >= 0) {
    const float* in = a.tri36 + (size_t)t * 36;
    float* o = a.out + (size_t)at * 36;
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = pn[i], o[9 + i] = pn[9 + i % 3];
#pragma unroll
    for (int i = 18; i < 36; i++) o[i] = in[i]; // D8: the source row's material on the bits
  }
}
