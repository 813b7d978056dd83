// ezrt_boundary_kernels.h -- the kernels of the boundary loops and of the cap (include/ezrt_boundary.h, rules B1 to B8 and C1 to C4):
// the holes of a mesh as ordered cycles of half-edges, their area vectors, and the fan of triangles that closes each.  Included by
// ezrt_mesh.hip, after ezrt_orient_kernels.h (it uses orient_takes, orient_runs, orient_block_sum, orient_block_max, topo_finite;
// its three prefix sums are scan_tiled of ezrt_scan_kernels.h, launched by the host).
//
//   bd_init_kernel       the union-find, the predecessors, the open marks, the counts and the summary, whatever `work` held
//   bd_next_kernel       B1, B2, B6: one lane per half-edge; the walk about the end vertex, next, the predecessor, the flag that the first
//                        prefix sum compacts, the dead ends of summary[4], A
//   bd_union_kernel      B3: one lane per half-edge; h and next[h] are united, the lower root survives
//   bd_open_kernel       B3: the one member of a path that has no successor finds its root and marks it open
//   bd_rank_init_kernel  B3: one lane per half-edge; the compacted list, and each member's (predecessor, 1) -- a cycle is cut before its root
//   bd_jump_kernel       B3: one round of pointer jumping over the compacted list, from one buffer into the other; lanes beyond B leave
//   bd_flag_kernel       B4: 1 at each head, for the second prefix sum
//   bd_number_kernel     B4, B5, B8: loop and pos of every member; the last member of a chain writes its length, flag and zeroes its sums
//   bd_scatter_kernel    B4, B7: order, loop_offsets; r_k summed over runs of lanes with one loop, one atomicAdd per run and component
//   cap_rows_kernel      C1 .. C4: one lane per row of the cap
//
// The discipline is that of ezrt_orient_kernels.h.  INSIDE a launch, a word that one workgroup writes and another reads is touched by
// agent-scope atomics ONLY: par in the union (relaxed agent-scope atomic load, atomicCAS); the words of the summary, A and area2
// (atomicAdd, atomicMax), which nobody reads in the launch that adds to them.  EVERYTHING ELSE crosses a launch boundary on one stream:
// pred[c] has one writer (B2: the successor map is injective) and is read one launch later; par is read by bd_open_kernel and
// bd_rank_init_kernel with plain loads, after the union; open has one writer per chain (a path has one end) and is read by the rank
// init; a round of the ranking reads one buffer and writes the other.
//
// Bounds.  twin and edge_class are the caller's and are NOT trusted: the walk reads twin[g] and edge_class of triangle g / 3 only after
// 0 <= g < 3 n_tri, and runs at most 3 n_tri steps.  Everything after bd_next_kernel depends on next and pred alone, which are a
// partial injection whatever the arrays held; every index read back from `work` is checked against its array before it is used.
//
// Cost.  A border vertex of valence k costs its incoming boundary half-edge k serial steps; a loop of length n is ranked in log2 n
// of the ceil(log2(3 n_tri)) rounds, and the rounds after that copy.  The sums of B7 go through runs of neighbouring lanes as the
// orientation's volumes do: one loop of 10^6 half-edges would otherwise put 3 * 10^6 atomics on three addresses.
#pragma once

constexpr int BD_BLOCK = OR_BLOCK;          // orient_block_sum and orient_block_max are written for workgroups of OR_BLOCK
constexpr unsigned long long BD_LOW = 0xFFFFFFFFull;

struct BoundaryArgs {
  const float4* tri_geom;
  int32_t n_tri;
  const int32_t* twin;
  const uint8_t* edge_class;
  // work
  long long* scan_c;           // 3 n_tri + 1: 1 at a BOUNDARY half-edge, then its exclusive prefix sum, [3 n_tri] = B; afterwards `lens`
  long long* scan_n;           // 3 n_tri + 1: first `open`; then 1 at a head of the compacted list and its prefix sum, [B] = L
  long long* tiles;            // ceil(3 n_tri / SCAN_TILE) + 1: the sums of a scan's tiles
  unsigned long long* jump[2]; // 3 n_tri each: per compacted member, ancestor << 32 | steps to it
  long long* cnt;              // 4: B, L, the bits of A, 0
  int32_t* pred;               // 3 n_tri: the half-edge whose next this is, or -1
  uint32_t* par;               // 3 n_tri: the union-find, par[h] <= h
  int32_t* comp;               // 3 n_tri: the BOUNDARY half-edges in ascending order
  uint32_t* open;              // 3 n_tri, the first words of scan_n: at a root, 1 when its chain is a path
  long long* lens;             // scan_c once the list is compacted: a loop's length, then loop_offsets, [L] = B
  int32_t rounds;              // of the ranking: ceil(log2(3 n_tri)); the result is in jump[rounds & 1]
  // outputs
  int32_t *next, *loop, *pos, *order, *loop_offsets;
  uint8_t* lflags;
  long long* area2; // or nullptr: the area group
  unsigned long long* summary;
};

__global__ __launch_bounds__(BD_BLOCK) void bd_init_kernel(BoundaryArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * BD_BLOCK, i0 = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  for (uint64_t i = i0; i < H; i += stride) a.par[i] = (uint32_t)i, a.pred[i] = -1, a.open[i] = 0u;
  if (i0 < 8) a.summary[i0] = 0ull;
  if (i0 < 4) a.cnt[i0] = 0;
}

// B2: the successor of the BOUNDARY half-edge h = 3 t + e, or -1.  The step c -> 3 (twin[c] / 3) + (twin[c] % 3 + 1) % 3 is injective
// (twin[twin[c]] == c is tested) and the start has no predecessor (its own triangle's half-edge before it is h, of class 1, not 2): the
// walk visits no half-edge twice and two walks share none, so all walks of a launch together make at most 3 n_tri steps.
__device__ inline int32_t bd_walk(const BoundaryArgs& a, uint32_t h) {
  const uint32_t H = 3u * (uint32_t)a.n_tri, t = h / 3u, e = h - 3u * t;
  uint32_t c = 3u * t + (e + 1u) % 3u;
  for (uint32_t step = 0; step < H; step++) { // at most 3 n_tri steps, and by the above never that many
    const uint32_t cls = a.edge_class[c];
    if (cls == 1u) return (int32_t)c;
    if (cls != 2u) return -1;
    const int32_t g = a.twin[c];
    if (g < 0 || (uint32_t)g >= H) return -1;
    const uint32_t tg = (uint32_t)g / 3u;
    if (tg == c / 3u || !orient_takes(a.edge_class, (int32_t)tg) || a.edge_class[g] != 2u || a.twin[g] != (int32_t)c) return -1;
    c = 3u * tg + ((uint32_t)g - 3u * tg + 1u) % 3u;
  }
  return -1;
}

__global__ __launch_bounds__(BD_BLOCK) void bd_next_kernel(BoundaryArgs a) {
  __shared__ uint32_t part[BD_BLOCK / 64];
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * BD_BLOCK;
  uint32_t dead_ends = 0u, big = 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x; i < H; i += stride) {
    const uint32_t h = (uint32_t)i, t = h / 3u, e = h - 3u * t;
    const bool takes = orient_takes(a.edge_class, (int32_t)t), boundary = takes && a.edge_class[h] == 1u; // B1
    int32_t nx = -1;
    if (boundary) {
      nx = bd_walk(a, h);
      if (nx >= 0) a.pred[nx] = (int32_t)h; // one writer: the successor map is injective
      else dead_ends++;
    }
    a.next[h] = nx;
    a.loop[h] = -1, a.pos[h] = -1; // bd_number_kernel writes those of the BOUNDARY half-edges, three launches on
    a.scan_c[h] = boundary ? 1 : 0;
    if (a.area2 && takes && e == 0u) { // B6: the largest finite |coordinate|, on the bits
      const float4* g = a.tri_geom + (size_t)t * 3;
#pragma unroll
      for (int v = 0; v < 3; v++) {
        const float4 q = g[v];
        const uint32_t ux = __float_as_uint(q.x) & 0x7FFFFFFFu, uy = __float_as_uint(q.y) & 0x7FFFFFFFu, uz = __float_as_uint(q.z) & 0x7FFFFFFFu;
        big = topo_finite(ux) && ux > big ? ux : big;
        big = topo_finite(uy) && uy > big ? uy : big;
        big = topo_finite(uz) && uz > big ? uz : big;
      }
    }
  }
  dead_ends = orient_block_sum(dead_ends, part);
  big = orient_block_max(big, part);
  if (threadIdx.x == 0) { // one atomic per workgroup and figure
    if (dead_ends) atomicAdd(&a.summary[4], (unsigned long long)dead_ends);
    if (big) atomicMax((unsigned long long*)&a.cnt[2], (unsigned long long)big);
  }
}

// B3, the union-find over half-edges: par[h] <= h, a root is hooked ONCE, by atomicCAS, under a lower root, and a word only ever moves
// to a lower ancestor.  The surviving root of a chain is its lowest member whatever the order: of a cycle, its HEAD.
__device__ inline uint32_t bd_word(const uint32_t* par, uint32_t x) { return __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline uint32_t bd_find(uint32_t* par, uint32_t x) {
  for (uint32_t p = bd_word(par, x); p < x;) { // strictly descending: at most x steps
    const uint32_t gp = bd_word(par, p);
    if (gp < p) atomicCAS(&par[x], p, gp); // path halving: an ancestor, and lower than what the word holds
    x = p, p = gp;
  }
  return x;
}
__global__ __launch_bounds__(BD_BLOCK) void bd_union_kernel(BoundaryArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * BD_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x; i < H; i += stride) {
    const int32_t nx = a.next[i]; // of the launch before
    if (nx < 0 || (uint64_t)nx >= H) continue;
    uint32_t x = (uint32_t)i, y = (uint32_t)nx;
    for (uint64_t tries = 0; tries <= H; tries++) { // a failed hook means the root was hooked lower meanwhile: finitely often
      x = bd_find(a.par, x), y = bd_find(a.par, y);
      if (x == y) break;
      const uint32_t hi = x > y ? x : y, lo = x > y ? y : x;
      if (atomicCAS(&a.par[hi], hi, lo) == hi) break;
    }
  }
}

// A chain with a member that has no successor is a path, and a path has exactly one such member: it alone writes its root's mark.
// par is final and read with plain loads; scan_c still holds the flags.
__global__ __launch_bounds__(BD_BLOCK) void bd_open_kernel(BoundaryArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * BD_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x; i < H; i += stride) {
    if (a.scan_c[i] != 1 || a.next[i] >= 0) continue;
    uint32_t x = (uint32_t)i;
    for (uint32_t p = a.par[x]; p < x; p = a.par[x]) x = p; // strictly descending
    a.open[x] = 1u;
  }
}

// scan_c is summed: a BOUNDARY half-edge h is member scan_c[h] of the compacted list.  A member starts at its predecessor with one
// step to it; a head -- of a path the member without a predecessor, of a cycle its root, before which the cycle is cut -- at itself
// with none.
__global__ __launch_bounds__(BD_BLOCK) void bd_rank_init_kernel(BoundaryArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * BD_BLOCK, i0 = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  const long long B = a.scan_c[H];
  for (uint64_t i = i0; i < H; i += stride) {
    const long long k = a.scan_c[i];
    if (a.scan_c[i + 1] - k != 1 || k < 0 || k >= (long long)H) continue;
    a.comp[k] = (int32_t)i;
    int32_t p = a.pred[i];
    if (a.par[i] == (uint32_t)i && a.open[i] == 0u) p = -1; // the root of a chain that is no path: the head of a cycle
    long long pk = p >= 0 && (uint64_t)p < H ? a.scan_c[p] : -1;
    if (pk < 0 || pk >= B) pk = -1;
    a.jump[0][k] = pk < 0 ? ((unsigned long long)k << 32) : (((unsigned long long)pk << 32) | 1ull);
  }
  if (i0 == 0) a.cnt[0] = B < 0 ? 0 : (B > (long long)H ? (long long)H : B);
}

// One round: (ancestor, steps) becomes (the ancestor's ancestor, the sum).  A head is its own ancestor at 0 steps, so a member that
// has reached its head stays.  After r rounds a member has gone min(pos, 2^r) steps: ceil(log2(3 n_tri)) rounds reach every head.
__global__ __launch_bounds__(BD_BLOCK) void bd_jump_kernel(BoundaryArgs a, int from) {
  const unsigned long long* src = a.jump[from];
  unsigned long long* dst = a.jump[from ^ 1];
  const uint64_t B = (uint64_t)a.cnt[0], stride = (uint64_t)gridDim.x * BD_BLOCK;
  for (uint64_t k = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x; k < B; k += stride) { // a lane beyond B leaves at once
    unsigned long long w = src[k];
    const uint64_t up = w >> 32;
    if (up != k && up < B) {
      const unsigned long long w2 = src[up];
      w = (w2 & ~BD_LOW) | ((w + w2) & BD_LOW); // steps stay below B < 2^32
    }
    dst[k] = w;
  }
}

__global__ __launch_bounds__(BD_BLOCK) void bd_flag_kernel(BoundaryArgs a) {
  const unsigned long long* fin = a.jump[a.rounds & 1];
  const uint64_t B = (uint64_t)a.cnt[0], stride = (uint64_t)gridDim.x * BD_BLOCK;
  for (uint64_t k = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x; k < B; k += stride) a.scan_n[k] = (fin[k] >> 32) == k ? 1 : 0;
}

// scan_n is summed over the compacted list, which is in ascending order of the half-edges: a head's entry is its loop's number (B4).
// The last member of a chain -- no successor, or the successor is the head: then the chain is a cycle -- writes what is one per loop.
__global__ __launch_bounds__(BD_BLOCK) void bd_number_kernel(BoundaryArgs a) {
  __shared__ uint32_t part[BD_BLOCK / 64];
  const unsigned long long* fin = a.jump[a.rounds & 1];
  const uint64_t H = 3ull * (uint64_t)a.n_tri, B = (uint64_t)a.cnt[0], stride = (uint64_t)gridDim.x * BD_BLOCK;
  const uint64_t i0 = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  long long L = a.scan_n[B];
  L = L < 0 ? 0 : (L > (long long)B ? (long long)B : L);
  uint32_t closed = 0u, longest = 0u;
  for (uint64_t k = i0; k < B; k += stride) {
    const unsigned long long w = fin[k];
    const uint64_t hk = w >> 32;
    const int32_t h = a.comp[k];
    if (hk >= B || h < 0 || (uint64_t)h >= H) continue;
    const long long l = a.scan_n[hk];
    const int32_t hh = a.comp[hk];
    if (l < 0 || l >= L) continue;
    const uint32_t p = (uint32_t)(w & BD_LOW);
    a.loop[h] = (int32_t)l;
    a.pos[h] = (int32_t)p;
    const int32_t nx = a.next[h];
    if (nx < 0 || nx == hh) {
      const bool cycle = nx >= 0;
      a.lens[l] = (long long)p + 1;
      a.lflags[l] = cycle ? 1 : 0; // B5
      if (a.area2) a.area2[3 * l] = 0, a.area2[3 * l + 1] = 0, a.area2[3 * l + 2] = 0;
      closed += cycle ? 1u : 0u;
      longest = p + 1u > longest ? p + 1u : longest;
    }
  }
  closed = orient_block_sum(closed, part);
  longest = orient_block_max(longest, part);
  if (threadIdx.x == 0) { // B8: one atomic per workgroup and figure
    if (closed) atomicAdd(&a.summary[2], (unsigned long long)closed);
    if (longest) atomicMax(&a.summary[3], (unsigned long long)longest);
  }
  if (i0 == 0) a.cnt[1] = L, a.summary[0] = (unsigned long long)B, a.summary[1] = (unsigned long long)L;
}

// B6: S2 = 2 E - 30 from the bits of A
__device__ inline int bd_scale(uint32_t abits) {
  int E = 0;
  const uint32_t ex = abits >> 23, man = abits & 0x007FFFFFu;
  if (ex) E = (int)ex - 126;                       // a normal number lies in [2^(ex - 127), 2^(ex - 126))
  else if (man) E = (32 - __clz((int)man)) - 149;  // a denormal is man * 2^-149
  return 2 * E - 30;
}
// B7: r_k.  Every operation is one fp64 instruction as written (contraction is off in every build of the library).
__device__ inline long long bd_round(double c, int S2) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(c);
  if ((u & 0x7FF0000000000000ull) == 0x7FF0000000000000ull) return 0; // not finite
  return llrint(ldexp(c, -S2));
}

// lens is summed: lens[l] is loop_offsets[l].  loop, pos, cnt and A are of earlier launches.
__global__ __launch_bounds__(BD_BLOCK) void bd_scatter_kernel(BoundaryArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, B = (uint64_t)a.cnt[0], L = (uint64_t)a.cnt[1], stride = (uint64_t)gridDim.x * BD_BLOCK;
  const uint64_t rounds = (B + stride - 1) / stride; // every lane runs the same number of rounds: the ballots are uniform
  const uint32_t lane = threadIdx.x & 63u;
  const int S2 = bd_scale((uint32_t)a.cnt[2]);
  uint64_t k = (uint64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, k += stride) {
    uint32_t key = 0xFFFFFFFFu;
    long long r0 = 0, r1 = 0, r2 = 0;
    if (k < B) {
      const int32_t h = a.comp[k];
      if (h >= 0 && (uint64_t)h < H) {
        const int32_t l = a.loop[h], p = a.pos[h];
        if (l >= 0 && (uint64_t)l < L && p >= 0) {
          const long long at = a.lens[l] + p;
          if (at >= 0 && (uint64_t)at < B) {
            a.order[at] = h;
            if (p == 0) a.loop_offsets[l] = (int32_t)at;
            if (a.area2) {
              key = (uint32_t)l;
              const uint32_t t = (uint32_t)h / 3u, e = (uint32_t)h - 3u * t;
              const float4 fa = a.tri_geom[(size_t)t * 3 + e], fb = a.tri_geom[(size_t)t * 3 + (e + 1u) % 3u];
              const double ax = fa.x, ay = fa.y, az = fa.z, bx = fb.x, by = fb.y, bz = fb.z;
              const double c0 = ay * bz - az * by, c1 = az * bx - ax * bz, c2 = ax * by - ay * bx;
              r0 = bd_round(c0, S2), r1 = bd_round(c1, S2), r2 = bd_round(c2, S2);
            }
          }
        }
      }
    }
    if (a.area2) { // uniform: one atomicAdd per run of lanes with one loop and component; integers, the order does not matter
      uint32_t start;
      bool last;
      orient_runs(key, lane, start, last);
      for (uint32_t o = 1; o < 64u; o <<= 1) {
        const long long y0 = __shfl_up(r0, o), y1 = __shfl_up(r1, o), y2 = __shfl_up(r2, o);
        if (lane >= start + o) r0 += y0, r1 += y1, r2 += y2;
      }
      if (last && key != 0xFFFFFFFFu) {
        unsigned long long* sum = (unsigned long long*)a.area2 + 3ull * key;
        if (r0) atomicAdd(sum, (unsigned long long)r0);
        if (r1) atomicAdd(sum + 1, (unsigned long long)r1);
        if (r2) atomicAdd(sum + 2, (unsigned long long)r2);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.loop_offsets[L] = (int32_t)B; // B4 (with L == 0 this is entry 0, and B is 0)
    a.summary[5] = a.area2 ? (unsigned long long)(long long)S2 : 0ull;
  }
}

// C1 .. C4: one lane per row j < 3 n_tri; nothing of the loops arrays is trusted
__global__ __launch_bounds__(BD_BLOCK) void cap_rows_kernel(const float* tri36, int32_t n_tri, const int32_t* order, const int32_t* loop,
                                                            const int32_t* pos, const int32_t* loop_offsets, const uint8_t* lflags,
                                                            const long long* summary, float* cap, uint8_t* cap_valid) {
  const long long H = 3ll * n_tri, j = (long long)blockIdx.x * BD_BLOCK + threadIdx.x;
  long long B = summary[0], L = summary[1];
  B = B < 0 ? 0 : (B > H ? H : B), L = L < 0 ? 0 : (L > H ? H : L);
  if (j >= B) return; // rows at and beyond B are not touched
  float* row = cap + (size_t)j * 36;
  bool valid = false;
  const int32_t h = order[j];
  int32_t head = -1;
  if (h >= 0 && h < H) {
    const int32_t l = loop[h], p = pos[h];
    if (l >= 0 && l < L) {
      const long long lo = loop_offsets[l], k = (long long)loop_offsets[l + 1] - lo;
      if (lo >= 0 && lo < B && (lflags[l] & 1u) && k >= 3 && p >= 1 && p <= k - 2 && lo + p == j) {
        head = order[lo];
        valid = head >= 0 && head < H;
      }
    }
  }
  if (!valid) {
#pragma unroll
    for (int i = 0; i < 36; i++) row[i] = 0.0f;
    cap_valid[j] = 0;
    return;
  }
  const uint32_t t = (uint32_t)h / 3u, e = (uint32_t)h - 3u * t;
  const float* src = tri36 + (size_t)t * 36;
  const float *v0 = tri36 + (size_t)(head / 3) * 36 + 3 * (head % 3), *v1 = src + 3u * ((e + 1u) % 3u), *v2 = src + 3u * e;
  float p9[9];
#pragma unroll
  for (int i = 0; i < 3; i++) p9[i] = v0[i], p9[3 + i] = v1[i], p9[6 + i] = v2[i]; // C2: (H, end(h), start(h)), on the bits
  float nx, ny, nz;
  ezi::tri_normal(p9, nx, ny, nz); // C3: N1 of ezrt_vertices.h
#pragma unroll
  for (int i = 0; i < 9; i++) row[i] = p9[i];
#pragma unroll
  for (int i = 0; i < 3; i++) row[9 + 3 * i] = nx, row[10 + 3 * i] = ny, row[11 + 3 * i] = nz;
#pragma unroll
  for (int i = 18; i < 36; i++) row[i] = src[i];
  cap_valid[j] = 1;
}
