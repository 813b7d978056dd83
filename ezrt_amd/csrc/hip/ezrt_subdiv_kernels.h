// ezrt_subdiv_kernels.h -- the kernels of the subdivision (include/ezrt_subdivide.h, rules S1 to S9): four rows per caller's row, by
// midpoints or by Loop's scheme.  Included by ezrt_mesh.hip, after ezrt_clip_kernels.h (it uses topo_bits of ezrt_topology_kernels.h
// and ezi::tri_normal, the N1 of ezrt_vertices.h).
//
//   subdiv_vertex_kernel   S4 .. S7, Loop mode: one lane per corner; the lane that is the FIRST corner of its vertex's star walks the
//                          star once and leaves the vertex's term and rule in `work`
//   subdiv_fill_kernel     S1 .. S3, S5 .. S9: a workgroup per tile of consecutive source rows; STAGED or per lane
//
// The vertex's slot (four words of `work` per possible vertex).  S5 and S6 are p * w + T with T a function of the STAR alone and w of
// its length: words 0-2 hold T = (beta * 0.5f) * S or 0.125f * B, word 3 the rule in bits 0-1 (SD_KEEP, SD_SMOOTH, SD_BORDER) and the
// valence k above them.  The corner's own p is multiplied in by the fill, so S7 copies the corner's bits, a corner that holds -0
// where its vertex's first corner holds +0 is still computed from its own value, and arrays that send corners with different
// positions to one vertex give each what S5 says.  Slot v is written by corner c exactly when vertex[c] == v, v's offsets are usable
// and star[star_offsets[v]] == c: at most one lane, and the fill reads slot v under the same three tests, so it never reads a word
// that nobody wrote, whatever the arrays hold (`work` is not cleared).  Where the tests fail for a usable corner -- never on arrays
// that a weld wrote -- the fill's lane walks the star itself, by the same function, to the same bits.  Only stars of vertices that a
// corner names are walked: entries of star_offsets beyond V, which the weld leaves untouched, are never looked at.
//
// The fill is a write: 144 B in, 576 B out per row.  A lane that writes its own rows at a stride of 576 B issues stores that its
// neighbours cannot merge.  The STAGED fill loads a tile's rows into LDS with the lanes laid over their float4s, computes the six
// new points of every row (and their normals) into LDS, one lane per corner and half-edge, and then lays the lanes over the tile's
// OUTPUT float4s -- lane tid holds part tid % 9 of output row 28 round + tid / 9 -- assembling each from LDS, so that a wave stores
// 1 KiB of consecutive addresses per instruction.  That route needs tri36 and out 16-byte aligned; otherwise, and in the measurement variant
// EZRT_SUBDIV_PER_LANE, the host launches the per-lane instance, in which every lane reads and writes its own row float by float.
// Both call subdiv_corner, subdiv_edge, subdiv_edge_normal and subdiv_face_normal, so they give the same bits.
//
// Bounds (S4).  The topology and weld arrays are the caller's and are NOT trusted: every index read from them is checked against
// 3 n_rows before it is used, star_offsets[v + 1] is read for v < 3 n_rows only (the array has 3 n_rows + 1 entries), and rows of
// tri36 are read at ids below n_rows only.  out is written at rows below 4 n_rows, slot at vertices below 3 n_rows.  The only loops
// that are not bounded by a constant are the walk of a star, at most 3 n_rows steps, and the staged fill's stride over its tiles.
// No floating-point atomics; the summary is reduced over the wave and the workgroup and added with one int64 atomic per workgroup
// and term; the slots cross a launch boundary.
#pragma once

constexpr int SD_BLOCK = 256;          // lanes of a workgroup; rows of a per-lane tile
constexpr int SD_TILE = 63;            // source rows of a staged tile: 2268 output float4s, nine for each of 252 lanes
constexpr int SD_LANES = 252;          // lanes that move float4s: 28 output rows of nine parts per round
constexpr int SD_REC = 72;             // floats of a row's record in LDS: the row, six points, 18 floats of normals; 63 records are 18 144 B
constexpr unsigned SD_GRID_MAX = 2048; // workgroups of the staged fill, which strides over the tiles: 8 per CU, what 18 KiB of LDS and 4 waves allow
constexpr uint32_t SD_KEEP = 0u, SD_SMOOTH = 1u, SD_BORDER = 2u;
// S1: the point (0-2 Pk, 3-5 Ee) of vertex m of piece j, four bits each at 4 (3 j + m): (P0 E0 E2) (E0 P1 E1) (E2 E1 P2) (E0 E1 E2)
constexpr unsigned long long SD_PIECES = 0x543245413530ull;
__host__ __device__ constexpr uint32_t subdiv_piece_point(uint32_t j, uint32_t m) { return (uint32_t)(SD_PIECES >> (4u * (3u * j + m))) & 7u; }

struct SubdivArgs {
  const float* tri36;
  int32_t n_rows;
  int32_t mode;
  const int32_t* twin; // the six arrays: nullptr in midpoint mode
  const uint8_t* edge_class;
  const int32_t* vertex;
  const int32_t* star_offsets;
  const int32_t* star;
  const uint8_t* vert_flags;
  float* out;
  unsigned long long* summary;
  uint32_t* slot; // work: four words per possible vertex (Loop mode)
};

// S4: the star of corner c's vertex, when the arrays are usable that far (the star's entries are checked by the walk)
__device__ inline bool subdiv_range(const SubdivArgs& a, uint32_t H, uint32_t c, int32_t& v, int32_t& lo, int32_t& hi) {
  v = a.vertex[c];
  if (v < 0 || (uint32_t)v >= H) return false;
  lo = a.star_offsets[v], hi = a.star_offsets[v + 1];
  return lo >= 0 && lo < hi && (uint32_t)hi <= H;
}
// S4 .. S7 of vertex v with the usable range lo .. hi: the walk of its star.  The rule and k, and the term T that does not depend on p.
__device__ inline uint32_t subdiv_star(const SubdivArgs& a, uint32_t H, int32_t v, int32_t lo, int32_t hi, float T[3]) {
  T[0] = T[1] = T[2] = 0.0f;
  const uint32_t fl = a.vert_flags[v];
  if (fl > 1u) return SD_KEEP; // S7: a non-manifold edge or a pinched vertex
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  uint32_t r = 0u;
  for (int32_t j = lo; j < hi; j++) { // at most 3 n_rows steps
    const int32_t o = a.star[j];
    if (o < 0 || (uint32_t)o >= H) return SD_KEEP; // S4: not usable
    const uint32_t t = (uint32_t)o / 3u, k = (uint32_t)o - 3u * t, ka = k == 2u ? 0u : k + 1u, kb = ka == 2u ? 0u : ka + 1u;
    const float* row = a.tri36 + (size_t)t * 36;
    const float *pa = row + 3u * ka, *pb = row + 3u * kb;
    if (fl == 0u) { // S5: the inner sum first
      sx = sx + (pa[0] + pb[0]), sy = sy + (pa[1] + pb[1]), sz = sz + (pa[2] + pb[2]);
    } else { // S6: the half-edge that leaves the corner is 3 t + k, the one that enters it 3 t + kb
      if (a.edge_class[o] == 1u) sx = sx + pa[0], sy = sy + pa[1], sz = sz + pa[2], r++;
      if (a.edge_class[3u * t + kb] == 1u) sx = sx + pb[0], sy = sy + pb[1], sz = sz + pb[2], r++;
    }
  }
  if (fl == 0u) {
    const uint32_t k = (uint32_t)(hi - lo);
    const float beta = k == 3u ? 0.1875f : 0.375f / (float)k, h = beta * 0.5f;
    T[0] = h * sx, T[1] = h * sy, T[2] = h * sz;
    return SD_SMOOTH | (k << 2); // k <= 3 n_rows < 2^30
  }
  if (r != 2u) return SD_KEEP;
  T[0] = 0.125f * sx, T[1] = 0.125f * sy, T[2] = 0.125f * sz;
  return SD_BORDER;
}
// S2, S4 .. S7: the new point of corner c, whose own position is p.  Returns the rule.
__device__ inline uint32_t subdiv_corner(const SubdivArgs& a, uint32_t H, uint32_t c, const float* p, float P[3]) {
  P[0] = p[0], P[1] = p[1], P[2] = p[2];
  if (a.mode != EZRT_SUBDIVIDE_LOOP) return SD_KEEP;
  int32_t v, lo, hi;
  if (!subdiv_range(a, H, c, v, lo, hi)) return SD_KEEP;
  const int32_t c0 = a.star[lo];
  uint32_t bits;
  float T[3];
  if (c0 >= 0 && (uint32_t)c0 < H && a.vertex[c0] == v) { // lane c0 of the vertex pass wrote the slot
    const uint32_t* w = a.slot + 4u * (size_t)v;
    T[0] = __uint_as_float(w[0]), T[1] = __uint_as_float(w[1]), T[2] = __uint_as_float(w[2]), bits = w[3];
  } else {
    bits = subdiv_star(a, H, v, lo, hi, T);
  }
  const uint32_t rule = bits & 3u;
  if (rule == SD_SMOOTH) {
    const uint32_t k = bits >> 2;
    const float beta = k == 3u ? 0.1875f : 0.375f / (float)k, w = 1.0f - (float)k * beta;
    P[0] = w * p[0] + T[0], P[1] = w * p[1] + T[1], P[2] = w * p[2] + T[2];
  } else if (rule == SD_BORDER) {
    P[0] = 0.75f * p[0] + T[0], P[1] = 0.75f * p[1] + T[1], P[2] = 0.75f * p[2] + T[2];
  }
  return rule;
}
__device__ inline bool subdiv_same_key(const float* x, const float* y) {
  return topo_bits(x[0]) == topo_bits(y[0]) && topo_bits(x[1]) == topo_bits(y[1]) && topo_bits(x[2]) == topo_bits(y[2]);
}
// S2, S3: the new point of half-edge e of row t, whose own floats are `own` (LDS or global).  Returns whether it is INTERIOR.
__device__ inline bool subdiv_edge(const SubdivArgs& a, uint32_t H, uint32_t t, uint32_t e, const float* own, float E[3]) {
  const uint32_t e1 = e == 2u ? 0u : e + 1u, e2 = e1 == 2u ? 0u : e1 + 1u;
  const float *pa = own + 3u * e, *pb = own + 3u * e1, *pc = own + 3u * e2;
  const float abx = pa[0] + pb[0], aby = pa[1] + pb[1], abz = pa[2] + pb[2];
  E[0] = abx * 0.5f, E[1] = aby * 0.5f, E[2] = abz * 0.5f;
  if (a.mode != EZRT_SUBDIVIDE_LOOP) return false;
  const uint32_t h = 3u * t + e, cls = a.edge_class[h];
  if (cls != 2u && cls != 3u) return false;
  const int32_t g = a.twin[h];
  if (g < 0 || (uint32_t)g >= H) return false;
  const uint32_t tg = (uint32_t)g / 3u, eg = (uint32_t)g - 3u * tg;
  if (tg == t) return false;
  const uint32_t g1 = eg == 2u ? 0u : eg + 1u, g2 = g1 == 2u ? 0u : g1 + 1u;
  const float* other = a.tri36 + (size_t)tg * 36;
  const float *qa = other + 3u * eg, *qb = other + 3u * g1, *pd = other + 3u * g2;
  const bool same = (subdiv_same_key(pa, qa) && subdiv_same_key(pb, qb)) || (subdiv_same_key(pa, qb) && subdiv_same_key(pb, qa));
  if (!same) return false;
  E[0] = 0.375f * abx + 0.125f * (pc[0] + pd[0]);
  E[1] = 0.375f * aby + 0.125f * (pc[1] + pd[1]);
  E[2] = 0.375f * abz + 0.125f * (pc[2] + pd[2]);
  return true;
}
// S2: the normal of the midpoint of half-edge e, from the row's own two corner normals
__device__ inline void subdiv_edge_normal(uint32_t e, const float* own, float N[3]) {
  const uint32_t e1 = e == 2u ? 0u : e + 1u;
  const float *na = own + 9u + 3u * e, *nb = own + 9u + 3u * e1;
  N[0] = (na[0] + nb[0]) * 0.5f, N[1] = (na[1] + nb[1]) * 0.5f, N[2] = (na[2] + nb[2]) * 0.5f;
}
// S8: N1 of piece j of a row whose six points are pts (18 floats)
__device__ inline void subdiv_face_normal(uint32_t j, const float* pts, float N[3]) {
  float q[9];
#pragma unroll
  for (uint32_t m = 0; m < 3u; m++) {
    const float* p = pts + 3u * subdiv_piece_point(j, m);
    q[3 * m] = p[0], q[3 * m + 1] = p[1], q[3 * m + 2] = p[2];
  }
  ezi::tri_normal(q, N[0], N[1], N[2]);
}
// S9: the counts of a workgroup's lanes (c[0 .. 4] are summary[1 .. 5]), reduced over the wave by shuffles and over the workgroup through
// LDS, then ONE int64 atomic per workgroup and non-zero term.  (One per wave was the first design, and 160 000 atomics on two words
// were most of the fill's time at 10^6 rows: about 9 ns each.)  Midpoint mode counts nothing: its summary is known.
__device__ inline void subdiv_add_summary(const SubdivArgs& a, uint32_t c[5]) {
  __shared__ uint32_t red[(SD_BLOCK / 64) * 5];
  if (a.mode == EZRT_SUBDIVIDE_LOOP) {
#pragma unroll
    for (int f = 0; f < 5; f++) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c[f] += __shfl_xor(c[f], o);
      if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 5 + f] = c[f];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
      unsigned long long x = 0ull;
#pragma unroll
      for (int w = 0; w < SD_BLOCK / 64; w++) x += red[w * 5 + threadIdx.x];
      if (x) atomicAdd(&a.summary[1 + threadIdx.x], x);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long n = (unsigned long long)a.n_rows;
    atomicAdd(&a.summary[0], 4ull * n);
    if (a.mode == EZRT_SUBDIVIDE_LOOP) {
      atomicAdd(&a.summary[6], (unsigned long long)a.mode);
    } else {
      atomicAdd(&a.summary[3], 3ull * n);
      atomicAdd(&a.summary[5], 3ull * n);
    }
  }
}
__device__ inline void subdiv_count(uint32_t c[5], uint32_t rule, bool interior) {
  c[0] += rule == SD_SMOOTH, c[1] += rule == SD_BORDER, c[2] += rule == SD_KEEP, c[3] += interior, c[4] += !interior;
}

// S4 .. S7, Loop mode: the slot of every vertex, written by the first corner of its star
__global__ __launch_bounds__(SD_BLOCK) void subdiv_vertex_kernel(SubdivArgs a) {
  const uint32_t H = 3u * (uint32_t)a.n_rows;
  const uint64_t c64 = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
  if (c64 >= H) return;
  const uint32_t c = (uint32_t)c64;
  int32_t v, lo, hi;
  if (!subdiv_range(a, H, c, v, lo, hi) || a.star[lo] != (int32_t)c) return;
  float T[3];
  const uint32_t bits = subdiv_star(a, H, v, lo, hi, T);
  uint32_t* w = a.slot + 4u * (size_t)v;
  w[0] = __float_as_uint(T[0]), w[1] = __float_as_uint(T[1]), w[2] = __float_as_uint(T[2]), w[3] = bits;
}

// The staged fill.  A workgroup takes tiles of SD_TILE = 63 rows, blockIdx.x, blockIdx.x + gridDim.x, ...: 63 rows are 2268 = 9 * 252
// output float4s, so with 252 lanes at work lane tid always holds part tid % 9 of output row 28 * round + tid / 9, which is always piece
// (tid / 9) % 4 of its source row: where in the row's record its four floats come from is worked out once per lane, not per float4.
// The record of a row in LDS is SD_REC = 72 floats: its 36 floats, its six points (P0 P1 P2 E0 E1 E2) and 18 floats of normals (midpoint
// mode: of the same six; Loop mode: the four pieces' face normals).
template <bool STAGED>
__global__ __launch_bounds__(SD_BLOCK) void subdiv_fill_kernel(SubdivArgs a) {
  const uint32_t H = 3u * (uint32_t)a.n_rows;
  const bool loop = a.mode == EZRT_SUBDIVIDE_LOOP;
  uint32_t cnt[5] = {0u, 0u, 0u, 0u, 0u};
  if constexpr (STAGED) {
    __shared__ float4 rec4[SD_TILE * SD_REC / 4];
    float* rec = (float*)rec4;
    const uint32_t tid = threadIdx.x, q = tid / 9u, part = tid - 9u * q, j = q & 3u;
    uint32_t off[4]; // of this lane's four floats within a record
#pragma unroll
    for (uint32_t u = 0; u < 4u; u++) {
      const uint32_t i = 4u * part + u, i9 = i < 9u ? i : i - 9u, m = i9 < 9u ? i9 / 3u : 0u, cmp = i9 - 3u * (i9 / 3u), pt = subdiv_piece_point(j, m);
      off[u] = i >= 18u ? i : (i < 9u ? 36u + 3u * pt + cmp : 54u + 3u * (loop ? j : pt) + cmp);
    }
    const uint64_t tiles = ((uint64_t)a.n_rows + SD_TILE - 1) / SD_TILE;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // at most `tiles` rounds
      const uint64_t base = tile * SD_TILE;
      const uint32_t rows = (uint32_t)(((uint64_t)a.n_rows - base) < (uint64_t)SD_TILE ? (uint64_t)a.n_rows - base : (uint64_t)SD_TILE);
      const float4* in4 = (const float4*)a.tri36 + base * 9; // 16-byte aligned: the host chose this instance
      if (tid < SD_LANES) {
#pragma unroll
        for (uint32_t round = 0; round < 3u; round++) {
          const uint32_t r = 28u * round + q;
          if (r < rows) rec4[r * (SD_REC / 4) + part] = in4[r * 9u + part];
        }
      }
      __syncthreads();
      if (tid < rows * 3u) { // one lane per corner and half-edge
        const uint32_t r = tid / 3u, e = tid - 3u * r, t = (uint32_t)base + r;
        float* own = rec + r * SD_REC;
        float P[3], E[3];
        const uint32_t rule = subdiv_corner(a, H, 3u * t + e, own + 3u * e, P);
        const bool interior = subdiv_edge(a, H, t, e, own, E);
        subdiv_count(cnt, rule, interior);
        float* o = own + 36u + 3u * e;
        o[0] = P[0], o[1] = P[1], o[2] = P[2], o[9] = E[0], o[10] = E[1], o[11] = E[2];
        if (!loop) {
          float N[3];
          subdiv_edge_normal(e, own, N);
          float* n = own + 54u + 3u * e;
          n[0] = own[9u + 3u * e], n[1] = own[10u + 3u * e], n[2] = own[11u + 3u * e], n[9] = N[0], n[10] = N[1], n[11] = N[2];
        }
      }
      __syncthreads();
      if (loop) { // (the same for every lane of the launch)
        if (tid < rows * 4u) { // one lane per piece
          float* own = rec + (tid >> 2) * SD_REC;
          float N[3];
          subdiv_face_normal(tid & 3u, own + 36u, N);
          float* n = own + 54u + 3u * (tid & 3u);
          n[0] = N[0], n[1] = N[1], n[2] = N[2];
        }
        __syncthreads();
      }
      float4* out4 = (float4*)a.out + base * 36;
      if (tid < SD_LANES) {
#pragma unroll
        for (uint32_t round = 0; round < 9u; round++) {
          const uint32_t r = 7u * round + (q >> 2); // output row 28 round + q of the tile
          if (r < rows) {
            const float* b = rec + r * SD_REC;
            out4[(28u * round + q) * 9u + part] = make_float4(b[off[0]], b[off[1]], b[off[2]], b[off[3]]);
          }
        }
      }
      __syncthreads(); // the records are the next tile's
    }
  } else {
    const uint64_t t64 = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
    if (t64 < (uint64_t)a.n_rows) {
      const uint32_t t = (uint32_t)t64;
      const float* own = a.tri36 + (size_t)t * 36;
      float pts[18], nrm[18];
#pragma unroll
      for (uint32_t e = 0; e < 3u; e++) {
        const uint32_t rule = subdiv_corner(a, H, 3u * t + e, own + 3u * e, pts + 3u * e);
        const bool interior = subdiv_edge(a, H, t, e, own, pts + 9u + 3u * e);
        subdiv_count(cnt, rule, interior);
        if (!loop) {
          nrm[3 * e] = own[9u + 3u * e], nrm[3 * e + 1] = own[10u + 3u * e], nrm[3 * e + 2] = own[11u + 3u * e];
          subdiv_edge_normal(e, own, nrm + 9u + 3u * e);
        }
      }
      if (loop) {
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) subdiv_face_normal(j, pts, nrm + 3u * j);
      }
      float* o = a.out + (size_t)t * 144;
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) {
#pragma unroll
        for (uint32_t m = 0; m < 3u; m++) {
          const uint32_t pt = subdiv_piece_point(j, m);
#pragma unroll
          for (uint32_t cmp = 0; cmp < 3u; cmp++) {
            o[36u * j + 3u * m + cmp] = pts[3u * pt + cmp];
            o[36u * j + 9u + 3u * m + cmp] = loop ? nrm[3u * j + cmp] : nrm[3u * pt + cmp];
          }
        }
#pragma unroll
        for (uint32_t i = 18; i < 36u; i++) o[36u * j + i] = own[i]; // S1: the source row's material on the bits
      }
    }
  }
  subdiv_add_summary(a, cnt);
}
