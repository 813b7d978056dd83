// ezrt_clip_kernels.h -- the kernels of the plane clipping (include/ezrt_clip.h, rules K1 to K8): the rows of the caller's mesh on the
// side a x + b y + c z >= d of a plane.  Included by ezrt_mesh.hip, after ezrt_boundary_kernels.h (it uses plane_load, plane_side and
// plane_point of ezrt_device.h; the prefix sum between the two kernels is scan_tiled of ezrt_scan_kernels.h,
// launched by the host).
//
//   clip_count_kernel    K2, K3, K7: one lane per row; the row's count into offsets[k], the terms of the summary reduced over the wave
//   clip_fill_kernel     K3 .. K6, K8: a workgroup per tile of CL_BLOCK consecutive rows; STAGED or per lane
//
// The fill is a copy: in a typical cut almost every row is kept whole or dropped.  A lane that moves its own row of 144 B at a stride
// of 144 B issues accesses that its neighbours cannot merge.  The STAGED fill therefore classifies the tile one lane per row, puts the
// destination of every row that is kept whole into LDS, and moves those rows with the lanes laid over the tile's float4s: entry f
// belongs to row f / 9, part f % 9, so a wave loads 1 KiB of consecutive addresses per instruction and stores consecutive addresses
// wherever kept rows follow one another (their destinations do: K6).  The cut rows, which are few, are written afterwards by their own
// lanes.  That route needs tri36 and out 16-byte aligned (a row is nine float4s, so then every row is); otherwise, and in the
// measurement variant EZRT_CLIP_PER_LANE, the host launches the per-lane instance, in which every lane copies its own row float by
// float.  Both copy bits and share clip_classify and clip_cut, so they give the same bits.
//
// Bounds (K8).  offsets is the caller's and is NOT trusted: a row is written only when 0 <= offsets[k], offsets[k] + c <= capacity and
// offsets[k + 1] - offsets[k] == c with c recomputed here, so every row index written is below capacity and a row is written whole
// or not at all.  tri36 is read at rows below n_rows only.  There is no loop but the copy's nine rounds.
#pragma once

constexpr int CL_BLOCK = 256; // lanes of a workgroup, and rows of a fill tile: 36 KiB of rows, nine float4s per lane

// what a row emits (K3), packed: bits 0-1 the count; bits 2-3 the kind; bits 4-5 the index i of U or D; bit 6 piece (a, b, Pb) is
// emitted, bit 7 piece (a, Pb, Pa) is (kind ONE_DOWN only); bit 8 the row has a non-finite coordinate
constexpr uint32_t CL_NONE = 0u, CL_WHOLE = 1u, CL_ONE_UP = 2u, CL_ONE_DOWN = 3u;
__device__ inline uint32_t clip_count_of(uint32_t w) { return w & 3u; }
__device__ inline uint32_t clip_kind_of(uint32_t w) { return (w >> 2) & 3u; }

// K2, K3 from the row's nine coordinates: v and s are left for clip_cut.  The count depends on the three sides alone.
__device__ inline uint32_t clip_classify(const float* __restrict__ row, const PlaneEq& pl, double v[9], double s[3]) {
  const float inf = __builtin_inff();
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const float x = row[i];
    fin = fin && ez_abs(x) < inf;
    v[i] = (double)x;
  }
#pragma unroll
  for (int i = 0; i < 3; i++) s[i] = plane_side(pl, v[3 * i], v[3 * i + 1], v[3 * i + 2]);
  if (!fin) return 1u << 8;
  if (!pl.live) return 0u;
  const bool u0 = s[0] >= 0.0, u1 = s[1] >= 0.0, u2 = s[2] >= 0.0;
  const int up = (int)u0 + (int)u1 + (int)u2;
  if (up == 3) return (CL_WHOLE << 2) | 1u;
  if (up == 0) return 0u;
  if (up == 1) {
    const uint32_t i = u0 ? 0u : (u1 ? 1u : 2u);
    const double su = u0 ? s[0] : (u1 ? s[1] : s[2]);
    return su != 0.0 ? ((i << 4) | (CL_ONE_UP << 2) | 1u) : 0u; // a row that only touches the plane emits nothing
  }
  const uint32_t i = !u0 ? 0u : (!u1 ? 1u : 2u);
  const double sa = !u0 ? s[1] : (!u1 ? s[2] : s[0]), sb = !u0 ? s[2] : (!u1 ? s[0] : s[1]);
  const uint32_t first = sb != 0.0 ? 1u : 0u, second = sa != 0.0 ? 1u : 0u;
  if (first + second == 0u) return 0u;
  return (second << 7) | (first << 6) | (i << 4) | (CL_ONE_DOWN << 2) | (first + second);
}
// K6: the output rows of a row that have a cut edge
__device__ inline uint32_t clip_cut_edges(uint32_t w, const double s[3]) {
  const uint32_t kind = clip_kind_of(w);
  if (kind == CL_ONE_UP) return 1u;
  if (kind != CL_ONE_DOWN) return 0u;
  const uint32_t i = (w >> 4) & 3u;
  const double sa = i == 0u ? s[1] : (i == 1u ? s[2] : s[0]);
  return ((w >> 7) & 1u) + (((w >> 6) & 1u) && sa == 0.0 ? 1u : 0u);
}

// K4, K5: the new vertex of the edge with the ends X and Y (positions, normals, sides; one UP, one DOWN), whichever way round they are
// given.  The position is plane_point's; A < B, sa, sb and t are recomputed as plane_point computes them.
__device__ inline void clip_vertex(const float X[3], const float nX[3], double sx, const float Y[3], const float nY[3], double sy, float P[3],
                                   float nP[3]) {
  const double Xx = (double)X[0], Xy = (double)X[1], Xz = (double)X[2], Yx = (double)Y[0], Yy = (double)Y[1], Yz = (double)Y[2];
  const f3 p = plane_point(Xx, Xy, Xz, sx, Yx, Yy, Yz, sy);
  P[0] = p.x, P[1] = p.y, P[2] = p.z;
  const bool sw = Yx < Xx || (Yx == Xx && (Yy < Xy || (Yy == Xy && Yz < Xz))); // less(Y, X)
  const double sa = sw ? sy : sx, sb = sw ? sx : sy;
  const double t = sa / (sa - sb);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float a = sw ? nY[c] : nX[c], b = sw ? nX[c] : nY[c];
    const float l = (float)((double)a + t * ((double)b - (double)a));
    nP[c] = sa == 0.0 ? a : (sb == 0.0 ? b : l);
  }
}

struct ClipFillArgs {
  const float* tri36;
  int32_t n_rows;
  const float* plane4;
  const long long* offsets;
  long long capacity;
  float* out;
  int32_t* src;     // or nullptr
  int8_t* cut_edge; // or nullptr
};

__device__ inline void clip_put(const ClipFillArgs& a, long long r, int32_t k, const float* V0, const float* N0, const float* V1, const float* N1,
                                const float* V2, const float* N2, int ce) {
  float* o = a.out + (size_t)r * 36;
  const float* m = a.tri36 + (size_t)k * 36 + 18;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    o[c] = V0[c], o[3 + c] = V1[c], o[6 + c] = V2[c];
    o[9 + c] = N0[c], o[12 + c] = N1[c], o[15 + c] = N2[c];
  }
#pragma unroll
  for (int c = 0; c < 18; c++) o[18 + c] = m[c]; // K5: the source row's material on the bits
  if (a.src) a.src[r] = k;
  if (a.cut_edge) a.cut_edge[r] = (int8_t)ce;
}
// K3 .. K6 of a row of kind ONE_UP or ONE_DOWN, into output rows r, r + 1.  The row is turned so that U or D is vertex 0 (under selects
// of scalars: nothing is indexed); both kinds then need the same two points, E01 of edge 0 -> 1 and E20 of edge 2 -> 0.
__device__ inline void clip_cut(const ClipFillArgs& a, uint32_t w, int32_t k, const double s[3], long long r) {
  const float* row = a.tri36 + (size_t)k * 36;
  const uint32_t i = (w >> 4) & 3u;
  float V[9], N[9];
  double sr[3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const int m1 = (m + 1) % 3, m2 = (m + 2) % 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float p0 = row[3 * m + c], p1 = row[3 * m1 + c], p2 = row[3 * m2 + c];
      const float n0 = row[9 + 3 * m + c], n1 = row[9 + 3 * m1 + c], n2 = row[9 + 3 * m2 + c];
      V[3 * m + c] = i == 0u ? p0 : (i == 1u ? p1 : p2);
      N[3 * m + c] = i == 0u ? n0 : (i == 1u ? n1 : n2);
    }
    sr[m] = i == 0u ? s[m] : (i == 1u ? s[m1] : s[m2]);
  }
  float E01[3], N01[3], E20[3], N20[3];
  clip_vertex(V, N, sr[0], V + 3, N + 3, sr[1], E01, N01);
  clip_vertex(V + 6, N + 6, sr[2], V, N, sr[0], E20, N20);
  if (clip_kind_of(w) == CL_ONE_UP) {
    clip_put(a, r, k, V, N, E01, N01, E20, N20, 1); // (U, q0, q1)
    return;
  }
  if ((w >> 6) & 1u) { // (a, b, Pb)
    clip_put(a, r, k, V + 3, N + 3, V + 6, N + 6, E20, N20, sr[1] == 0.0 ? 2 : -1);
    r++;
  }
  if ((w >> 7) & 1u) clip_put(a, r, k, V + 3, N + 3, E20, N20, E01, N01, 1); // (a, Pb, Pa)
}

// K2, K3, K7.  The six terms of the summary are at most 128 per wave each: they travel as 10-bit fields of one word.
__global__ __launch_bounds__(CL_BLOCK) void clip_count_kernel(const float* tri36, int32_t n_rows, const float* plane4, long long* offsets,
                                                              unsigned long long* summary) {
  PlaneEq pl;
  plane_load(plane4, pl);
  const uint64_t k = (uint64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  unsigned long long term = 0ull;
  if (k < (uint64_t)n_rows) {
    double v[9], s[3];
    const uint32_t w = clip_classify(tri36 + (size_t)k * 36, pl, v, s);
    const uint32_t c = clip_count_of(w), kind = clip_kind_of(w);
    offsets[k] = (long long)c;
    const int field = (w >> 8) & 1u ? 4 : (kind == CL_WHOLE ? 1 : (c ? 2 : 3));
    term = (unsigned long long)c | (1ull << (10 * field)) | ((unsigned long long)clip_cut_edges(w, s) << 50);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
  if ((threadIdx.x & 63) == 0) { // one int64 atomic per wave and term
#pragma unroll
    for (int f = 0; f < 6; f++) {
      const unsigned long long x = (term >> (10 * f)) & 1023ull;
      if (x) atomicAdd(&summary[f], x);
    }
  }
  if (k == 0 && pl.live) atomicAdd(&summary[6], 1ull);
}

template <bool STAGED>
__global__ __launch_bounds__(CL_BLOCK) void clip_fill_kernel(ClipFillArgs a) {
  __shared__ long long whole_at[STAGED ? CL_BLOCK : 1]; // the destination of a row that is kept whole, or -1
  PlaneEq pl;
  plane_load(a.plane4, pl);
  const uint64_t base = (uint64_t)blockIdx.x * CL_BLOCK, k = base + threadIdx.x;
  double v[9], s[3];
  uint32_t w = 0u;
  long long at = -1;
  if (k < (uint64_t)a.n_rows) {
    w = clip_classify(a.tri36 + (size_t)k * 36, pl, v, s);
    const long long c = (long long)clip_count_of(w), o = a.offsets[k], o1 = a.offsets[k + 1];
    if (c > 0 && o >= 0 && o <= a.capacity - c && o1 >= o && o1 - o == c) at = o; // K8
  }
  const bool whole = at >= 0 && clip_kind_of(w) == CL_WHOLE;
  if (whole) {
    if (a.src) a.src[at] = (int32_t)k;
    if (a.cut_edge) a.cut_edge[at] = (int8_t)-1;
  }
  if (STAGED) {
    whole_at[threadIdx.x] = whole ? at : -1;
    __syncthreads();
    const float4* in4 = (const float4*)a.tri36 + base * 9; // 16-byte aligned: the host chose this instance
    float4* out4 = (float4*)a.out;
#pragma unroll
    for (int j = 0; j < 9; j++) {
      const uint32_t f = (uint32_t)j * CL_BLOCK + threadIdx.x, r = f / 9u, part = f - 9u * r;
      const long long d = whole_at[r]; // -1 for every row at and beyond n_rows: nothing is read there
      if (d >= 0) out4[(size_t)d * 9 + part] = in4[f];
    }
  } else if (whole) {
    const float* in = a.tri36 + (size_t)k * 36;
    float* o = a.out + (size_t)at * 36;
#pragma unroll
    for (int c = 0; c < 36; c++) o[c] = in[c];
  }
  if (at >= 0 && !whole) clip_cut(a, w, (int32_t)k, s, at);
}
