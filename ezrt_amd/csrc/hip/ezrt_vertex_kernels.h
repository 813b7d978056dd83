// ezrt_vertex_kernels.h -- the kernels of the vertex weld and the smooth normals (include/ezrt_vertices.h, rules W1 to W7 and N1 to
// N4): the indexed mesh of the scene's triangles, the star of every vertex, its fans and flags, and the reference's smooth normals
// over the stars.  Included by ezrt_mesh.hip, after ezrt_scan_kernels.h and ezrt_topology_kernels.h (it uses the topology's keys and
// union-find, and loops_hash; its two prefix sums are scan_tiled, launched by the host).
//
//   weld_init_kernel     the table, the counters, the union-find, the accumulators and the summary, whatever `work` held
//   weld_join_kernel     W1, W2: one lane per corner; claims or finds the slot of its key; atomicMin leaves the key's lowest corner
//   weld_flag_kernel     W2: one lane per corner; 1 where the corner is the lowest of its key (scan_tiled numbers them); L
//   weld_id_kernel       W2, W3: one lane per corner; vertex, vert_corner, and the valence counted into cnt (scan_tiled sums)
//   weld_scatter_kernel  W3: one lane per corner; its star's entries in arrival order into tmp; star_offsets; the largest valence
//   weld_rank_kernel     W3: one lane per corner; its rank among its star's corners: star comes out ascending whatever the order
//   weld_link_kernel     W4, W5, W6: one lane per corner; walks its star: m of its two edges, and unites itself with lower corners
//   weld_fans_kernel     W5: one lane per corner; a root of the union-find counts a fan of its vertex
//   weld_finish_kernel   W6, W7: one lane per vertex; fans, vert_flags, the three counts
//   weld_at_kernel       the rule for pairs already held: one lane per pair, no table
//   vn_face_kernel       N1: one lane per triangle of the caller's rows; its face normal into `work`
//   vn_corner_kernel     N2, N3, N4: one lane per corner; the sum over its star in ascending order, normalised, into floats 9-17
//
// The discipline is that of ezrt_topology_kernels.h.  INSIDE a launch, a word that one workgroup writes and another reads is touched
// by agent-scope atomics ONLY: rep (atomicCAS, atomicMin) in the join; cnt and cur (atomicAdd); parent (relaxed agent-scope atomic
// load, atomicCAS, atomicMin) in the link; flagw (atomicOr), fanc (atomicAdd) and the summary (atomicAdd, atomicMax), which nobody
// reads in the launch that adds to them.  EVERYTHING ELSE crosses a launch boundary on one stream: slot, ids, tmp, and the outputs
// vertex, star_offsets and star, which later launches of the same call read back with plain loads.  vertex[c] doubles as the
// liveness of corner c between the launches (the join stores -1 or 0, the id launch the number).  tri_geom is written by nobody while
// a query runs.  No floating-point atomics: a vertex's sum is one lane's loop over the star, in the star's order.
//
// Bounds.  Every probe loop runs at most T times (T >= 6 n_tri slots for at most 3 n_tri keys), every walk of a star at most
// 3 n_tri steps (its offsets are clamped to 0 .. 3 n_tri), every find at most 3 n_tri steps along a strictly descending parent, every
// unite at most 3 n_tri retries; every index read back from `work`, or from the caller's weld arrays in the normals, is checked
// against its array before it is used.
//
// Cost.  A vertex of valence k costs k lanes k steps each in the rank and again in the link: O(k^2) for the vertex, but spread over
// the k lanes of its own corners -- a large star is already split across waves, and all of its lanes read the same entries.  What
// stays serial is contention: k atomicAdds on one counter, and the unions of one star on one chain of parents.
#pragma once

constexpr int WD_BLOCK = 256;

struct WeldArgs {
  const float4* tri_geom;
  int32_t n_tri;
  uint64_t T;        // slots, a power of two, at most 2^32
  // work
  long long* ids;    // 3 n_tri + 1: 1 at the lowest corner of a key, then its exclusive prefix sum; [3 n_tri] = V
  long long* cnt;    // 3 n_tri + 1: the valence of vertex v, then its exclusive prefix sum; [V] = L
  long long* tiles;  // ceil(3 n_tri / SCAN_TILE) + 1: the sums of a scan's tiles, then their exclusive prefix sum
  int32_t* rep;      // T: a corner of the slot's key, in the end the lowest; -1 empty
  uint32_t* slot;    // 3 n_tri
  int32_t* cur;      // 3 n_tri: the entries of star v scattered so far
  int32_t* tmp;      // 3 n_tri: the stars in arrival order
  int32_t* parent;   // 3 n_tri: the union-find over corners, parent[c] <= c
  uint32_t* flagw;   // 3 n_tri: bits 0 and 1 of vertex v
  int32_t* fanc;     // 3 n_tri: the fans of vertex v
  // outputs
  int32_t *vertex, *vert_corner, *star_offsets, *star, *fans;
  uint8_t* vert_flags;
  unsigned long long* summary;
};

// W1: the key of corner c (stored vertex c % 3 of triangle c / 3); the caller has checked c
__device__ inline TopoKey weld_key(const float4* __restrict__ tri_geom, int32_t c) {
  const float4 p = tri_geom[c];
  TopoKey k;
  k.x = topo_bits(p.x), k.y = topo_bits(p.y), k.z = topo_bits(p.z);
  return k;
}
// the largest x of a wave (every lane of the wave calls it)
__device__ inline uint32_t weld_wave_max(uint32_t x) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, o);
    x = y > x ? y : x;
  }
  return x;
}
// the star of vertex v as a range of positions clamped to 0 <= lo <= hi <= H; false when v is no vertex
__device__ inline bool weld_range(const long long* cnt, int32_t v, uint64_t H, uint64_t& lo, uint64_t& hi) {
  lo = hi = 0;
  if (v < 0 || (uint64_t)v >= H) return false;
  const long long a = cnt[v], b = cnt[v + 1];
  if (a < 0 || b < a || (uint64_t)b > H) return false;
  lo = (uint64_t)a, hi = (uint64_t)b;
  return true;
}
// the numbers of the two other vertices of corner c's triangle: a the next stored vertex, b the one after
__device__ inline void weld_others(const int32_t* vertex, int32_t c, int32_t& va, int32_t& vb) {
  const int32_t t3 = c / 3 * 3, k = c - t3;
  va = vertex[t3 + (k == 2 ? 0 : k + 1)];
  vb = vertex[t3 + (k == 0 ? 2 : k - 1)];
}

__global__ __launch_bounds__(WD_BLOCK) void weld_init_kernel(WeldArgs a, bool flags) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK, i0 = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x;
  for (uint64_t i = i0; i < a.T; i += stride) a.rep[i] = -1;
  for (uint64_t i = i0; i <= H; i += stride) a.cnt[i] = 0;
  for (uint64_t i = i0; i < H; i += stride) a.cur[i] = 0;
  if (flags)
    for (uint64_t i = i0; i < H; i += stride) a.parent[i] = (int32_t)i, a.flagw[i] = 0u, a.fanc[i] = 0;
  if (i0 < 8) a.summary[i0] = 0ull;
}

// W1, W2, the join.  rep[p] is claimed by atomicCAS and afterwards only ever replaced, by atomicMin, with another corner of the SAME
// key: whoever reads it, at any time, reads a corner that carries the slot's key.
__global__ __launch_bounds__(WD_BLOCK) void weld_join_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  const uint32_t mask = (uint32_t)(a.T - 1);
  for (uint64_t c = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x; c < H; c += stride) {
    const int32_t t = (int32_t)(c / 3);
    TopoKey k[3];
    uint32_t my_slot = 0u;
    bool found = false;
    if (topo_tri(a.tri_geom, t, k)) {
      const TopoKey me = topo_vertex(k, (int)(c - 3ull * (uint64_t)t));
      uint32_t p = loops_hash(me.x, me.y, me.z) & mask;
      for (uint64_t probe = 0; probe < a.T && !found; probe++) {
        const int32_t old = atomicCAS(&a.rep[p], -1, (int32_t)c);
        if (old == -1) found = true;
        else if (old >= 0 && (uint64_t)old < H) found = topo_eq(weld_key(a.tri_geom, old), me);
        if (!found) p = (p + 1u) & mask;
      }
      if (found) {
        atomicMin(&a.rep[p], (int32_t)c);
        my_slot = p;
      }
    }
    // one exit: a corner that takes no part (W1) -- or that found no slot, which cannot happen in a table at most half full -- is -1
    a.slot[c] = my_slot;
    a.vertex[c] = found ? 0 : -1;
  }
}

// every word read from here on was written by an earlier launch
__global__ __launch_bounds__(WD_BLOCK) void weld_flag_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  const uint64_t rounds = (H + stride - 1) / stride; // every lane of a wave runs the same number of rounds: the ballot is uniform
  uint64_t c = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, c += stride) {
    bool live = false;
    if (c < H) {
      live = a.vertex[c] >= 0;
      const uint32_t s = a.slot[c];
      a.ids[c] = live && (uint64_t)s < a.T && a.rep[s] == (int32_t)c ? 1 : 0;
    }
    const unsigned long long b = __ballot(live);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&a.summary[0], (unsigned long long)__popcll(b));
  }
}

// (the prefix sums of W2 and W3 run between these launches: scan_tiled of ezrt_scan_kernels.h, over many workgroups -- one workgroup
// took 5.3 of the weld's 6.2 ms per 10^6 corners)
__global__ __launch_bounds__(WD_BLOCK) void weld_id_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  for (uint64_t c = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x; c < H; c += stride) {
    if (a.vertex[c] < 0) continue;
    const uint32_t s = a.slot[c];
    const int32_t r = (uint64_t)s < a.T ? a.rep[s] : -1;
    const long long v = r >= 0 && (uint64_t)r < H ? a.ids[r] : -1;
    const bool ok = v >= 0 && (uint64_t)v < H;
    a.vertex[c] = ok ? (int32_t)v : -1;
    if (!ok) continue;
    if ((uint64_t)r == c) a.vert_corner[v] = (int32_t)c;
    atomicAdd((unsigned long long*)&a.cnt[v], 1ull);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.summary[1] = (unsigned long long)a.ids[H];
}

__global__ __launch_bounds__(WD_BLOCK) void weld_scatter_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  const uint64_t rounds = (H + 1 + stride - 1) / stride;
  const long long V = a.ids[H];
  uint64_t i = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride) {
    uint32_t valence = 0;
    if (i < H) {
      const int32_t v = a.vertex[i];
      uint64_t lo, hi;
      if (weld_range(a.cnt, v, H, lo, hi)) {
        const int32_t k = atomicAdd(&a.cur[v], 1);
        if (k >= 0 && lo + (uint64_t)k < hi) a.tmp[lo + (uint64_t)k] = (int32_t)i;
      }
    }
    if (V >= 0 && (uint64_t)V <= H && i <= (uint64_t)V) {
      uint64_t lo, hi;
      const bool ok = weld_range(a.cnt, (int32_t)i, H, lo, hi); // false at i == V == H: there is no entry behind cnt[H]
      a.star_offsets[i] = (int32_t)(i < (uint64_t)V ? (ok ? lo : 0) : a.cnt[V]);
      if (ok && i < (uint64_t)V) valence = (uint32_t)(hi - lo);
    }
    valence = weld_wave_max(valence);
    if ((threadIdx.x & 63) == 0 && valence) atomicMax(&a.summary[2], (unsigned long long)valence);
  }
}

// W3: the rank of a corner among the corners of its star is its position, so star is ascending whatever order tmp came in
__global__ __launch_bounds__(WD_BLOCK) void weld_rank_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  for (uint64_t c = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x; c < H; c += stride) {
    uint64_t lo, hi;
    if (!weld_range(a.cnt, a.vertex[c], H, lo, hi)) continue;
    uint64_t rank = 0;
    for (uint64_t j = lo; j < hi; j++) rank += a.tmp[j] < (int32_t)c ? 1u : 0u; // at most 3 n_tri steps
    if (lo + rank < hi) a.star[lo + rank] = (int32_t)c;
  }
}

// W4, W5, W6.  Corner c of vertex v holds the edges {v, va} and {v, vb}; m of each is counted over the star, and c is united with
// every LOWER corner of the star that shares one of them (the higher root is hooked under the lower: topo_unite_kernel's rule).
__global__ __launch_bounds__(WD_BLOCK) void weld_link_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  for (uint64_t c = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x; c < H; c += stride) {
    const int32_t v = a.vertex[c];
    uint64_t lo, hi;
    if (!weld_range(a.cnt, v, H, lo, hi)) continue;
    int32_t va, vb;
    weld_others(a.vertex, (int32_t)c, va, vb);
    uint32_t ma = 0, mb = 0;
    for (uint64_t j = lo; j < hi; j++) { // at most 3 n_tri steps
      const int32_t o = a.star[j];
      if (o < 0 || (uint64_t)o >= H) continue;
      int32_t oa, ob;
      weld_others(a.vertex, o, oa, ob);
      const bool sa = oa == va || ob == va, sb = oa == vb || ob == vb;
      ma += sa ? 1u : 0u, mb += sb ? 1u : 0u;
      if ((sa || sb) && (uint64_t)o < c) {
        int32_t x = (int32_t)c, y = o;
        for (uint64_t tries = 0; tries <= H; tries++) { // a failed hook means the root was hooked lower meanwhile: finitely often
          x = topo_find(a.parent, x), y = topo_find(a.parent, y);
          if (x == y) break;
          const int32_t up = x > y ? x : y, dn = x > y ? y : x;
          if (atomicCAS(&a.parent[up], up, dn) == up) break;
        }
      }
    }
    const uint32_t f = (ma == 1 || mb == 1 ? 1u : 0u) | (ma >= 3 || mb >= 3 ? 2u : 0u);
    if (f) atomicOr(&a.flagw[v], f);
  }
}
// parent is final (the link is an earlier launch), and plain loads read it
__global__ __launch_bounds__(WD_BLOCK) void weld_fans_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  for (uint64_t c = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x; c < H; c += stride) {
    const int32_t v = a.vertex[c];
    if (v >= 0 && (uint64_t)v < H && a.parent[c] == (int32_t)c) atomicAdd(&a.fanc[v], 1);
  }
}
__global__ __launch_bounds__(WD_BLOCK) void weld_finish_kernel(WeldArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * WD_BLOCK;
  const long long Vs = a.ids[H];
  const uint64_t V = Vs < 0 ? 0 : ((uint64_t)Vs > H ? H : (uint64_t)Vs), rounds = (V + stride - 1) / stride;
  uint64_t v = (uint64_t)blockIdx.x * WD_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, v += stride) {
    uint32_t f = 0;
    if (v < V) {
      const int32_t n = a.fanc[v];
      f = (a.flagw[v] & 3u) | (n > 1 ? 4u : 0u);
      a.fans[v] = n;
      a.vert_flags[v] = (uint8_t)f;
    }
    const unsigned long long b0 = __ballot((f & 1u) != 0), b1 = __ballot((f & 2u) != 0), b2 = __ballot((f & 4u) != 0);
    if ((threadIdx.x & 63) == 0) {
      if (b0) atomicAdd(&a.summary[3], (unsigned long long)__popcll(b0));
      if (b1) atomicAdd(&a.summary[4], (unsigned long long)__popcll(b1));
      if (b2) atomicAdd(&a.summary[5], (unsigned long long)__popcll(b2));
    }
  }
}

// the rule for pairs already held: are two corners the same vertex?
__global__ __launch_bounds__(WD_BLOCK) void weld_at_kernel(const float4* tri_geom, int32_t n_tri, const int32_t* corner_a, const int32_t* corner_b,
                                                           uint32_t n, int8_t* same) {
  const uint32_t i = blockIdx.x * WD_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t ca = corner_a[i], cb = corner_b[i];
  const int64_t H = 3ll * n_tri;
  int8_t r = -1;
  TopoKey ka[3], kb[3];
  if (ca >= 0 && ca < H && cb >= 0 && cb < H && topo_tri(tri_geom, ca / 3, ka) && topo_tri(tri_geom, cb / 3, kb))
    r = topo_eq(topo_vertex(ka, ca % 3), topo_vertex(kb, cb % 3)) ? 1 : 0;
  same[i] = r;
}

// ---- the smooth normals: positions from the CALLER's rows, the weld from the caller's arrays, none of them trusted
struct VertexNormalArgs {
  float* tri36;
  int32_t n_tri;
  const int32_t *vertex, *star_offsets, *star;
  float* face; // work: 3 n_tri, the face normals
};
// N1
__global__ __launch_bounds__(WD_BLOCK) void vn_face_kernel(VertexNormalArgs a) {
  const uint32_t t = blockIdx.x * WD_BLOCK + threadIdx.x;
  if (t >= (uint32_t)a.n_tri) return;
  const float* row = a.tri36 + (size_t)t * 36;
  float p[9];
#pragma unroll
  for (int i = 0; i < 9; i++) p[i] = row[i];
  float nx, ny, nz;
  ezi::tri_normal(p, nx, ny, nz);
  float* f = a.face + (size_t)t * 3;
  f[0] = nx, f[1] = ny, f[2] = nz;
}
// N2, N3, N4: the face normals were written by the launch before
__global__ __launch_bounds__(WD_BLOCK) void vn_corner_kernel(VertexNormalArgs a) {
  const uint32_t H = 3u * (uint32_t)a.n_tri, c = blockIdx.x * WD_BLOCK + threadIdx.x;
  if (c >= H) return;
  const uint32_t t = c / 3, k = c - 3 * t;
  const int32_t v = a.vertex[c];
  bool usable = v >= 0 && (uint32_t)v < H;
  f3 s = mk(0.0f, 0.0f, 0.0f);
  if (usable) {
    const int32_t lo = a.star_offsets[v], hi = a.star_offsets[v + 1];
    usable = lo >= 0 && lo <= hi && (uint32_t)hi <= H;
    if (usable)
      for (int32_t j = lo; j < hi; j++) { // at most 3 n_tri steps
        const int32_t o = a.star[j];
        if (o < 0 || (uint32_t)o >= H) {
          usable = false;
          break;
        }
        const float* f = a.face + (size_t)(o / 3) * 3;
        s = s + mk(f[0], f[1], f[2]);
      }
  }
  f3 n;
  if (usable) {
    n = normalize(s);
  } else {
    const float* f = a.face + (size_t)t * 3;
    n = mk(f[0], f[1], f[2]);
  }
  float* out = a.tri36 + (size_t)t * 36 + 9 + 3 * k;
  out[0] = n.x, out[1] = n.y, out[2] = n.z;
}
