// ezrt_orient_kernels.h -- the kernels of the mesh orientation (include/ezrt_orient.h, rules O1 to O8): the patches of a mesh, a
// consistent winding of each, its signed volume, and the reversal of the marked rows.  Included by ezrt_mesh.hip, after
// ezrt_vertex_kernels.h (it uses topo_finite; its prefix sum is scan_tiled of ezrt_scan_kernels.h, launched by the host).
//
//   orient_init_kernel      the union-find, the accumulators, A and the summary, whatever `work` held
//   orient_union_kernel     O2, O3, O4: one lane per half-edge; a link, taken at its lower half-edge, unites its two triangles with parity
//   orient_flatten_kernel   O3, O6: one lane per triangle; (root, parity to root), the root's size, the flag that the scan numbers, A
//   orient_check_kernel     O4, O5: one lane per triangle; NONORIENTABLE where a link's parities violate its sign, OPEN at a non-link,
//                           and whether f0 is 1 anywhere, OR-ed over runs of lanes with one root and then into the root's word
//   orient_volume_kernel    O6: one lane per triangle; q(t) signed by f0, summed over runs of lanes with one root, one atomicAdd per run
//   orient_finish_kernel    O7, O8: one lane per triangle; flip, patch; a root writes its patch's row; the counts, one atomic per workgroup
//   rewind_kernel           one lane per row of the caller's array: p2 <-> p3 and n2 <-> n3 where flip[t] != 0
//
// The discipline is that of ezrt_topology_kernels.h.  INSIDE a launch, a word that one workgroup writes and another reads is touched
// by agent-scope atomics ONLY: par (relaxed agent-scope atomic load, atomicCAS) in the union; psz, pf, vol, amax and the summary
// (atomicAdd, atomicOr, atomicMax), which nobody reads in the launch that adds to them.  EVERYTHING ELSE crosses a launch boundary on
// one stream: par is read by the flatten with plain loads, one launch after the union; flat by the check, the volume and the finish;
// pf by the volume (f0 is 0 on a non-orientable patch) and the finish; vol and scan by the finish.  twin, edge_class and tri_geom are
// written by nobody while the call runs.
//
// Bounds.  twin and edge_class are the caller's and are NOT trusted: orient_link reads twin[g] and edge_class of triangle g / 3 only
// after 0 <= g < 3 n_tri.  Every find runs at most n_tri steps along a strictly descending parent (par[t] >> 1 <= t always, and a
// word only ever moves to a lower parent), every union at most n_tri retries; every index read back from `work` is checked against
// its array before it is used.
//
// Cost.  Every launch is one pass over the triangles or the half-edges with a few gathered words each, except for the walks of the
// union-find: the KNOWN LIMIT of the header.  One patch of 10^6 triangles puts 10^6 lanes on one root's accumulators, and atomics on
// one address are served one after the other (about 11 ns each: 11.3 ms for the sizes and 12.0 ms for the volumes when every lane
// issued its own).  So the flatten, the check and the volume first combine the lanes of a wave that share a root and are neighbours
// (orient_runs: the run's length, or a segmented scan by __shfl_up) and issue one atomic per run, and the counts of the summary are
// summed over the workgroup first.
#pragma once

// EZRT_ORIENT_LANE_ATOMICS=1 is a measurement variant (Makefile: build_ab/libezrt_hip_orient_lane_atomics.so; tools/orient_rates.py
// times it): the volume launch without the runs, one atomicAdd per lane.  The same sums, by another route; never the product.
#ifndef EZRT_ORIENT_LANE_ATOMICS
#define EZRT_ORIENT_LANE_ATOMICS 0
#endif

constexpr int OR_BLOCK = 256;
constexpr uint32_t OR_DEAD = 0xFFFFFFFFu;  // flat[t] of a triangle that does not take part (a word is at most 2 n_tri - 1 < 2^31)
constexpr uint32_t OR_OPEN = 1u, OR_NONORIENTABLE = 2u, OR_ODD = 4u;   // pf at a root; OR_ODD: f0 is 1 somewhere in the patch

struct OrientArgs {
  const float4* tri_geom;
  int32_t n_tri;
  const int32_t* twin;
  const uint8_t* edge_class;
  int32_t outward;
  // work
  long long* scan;   // n_tri + 1: 1 at a root, then its exclusive prefix sum; [n_tri] = P
  long long* tiles;  // ceil(n_tri / SCAN_TILE) + 1: the sums of the scan's tiles
  long long* vol;    // n_tri: at a root, vol6_0 of its patch
  uint32_t* par;     // n_tri: parent << 1 | parity(t -> parent), parent <= t
  uint32_t* flat;    // n_tri: root << 1 | parity(t -> root), or OR_DEAD
  uint32_t* pf;      // n_tri: at a root, OR_OPEN | OR_NONORIENTABLE | OR_ODD
  int32_t* psz;      // n_tri: at a root, its patch's triangles
  uint32_t* amax;    // 1 (and a word of padding): the bits of A
  // outputs
  uint8_t* flip;
  int32_t *patch_root, *patch, *proot, *psize;
  uint8_t* pflags;
  long long* vol6;
  unsigned long long* summary;
};

// O1: whether triangle t takes part; the caller has checked t
__device__ inline bool orient_takes(const uint8_t* __restrict__ edge_class, int32_t t) {
  const uint8_t* c = edge_class + (size_t)t * 3;
  const uint32_t c0 = c[0], c1 = c[1], c2 = c[2];
  return ((c0 - 1u) < 4u) & ((c1 - 1u) < 4u) & ((c2 - 1u) < 4u);
}
// O2: the half-edge that h = 3 t + e is a link to, or -1, and the link's sign; the caller has checked h, and that t takes part
__device__ inline int32_t orient_link(const OrientArgs& a, uint32_t h, uint32_t& sigma) {
  const uint32_t H = 3u * (uint32_t)a.n_tri, c = a.edge_class[h];
  sigma = c == 3u ? 1u : 0u;
  if (c != 2u && c != 3u) return -1;
  const int32_t g = a.twin[h];
  if (g < 0 || (uint32_t)g >= H) return -1;
  const int32_t tg = g / 3;
  if ((uint32_t)tg == h / 3u || !orient_takes(a.edge_class, tg)) return -1;
  if (a.edge_class[g] != c || a.twin[g] != (int32_t)h) return -1;
  return g;
}

__global__ __launch_bounds__(OR_BLOCK) void orient_init_kernel(OrientArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * OR_BLOCK, i0 = (uint64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
  for (uint64_t i = i0; i < (uint64_t)a.n_tri; i += stride) a.par[i] = (uint32_t)i << 1, a.vol[i] = 0, a.pf[i] = 0u, a.psz[i] = 0;
  if (i0 < 8) a.summary[i0] = 0ull;
  if (i0 < 2) a.amax[i0] = 0u;
}

// O3, O4, the union-find with parity.  A word of par is (parent << 1 | parity to that parent).  A root's word is (t << 1); it is
// hooked ONCE, by atomicCAS, under a lower root, and afterwards only ever replaced, by atomicCAS from the word read, with (grandparent,
// the sum of the two parities): in an orientable patch every word is a true relation between two triangles for ever, and in a
// non-orientable one the parents are right all the same and the parities are not used (O4).
__device__ inline uint32_t orient_word(const uint32_t* par, uint32_t t) {
  return __hip_atomic_load(par + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of t and the parity of t to it
__device__ inline uint32_t orient_find(uint32_t* par, uint32_t t, uint32_t& parity) {
  uint32_t p = 0;
  for (uint32_t w = orient_word(par, t); (w >> 1) < t;) { // strictly descending: at most t steps
    const uint32_t up = w >> 1, w2 = orient_word(par, up), gp = w2 >> 1;
    if (gp < up) atomicCAS(&par[t], w, (gp << 1) | ((w ^ w2) & 1u)); // path halving: an ancestor, and lower than what the word holds
    p ^= w & 1u;
    t = up, w = w2;
  }
  parity = p;
  return t;
}
__global__ __launch_bounds__(OR_BLOCK) void orient_union_kernel(OrientArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * OR_BLOCK;
  for (uint64_t h = (uint64_t)blockIdx.x * OR_BLOCK + threadIdx.x; h < H; h += stride) {
    const int32_t t = (int32_t)(h / 3);
    if (!orient_takes(a.edge_class, t)) continue;
    uint32_t sigma;
    const int32_t g = orient_link(a, (uint32_t)h, sigma);
    if (g < 0 || (uint64_t)g < h) continue; // a link is symmetric (O2): its lower half-edge unites the two
    uint32_t x = (uint32_t)t, y = (uint32_t)(g / 3), px = 0, py = 0;
    for (int32_t tries = 0; tries <= a.n_tri; tries++) { // a failed hook means the root was hooked lower meanwhile: finitely often
      uint32_t qx, qy;
      x = orient_find(a.par, x, qx), y = orient_find(a.par, y, qy);
      px ^= qx, py ^= qy; // the parity of the link's two triangles to x and to y
      if (x == y) break;
      const uint32_t hi = x > y ? x : y, lo = x > y ? y : x;
      if (atomicCAS(&a.par[hi], hi << 1, (lo << 1) | (px ^ py ^ sigma)) == (hi << 1)) break;
    }
  }
}

// The runs of a wave: lanes that are neighbours and carry one key.  start is the first lane of this lane's run, last says that this
// lane ends its run.  Every lane of the wave calls it.
__device__ inline void orient_runs(uint32_t key, uint32_t lane, uint32_t& start, bool& last) {
  const uint32_t before = (uint32_t)__shfl_up((int)key, 1);
  const unsigned long long heads = __ballot(lane == 0 || before != key); // bit 0 is always set
  start = 63u - (uint32_t)__clzll(heads & (~0ull >> (63u - lane)));
  last = lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull;
}

// the sum and the largest of v over the workgroup, valid in thread 0: a wave's by __shfl_xor, the waves' through `part` (OR_BLOCK / 64
// words of LDS).  Every thread of the workgroup calls them.  What they save: one atomic per workgroup on a word of the summary
// instead of one per wave -- atomics on ONE address are served one after the other, about 11 ns each.
__device__ inline uint32_t orient_block_sum(uint32_t v, uint32_t* part) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  __syncthreads(); // (an earlier use of part has been read)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < OR_BLOCK / 64; w++) s += part[w];
  return s;
}
__device__ inline uint32_t orient_block_max(uint32_t v, uint32_t* part) {
  v = weld_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < OR_BLOCK / 64; w++) s = part[w] > s ? part[w] : s;
  return s;
}

// one lane per triangle: par is final (the union is an earlier launch), and plain loads read it
__global__ __launch_bounds__(OR_BLOCK) void orient_flatten_kernel(OrientArgs a) {
  __shared__ uint32_t part[OR_BLOCK / 64];
  const uint64_t N = (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * OR_BLOCK;
  const uint64_t rounds = (N + stride - 1) / stride; // every lane of a workgroup runs the same number of rounds: the ballots are uniform
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t big = 0u, taking = 0u;
  uint64_t i = (uint64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride) {
    uint32_t key = OR_DEAD;
    if (i < N) {
      const uint32_t t = (uint32_t)i;
      if (orient_takes(a.edge_class, (int32_t)t)) {
        uint32_t x = t, p = 0u;
        for (uint32_t w = a.par[x]; (w >> 1) < x; w = a.par[x]) p ^= w & 1u, x = w >> 1; // strictly descending
        key = x;
        taking++;
        a.flat[t] = (x << 1) | p;
        a.patch_root[t] = (int32_t)x;
        a.scan[t] = x == t ? 1 : 0;
        const float4* g = a.tri_geom + (size_t)t * 3;
#pragma unroll
        for (int v = 0; v < 3; v++) { // O6: the largest finite |coordinate|, on the bits
          const float4 q = g[v];
          const uint32_t ux = __float_as_uint(q.x) & 0x7FFFFFFFu, uy = __float_as_uint(q.y) & 0x7FFFFFFFu, uz = __float_as_uint(q.z) & 0x7FFFFFFFu;
          big = topo_finite(ux) && ux > big ? ux : big;
          big = topo_finite(uy) && uy > big ? uy : big;
          big = topo_finite(uz) && uz > big ? uz : big;
        }
      } else {
        a.flat[t] = OR_DEAD;
        a.patch_root[t] = -1;
        a.scan[t] = 0;
      }
    }
    // the patch's size: one atomicAdd per run of lanes with one root, by the run's length (10^6 lanes on one root's counter took 11.3 ms)
    uint32_t start;
    bool last;
    orient_runs(key, lane, start, last);
    if (last && key != OR_DEAD) atomicAdd(&a.psz[key], (int32_t)(lane - start + 1u));
  }
  taking = orient_block_sum(taking, part);
  big = orient_block_max(big, part);
  if (threadIdx.x == 0) {
    if (taking) atomicAdd(&a.summary[0], (unsigned long long)taking);
    if (big) atomicMax(a.amax, big);
  }
}

// O4, O5.  flat was written by the launch before.
__global__ __launch_bounds__(OR_BLOCK) void orient_check_kernel(OrientArgs a) {
  const uint64_t N = (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * OR_BLOCK;
  const uint64_t rounds = (N + stride - 1) / stride;
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t i = (uint64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride) {
    uint32_t key = OR_DEAD, bits = 0u;
    if (i < N) {
      const uint32_t t = (uint32_t)i, f = a.flat[t];
      if (f != OR_DEAD && (f >> 1) < (uint32_t)a.n_tri) {
        key = f >> 1;
        bits = (f & 1u) ? OR_ODD : 0u;
        for (uint32_t e = 0; e < 3u; e++) {
          uint32_t sigma;
          const int32_t g = orient_link(a, 3u * t + e, sigma);
          if (g < 0) bits |= OR_OPEN;
          else if (((f ^ a.flat[g / 3]) & 1u) != sigma) bits |= OR_NONORIENTABLE;
        }
      }
    }
    uint32_t start;
    bool last;
    orient_runs(key, lane, start, last);
    for (uint32_t o = 1; o < 64u; o <<= 1) { // an inclusive OR over the run
      const uint32_t y = (uint32_t)__shfl_up((int)bits, o);
      if (lane >= start + o) bits |= y;
    }
    if (last && key != OR_DEAD && bits) atomicOr(&a.pf[key], bits);
  }
}

// O6: S = 3 E - 30 from the bits of A
__device__ inline int orient_scale(uint32_t abits) {
  int E = 0;
  const uint32_t ex = abits >> 23, man = abits & 0x007FFFFFu;
  if (ex) E = (int)ex - 126;                       // a normal number lies in [2^(ex - 127), 2^(ex - 126))
  else if (man) E = (32 - __clz((int)man)) - 149;  // a denormal is man * 2^-149
  return 3 * E - 30;
}
// O6: q(t).  Every operation is one fp64 instruction as written (contraction is off in every build of the library).
__device__ inline long long orient_q(const float4* __restrict__ g, int S) {
  const float4 fa = g[0], fb = g[1], fc = g[2];
  const double ax = fa.x, ay = fa.y, az = fa.z, bx = fb.x, by = fb.y, bz = fb.z, cx = fc.x, cy = fc.y, cz = fc.z;
  const double m0 = by * cz - bz * cy, m1 = bz * cx - bx * cz, m2 = bx * cy - by * cx;
  const double d = (ax * m0 + ay * m1) + az * m2;
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  if ((u & 0x7FF0000000000000ull) == 0x7FF0000000000000ull) return 0; // not finite
  return llrint(ldexp(d, -S));
}
// flat, pf and amax were written by earlier launches
__global__ __launch_bounds__(OR_BLOCK) void orient_volume_kernel(OrientArgs a) {
  const uint64_t N = (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * OR_BLOCK;
  const uint64_t rounds = (N + stride - 1) / stride;
  const uint32_t lane = threadIdx.x & 63u;
  const int S = orient_scale(a.amax[0]);
  uint64_t i = (uint64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride) {
    uint32_t key = OR_DEAD;
    long long q = 0;
    if (i < N) {
      const uint32_t t = (uint32_t)i, f = a.flat[t];
      if (f != OR_DEAD && (f >> 1) < (uint32_t)a.n_tri) {
        key = f >> 1;
        q = orient_q(a.tri_geom + (size_t)t * 3, S);
        const bool f0 = (f & 1u) && !(a.pf[key] & OR_NONORIENTABLE);
        q = f0 ? -q : q;
      }
    }
#if EZRT_ORIENT_LANE_ATOMICS
    (void)lane;
    if (key != OR_DEAD && q) atomicAdd((unsigned long long*)&a.vol[key], (unsigned long long)q);
#else
    uint32_t start;
    bool last;
    orient_runs(key, lane, start, last);
    for (uint32_t o = 1; o < 64u; o <<= 1) { // an inclusive sum over the run: integers, the order does not matter
      const long long y = __shfl_up(q, o);
      if (lane >= start + o) q += y;
    }
    if (last && key != OR_DEAD && q) atomicAdd((unsigned long long*)&a.vol[key], (unsigned long long)q);
#endif
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.summary[6] = (unsigned long long)(long long)S;
}

// O7, O8: everything read here was written by an earlier launch
__global__ __launch_bounds__(OR_BLOCK) void orient_finish_kernel(OrientArgs a) {
  const uint64_t N = (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * OR_BLOCK;
  const uint64_t rounds = (N + stride - 1) / stride;
  __shared__ uint32_t part[OR_BLOCK / 64];
  uint32_t c2 = 0u, c3 = 0u, c4 = 0u, c5 = 0u;
  uint64_t i = (uint64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride) {
    bool flipped = false, is_root = false, orientable = false, closed = false, inward = false;
    if (i < N) {
      const uint32_t t = (uint32_t)i, f = a.flat[t];
      int32_t p = -1;
      if (f != OR_DEAD && (f >> 1) < (uint32_t)a.n_tri) {
        const uint32_t root = f >> 1, bits = a.pf[root];
        const long long v = a.vol[root], c = a.scan[root];
        orientable = !(bits & OR_NONORIENTABLE), closed = !(bits & OR_OPEN);
        inward = orientable && closed && v < 0;
        const bool act = a.outward != 0 && inward;
        flipped = orientable && (((f & 1u) != 0u) != act);
        if (c >= 0 && c < (long long)a.n_tri) {
          p = (int32_t)c;
          is_root = root == t;
          if (is_root) {
            const bool rewound = orientable && (act || (bits & OR_ODD)); // the root itself is reversed when `outward` acts
            a.proot[p] = (int32_t)t;
            a.psize[p] = a.psz[t];
            a.pflags[p] = (uint8_t)((closed ? 0u : 1u) | (orientable ? 0u : 2u) | (rewound ? 4u : 0u) | (inward ? 8u : 0u));
            a.vol6[p] = act ? -v : v;
          }
        }
      }
      a.flip[t] = flipped ? 1 : 0;
      a.patch[t] = p;
    }
    c2 += is_root && orientable ? 1u : 0u, c3 += is_root && closed ? 1u : 0u, c4 += flipped ? 1u : 0u, c5 += is_root && inward ? 1u : 0u;
  }
  c2 = orient_block_sum(c2, part), c3 = orient_block_sum(c3, part), c4 = orient_block_sum(c4, part), c5 = orient_block_sum(c5, part);
  if (threadIdx.x == 0) { // O8: one atomic per workgroup and figure
    if (c2) atomicAdd(&a.summary[2], (unsigned long long)c2);
    if (c3) atomicAdd(&a.summary[3], (unsigned long long)c3);
    if (c4) atomicAdd(&a.summary[4], (unsigned long long)c4);
    if (c5) atomicAdd(&a.summary[5], (unsigned long long)c5);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.summary[1] = (unsigned long long)a.scan[a.n_tri];
}

// the reversal of the marked rows of the caller's array: one lane per row
__global__ __launch_bounds__(OR_BLOCK) void rewind_kernel(float* tri36, uint32_t n_tri, const uint8_t* flip) {
  const uint32_t t = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (t >= n_tri || flip[t] == 0) return;
  float* row = tri36 + (size_t)t * 36;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float p2 = row[3 + k], p3 = row[6 + k], n2 = row[12 + k], n3 = row[15 + k];
    row[3 + k] = p3, row[6 + k] = p2, row[12 + k] = n3, row[15 + k] = n2;
  }
}
