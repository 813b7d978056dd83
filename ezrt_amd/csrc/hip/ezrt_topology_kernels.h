// ezrt_topology_kernels.h -- the kernels of the mesh topology (include/ezrt_topology.h, rules M1 to M7): edge twins, edge classes and
// edge-connected components of the whole mesh, on bits alone.  Included by ezrt_mesh.hip, after ezrt_scan_kernels.h (it uses
// loops_hash; the host numbers the components with scan_small).
//
//   topo_init_kernel      the table, the union-find, the accumulators and the summary, whatever `work` held
//   topo_join_kernel      M3: one lane per half-edge; claims or finds the slot of its undirected edge, pushes itself onto the slot's list
//   topo_rank_kernel      M4, M5, M7: one lane per half-edge; walks its slot's list: m, its direction group, its rank; twin, class, mult
//   topo_unite_kernel     M6: one lane per half-edge; unites its triangle with the triangle of its slot's representative
//   topo_flatten_kernel   M6: one lane per triangle; its root, the root's size and flags, the flag that scan_block_kernel numbers
//   topo_scatter_kernel   M6: one lane per triangle; component, and comp_root / comp_size / comp_flags of a root; summary[6]
//   topo_at_kernel        the same rule for pairs already held: one lane per pair, no table
//
// ONE data structure is shared by all workgroups of a launch, and workgroups of one launch run on different XCDs, whose L2s are not
// coherent and whose CUs' vector caches never see another CU's stores.  The discipline, kernel by kernel:
// * INSIDE a launch, a word that one workgroup writes and another reads is touched by agent-scope atomics ONLY: rep (atomicCAS), head
//   (atomicExch) in the join; parent (relaxed agent-scope atomic load, atomicCAS, atomicMin) in the unite; the accumulators (atomicAdd,
//   atomicOr, atomicMax; nobody reads them in the launch that adds to them).  Atomics are performed in memory-side L2 and are coherent.
// * EVERYTHING ELSE crosses a launch boundary on one stream: link and slot are plain stores of the join, each to the lane's own entry,
//   read by the rank and the unite; rep and head are read there with plain loads, one launch after the last atomic wrote them; parent
//   is read by the flatten with plain loads, one launch after the unite; root, the sizes, the flags and the scan likewise.
// * tri_geom is written by nobody while a query runs (a refit waits for it): the keys of a representative are plain loads.
//
// Bounds.  Every probe loop runs at most T times (the table is at most half full: 3 n_tri edges at the most in T >= 6 n_tri slots),
// every list walk at most 3 n_tri steps, every find at most n_tri steps along a strictly descending parent (parent[t] <= t always, and
// a word of parent only ever decreases), every unite at most n_tri retries; every index read back from `work` is checked against its
// array before it is used, so that nothing outside the stated arrays is read or written whatever happens.
//
// Cost.  The join is one probe, one exchange and two stores per half-edge.  A half-edge of an edge of multiplicity m <= 2 is ranked
// in one walk of m steps.  On a NONMANIFOLD edge a lane also looks for the member that holds a given rank in a direction group, which
// is a walk per candidate: O(m^2) per half-edge, O(m^3) for the edge.  Multiplicities above 2 are defects and rare, and the known
// limit: a mesh that stores one face thousands of times is ranked slowly (200 copies: 40 000 steps per lane).
#pragma once

constexpr int TP_BLOCK = 256;
constexpr uint32_t TP_END = 0xFFFFFFFFu;   // the end of a slot's list, an empty head
constexpr uint32_t TP_DEAD = 0xFFFFFFFEu;  // link[h] of a half-edge whose triangle is not TOPO-live (an entry is at most 0xFFFFFFFB)

struct TopoArgs {
  const float4* tri_geom;
  int32_t n_tri;
  uint64_t T;            // slots, a power of two, at most 2^32
  // work
  long long* scan;       // n_tri + 1: 1 for a root, then its exclusive prefix sum
  int32_t* rep;          // T: the representative half-edge of the slot's edge, -1 empty
  uint32_t* head;        // T: the newest entry of the slot's list, TP_END empty; an entry is h * 2 + direction
  uint32_t* link;        // 3 n_tri: the entry pushed before h, TP_END, or TP_DEAD
  uint32_t* slot;        // 3 n_tri
  int32_t* parent;       // n_tri
  int32_t* csize;        // n_tri: at a root, its component's triangles
  uint32_t* cflag;       // n_tri: at a root, its component's flags
  // outputs
  int32_t* twin;
  uint8_t* edge_class;
  int32_t* mult;
  int32_t *root, *component, *comp_root, *comp_size;
  uint8_t* comp_flags;
  unsigned long long* summary;
};

// M1: the key of a vertex -- its three bit patterns, -0 as +0
struct TopoKey {
  uint32_t x, y, z;
};
__device__ inline uint32_t topo_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return u == 0x80000000u ? 0u : u;
}
__device__ inline bool topo_finite(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }
__device__ inline bool topo_eq(const TopoKey& a, const TopoKey& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// an order of the keys (lexicographic on the bit patterns): what `direction` and the edge's hash are taken from
__device__ inline bool topo_less(const TopoKey& a, const TopoKey& b) {
  return a.x != b.x ? a.x < b.x : (a.y != b.y ? a.y < b.y : a.z < b.z);
}
// M2: the three keys of triangle t, and whether it is TOPO-live
__device__ inline bool topo_tri(const float4* __restrict__ tri_geom, int32_t t, TopoKey k[3]) {
  const float4* g = tri_geom + (size_t)t * 3;
  unsigned ok = 1u; // (bitwise: no short-circuit branches)
#pragma unroll
  for (int v = 0; v < 3; v++) {
    const float4 p = g[v];
    k[v].x = topo_bits(p.x), k[v].y = topo_bits(p.y), k[v].z = topo_bits(p.z);
    ok &= (unsigned)topo_finite(k[v].x) & (unsigned)topo_finite(k[v].y) & (unsigned)topo_finite(k[v].z);
  }
  ok &= (unsigned)!topo_eq(k[0], k[1]) & (unsigned)!topo_eq(k[1], k[2]) & (unsigned)!topo_eq(k[0], k[2]);
  return ok != 0u;
}
// vertex v % 3 of a triangle, v in 0 .. 3, by selection: constant indices keep the keys in registers
__device__ inline TopoKey topo_vertex(const TopoKey k[3], int v) {
  const TopoKey k0 = k[0], k1 = k[1], k2 = k[2];
  TopoKey r;
  r.x = v == 1 ? k1.x : (v == 2 ? k2.x : k0.x);
  r.y = v == 1 ? k1.y : (v == 2 ? k2.y : k0.y);
  r.z = v == 1 ? k1.z : (v == 2 ? k2.z : k0.z);
  return r;
}
// the two keys of half-edge e of a triangle in the order of topo_less (lo, hi); direction: 1 when the half-edge runs from lo to hi
__device__ inline uint32_t topo_edge(const TopoKey k[3], int e, TopoKey& lo, TopoKey& hi) {
  const TopoKey a = topo_vertex(k, e), b = topo_vertex(k, e + 1);
  const bool fwd = topo_less(a, b);
  lo = fwd ? a : b, hi = fwd ? b : a;
  return fwd ? 1u : 0u;
}
__device__ inline uint32_t topo_hash(const TopoKey& lo, const TopoKey& hi) {
  return loops_hash(loops_hash(lo.x, lo.y, lo.z), loops_hash(hi.x, hi.y, hi.z) * 0x9E3779B1u + 0x7F4A7C15u, hi.x ^ lo.z);
}

__global__ __launch_bounds__(TP_BLOCK) void topo_init_kernel(TopoArgs a, bool components) {
  const uint64_t stride = (uint64_t)gridDim.x * TP_BLOCK, i0 = (uint64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
  for (uint64_t i = i0; i < a.T; i += stride) a.rep[i] = -1, a.head[i] = TP_END;
  if (components)
    for (uint64_t i = i0; i < (uint64_t)a.n_tri; i += stride) a.parent[i] = (int32_t)i, a.csize[i] = 0, a.cflag[i] = 0u;
  if (i0 < 8) a.summary[i0] = 0ull;
}

// M3, the join.  rep[p] is claimed ONCE, by atomicCAS, and never changes afterwards; a lane that loses the race compares its edge with
// the winner's by reading the winner's vertices in tri_geom.
__global__ __launch_bounds__(TP_BLOCK) void topo_join_kernel(TopoArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * TP_BLOCK;
  const uint32_t mask = (uint32_t)(a.T - 1);
  for (uint64_t h = (uint64_t)blockIdx.x * TP_BLOCK + threadIdx.x; h < H; h += stride) {
    const int32_t t = (int32_t)(h / 3);
    const int e = (int)(h - 3ull * (uint64_t)t);
    TopoKey k[3], lo, hi;
    // one exit: a half-edge that takes no part (M2) -- or that found no slot, which cannot happen in a table at most half full --
    // stores TP_DEAD and is walked by nobody
    uint32_t my_slot = 0u, my_link = TP_DEAD;
    if (topo_tri(a.tri_geom, t, k)) {
      const uint32_t dir = topo_edge(k, e, lo, hi);
      uint32_t p = topo_hash(lo, hi) & mask;
      bool found = false;
      for (uint64_t probe = 0; probe < a.T && !found; probe++) {
        const int32_t old = atomicCAS(&a.rep[p], -1, (int32_t)h);
        if (old == -1) {
          found = true;
        } else if (old >= 0 && (uint64_t)old < H) {
          const int32_t ot = old / 3;
          TopoKey ok[3], olo, ohi;
          (void)topo_tri(a.tri_geom, ot, ok);
          (void)topo_edge(ok, old - 3 * ot, olo, ohi);
          found = topo_eq(olo, lo) && topo_eq(ohi, hi);
        }
        if (!found) p = (p + 1u) & mask;
      }
      if (found) {
        my_slot = p;
        my_link = atomicExch(&a.head[p], (uint32_t)h * 2u + dir);
      }
    }
    a.slot[h] = my_slot;
    a.link[h] = my_link;
  }
}

// the entry behind x in a list, and its half-edge and direction; false at the end of the list or on a word that is no entry
__device__ inline bool topo_entry(const TopoArgs& a, uint64_t H, uint32_t x, uint32_t& h, uint32_t& dir) {
  h = x >> 1, dir = x & 1u;
  return x < TP_DEAD && (uint64_t)h < H;
}
// the half-edge of direction `dir` that has exactly `rank` members of its direction below it in the list of `first`, or -1
__device__ inline int32_t topo_select(const TopoArgs& a, uint64_t H, uint32_t first, uint32_t dir, uint32_t rank) {
  uint32_t c, cd;
  uint64_t so = 0;
  for (uint32_t x = first; topo_entry(a, H, x, c, cd) && so < H; x = a.link[c], so++) {
    if (cd != dir) continue;
    uint32_t below = 0, o, od;
    uint64_t si = 0;
    for (uint32_t y = first; topo_entry(a, H, y, o, od) && si < H; y = a.link[o], si++) below += (od == dir && o < c) ? 1u : 0u;
    if (below == rank) return (int32_t)c;
  }
  return -1;
}

// M4, M5, M7.  Every word read here was written by an earlier launch.
__global__ __launch_bounds__(TP_BLOCK) void topo_rank_kernel(TopoArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * TP_BLOCK;
  const uint64_t rounds = (H + stride - 1) / stride; // every lane of a wave runs the same number of rounds: the ballots are uniform
  uint64_t h = (uint64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, h += stride) {
    uint32_t m = 0, cls = 0;
    bool live = false, lowest = false;
    if (h < H) {
      int32_t tw = -1;
      const uint32_t lk = a.link[h];
      live = lk != TP_DEAD;
      if (live) {
        const uint32_t s = a.slot[h], first = (uint64_t)s < a.T ? a.head[s] : TP_END;
        uint32_t mine = 0, n_same = 0, n_opp = 0, same_below = 0, opp_below = 0, other = TP_END, o, od;
        uint64_t steps = 0;
        for (uint32_t x = first; topo_entry(a, H, x, o, od) && steps < H; x = a.link[o], steps++)
          if ((uint64_t)o == h) mine = od;
        steps = 0;
        for (uint32_t x = first; topo_entry(a, H, x, o, od) && steps < H; x = a.link[o], steps++) {
          if ((uint64_t)o == h) continue;
          other = o;
          if (od == mine) n_same++, same_below += (uint64_t)o < h ? 1u : 0u;
          else n_opp++, opp_below += (uint64_t)o < h ? 1u : 0u;
        }
        m = 1u + n_same + n_opp;
        lowest = same_below + opp_below == 0;
        if (m == 1) cls = 1;
        else if (m == 2) cls = n_opp == 1 ? 2 : 3, tw = (int32_t)other;
        else {
          cls = 4;
          const uint32_t g = n_same + 1, rk = same_below; // my group's size and my rank in it
          if (rk < n_opp) tw = topo_select(a, H, first, mine ^ 1u, rk);
          else { // one of the g - n_opp left over: they pair among themselves in ascending order
            const uint32_t u = rk - n_opp, v = u ^ 1u;
            if (n_opp + v < g) tw = topo_select(a, H, first, mine, n_opp + v);
          }
        }
      }
      a.twin[h] = tw;
      a.edge_class[h] = (uint8_t)cls;
      if (a.mult) a.mult[h] = (int32_t)m;
    }
    // M7: one atomic per wave and figure, not one per lane
    const bool first_of_tri = live && h % 3 == 0;
    const unsigned long long b_tri = __ballot(first_of_tri), b_edge = __ballot(lowest);
    const unsigned long long b1 = __ballot(lowest && cls == 1), b2 = __ballot(lowest && cls == 2), b3 = __ballot(lowest && cls == 3),
                             b4 = __ballot(lowest && cls == 4);
    uint32_t mx = m;
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t y = (uint32_t)__shfl_xor((int)mx, o);
      mx = y > mx ? y : mx;
    }
    if ((threadIdx.x & 63) == 0) {
      if (b_tri) atomicAdd(&a.summary[0], (unsigned long long)__popcll(b_tri));
      if (b_edge) atomicAdd(&a.summary[1], (unsigned long long)__popcll(b_edge));
      if (b1) atomicAdd(&a.summary[2], (unsigned long long)__popcll(b1));
      if (b2) atomicAdd(&a.summary[3], (unsigned long long)__popcll(b2));
      if (b3) atomicAdd(&a.summary[4], (unsigned long long)__popcll(b3));
      if (b4) atomicAdd(&a.summary[5], (unsigned long long)__popcll(b4));
      if (mx) atomicMax(&a.summary[7], (unsigned long long)mx);
    }
  }
}

// M6, the union-find.  parent[t] <= t always; a root is hooked under a LOWER root by atomicCAS and under nothing else, so the root that
// survives a component is its lowest id whatever the order of the unions.  Inside this launch parent is touched by agent-scope atomics
// only: a plain load could be served by this CU's vector cache and never see a hook made on another XCD.
__device__ inline int32_t topo_parent(const int32_t* parent, int32_t t) {
  return __hip_atomic_load(parent + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline int32_t topo_find(int32_t* parent, int32_t t) {
  for (int32_t p = topo_parent(parent, t); p < t && p >= 0;) { // strictly descending: at most t steps
    const int32_t g = topo_parent(parent, p);
    if (g < p && g >= 0) atomicMin(&parent[t], g); // path halving: an ancestor, and lower than what the word holds
    t = p, p = g;
  }
  return t;
}
__global__ __launch_bounds__(TP_BLOCK) void topo_unite_kernel(TopoArgs a) {
  const uint64_t H = 3ull * (uint64_t)a.n_tri, stride = (uint64_t)gridDim.x * TP_BLOCK;
  for (uint64_t h = (uint64_t)blockIdx.x * TP_BLOCK + threadIdx.x; h < H; h += stride) {
    if (a.link[h] == TP_DEAD) continue;
    const uint32_t s = a.slot[h];
    const int32_t r = (uint64_t)s < a.T ? a.rep[s] : -1;
    if (r < 0 || (uint64_t)r >= H) continue;
    int32_t x = (int32_t)(h / 3), y = r / 3;
    for (int32_t tries = 0; tries <= a.n_tri; tries++) { // a failed hook means the root was hooked lower meanwhile: finitely often
      x = topo_find(a.parent, x), y = topo_find(a.parent, y);
      if (x == y) break;
      const int32_t hi = x > y ? x : y, lo = x > y ? y : x;
      if (atomicCAS(&a.parent[hi], hi, lo) == hi) break;
    }
  }
}
// one lane per triangle: parent is final (the unite is an earlier launch), and plain loads read it
__global__ __launch_bounds__(TP_BLOCK) void topo_flatten_kernel(TopoArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * TP_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * TP_BLOCK + threadIdx.x; i < (uint64_t)a.n_tri; i += stride) {
    const int32_t t = (int32_t)i;
    if (a.link[3 * i] == TP_DEAD) {
      a.root[t] = -1;
      a.scan[t] = 0;
      continue;
    }
    int32_t r = t;
    for (int32_t p = a.parent[r]; p < r && p >= 0; p = a.parent[r]) r = p;
    a.root[t] = r;
    a.scan[t] = r == t ? 1 : 0;
    atomicAdd(&a.csize[r], 1);
    uint32_t f = 0;
    for (int e = 0; e < 3; e++) {
      const uint32_t c = a.edge_class[3 * i + e];
      f |= c == 1 ? 1u : (c == 3 ? 2u : (c == 4 ? 4u : 0u));
    }
    if (f) atomicOr(&a.cflag[r], f);
  }
}
__global__ __launch_bounds__(TP_BLOCK) void topo_scatter_kernel(TopoArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * TP_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * TP_BLOCK + threadIdx.x; i < (uint64_t)a.n_tri; i += stride) {
    const int32_t t = (int32_t)i, r = a.root[t];
    if (r < 0 || r > t) {
      a.component[t] = -1;
      continue;
    }
    const long long c = a.scan[r];
    const bool ok = c >= 0 && c < (long long)a.n_tri;
    a.component[t] = ok ? (int32_t)c : -1;
    if (ok && r == t) {
      a.comp_root[c] = t;
      a.comp_size[c] = a.csize[t];
      a.comp_flags[c] = (uint8_t)a.cflag[t];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.summary[6] = (unsigned long long)a.scan[a.n_tri];
}

// the rule for pairs already held: which edge of tri_b is the undirected edge of (tri_a, edge_a), and whether the two run opposite ways
__global__ __launch_bounds__(TP_BLOCK) void topo_at_kernel(const float4* tri_geom, int32_t n_tri, const int32_t* tri_a, const int32_t* edge_a,
                                                           const int32_t* tri_b, uint32_t n, int8_t* shared, int8_t* opposite) {
  const uint32_t i = blockIdx.x * TP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t ta = tri_a[i], ea = edge_a[i], tb = tri_b[i];
  int8_t sh = -1, op = -1;
  TopoKey ka[3], kb[3];
  if (ta >= 0 && ta < n_tri && tb >= 0 && tb < n_tri && ea >= 0 && ea <= 2 && topo_tri(tri_geom, ta, ka) && topo_tri(tri_geom, tb, kb)) {
    const TopoKey a0 = topo_vertex(ka, ea), a1 = topo_vertex(ka, ea + 1);
#pragma unroll
    for (int e = 0; e < 3; e++) {
      const TopoKey b0 = topo_vertex(kb, e), b1 = topo_vertex(kb, e + 1);
      if (topo_eq(a0, b0) && topo_eq(a1, b1)) sh = (int8_t)e, op = 0;
      else if (topo_eq(a0, b1) && topo_eq(a1, b0)) sh = (int8_t)e, op = 1;
    }
  }
  shared[i] = sh;
  if (opposite) opposite[i] = op;
}
