// ezrt_point_queries.h -- the gfx950 kernels of the point queries: closest point (include/ezrt_closest_point.h), nearest K
// (include/ezrt_nearest.h), inside and signed distance (include/ezrt_inside.h), and of the box-overlap, triangle-overlap,
// self-overlap, triangle-distance, sphere-cast, segment, oriented-box, winding-number and plane queries (include/ezrt_box_overlap.h,
// include/ezrt_tri_overlap.h, include/ezrt_self_overlap.h, include/ezrt_tri_distance.h, include/ezrt_sphere_cast.h, include/ezrt_segment.h,
// include/ezrt_obb_overlap.h, include/ezrt_winding.h, include/ezrt_plane.h).  One query point, box, triangle, ray or segment per lane
// (the plane queries: one TRIANGLE per lane, the plane uniform), a workgroup of one wave.  Included by ezrt_queries.hip alone, after ezrt_scan_kernels.h.
//
//   point_walk                       the best-first walk over the 4-wide records that closest point, nearest, signed distance and
//                                    triangle distance share: the lower bound of a slot's box is the caller's
//   closest_point_kernel<WALK>       closest_point_search + closest_point_store
//   nearest_kernel<WALK, COUNT>      point_walk carrying a K-entry sorted list instead of one winner
//   closest_point_at_kernel          closest_point_triangle for pairs the caller holds
//   slot_walk                        the depth-first walk over the 4-wide records that inside, box overlap and triangle overlap share
//   inside_kernel<WALK>              inside_count: slot_walk on the rows its axis needs
//   signed_distance_kernel<WALK>     inside_count + closest_point_search + closest_point_store
//   collect_rows                     a K-entry list of the lowest ids and a count over the caller's traversal, and the wave's row finish
//   fill_rows<WALK>                  collect_rows for a row of the caller's length (include/ezrt_overlap_list.h): every id, not the lowest K
//   overlap_rows                     collect_rows or fill_rows over slot_walk on the query's box
//   *_overlap_list_kernel<WALK>      the five overlap kernels' bodies with a list's arguments: fill_rows instead of collect_rows
//   overlap_sort_kernel              sorts the rows that fill_rows appended on the walk route, in LDS or in place in global memory
//   box_overlap_kernel<WALK>         overlap_rows with the box as the gate and box_overlaps as the rule
//   box_overlap_at_kernel            box_overlaps for pairs the caller holds
//   tri_overlap_kernel<WALK>         overlap_rows with the query triangle's bounding box as the gate and tri_overlaps as the rule
//   tri_overlap_at_kernel            tri_overlaps for pairs the caller holds
//   self_overlap_kernel<WALK>        overlap_rows with a scene triangle's bounding box as the gate and self_crosses as the rule
//   self_overlap_at_kernel           self_crosses for pairs of ids the caller holds
//   tri_distance_kernel<WALK>        point_walk with tri_distance_box as the bound and tri_distance_pair as the rule
//   tri_distance_at_kernel           tri_distance_pair for pairs the caller holds
//   sphere_cast_kernel<WALK>         closest_point_search with B = r * r, then point_walk with sphere_cast_box as the bound and
//                                    sphere_cast_pair as the rule
//   sphere_cast_at_kernel            sphere_cast_at for pairs the caller holds
//   segment_distance_kernel<WALK>    point_walk with tri_distance_box of the segment's box as the bound and segment_pair as the rule
//   segment_distance_at_kernel       segment_pair for pairs the caller holds
//   capsule_overlap_kernel<WALK>     collect_rows over point_walk with the constant radius R2 and segment_pair's dist2 <= R2 as the rule
//   obb_overlap_kernel<WALK>         collect_rows over slot_walk with the hull and the face directions as the gates and obb_overlaps as the rule
//   obb_overlap_at_kernel            obb_overlaps for pairs the caller holds
//   winding_kernel<ATOMIC, TILE>     no walk: every lane sums winding_term over a slice of the triangles (include/ezrt_winding.h)
//   winding_finish_kernel            the int64 sums of a sliced call to float
//   winding_at_kernel                winding_pair for pairs the caller holds
//   plane_kernel<FILL>               no walk: one triangle per lane against a tile of planes, a ballot per plane (include/ezrt_plane.h)
//   plane_total_kernel               part's rows summed to n_cross
//   plane_offsets_kernel             the exclusive prefix sum of n_cross
//   plane_at_kernel                  the plane rule for pairs the caller holds
//   loops_chain_kernel<LDS>          a workgroup per plane: the bit-exact join of a section's rows and their ranking into chains,
//                                    in LDS or in the caller's work memory (include/ezrt_plane_loops.h)
//   (scan_block_kernel               ezrt_scan_kernels.h: an exclusive prefix sum in place -- the planes' loop counts, the loops' lengths)
//   loops_length_kernel              the tail of every chain writes its loop's length
//   loops_scatter_kernel             order, next, loop_offsets and closed
#pragma once
#include "ezrt_device.h"
#include "ezrt_records.h"

namespace ezd {

// What every point query reads of the scene (ezrt_queries.hip: point_scene fills it and chooses the route).
struct PointScene {
  const float4* tri_geom;
  const float4* inner4;     // WALK: the 4-wide records, record 0 the root
  const int32_t* uncovered; // WALK: triangles below no leaf
  int32_t n_uncovered;
  int32_t n_tri;
};
constexpr int CP_BLOCK = 64; // one wave per workgroup: the stack column is 2 x 4 B per entry, and LDS is what bounds the occupancy

// The bound of point i: B = +inf, or d_max[i]^2.  False -- no candidates -- for a non-finite p (every dist2 is then inf or NaN) and
// for a negative or NaN d_max.
EZD bool point_bound(f3 p, const float* d_max, uint32_t i, float& B) {
  const float inf = __builtin_inff();
  bool live = ez_abs(p.x) < inf && ez_abs(p.y) < inf && ez_abs(p.z) < inf;
  B = inf;
  if (d_max) {
    const float dm = d_max[i];
    if (dm >= 0.0f) B = dm * dm;
    else live = false;
  }
  return live;
}

// The pruned route's walk (the scene prunes: boxes nested, every leaf box holds its triangles): visit(k) for every triangle k below
// a leaf whose boxes, from the root down, all have lb <= radius() at the moment they are met.  A best-first walk over the
// 4-WIDE records (ezrt_records.h) -- chosen over the binary records because one 128-byte line gives four boxes, so a point needs
// half the dependent loads on its way down, and because their boxes qualify: a slot's box is a caller's node box (nested, its
// leaves hold their triangles) or an exact union of caller leaf boxes (retree_leaves, and every box after a refit), i.e. a
// superset of the bounding box of every triangle below it.  The four slots are sorted by lb = bound(lo, hi) -- the caller's lower
// bound of the dist2 of every triangle below the box: closest_point_box for a point, tri_distance_box for a triangle --, the walk goes on
// with the nearest and pushes the others, farthest first, as {lb, ref} pairs on the lane's LDS stack column (two rows per entry:
// entry sp at rows 2 sp and 2 sp + 1, stride CP_BLOCK; launched with 2 * (stack_need_cp + 1) rows: the exact worst case when any
// slot may be the nearest, + 1 of slack).  A slot is skipped only when lb > radius -- on equality it is descended: the tie rules
// need every triangle at the radius -- or when lb is not finite (no finite dist2 below it); with RECHECK a popped entry is checked
// against the radius of that moment again (a caller whose radius never shrinks may leave it out: the entry passed at its push).
// Why no margin is needed: for a triangle T below a box [lo, hi], q_T is clamped to T's bounding box, which lies in [lo, hi].  Per
// axis either g = 0 <= |e|, or g = fl(lo - p) with q >= lo > p: q - p >= lo - p in the reals, rounding is monotone and
// |fl(p - q)| = fl(q - p), so |e| >= g (the same on the hi side).  fl(x * x) is monotone in |x| and fl(fl(X + Y) + Z) in each of
// X, Y, Z >= 0, so lb = dot(g, g) <= dot(e, e) = dist2_T ON THE BITS, overflow to +inf included.  Hence a skipped subtree holds no
// triangle with dist2 <= radius: with a radius that no candidate's dist2 exceeds, neither a winner nor a tie is lost, and the order
// of the visits is the caller's to be indifferent to.  p is finite.  (The same for a query triangle, with its bounding box in the
// place of p: tri_distance_kernel.)
// The stack: a pop only removes, so below a record with m slots at most m - 1 entries of it are pending while one child subtree is
// walked -- stack_need_cp = the fold of (m - 1 + deepest child) -- whatever the radius admits: a wider radius pushes more of the
// m - 1, never more than them.
template <bool RECHECK, class Bound, class Radius, class Visit>
EZD void point_walk(const float4* __restrict__ inner4, Bound bound, int* __restrict__ stack, Radius radius, Visit visit) {
  const float inf = __builtin_inff();
  int sp = 0;
  uint32_t ref = 0u;
  for (;;) {
    bool descend = false;
    if (ref & LEAF_BIT) {
      const int first = (int)(ref & 0x00ffffffu);
      const int n = (int)((ref >> 24) & 0x7fu) + 1;
      for (int k = first; k < first + n; k++) visit(k);
    } else {
      const float4* rec = inner4 + (size_t)(ref & REF_INDEX) * N4_FLOAT4;
      const float4 ax = rec[N4_ROW_AA], ay = rec[N4_ROW_AA + 1], az = rec[N4_ROW_AA + 2], rf = rec[N4_ROW_REF];
      const float4 bx = rec[N4_ROW_BB], by = rec[N4_ROW_BB + 1], bz = rec[N4_ROW_BB + 2];
      float l[4] = {bound(mk(ax.x, ay.x, az.x), mk(bx.x, by.x, bz.x)), bound(mk(ax.y, ay.y, az.y), mk(bx.y, by.y, bz.y)),
                    bound(mk(ax.z, ay.z, az.z), mk(bx.z, by.z, bz.z)), bound(mk(ax.w, ay.w, az.w), mk(bx.w, by.w, bz.w))};
      uint32_t r[4] = {__float_as_uint(rf.x), __float_as_uint(rf.y), __float_as_uint(rf.z), __float_as_uint(rf.w)};
      // (an unused slot -- an all-NaN box -- gets lb = inf: never descended)
#pragma unroll
      for (int j = 0; j < 4; j++) l[j] = r[j] == REF_EMPTY ? inf : l[j];
      auto cswap = [&](int a, int b) {
        if (l[b] < l[a]) {
          const float tl = l[a];
          l[a] = l[b], l[b] = tl;
          const uint32_t tr = r[a];
          r[a] = r[b], r[b] = tr;
        }
      };
      cswap(0, 1);
      cswap(2, 3);
      cswap(0, 2);
      cswap(1, 3);
      cswap(1, 2);
      // ascending now: the slots worth a visit are a prefix
      const float rad = radius();
#pragma unroll
      for (int j = 3; j > 0; j--)
        if (l[j] <= rad && l[j] < inf) {
          stack[(2 * sp) * CP_BLOCK] = (int)__float_as_uint(l[j]);
          stack[(2 * sp + 1) * CP_BLOCK] = (int)r[j];
          sp++;
        }
      if (l[0] <= rad && l[0] < inf) {
        ref = r[0];
        descend = true;
      }
    }
    if (descend) continue;
    while (sp > 0) {
      sp--;
      if (!RECHECK || __uint_as_float((uint32_t)stack[(2 * sp) * CP_BLOCK]) <= radius()) {
        ref = (uint32_t)stack[(2 * sp + 1) * CP_BLOCK];
        descend = true;
        break;
      }
    }
    if (!descend) break;
  }
}
// visit(k) for every triangle that may hold a candidate.  WALK = true, the pruned route: point_walk, then the triangles that no leaf
// holds (a caller's array may have some).  WALK = false, the sweep route: tri_geom[0 .. n_tri), no tree, for scenes that do not prune.
// bound(lo, hi) is the walk's lower bound of a box.
template <bool WALK, bool RECHECK, class Bound, class Radius, class Visit>
EZD void bound_visit(const PointScene& sc, Bound bound, int* __restrict__ stack, Radius radius, Visit visit) {
  if (WALK) {
    point_walk<RECHECK>(sc.inner4, bound, stack, radius, visit);
    for (int u = 0; u < sc.n_uncovered; u++) visit(sc.uncovered[u]);
  } else {
    for (int k = 0; k < sc.n_tri; k++) visit(k);
  }
}
// ... for a query point p: the bound is closest_point_box
template <bool WALK, bool RECHECK, class Radius, class Visit>
EZD void point_visit(const PointScene& sc, f3 p, int* __restrict__ stack, Radius radius, Visit visit) {
  bound_visit<WALK, RECHECK>(sc, [&](f3 lo, f3 hi) { return closest_point_box(p, lo, hi); }, stack, radius, visit);
}

// ---- closest-point queries (include/ezrt_closest_point.h).  The radius of the walk is the best dist2 of the moment, which
// closest_point_candidate never lets a later winner or tie exceed, and the order of the visits does not matter to it.
struct ClosestPointArgs {
  PointScene sc;
  const float* points;      // n x 3
  const float* d_max;       // n, or null
  uint32_t n;
  int32_t* tri;             // n
  float* point;             // n x 3, or null
  float* dist;              // n, or null
  float* bary;              // n x 2, or null
};
template <bool WALK>
EZD ClosestBest closest_point_search(const ClosestPointArgs& a, uint32_t i, f3 p, int* __restrict__ stack) {
  ClosestBest r;
  r.tri = -1;
  r.v = r.w = 0.0f;
  r.q = mk(0.0f, 0.0f, 0.0f);
  if (point_bound(p, a.d_max, i, r.best))
    point_visit<WALK, true>(a.sc, p, stack, [&] { return r.best; }, [&](int32_t k) { closest_point_candidate(r, a.sc.tri_geom, k, p); });
  return r;
}
// `sign` is ORed into dist: 0, or the sign bit of a signed distance (|sdist| is dist on the bits)
EZD void closest_point_store(const ClosestPointArgs& a, uint32_t i, const ClosestBest& r, uint32_t sign) {
  a.tri[i] = r.tri;
  if (a.point) st3(a.point + (size_t)i * 3, r.q);
  if (a.dist) a.dist[i] = __uint_as_float(__float_as_uint(r.tri >= 0 ? __builtin_sqrtf(r.best) : __builtin_inff()) | sign);
  if (a.bary) {
    a.bary[(size_t)i * 2] = r.v;
    a.bary[(size_t)i * 2 + 1] = r.w;
  }
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void closest_point_kernel(ClosestPointArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const uint32_t i = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const f3 p = ld3(a.points + (size_t)i * 3);
  closest_point_store(a, i, closest_point_search<WALK>(a, i, p, lds_stack + threadIdx.x), 0u);
}

// ---- nearest-K queries (include/ezrt_nearest.h): point_walk carrying a K-entry sorted list instead of one winner.
//
// The list.  L = the candidates (finite dist2 <= B) sorted by the pair (dist2, k); the first K of them are the answer.  They live in
// the point's own output rows, as all_hits_kernel's do (K entries in registers would cost the walk its occupancy, 64 x K in LDS do
// not fit beside the stack): `dist` holds dist2 during the walk, `nb` entries are filled, and once the row is full `last` /
// `last_id` hold the pair of entry K - 1.  A candidate that does not precede that pair is counted and touches no memory.  An
// insertion shifts the entries whose PAIR is greater up one slot (the K-th falls out): the tree meets triangles in no id order, so
// -- unlike all-hits, where arrival order is the rule -- equal dist2 are ordered by id explicitly.  The list after any sequence of
// insertions is the first min(K, seen) pairs of what was seen, so the order of the visits does not matter.
// The radius of the walk:
//   COUNT = false: B until the row is full, then the dist2 of entry K - 1 (`last`, which starts as B).  A skipped subtree holds
//     only triangles with dist2 > radius >= last: they precede no entry of the row -- at equal dist2 a lower id would, hence the
//     descent on equality.
//   COUNT = true (n_within is wanted): B throughout -- every triangle within d_max must be counted, so the walk cannot shrink below
//     B, and with d_max == NULL it visits every triangle.  A pushed entry still passes when it is popped: no check again.
// Afterwards each wave finishes its 64 rows together, consecutive lanes on consecutive words: a filled slot gets sqrtf(dist2), an
// unused one {-1, +inf}.  Lanes past n take part with nb = 0 and nothing is written past row n - 1.
struct NearestArgs {
  PointScene sc;
  const float* points;      // n x 3
  const float* d_max;       // n, or null
  uint32_t n;
  int32_t K;
  FastDiv div_k;            // / K (the finishing pass)
  int32_t* tri;             // n x K
  float* dist;              // n x K (dist2 during the walk)
  int32_t* n_within;        // n, or null (COUNT = false)
};
template <bool WALK, bool COUNT>
__global__ __launch_bounds__(CP_BLOCK) void nearest_kernel(NearestArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const uint32_t lane = threadIdx.x;
  const uint32_t i = blockIdx.x * CP_BLOCK + lane;
  const int K = a.K;
  const float inf = __builtin_inff();
  int nb = 0;
  if (i < a.n) {
    const f3 p = ld3(a.points + (size_t)i * 3);
    float B;
    const bool live = point_bound(p, a.d_max, i, B);
    int32_t* ri = a.tri + (size_t)i * K;
    float* rd = a.dist + (size_t)i * K;
    uint32_t count = 0;
    float last = B; // the dist2 of entry K - 1 once the row is full (a put to slot K - 1 happens only then); B before
    int32_t last_id = -1;
    auto put = [&](int j, int32_t id, float d2) {
      ri[j] = id;
      rd[j] = d2;
      if (j == K - 1) last = d2, last_id = id;
    };
    auto candidate = [&](int32_t k) {
      f3 q;
      float v, w;
      const float d2 = closest_point_triangle(a.sc.tri_geom + (size_t)k * 3, p, q, v, w);
      if (!(d2 < inf && d2 <= B)) return; // (false for a NaN d2)
      count++;
      if (nb == K && !(d2 < last || (d2 == last && k < last_id))) return; // behind a full row: counted only
      int j = nb < K ? nb++ : K - 1;
      while (j > 0) {
        const float dp = rd[j - 1];
        const int32_t ip = ri[j - 1];
        if (!(dp > d2 || (dp == d2 && ip > k))) break;
        put(j, ip, dp);
        j--;
      }
      put(j, k, d2);
    };
    if (live) point_visit<WALK, !COUNT>(a.sc, p, lds_stack + lane, [&] { return COUNT ? B : last; }, candidate);
    if (COUNT) a.n_within[i] = (int32_t)count;
  }
  // the wave's 64 rows, one flat run of 64 K words from its first row; the rows were written by other lanes of this wave, whose
  // accesses are performed in program order (the fence states it to the compiler and costs nothing at this scope)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const size_t base = (size_t)(i - lane) * K;
  for (uint32_t e = lane; e < 64u * (uint32_t)K; e += 64u) {
    const uint32_t row = fastdiv(e, a.div_k);
    const uint32_t slot = e - row * (uint32_t)K;
    const int used = __shfl(nb, (int)row);
    if (i - lane + row < a.n) {
      if (slot < (uint32_t)used) {
        a.dist[base + e] = __builtin_sqrtf(a.dist[base + e]);
      } else {
        a.tri[base + e] = -1;
        a.dist[base + e] = inf;
      }
    }
  }
}

// ezrt_closest_point_at_device: closest_point_triangle for pairs the caller holds -- point i against triangle tri_id[i].  An id
// outside the scene or a non-finite dist2 writes (zeros, +inf, zeros); point / dist / bary may each be null (not written).
__global__ __launch_bounds__(256) void closest_point_at_kernel(const float4* tri_geom, int32_t n_tri, const float* points,
                                                               const int32_t* tri_id, uint32_t n, float* point, float* dist,
                                                               float* bary) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  f3 Q = mk(0.0f, 0.0f, 0.0f);
  float D = __builtin_inff(), V = 0.0f, W = 0.0f;
  if ((uint32_t)tri < (uint32_t)n_tri) {
    f3 q;
    float v, w;
    const float d2 = closest_point_triangle(tri_geom + (size_t)tri * 3, ld3(points + (size_t)i * 3), q, v, w);
    if (d2 < __builtin_inff()) Q = q, D = __builtin_sqrtf(d2), V = v, W = w; // (false for a NaN d2)
  }
  if (point) st3(point + (size_t)i * 3, Q);
  if (dist) dist[i] = D;
  if (bary) {
    bary[(size_t)i * 2] = V;
    bary[(size_t)i * 2 + 1] = W;
  }
}

// The depth-first walk over the 4-wide records that inside_count and box_overlap_kernel share (the scene prunes: boxes nested, every
// leaf box holds its triangles).  slots(rec, take) looks at one record and calls take(pass, ref) for each of its four slots --
// pass() says whether the slot's box may hold a triangle that counts, and is asked only for a slot in use (a callable, not a bool:
// with the test evaluated before the call inside_kernel<true> took 100 VGPRs for its 98); visit(k) takes every triangle k below a
// leaf that is reached.  Of a record
// the first slot that passes is descended and the others that pass are pushed as bare references, one row of 4 B per entry on the
// lane's LDS column (stride CP_BLOCK); an unused slot (REF_EMPTY, an all-NaN box) is never taken.  The stack bound is argued above
// inside_count: stack_need_cp entries, launched with stack_need_cp + 1 rows.
template <class Slots, class Visit>
EZD void slot_walk(const float4* __restrict__ inner4, int* __restrict__ stack, Slots slots, Visit visit) {
  int sp = 0;
  uint32_t ref = 0u;
  for (;;) {
    uint32_t next = REF_EMPTY;
    if (ref & LEAF_BIT) {
      const int first = (int)(ref & 0x00ffffffu);
      const int n = (int)((ref >> 24) & 0x7fu) + 1;
#pragma unroll 1
      for (int k = first; k < first + n; k++) visit(k);
    } else {
      slots(inner4 + (size_t)(ref & REF_INDEX) * N4_FLOAT4, [&](auto pass, uint32_t r) {
        if (r != REF_EMPTY && pass()) {
          if (next == REF_EMPTY) next = r;
          else stack[(sp++) * CP_BLOCK] = (int)r;
        }
      });
    }
    if (next == REF_EMPTY) {
      if (sp == 0) break;
      next = (uint32_t)stack[(--sp) * CP_BLOCK];
    }
    ref = next;
  }
}

// ---- inside and signed-distance queries (include/ezrt_inside.h).
//
// inside_count<WALK> returns crossings(p): the number of triangles with inside_crossed (ezrt_device.h: G1 .. G6 of the header).
// WALK = true, the pruned route: slot_walk, the depth-first walk over the 4-wide records, not point_walk.  Only the rows of the record that the
// axis needs are loaded -- lo and hi of s and t, and the far plane of u (hi for a positive axis, lo for a negative one;
// g * plane > p.u is hi > p or lo < p, exactly) -- and a slot is descended when lo.s <= p.s <= hi.s, lo.t <= p.t <= hi.t and the far
// plane lies ahead.  These are comparisons on the stored fp32 values: G1 - G3 make a crossed triangle's own bounding box pass them,
// hence every box that holds the triangle (the scene prunes: nested boxes, every leaf box holds its triangles), so no crossed
// triangle is skipped and no slack is needed.  An unused slot (an all-NaN box) fails every comparison.  The count is an integer
// sum: the order of the visits does not matter.
// The stack.  Bare references, one row of 4 B per entry on the lane's LDS column.  Of a record with m slots the first that passes
// is descended and the others that pass are pushed: at most m - 1 entries; a pop only removes.  So while one child subtree is
// walked at most m - 1 entries of the record are pending, and the pending entries of any walk are bounded by the fold of
// (m - 1 + deepest child) over the tree -- which is stack_need_cp (ezrt_scene_build.hip), the bound of every walk that descends
// one slot and pushes at most three.  Launched with stack_need_cp + 1 rows.
// Triangles that no leaf holds are swept after the walk.  WALK = false, the sweep route: every triangle, no tree.
template <bool WALK>
EZD int32_t inside_count(const PointScene& sc, int axis, f3 p, int* __restrict__ stack) {
  const float inf = __builtin_inff();
  if (!(ez_abs(p.x) < inf && ez_abs(p.y) < inf && ez_abs(p.z) < inf)) return 0; // a non-finite p has no crossings
  const InsideFrame f = inside_frame(axis, p);
  int32_t count = 0;
  if (WALK) {
    const int cs = f.c == 2 ? 0 : f.c + 1, ct = cs == 2 ? 0 : cs + 1;
    const int row_u = ((axis & 1) ? N4_ROW_AA : N4_ROW_BB) + f.c;
    slot_walk(
        sc.inner4, stack,
        [&](const float4* rec, auto take) {
          const float4 ls = rec[N4_ROW_AA + cs], lt = rec[N4_ROW_AA + ct], rf = rec[N4_ROW_REF];
          const float4 hs = rec[N4_ROW_BB + cs], ht = rec[N4_ROW_BB + ct], fu = rec[row_u];
          auto pass = [&](float lo_s, float hi_s, float lo_t, float hi_t, float far_u) {
            return [=, &f] { return lo_s <= f.ps && f.ps <= hi_s && lo_t <= f.pt && f.pt <= hi_t && f.g * far_u > f.pu; };
          };
          take(pass(ls.x, hs.x, lt.x, ht.x, fu.x), __float_as_uint(rf.x));
          take(pass(ls.y, hs.y, lt.y, ht.y, fu.y), __float_as_uint(rf.y));
          take(pass(ls.z, hs.z, lt.z, ht.z, fu.z), __float_as_uint(rf.z));
          take(pass(ls.w, hs.w, lt.w, ht.w, fu.w), __float_as_uint(rf.w));
        },
        [&](int32_t k) { count += inside_crossed(sc.tri_geom + (size_t)k * 3, f) ? 1 : 0; });
#pragma unroll 1
    for (int u = 0; u < sc.n_uncovered; u++) count += inside_crossed(sc.tri_geom + (size_t)sc.uncovered[u] * 3, f) ? 1 : 0;
  } else {
#pragma unroll 1
    for (int k = 0; k < sc.n_tri; k++) count += inside_crossed(sc.tri_geom + (size_t)k * 3, f) ? 1 : 0;
  }
  return count;
}
struct InsideArgs {
  PointScene sc;
  const float* points;      // n x 3
  uint32_t n;
  int32_t axis;             // 0..5
  uint8_t* inside;          // n
  int32_t* crossings;       // n, or null
};
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void inside_kernel(InsideArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const uint32_t i = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const f3 p = ld3(a.points + (size_t)i * 3);
  const int32_t count = inside_count<WALK>(a.sc, a.axis, p, lds_stack + threadIdx.x);
  a.inside[i] = (uint8_t)(count & 1);
  if (a.crossings) a.crossings[i] = count;
}

// ezrt_query_signed_distance_device: one launch; each lane runs the crossing walk and then closest_point_kernel's search on the same
// LDS stack column (launched with that kernel's 2 * (stack_need_cp + 1) rows: the crossing walk uses the first stack_need_cp of them
// and leaves nothing pending).  tri, point and bary are that kernel's and |sdist| its dist: the same functions write them.
struct SignedDistanceArgs {
  ClosestPointArgs cp; // (cp.dist is sdist)
  int32_t axis;        // 0..5
  uint8_t* inside;     // n, or null
};
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void signed_distance_kernel(SignedDistanceArgs sa) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const ClosestPointArgs& a = sa.cp;
  const uint32_t i = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const f3 p = ld3(a.points + (size_t)i * 3);
  int* stack = lds_stack + threadIdx.x;
  const bool in = (inside_count<WALK>(a.sc, sa.axis, p, stack) & 1) != 0;
  closest_point_store(a, i, closest_point_search<WALK>(a, i, p, stack), in ? 0x80000000u : 0u);
  if (sa.inside) sa.inside[i] = in ? 1u : 0u;
}

// ---- box-overlap queries (include/ezrt_box_overlap.h).
//
// box_overlap_kernel<WALK>: one box per lane.  WALK = true, the pruned route: slot_walk, descending a slot when slot.lo[c] <= hi[c]
// && slot.hi[c] >= lo[c] on all three axes.  These are comparisons on the stored fp32 values: by H1 an overlapping triangle's own
// bounding box passes them, hence so does every box that holds the triangle (the scene prunes), so no overlapping triangle is skipped
// and no slack is needed; an unused slot (an all-NaN box) fails them.  Triangles that no leaf holds are swept after the walk.
// WALK = false, the sweep route: every triangle, no tree.  Both call box_overlaps (ezrt_device.h: H1 .. H3 of the header).
// The list, kept as nearest_kernel keeps its own: the lowest ids seen so far, ascending, in the box's own output row; `nb` entries
// are filled, and once the row is full `last_id` holds entry K - 1.  A later overlap with a higher id is counted and touches no
// memory; a lower one is inserted by shifting the greater entries up one slot (the K-th falls out).  With K == 0 the row is full
// from the start and nothing is stored.
// The visit order does not matter: the count is an integer sum over the triangles, each met once, and the row after any sequence of
// insertions is the min(K, seen) lowest ids of what was seen.
// Afterwards each wave finishes its 64 rows together, consecutive lanes on consecutive words: -1 into the unused slots.  Lanes past n
// and boxes that are not live take part with nb = 0, and nothing is written past row n - 1.
struct BoxOverlapArgs {
  PointScene sc;
  const float* lo;          // n x 3
  const float* hi;          // n x 3
  uint32_t n;
  int32_t K;                // 0 .. 64
  FastDiv div_k;            // / max(K, 1) (the finishing pass)
  int32_t* tri;             // n x K (not read or written when K == 0)
  int32_t* n_overlap;       // n, or null
};
// The body that box_overlap_kernel and tri_overlap_kernel share: the walk or the sweep of lane i's query, its list and count, and
// the wave's row finish.  `a` has sc, n, K, div_k, tri and n_overlap; load(i, q) reads query i into q and says whether it is live;
// q.lo and q.hi are the gate of the walk (the box itself, or the query triangle's bounding box); overlaps(tri_geom_k, q) is the
// per-triangle rule, of which the gate is a necessary condition on the triangle's own bounding box (H1, T1).
// (collect_rows is that body with the traversal left to the caller: search(q, visit) calls visit(k) for every triangle that may pass
// `overlaps` -- overlap_rows' depth-first slot_walk on the query's box, or capsule_overlap_kernel's point_walk on a distance bound.)
template <class Query, class Args, class Load, class Overlaps, class Search>
EZD void collect_rows(const Args& a, Load load, Overlaps overlaps, Search search) {
  const uint32_t lane = threadIdx.x;
  const uint32_t i = blockIdx.x * CP_BLOCK + lane;
  const int K = a.K;
  int nb = 0;
  if (i < a.n) {
    Query q;
    const bool live = load(i, q);
    int32_t* ri = a.tri + (size_t)i * K;
    int32_t count = 0;
    int32_t last_id = -1; // entry K - 1 once the row is full (with K == 0 it is full now, and every id is greater than -1)
    auto put = [&](int j, int32_t id) {
      ri[j] = id;
      if (j == K - 1) last_id = id; // (a put to slot K - 1 happens only when the row is full)
    };
    auto visit = [&](int32_t k) {
      if (!overlaps(a.sc.tri_geom + (size_t)k * 3, q)) return;
      count++;
      if (nb == K && k > last_id) return; // behind a full row: counted only
      int j = nb < K ? nb++ : K - 1;
      while (j > 0) {
        const int32_t ip = ri[j - 1];
        if (ip < k) break;
        put(j, ip);
        j--;
      }
      put(j, k);
    };
    if (live) search(q, visit);
    if (a.n_overlap) a.n_overlap[i] = count;
  }
  // the wave's 64 rows, one flat run of 64 K words from its first row; the rows were written by other lanes of this wave, whose
  // accesses are performed in program order (the fence states it to the compiler and costs nothing at this scope)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const size_t base = (size_t)(i - lane) * K;
  for (uint32_t e = lane; e < 64u * (uint32_t)K; e += 64u) {
    const uint32_t row = fastdiv(e, a.div_k);
    const uint32_t slot = e - row * (uint32_t)K;
    const int used = __shfl(nb, (int)row);
    if (i - lane + row < a.n && slot >= (uint32_t)used) a.tri[base + e] = -1;
  }
}
// ---- overlap lists (include/ezrt_overlap_list.h): the fill side of count / offsets / fill.
//
// fill_rows is collect_rows for a row of the caller's length: lane i's row is tri[offsets[i] .. offsets[i + 1]), and it holds EVERY
// triangle that passes `overlaps`, not the lowest K.  load, overlaps and search are collect_rows' own, so a list kernel is its
// max_k sibling with other arguments (the *_body functions below serve both).  A row that is no row -- offsets[i] < 0, offsets[i + 1] <
// offsets[i] or offsets[i + 1] > capacity -- has length 0 here: the traversal still runs and counts (n_found reports the truth), and
// nothing is stored.  Every store is ri[j] with 0 <= j < len, so whatever the offsets say nothing outside a row that is valid and
// fits is written.
//   len <= OL_INSERT_MAX on the walk: collect_rows' insertion with K = len, the row sorted at every moment.  When the offsets are
//     the count's, the row is never full before the last overlap, so no id is dropped; when they are not (n_found != len) the row
//     keeps the lowest len ids met, inside itself.
//   longer rows on the walk: appended in the order of the visits while count < len, and sorted afterwards by overlap_sort_kernel.
//   the sweep visits ascending ids: every row is appended and none needs a sort.
// There is no wave-level row finish: a row has no unused slots when the offsets are the count's, and where they are not its contents
// are unspecified.  OL_INSERT_MAX and OL_TILE_MAX are what ezrt_overlap_list_limits reports (the macros exist for the measured
// comparison of DESIGN.md "Overlap lists": `make olvariants` builds those libraries under build_ab/, the product's build sets none
// of them, and tools/gpu_overlap_list_variants.sh runs the tests on the insert_max = 16 one -- EZRT_OL_SKIP_SORT leaves pass 2 out, so that
// tools/overlap_list_rates.py can time the fill kernel alone: such a library's long rows are unsorted, and it is never the product).
#ifndef EZRT_OL_SKIP_SORT
#define EZRT_OL_SKIP_SORT 0
#endif
#ifndef EZRT_OL_INSERT_MAX
#define EZRT_OL_INSERT_MAX 0 // measured (profiles/r25/overlap_list_rates.txt): appending and sorting beats the insertion at every row length
#endif
#ifndef EZRT_OL_TILE_MAX
#define EZRT_OL_TILE_MAX 4096
#endif
constexpr int OL_INSERT_MAX = EZRT_OL_INSERT_MAX; // rows up to this length are kept sorted while they are filled (0 .. 64)
constexpr int OL_TILE_MAX = EZRT_OL_TILE_MAX;     // rows up to this length are sorted in LDS (a power of two; 4 B each)
constexpr bool OL_SKIP_SORT = EZRT_OL_SKIP_SORT != 0;
static_assert(OL_INSERT_MAX >= 0 && OL_INSERT_MAX <= 64, "the insertion is collect_rows': K <= 64");
static_assert(OL_TILE_MAX > 64 && (OL_TILE_MAX & (OL_TILE_MAX - 1)) == 0 && OL_TILE_MAX * 4 < 64 * 1024, "a power of two inside 64 KiB");
struct OverlapList {
  const long long* offsets; // n + 1
  long long capacity;
  int32_t* tri;             // capacity
  int32_t* n_found;         // n, or null
};
// the row [base, base + len) that offsets[i], offsets[i + 1] and the capacity describe; (0, 0) when they describe none
EZD void list_row(long long o0, long long o1, long long capacity, long long& base, long long& len) {
  const bool ok = o0 >= 0 && o1 >= o0 && o1 <= capacity;
  base = ok ? o0 : 0;
  len = ok ? o1 - o0 : 0;
}
template <bool WALK, class Query, class Args, class Load, class Overlaps, class Search>
EZD void fill_rows(const Args& a, Load load, Overlaps overlaps, Search search) {
  const uint32_t i = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  Query q;
  const bool live = load(i, q);
  long long base, len;
  list_row(a.offsets[i], a.offsets[(size_t)i + 1], a.capacity, base, len);
  int32_t* ri = a.tri + base; // (not dereferenced when len == 0: tri may be null with capacity == 0)
  const bool sorted = WALK && len <= (long long)OL_INSERT_MAX;
  const int K = sorted ? (int)len : 0;
  int32_t count = 0;
  int nb = 0;
  int32_t last_id = -1; // collect_rows': entry K - 1 once the row is full
  auto put = [&](int j, int32_t id) {
    ri[j] = id;
    if (j == K - 1) last_id = id; // (a put to slot K - 1 happens only when the row is full)
  };
  auto visit = [&](int32_t k) {
    if (!overlaps(a.sc.tri_geom + (size_t)k * 3, q)) return;
    const int32_t c = count++;
    if (!sorted) {
      if ((long long)c < len) ri[c] = k;
      return;
    }
    if (nb == K && k > last_id) return; // behind a full row (offsets that are not the count's): counted only
    int j = nb < K ? nb++ : K - 1;
    while (j > 0) {
      const int32_t ip = ri[j - 1];
      if (ip < k) break;
      put(j, ip);
      j--;
    }
    put(j, k);
  };
  if (live) search(q, visit);
  if (a.n_found) a.n_found[i] = count;
}
// collect_rows for the max_k calls' arguments, fill_rows for a list's
template <bool WALK, class Query, class Args, class Load, class Overlaps, class Search>
EZD void rows(const Args& a, Load load, Overlaps overlaps, Search search) {
  if constexpr (__is_base_of(OverlapList, Args)) fill_rows<WALK, Query>(a, load, overlaps, search);
  else collect_rows<Query>(a, load, overlaps, search);
}
template <bool WALK, class Query, class Args, class Load, class Overlaps>
EZD void overlap_rows(const Args& a, int* __restrict__ lds_stack, Load load, Overlaps overlaps) {
  rows<WALK, Query>(a, load, overlaps, [&](const Query& q, auto& visit) {
    if (WALK) {
      const f3 &lo = q.lo, &hi = q.hi;
      slot_walk(
          a.sc.inner4, lds_stack + threadIdx.x,
          [&](const float4* rec, auto take) {
            const float4 ax = rec[N4_ROW_AA], ay = rec[N4_ROW_AA + 1], az = rec[N4_ROW_AA + 2], rf = rec[N4_ROW_REF];
            const float4 bx = rec[N4_ROW_BB], by = rec[N4_ROW_BB + 1], bz = rec[N4_ROW_BB + 2];
            auto pass = [&](float lx, float ly, float lz, float hx, float hy, float hz) {
              return [=, &lo, &hi] { return lx <= hi.x && hx >= lo.x && ly <= hi.y && hy >= lo.y && lz <= hi.z && hz >= lo.z; };
            };
            take(pass(ax.x, ay.x, az.x, bx.x, by.x, bz.x), __float_as_uint(rf.x));
            take(pass(ax.y, ay.y, az.y, bx.y, by.y, bz.y), __float_as_uint(rf.y));
            take(pass(ax.z, ay.z, az.z, bx.z, by.z, bz.z), __float_as_uint(rf.z));
            take(pass(ax.w, ay.w, az.w, bx.w, by.w, bz.w), __float_as_uint(rf.w));
          },
          visit);
#pragma unroll 1
      for (int u = 0; u < a.sc.n_uncovered; u++) visit(a.sc.uncovered[u]);
    } else {
#pragma unroll 1
      for (int k = 0; k < a.sc.n_tri; k++) visit(k);
    }
  });
}
struct BoxQuery {
  f3 lo, hi;
};
struct BoxOverlapListArgs : OverlapList {
  PointScene sc;
  const float* lo;          // n x 3
  const float* hi;          // n x 3
  uint32_t n;
};
template <bool WALK, class Args>
EZD void box_overlap_body(const Args& a, int* __restrict__ lds_stack) {
  overlap_rows<WALK, BoxQuery>(
      a, lds_stack,
      [&](uint32_t i, BoxQuery& q) {
        q.lo = ld3(a.lo + (size_t)i * 3), q.hi = ld3(a.hi + (size_t)i * 3);
        return box_live(q.lo, q.hi);
      },
      [](const float4* tg, const BoxQuery& q) { return box_overlaps(tg, q.lo, q.hi); });
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void box_overlap_kernel(BoxOverlapArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  box_overlap_body<WALK>(a, lds_stack);
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void box_overlap_list_kernel(BoxOverlapListArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  box_overlap_body<WALK>(a, lds_stack);
}

// ezrt_box_overlap_at_device: box_overlaps for pairs the caller holds -- box i against triangle tri_id[i].  An id outside the scene
// or a box that is not live writes 0.
__global__ __launch_bounds__(256) void box_overlap_at_kernel(const float4* tri_geom, int32_t n_tri, const float* box_lo, const float* box_hi,
                                                             const int32_t* tri_id, uint32_t n, uint8_t* overlaps) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  const f3 lo = ld3(box_lo + (size_t)i * 3), hi = ld3(box_hi + (size_t)i * 3);
  bool o = false;
  if (box_live(lo, hi) && (uint32_t)tri < (uint32_t)n_tri) o = box_overlaps(tri_geom + (size_t)tri * 3, lo, hi);
  overlaps[i] = o ? 1u : 0u;
}

// ---- triangle-overlap queries (include/ezrt_tri_overlap.h).
//
// tri_overlap_kernel<WALK>: one query triangle per lane, through overlap_rows as box_overlap_kernel: the gate of the walk is the query
// triangle's own fp32 bounding box -- by T1 an overlapping triangle's bounding box passes it, hence every box that holds the
// triangle -- and the per-triangle rule is tri_overlaps (ezrt_device.h: liveness, T1 and the 29 directions of T2).  A query triangle
// that is not live takes part with an empty row and a count of 0.
struct TriOverlapArgs {
  PointScene sc;
  const float* tris;        // n x 9
  uint32_t n;
  int32_t K;                // 0 .. 64
  FastDiv div_k;            // / max(K, 1) (the finishing pass)
  int32_t* tri;             // n x K (not read or written when K == 0)
  int32_t* n_overlap;       // n, or null
};
struct TriOverlapListArgs : OverlapList {
  PointScene sc;
  const float* tris;        // n x 9
  uint32_t n;
};
template <bool WALK, class Args>
EZD void tri_overlap_body(const Args& a, int* __restrict__ lds_stack) {
  overlap_rows<WALK, TriQuery>(
      a, lds_stack,
      [&](uint32_t i, TriQuery& q) {
        const float* t = a.tris + (size_t)i * 9;
        return tri_query(ld3(t), ld3(t + 3), ld3(t + 6), q);
      },
      [](const float4* tg, const TriQuery& q) { return tri_overlaps(tg, q); });
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void tri_overlap_kernel(TriOverlapArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  tri_overlap_body<WALK>(a, lds_stack);
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void tri_overlap_list_kernel(TriOverlapListArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  tri_overlap_body<WALK>(a, lds_stack);
}

// ezrt_tri_overlap_at_device: tri_overlaps for pairs the caller holds -- query triangle i against triangle tri_id[i].  An id outside
// the scene or a query triangle that is not live writes 0.
__global__ __launch_bounds__(256) void tri_overlap_at_kernel(const float4* tri_geom, int32_t n_tri, const float* tris, const int32_t* tri_id,
                                                             uint32_t n, uint8_t* overlaps) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  const float* t = tris + (size_t)i * 9;
  TriQuery q;
  bool o = false;
  if (tri_query(ld3(t), ld3(t + 3), ld3(t + 6), q) && (uint32_t)tri < (uint32_t)n_tri) o = tri_overlaps(tri_geom + (size_t)tri * 3, q);
  overlaps[i] = o ? 1u : 0u;
}

// ---- self-overlap queries (include/ezrt_self_overlap.h).
//
// self_overlap_kernel<WALK>: one triangle of the scene per lane -- triangle ids[i], or triangle i when ids is null -- through
// overlap_rows as tri_overlap_kernel: the gate of the walk is that triangle's own fp32 bounding box (T1 is part of the rule where the
// two triangles share nothing and holds by itself where they share a value), and the per-triangle rule is self_crosses (ezrt_device.h)
// for every triangle but the query's own.  An id outside the scene and a triangle that is not live take part with an empty row and a
// count of 0.
struct SelfQuery : TriQuery {
  int32_t id; // the query's own triangle
};
struct SelfOverlapArgs {
  PointScene sc;
  const int32_t* ids;       // n, or null: query i is triangle i
  uint32_t n;
  int32_t K;                // 0 .. 64
  FastDiv div_k;            // / max(K, 1) (the finishing pass)
  int32_t* tri;             // n x K (not read or written when K == 0)
  int32_t* n_overlap;       // n, or null
};
// triangle `id` of the scene as a query; false when the id is outside the scene or the triangle is not live
EZD bool self_query(const PointScene& sc, int32_t id, TriQuery& q) {
  if ((uint32_t)id >= (uint32_t)sc.n_tri) return false;
  const float4* g = sc.tri_geom + (size_t)id * 3;
  const float4 ga = g[0], gb = g[1], gc = g[2];
  return tri_query(mk(ga.x, ga.y, ga.z), mk(gb.x, gb.y, gb.z), mk(gc.x, gc.y, gc.z), q);
}
struct SelfOverlapListArgs : OverlapList {
  PointScene sc;
  const int32_t* ids;       // n, or null: query i is triangle i
  uint32_t n;
};
template <bool WALK, class Args>
EZD void self_overlap_body(const Args& a, int* __restrict__ lds_stack) {
  overlap_rows<WALK, SelfQuery>(
      a, lds_stack,
      [&](uint32_t i, SelfQuery& q) {
        q.id = a.ids ? a.ids[i] : (int32_t)i;
        return self_query(a.sc, q.id, q);
      },
      [&](const float4* tg, const SelfQuery& q) { return tg != a.sc.tri_geom + (size_t)q.id * 3 && self_crosses(tg, q); });
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void self_overlap_kernel(SelfOverlapArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  self_overlap_body<WALK>(a, lds_stack);
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void self_overlap_list_kernel(SelfOverlapListArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  self_overlap_body<WALK>(a, lds_stack);
}

// ezrt_self_overlap_at_device: self_crosses for pairs the caller holds -- triangle tri_a[i] against triangle tri_b[i].  An id outside
// the scene, equal ids and a triangle that is not live write 0.
__global__ __launch_bounds__(256) void self_overlap_at_kernel(PointScene sc, const int32_t* tri_a, const int32_t* tri_b, uint32_t n,
                                                              uint8_t* crosses) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t ta = tri_a[i], tb = tri_b[i];
  TriQuery q;
  bool o = false;
  if (ta != tb && (uint32_t)tb < (uint32_t)sc.n_tri && self_query(sc, ta, q)) o = self_crosses(sc.tri_geom + (size_t)tb * 3, q);
  crosses[i] = o ? 1u : 0u;
}

// ---- triangle-distance queries (include/ezrt_tri_distance.h).
//
// tri_distance_kernel<WALK>: one query triangle per lane.  WALK = true, the pruned route: point_walk on the lane's stack column of
// 2 * (stack_need_cp + 1) rows, with the running best dist2 as the radius (RECHECK) and, as the lower bound of a slot's box [lo, hi],
// tri_distance_box against the query triangle's own fp32 bounding box [q.lo, q.hi]: lb = dot(g, g), g = max(lo - q.hi, 0, q.lo - hi).
// Why no margin is needed: every x of tri_distance_pair is a vertex of Q or a point clamped to the bounding box of Q or of one of its
// edges, so x lies in [q.lo, q.hi] per axis; every y is a vertex of the scene triangle or clamped to its bounding box or an edge's,
// which lies in every box above the triangle (the scene prunes).  Per axis either g = 0 <= |e|, or g = fl(lo - q.hi) with
// y >= lo > q.hi >= x: y - x >= lo - q.hi in the reals, rounding is monotone and |fl(x - y)| = fl(y - x), so |e| >= g (the same on
// the other side).  fl(x * x) is monotone in |x| and fl(fl(X + Y) + Z) in each of X, Y, Z >= 0, so lb <= d2 ON THE BITS for every
// finite sub-candidate, overflow included, hence lb <= the smallest of them; and a pair that crosses (dist2 = 0) passes T1, so its
// boxes overlap on every axis and lb = 0.  A skipped subtree therefore holds no pair with dist2 <= radius, neither a winner nor a tie.
// The pair gate: before the 15 sub-candidates and the fp64 tri_overlaps, the same lb of triangle k's OWN bounding box; a triangle
// with lb > best cannot win or tie, by the same inequality, so skipping it changes no result.  (A NaN lb -- a NaN vertex -- fails the
// comparison and goes on to tri_distance_pair, which finds the triangle not live.)
// Triangles that no leaf holds are swept after the walk.  WALK = false, the sweep route: every triangle, no tree.
struct TriDistanceArgs {
  PointScene sc;
  const float* tris;        // n x 9
  const float* d_max;       // n, or null
  uint32_t n;
  int32_t* tri;             // n
  float* dist;              // n, or null
  float* point_query;       // n x 3, or null
  float* point_scene;       // n x 3, or null
  uint8_t* crosses;         // n, or null
};
// row i of the outputs; tri < 0 writes the miss (-1, +inf, zeros, zeros, 0: the caller keeps x, y and crosses zero then)
EZD void tri_distance_store(float* dist, float* point_query, float* point_scene, uint8_t* crosses, uint32_t i, const TriDistanceBest& r) {
  if (dist) dist[i] = r.tri >= 0 ? __builtin_sqrtf(r.best) : __builtin_inff();
  if (point_query) st3(point_query + (size_t)i * 3, r.x);
  if (point_scene) st3(point_scene + (size_t)i * 3, r.y);
  if (crosses) crosses[i] = r.crosses ? 1u : 0u;
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void tri_distance_kernel(TriDistanceArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const uint32_t i = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const float* t = a.tris + (size_t)i * 9;
  const f3 p1 = ld3(t), p2 = ld3(t + 3), p3 = ld3(t + 6);
  TriDistanceBest r;
  r.tri = -1;
  r.x = r.y = mk(0.0f, 0.0f, 0.0f);
  r.crosses = false;
  r.best = __builtin_inff();
  bool live = true;
  if (a.d_max) { // B = d_max^2; a negative or NaN d_max gives no candidates
    const float dm = a.d_max[i];
    if (dm >= 0.0f) r.best = dm * dm;
    else live = false;
  }
  TriQuery q;
  if (live && tri_query(p1, p2, p3, q))
    bound_visit<WALK, true>(
        a.sc, [&](f3 lo, f3 hi) { return tri_distance_box(q.lo, q.hi, lo, hi); }, lds_stack + threadIdx.x, [&] { return r.best; },
        [&](int32_t k) {
          const float4* g = a.sc.tri_geom + (size_t)k * 3;
          const float4 ga = g[0], gb = g[1], gc = g[2];
          const f3 lo = mk(ez_min(ez_min(ga.x, gb.x), gc.x), ez_min(ez_min(ga.y, gb.y), gc.y), ez_min(ez_min(ga.z, gb.z), gc.z));
          const f3 hi = mk(ez_max(ez_max(ga.x, gb.x), gc.x), ez_max(ez_max(ga.y, gb.y), gc.y), ez_max(ez_max(ga.z, gb.z), gc.z));
          if (tri_distance_box(q.lo, q.hi, lo, hi) > r.best) return; // the pair gate
          tri_distance_candidate(r, a.sc.tri_geom, k, q, p1, p2, p3);
        });
  a.tri[i] = r.tri;
  tri_distance_store(a.dist, a.point_query, a.point_scene, a.crosses, i, r);
}

// ezrt_tri_distance_at_device: tri_distance_pair for pairs the caller holds -- query triangle i against triangle tri_id[i].  An id
// outside the scene, a triangle that is not live on either side or a pair without a finite sub-candidate writes (+inf, zeros, zeros, 0).
__global__ __launch_bounds__(256) void tri_distance_at_kernel(const float4* tri_geom, int32_t n_tri, const float* tris, const int32_t* tri_id,
                                                              uint32_t n, float* dist, float* point_query, float* point_scene, uint8_t* crosses) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  const float* t = tris + (size_t)i * 9;
  const f3 p1 = ld3(t), p2 = ld3(t + 3), p3 = ld3(t + 6);
  TriDistanceBest r;
  r.tri = -1;
  r.x = r.y = mk(0.0f, 0.0f, 0.0f);
  r.crosses = false;
  r.best = __builtin_inff();
  TriQuery q;
  if ((uint32_t)tri < (uint32_t)n_tri && tri_query(p1, p2, p3, q)) tri_distance_candidate(r, tri_geom, tri, q, p1, p2, p3);
  tri_distance_store(dist, point_query, point_scene, crosses, i, r);
}

// ---- sphere-cast queries (include/ezrt_sphere_cast.h).
//
// sphere_cast_kernel<WALK>: one query per lane, two walks on the lane's stack column of 2 * (stack_need_cp + 1) rows (each leaves
// nothing pending).  First closest_point_search with d_max = the radius (B = r * r): a winner is the touching answer.  Otherwise
// point_walk once more, with t in the place of dist2: the radius is t_max (+inf when NULL) until a candidate is found and the best t
// from then on (RECHECK), and the lower bound of a slot's box [lo, hi] is sphere_cast_box -- tnear of the slab test of the ray against
// the box inflated by r where tnear <= tfar, else +inf (never descended).
// Why no margin is needed: for a box [L, H] that holds [l, h], L <= l and H >= h per axis.  Every step of near and far is monotone
// under rounding: fl(L - r) <= fl(l - r) and fl(H + r) >= fl(h + r); subtracting o keeps the order; multiplying by inv, a constant of
// fixed sign, keeps it (inv > 0) or turns it (inv < 0, where the two are swapped); max and min keep it.  So tnear(outer) <= tnear(inner)
// and tfar(outer) >= tfar(inner) ON THE BITS; a flat axis that passes l - r <= o <= h + r passes the wider test; hence an outer box
// passes whenever an inner one does.  NaN and infinity: o, r and inv are finite and inv != 0, so 0 * inf cannot arise; a difference
// that overflows (l - r = -inf, (l - r) - o, the product) is an infinity of the right sign and stays ordered; inf - inf cannot arise
// from a finite o; a NaN bound of a box constrains nothing, which only widens.  The pair's t is max(its smallest sub-candidate,
// tnear of the triangle's own bounding box), so tnear(any box above T) <= tnear(T) <= t(pair): a subtree skipped at lb > radius holds
// neither a winner nor a tie, and on equality it is descended.  The pair gate: sphere_cast_pair runs the same slab test on the
// triangle's own bounding box before its seven sub-candidates and leaves a pair whose tnear exceeds the best t of the moment.
// Triangles that no leaf holds are swept after each walk.  WALK = false, the sweep route: every triangle, no tree, twice.
struct SphereCastArgs {
  ClosestPointArgs cp;      // sc, d_max = the radii, n, tri, point (points, dist and bary unused)
  const float* rays;        // n x 6
  const float* t_max;       // n, or null
  float* t;                 // n, or null
  uint8_t* touching;        // n, or null
};
// row i of the outputs; tri < 0 writes the miss (+inf, zeros, 0: the caller keeps point zero and touching false then)
EZD void sphere_cast_store(float* t, float* point, uint8_t* touching, uint32_t i, const SphereBest& r) {
  if (t) t[i] = r.tri >= 0 ? r.t : __builtin_inff();
  if (point) st3(point + (size_t)i * 3, r.point);
  if (touching) touching[i] = r.touching ? 1u : 0u;
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void sphere_cast_kernel(SphereCastArgs sa) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const ClosestPointArgs& a = sa.cp;
  const uint32_t i = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const float* ray = sa.rays + (size_t)i * 6;
  int* stack = lds_stack + threadIdx.x;
  SphereBest r;
  r.tri = -1;
  r.point = mk(0.0f, 0.0f, 0.0f);
  r.touching = false;
  r.t = __builtin_inff();
  SphereRay q;
  if (sphere_cast_live(ld3(ray), ld3(ray + 3), a.d_max[i], q)) {
    const ClosestBest c = closest_point_search<WALK>(a, i, q.o, stack);
    if (c.tri >= 0) {
      r.tri = c.tri, r.t = 0.0f, r.point = c.q, r.touching = true;
    } else {
      const float tm = sa.t_max ? sa.t_max[i] : __builtin_inff();
      if (tm >= 0.0f) { // (a negative or NaN t_max gives no candidates)
        r.t = tm;
        bound_visit<WALK, true>(
            a.sc, [&](f3 lo, f3 hi) { return sphere_cast_box(q, lo, hi); }, stack, [&] { return r.t; },
            [&](int32_t k) { sphere_cast_candidate(r, a.sc.tri_geom, k, q); });
      }
    }
  }
  a.tri[i] = r.tri;
  sphere_cast_store(sa.t, a.point, sa.touching, i, r);
}

// ezrt_sphere_cast_at_device: sphere_cast_at for pairs the caller holds -- query i against triangle tri_id[i].  An id outside the
// scene, a query or a triangle that is not live or a pair that is no candidate writes (+inf, zeros, 0).
__global__ __launch_bounds__(256) void sphere_cast_at_kernel(const float4* tri_geom, int32_t n_tri, const float* rays, const float* radius,
                                                             const int32_t* tri_id, uint32_t n, float* t, float* point, uint8_t* touching) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  const float* ray = rays + (size_t)i * 6;
  SphereBest r;
  r.tri = -1;
  r.point = mk(0.0f, 0.0f, 0.0f);
  r.touching = false;
  r.t = __builtin_inff();
  SphereRay q;
  if ((uint32_t)tri < (uint32_t)n_tri && sphere_cast_live(ld3(ray), ld3(ray + 3), radius[i], q)) sphere_cast_at(r, tri_geom, tri, q);
  sphere_cast_store(t, point, touching, i, r);
}

// ---- segment queries (include/ezrt_segment.h).
//
// segment_distance_kernel<WALK>: one query segment per lane, as tri_distance_kernel: point_walk on the lane's stack column of
// 2 * (stack_need_cp + 1) rows with the running best dist2 as the radius (RECHECK) and tri_distance_box against the segment's own fp32
// bounding box [qlo, qhi] = [min(a, b), max(a, b)] as the lower bound of a slot's box.
// Why no margin is needed, for THIS rule: every x of segment_pair is an end point -- a corner of [qlo, qhi] per axis -- or comes
// out of seg_point(a, b, ..), which clamps it into [min(a, b), max(a, b)] = [qlo, qhi]; every y is closest_point_abc's q, clamped to the
// triangle's bounding box, or seg_point's of an edge, clamped to the edge's box, which lies in the triangle's; and the triangle's box
// lies in every box above it (the scene prunes).  Per axis either g = 0 <= |e|, or g = fl(lo - qhi) with y >= lo > qhi >= x: y - x >=
// lo - qhi in the reals, rounding is monotone and |fl(x - y)| = fl(y - x), so |e| >= g (the same on the other side).  fl(x * x) is
// monotone in |x| and fl(fl(X + Y) + Z) in each of X, Y, Z >= 0, so lb <= d2 ON THE BITS for each of the five sub-candidates with a
// finite d2, overflow included, hence lb <= their smallest.  A pair that crosses has dist2 = 0 -- and passes T1, which is why T1 is in
// the rule: its boxes overlap on every axis, g = 0 on each and lb = 0.  A skipped subtree therefore holds no pair with dist2 <=
// radius, neither a winner nor a tie.  The pair gate: the same lb of triangle k's OWN bounding box (segment_gate) before the five
// sub-candidates and the fp64 test; a triangle with lb > best can neither win nor tie.
// Triangles that no leaf holds are swept after the walk.  WALK = false, the sweep route: every triangle, no tree.
struct SegmentDistanceArgs {
  PointScene sc;
  const float* segs;        // n x 6: a, b
  const float* d_max;       // n, or null
  uint32_t n;
  int32_t* tri;             // n
  float* dist;              // n, or null
  float* point_query;       // n x 3, or null
  float* point_scene;       // n x 3, or null
  uint8_t* crosses;         // n, or null
};
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void segment_distance_kernel(SegmentDistanceArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  const uint32_t i = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const float* t = a.segs + (size_t)i * 6;
  TriDistanceBest r;
  r.tri = -1;
  r.x = r.y = mk(0.0f, 0.0f, 0.0f);
  r.crosses = false;
  r.best = __builtin_inff();
  bool live = true;
  if (a.d_max) { // B = d_max^2; a negative or NaN d_max gives no candidates
    const float dm = a.d_max[i];
    if (dm >= 0.0f) r.best = dm * dm;
    else live = false;
  }
  SegQuery q;
  if (live && segment_query(ld3(t), ld3(t + 3), q))
    bound_visit<WALK, true>(
        a.sc, [&](f3 lo, f3 hi) { return tri_distance_box(q.qlo, q.qhi, lo, hi); }, lds_stack + threadIdx.x, [&] { return r.best; },
        [&](int32_t k) {
          if (segment_gate(a.sc.tri_geom + (size_t)k * 3, q) > r.best) return; // the pair gate
          segment_candidate(r, a.sc.tri_geom, k, q);
        });
  a.tri[i] = r.tri;
  tri_distance_store(a.dist, a.point_query, a.point_scene, a.crosses, i, r);
}

// ezrt_segment_distance_at_device: segment_pair for pairs the caller holds -- query segment i against triangle tri_id[i], no gate.  An
// id outside the scene, a segment or a triangle that is not live or a pair without a finite sub-candidate writes (+inf, zeros, zeros, 0).
__global__ __launch_bounds__(256) void segment_distance_at_kernel(const float4* tri_geom, int32_t n_tri, const float* segs, const int32_t* tri_id,
                                                                  uint32_t n, float* dist, float* point_query, float* point_scene, uint8_t* crosses) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  const float* t = segs + (size_t)i * 6;
  TriDistanceBest r;
  r.tri = -1;
  r.x = r.y = mk(0.0f, 0.0f, 0.0f);
  r.crosses = false;
  r.best = __builtin_inff();
  SegQuery q;
  if ((uint32_t)tri < (uint32_t)n_tri && segment_query(ld3(t), ld3(t + 3), q)) segment_candidate(r, tri_geom, tri, q);
  tri_distance_store(dist, point_query, point_scene, crosses, i, r);
}

// capsule_overlap_kernel<WALK>: one capsule per lane; the list, the count and the wave's row finish are collect_rows', as for the
// other overlap kernels.  What differs is the traversal: the rule is a distance (dist2 <= R2, R2 = radius * radius), so the walk is
// bound_visit's point_walk with the CONSTANT radius R2 (no RECHECK: an entry passed at its push) and, as in segment_distance_kernel,
// tri_distance_box against the segment's bounding box as the bound: a slot is descended when lb <= R2.  lb <= dist2 on the bits
// (above) makes that a necessary condition with no slack.  The segment's box is NOT inflated by the radius: fl(qhi + r) can round
// below qhi + r, and a triangle's box between the two would be cut off although its dist2 <= R2.  An unused slot (an all-NaN box)
// gets lb = +inf in point_walk, which is never descended, whatever R2 is -- +inf included.  The same lb of the triangle's own box
// gates the pair.  Launched with point_walk's column of 2 * (stack_need_cp + 1) rows.
struct CapsuleQuery : SegQuery {
  float R2;
};
struct CapsuleOverlapArgs {
  PointScene sc;
  const float* segs;        // n x 6: a, b
  const float* radius;      // n
  uint32_t n;
  int32_t K;                // 0 .. 64
  FastDiv div_k;            // / max(K, 1) (the finishing pass)
  int32_t* tri;             // n x K (not read or written when K == 0)
  int32_t* n_overlap;       // n, or null
};
struct CapsuleOverlapListArgs : OverlapList {
  PointScene sc;
  const float* segs;        // n x 6: a, b
  const float* radius;      // n
  uint32_t n;
};
template <bool WALK, class Args>
EZD void capsule_overlap_body(const Args& a, int* __restrict__ lds_stack) {
  rows<WALK, CapsuleQuery>(
      a,
      [&](uint32_t i, CapsuleQuery& q) {
        const float* t = a.segs + (size_t)i * 6;
        const float r = a.radius[i];
        q.R2 = r * r;
        return r >= 0.0f && r < __builtin_inff() && segment_query(ld3(t), ld3(t + 3), q); // (false for a NaN radius)
      },
      [](const float4* tg, const CapsuleQuery& q) {
        if (segment_gate(tg, q) > q.R2) return false; // the pair gate
        f3 x, y;
        float d2;
        bool crosses;
        return segment_pair(tg, q.a, q.b, q.lo, q.hi, d2, x, y, crosses) && d2 <= q.R2;
      },
      [&](const CapsuleQuery& q, auto& visit) {
        bound_visit<WALK, false>(
            a.sc, [&](f3 lo, f3 hi) { return tri_distance_box(q.qlo, q.qhi, lo, hi); }, lds_stack + threadIdx.x, [&] { return q.R2; }, visit);
      });
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void capsule_overlap_kernel(CapsuleOverlapArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  capsule_overlap_body<WALK>(a, lds_stack);
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void capsule_overlap_list_kernel(CapsuleOverlapListArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  capsule_overlap_body<WALK>(a, lds_stack);
}

// ---- oriented-box queries (include/ezrt_obb_overlap.h).
//
// obb_overlap_kernel<WALK>: one box per lane; the list, the count and the wave's row finish are collect_rows', as for the other
// overlap kernels, and the traversal is slot_walk directly -- overlap_rows is not widened: its gate is one fp32 box, this one has two.
// A slot is descended when it passes both, the second asked only behind the first:
//   1. the hull, by H0: slot.lo[c] <= hull_hi[c] && slot.hi[c] >= hull_lo[c] -- overlap_rows' six fp32 comparisons, against the hull
//      rounded inward once per box (obb_query), which compares as the fp64 hull does.  An unused slot (an all-NaN box) fails here.
//   2. the three face directions (obb_face_gate): p_j by the rule's own expression at the slot's corners chosen per component by the
//      sign of n_j[c]; the slot is left when pmin > r_j || pmax < -r_j.
// Why no margin is needed: by H0 an overlapping triangle's own bounding box passes 1, hence every box that holds the triangle (the
// scene prunes).  For 2, rounding to nearest is monotone, and d(x, c), a product with a fixed factor and a sum are each monotone in
// each operand: pmin <= p_j(v) <= pmax ON THE BITS for every fp32 point v in the slot's box, so with pmin > r_j no vertex below the
// slot has p_j <= r_j, and with pmax < -r_j none has p_j >= -r_j -- every triangle below it fails H1.  A NaN (0 times an infinite
// bound) fails both comparisons and the slot is descended.  Triangles that no leaf holds are swept after the walk.  WALK = false,
// the sweep route: every triangle, no tree.  Both call obb_overlaps (ezrt_device.h: H0 .. H3 of the header) with the numbers of the
// box -- n_j, r_j, the hull -- computed once, in obb_query.  Launched with slot_walk's column of stack_need_cp + 1 rows.
struct ObbOverlapArgs {
  PointScene sc;
  const float* centre;      // n x 3
  const float* axes;        // n x 9: u0 u1 u2
  uint32_t n;
  int32_t K;                // 0 .. 64
  FastDiv div_k;            // / max(K, 1) (the finishing pass)
  int32_t* tri;             // n x K (not read or written when K == 0)
  int32_t* n_overlap;       // n, or null
};
EZD bool obb_load(const float* centre, const float* axes, uint32_t i, ObbQuery& q) {
  const float* u = axes + (size_t)i * 9;
  return obb_query(ld3(centre + (size_t)i * 3), ld3(u), ld3(u + 3), ld3(u + 6), q);
}
struct ObbOverlapListArgs : OverlapList {
  PointScene sc;
  const float* centre;      // n x 3
  const float* axes;        // n x 9: u0 u1 u2
  uint32_t n;
};
template <bool WALK, class Args>
EZD void obb_overlap_body(const Args& a, int* __restrict__ lds_stack) {
  rows<WALK, ObbQuery>(
      a, [&](uint32_t i, ObbQuery& q) { return obb_load(a.centre, a.axes, i, q); },
      [](const float4* tg, const ObbQuery& q) { return obb_overlaps(tg, q); },
      [&](const ObbQuery& q, auto& visit) {
        if (WALK) {
          slot_walk(
              a.sc.inner4, lds_stack + threadIdx.x,
              [&](const float4* rec, auto take) {
                const float4 ax = rec[N4_ROW_AA], ay = rec[N4_ROW_AA + 1], az = rec[N4_ROW_AA + 2], rf = rec[N4_ROW_REF];
                const float4 bx = rec[N4_ROW_BB], by = rec[N4_ROW_BB + 1], bz = rec[N4_ROW_BB + 2];
                auto pass = [&](float lx, float ly, float lz, float hx, float hy, float hz) {
                  return [=, &q] {
                    const f3 lo = mk(lx, ly, lz), hi = mk(hx, hy, hz);
                    return obb_hull_gate(q, lo, hi) && obb_face_gate(q, lo, hi);
                  };
                };
                take(pass(ax.x, ay.x, az.x, bx.x, by.x, bz.x), __float_as_uint(rf.x));
                take(pass(ax.y, ay.y, az.y, bx.y, by.y, bz.y), __float_as_uint(rf.y));
                take(pass(ax.z, ay.z, az.z, bx.z, by.z, bz.z), __float_as_uint(rf.z));
                take(pass(ax.w, ay.w, az.w, bx.w, by.w, bz.w), __float_as_uint(rf.w));
              },
              visit);
#pragma unroll 1
          for (int u = 0; u < a.sc.n_uncovered; u++) visit(a.sc.uncovered[u]);
        } else {
#pragma unroll 1
          for (int k = 0; k < a.sc.n_tri; k++) visit(k);
        }
      });
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void obb_overlap_kernel(ObbOverlapArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  obb_overlap_body<WALK>(a, lds_stack);
}
template <bool WALK>
__global__ __launch_bounds__(CP_BLOCK) void obb_overlap_list_kernel(ObbOverlapListArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds_stack[];
  obb_overlap_body<WALK>(a, lds_stack);
}

// overlap_sort_kernel: pass 2 of a list call on the walk route -- in place, ascending, every row that is longer than OL_INSERT_MAX,
// valid and inside the capacity (fill_rows appended it in the order of the visits).  A workgroup of OL_SORT_BLOCK threads has
// OL_SORT_ROWS consecutive rows: its first OL_SORT_ROWS + 1 threads load one offset each into LDS, and a workgroup whose rows need
// nothing ends there.  The rows that need it are sorted one after the other by the whole workgroup, by the bitonic network in its
// one-direction form: stage h = 1, 2, 4, .. < len first compares i with its mirror in its block of 2 h (i ^ (2 h - 1)), then i with
// i + g for g = h / 2 .. 1, always the lower id to the lower index.  Every comparison points the same way, so a length that is no
// power of two is padded with +inf that never moves: a pair whose upper index is >= len is skipped, and nothing is stored.
//   len <= OL_TILE_MAX: the row is copied to LDS, sorted there and copied back.
//   longer rows stay in global memory, no second buffer: the steps of distance < OL_TILE_MAX act inside aligned chunks of
//     OL_TILE_MAX entries and are run chunk by chunk in LDS; only the steps of distance >= OL_TILE_MAX go through global memory,
//     with a barrier after each (the row belongs to this workgroup alone, and __syncthreads orders its global accesses).
// A row longer than the scene has triangles is no count's row; it is left as it is (its contents are unspecified) instead of
// being sorted for the time its length would take.  Indices: i < l < len <= n_tri < 2^31 in 32 bits, the row's base in 64.
constexpr int OL_SORT_BLOCK = 256, OL_SORT_ROWS = 16;
struct OverlapSortArgs {
  const long long* offsets; // n + 1
  long long capacity;
  int32_t* tri;             // capacity
  uint32_t n;
  int32_t n_tri;
};
// one step on p[0 .. m): thread t of the workgroup takes the pairs t, t + OL_SORT_BLOCK, ..; pair u of half-block h is
// i = 2 h (u / h) + u % h and l = i ^ (2 h - 1) (flip) or i + h
EZD void ol_step(int32_t* p, uint32_t m, uint32_t h, bool flip, uint32_t t) {
  for (uint32_t u = t; u < m; u += OL_SORT_BLOCK) { // (i >= u: no pair is lost, and 2 u does not wrap)
    const uint32_t i = ((u & ~(h - 1u)) << 1) | (u & (h - 1u));
    if (i >= m) break;
    const uint32_t l = flip ? i ^ (2u * h - 1u) : i | h;
    if (l < m) {
      const int32_t x = p[i], y = p[l];
      if (y < x) p[i] = y, p[l] = x;
    }
  }
}
// every stage of the network on p[0 .. m), m <= OL_TILE_MAX (LDS)
EZD void ol_sort_tile(int32_t* p, uint32_t m, uint32_t t) {
  for (uint32_t h = 1; h < m; h <<= 1) {
    ol_step(p, m, h, true, t);
    __syncthreads();
    for (uint32_t g = h >> 1; g > 0; g >>= 1) {
      ol_step(p, m, g, false, t);
      __syncthreads();
    }
  }
}
__global__ __launch_bounds__(OL_SORT_BLOCK) void overlap_sort_kernel(OverlapSortArgs a) {
  __shared__ int32_t tile[OL_TILE_MAX];
  __shared__ long long off[OL_SORT_ROWS + 1];
  const uint32_t t = threadIdx.x;
  const size_t i0 = (size_t)blockIdx.x * OL_SORT_ROWS;
  if (t <= (uint32_t)OL_SORT_ROWS) off[t] = i0 + t <= (size_t)a.n ? a.offsets[i0 + t] : -1;
  __syncthreads();
  for (int r = 0; r < OL_SORT_ROWS; r++) { // (every condition below is uniform across the workgroup)
    if (i0 + (size_t)r >= (size_t)a.n) break;
    long long base, len;
    list_row(off[r], off[r + 1], a.capacity, base, len);
    if (len <= (long long)(OL_INSERT_MAX > 1 ? OL_INSERT_MAX : 1) || len > (long long)a.n_tri) continue;
    int32_t* row = a.tri + base;
    const uint32_t m = (uint32_t)len;
    if (m <= (uint32_t)OL_TILE_MAX) {
      for (uint32_t e = t; e < m; e += OL_SORT_BLOCK) tile[e] = row[e];
      __syncthreads();
      ol_sort_tile(tile, m, t);
      for (uint32_t e = t; e < m; e += OL_SORT_BLOCK) row[e] = tile[e];
      __syncthreads(); // the tile is the next row's
      continue;
    }
    // chunk by chunk: all stages below OL_TILE_MAX (first) or the steps of distance < OL_TILE_MAX of a later stage
    auto chunks = [&](bool first) {
      for (uint32_t c = 0; c < m; c += (uint32_t)OL_TILE_MAX) {
        const uint32_t cm = m - c < (uint32_t)OL_TILE_MAX ? m - c : (uint32_t)OL_TILE_MAX;
        for (uint32_t e = t; e < cm; e += OL_SORT_BLOCK) tile[e] = row[c + e];
        __syncthreads();
        if (first) {
          ol_sort_tile(tile, cm, t);
        } else {
          for (uint32_t g = (uint32_t)OL_TILE_MAX >> 1; g > 0; g >>= 1) {
            ol_step(tile, cm, g, false, t);
            __syncthreads();
          }
        }
        for (uint32_t e = t; e < cm; e += OL_SORT_BLOCK) row[c + e] = tile[e];
        __syncthreads();
      }
    };
    chunks(true);
    for (uint32_t h = (uint32_t)OL_TILE_MAX; h < m; h <<= 1) {
      ol_step(row, m, h, true, t);
      __syncthreads();
      for (uint32_t g = h >> 1; g >= (uint32_t)OL_TILE_MAX; g >>= 1) {
        ol_step(row, m, g, false, t);
        __syncthreads();
      }
      chunks(false);
    }
  }
}

// ezrt_obb_overlap_at_device: obb_overlaps for pairs the caller holds -- box i against triangle tri_id[i].  An id outside the scene
// or a box that is not live writes 0.
__global__ __launch_bounds__(256) void obb_overlap_at_kernel(const float4* tri_geom, int32_t n_tri, const float* centre, const float* axes,
                                                             const int32_t* tri_id, uint32_t n, uint8_t* overlaps) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  ObbQuery q;
  bool o = false;
  if ((uint32_t)tri < (uint32_t)n_tri && obb_load(centre, axes, i, q)) o = obb_overlaps(tri_geom + (size_t)tri * 3, q);
  overlaps[i] = o ? 1u : 0u;
}

// ---- winding-number queries (include/ezrt_winding.h).
//
// winding_kernel<ATOMIC, TILE>: one point per lane, a workgroup of one wave; the grid is (point blocks) x (slices of the triangle
// range), and every lane of a workgroup loops over the same slice [blockIdx.y * per_slice, ...) and keeps its sum S in a 64-bit
// register pair.  An exact sum has nothing to prune: no tree is read, only tri_geom, and there is no stack.  ATOMIC = false, one
// slice: S is stored to fixed and, where asked for, converted to winding.  ATOMIC = true: the host zeroed fixed on the stream, every
// workgroup adds its partial sum with a 64-bit integer atomicAdd (an integer sum: the order costs no bit), and
// winding_finish_kernel converts afterwards.
// Reading the triangles.  TILE = true (the default): each lane sorts ONE triangle of a tile of WN_BLOCK (W1: winding_tri) and writes
// its WindingTri to LDS; the wave then reads the tile entry by entry at one address for all lanes, a broadcast without bank
// conflicts -- W1 costs each pair 1/64 of a lane's evaluation.  TILE = false, the alternative kept for measuring
// (EZRT_WINDING_SCALAR=1, read once per process): the triangle index is the loop counter, bounded by kernel arguments -- uniform
// across the wave, so the 48-byte record is read with scalar loads (s_load_dwordx8 + x4) into SGPRs; but gfx950 has no scalar
// floating-point compare or convert, so W1 is then evaluated by every wave for every triangle in the vector unit on uniform values,
// which costs about a quarter of the pair's time (profiles/r23/winding_rates.txt).  Both evaluate winding_tri and winding_term
// (ezrt_device.h) and give the same bits.
constexpr int WN_BLOCK = 64;
struct WindingArgs {
  const float4* tri_geom;
  int32_t n_tri;
  int32_t per_slice;        // triangles per slice: ceil(n_tri / slices)
  const float* points;      // n x 3
  uint32_t n;
  long long* fixed;         // n
  float* winding;           // n, or null (ATOMIC: written by winding_finish_kernel)
};
template <bool ATOMIC, bool TILE>
__global__ __launch_bounds__(WN_BLOCK) void winding_kernel(WindingArgs a) {
  const uint32_t i = blockIdx.x * WN_BLOCK + threadIdx.x;
  const int32_t k0 = (int32_t)blockIdx.y * a.per_slice;
  const int32_t k1 = a.n_tri - k0 < a.per_slice ? a.n_tri : k0 + a.per_slice;
  const float inf = __builtin_inff();
  f3 p = mk(0.0f, 0.0f, 0.0f);
  if (i < a.n) p = ld3(a.points + (size_t)i * 3);
  const bool live = i < a.n && ez_abs(p.x) < inf && ez_abs(p.y) < inf && ez_abs(p.z) < inf; // a non-finite p: S = 0
  const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
  long long S = 0;
  if (TILE) {
    __shared__ WindingTri tile[WN_BLOCK];
#pragma unroll 1
    for (int32_t base = k0; base < k1; base += WN_BLOCK) {
      const int32_t k = base + (int32_t)threadIdx.x;
      if (k < k1) winding_tri(a.tri_geom + (size_t)k * 3, tile[threadIdx.x]);
      __syncthreads();
      const int32_t m = k1 - base < WN_BLOCK ? k1 - base : WN_BLOCK;
      if (live) {
#pragma unroll 1
        for (int32_t j = 0; j < m; j++) {
          const WindingTri w = tile[j];
          if (w.sgn != 0.0f) S += winding_term(w, px, py, pz);
        }
      }
      __syncthreads();
    }
  } else if (live) {
#pragma unroll 1
    for (int32_t k = k0; k < k1; k++) {
      WindingTri w;
      winding_tri(a.tri_geom + (size_t)k * 3, w);
      if (w.sgn != 0.0f) S += winding_term(w, px, py, pz);
    }
  }
  if (i >= a.n) return;
  if (ATOMIC) {
    if (S != 0) atomicAdd((unsigned long long*)(a.fixed + i), (unsigned long long)S); // two's complement: the signed sum
  } else {
    a.fixed[i] = S;
    if (a.winding) a.winding[i] = winding_of(S);
  }
}
__global__ __launch_bounds__(256) void winding_finish_kernel(const long long* fixed, uint32_t n, float* winding) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) winding[i] = winding_of(fixed[i]);
}

// ezrt_winding_at_device: winding_pair for pairs the caller holds -- point i against triangle tri_id[i].  An id outside the scene
// writes 0.
__global__ __launch_bounds__(256) void winding_at_kernel(const float4* tri_geom, int32_t n_tri, const float* points, const int32_t* tri_id,
                                                         uint32_t n, long long* fixed, float* winding) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  long long q = 0;
  if ((uint32_t)tri < (uint32_t)n_tri) q = winding_pair(tri_geom + (size_t)tri * 3, ld3(points + (size_t)i * 3));
  fixed[i] = q;
  if (winding) winding[i] = winding_of(q);
}

// ---- plane queries (include/ezrt_plane.h).
//
// plane_kernel<FILL>: a workgroup of one wave per (tile of PL_TILE planes, slice of the triangle range): the grid is (tiles) x
// (slices).  The tile's planes are converted once (plane_load) into LDS, one per lane, and read from there at one address for all
// lanes -- a broadcast without bank conflicts.  The wave then goes through its slice in rounds of 64 triangles: each lane converts ONE
// triangle to nine doubles, and for every plane of the tile evaluates the three sides (18 fp64 operations) and P3; the ballot of the
// crossed lanes is uniform.
// FILL = false: its population count is added to the plane's counter, which lane p keeps for plane p of the tile, and is stored to
// part[i * slices + j] at the end: every (plane, slice) is written by exactly one lane of one workgroup, so nothing is zeroed first.
// FILL = true: lane p first fetches the first row of (its plane, this slice): offsets[i] + part[i][0 .. j) (the wave sums a row of
// part together, plane by plane).  A crossed lane's row is that base plus the number of set ballot bits below it -- the lanes hold
// ascending ids and the rounds ascend, so the rows are in ascending id without a sort, and no other workgroup writes them -- and
// only crossed lanes run P4's sort and division (plane_segment), behind a uniform branch on the ballot.  Rows >= capacity are not
// written.  Nothing is read of the tree; no atomics; the index of every load and store is checked against its array's extent
// (k < k1 <= n_tri, i < n, l < j <= slices, row < capacity).
constexpr int PL_BLOCK = 64, PL_TILE = 64;
struct PlaneArgs {
  const float4* tri_geom;
  int32_t n_tri;
  int32_t per_slice;        // L: triangles per slice, a multiple of 64
  int32_t slices;           // S
  const float* planes;      // n x 4
  uint32_t n;
  int32_t* part;            // n x S: written (FILL = false) or read (FILL = true)
  const long long* offsets; // FILL: n + 1
  long long capacity;       // FILL
  int32_t* tri_id;          // FILL: capacity
  float* seg;               // FILL: capacity x 6, or null
};
template <bool FILL>
__global__ __launch_bounds__(PL_BLOCK) void plane_kernel(PlaneArgs a) {
  __shared__ PlaneEq tile[PL_TILE];
  const int lane = (int)threadIdx.x;
  const uint32_t i = blockIdx.x * PL_TILE + threadIdx.x; // lane p's plane
  const int32_t j = (int32_t)blockIdx.y;
  const long long k0l = (long long)j * a.per_slice;
  const int32_t k0 = k0l < a.n_tri ? (int32_t)k0l : a.n_tri;
  const int32_t k1 = a.n_tri - k0 < a.per_slice ? a.n_tri : k0 + a.per_slice;
  const int m = a.n - blockIdx.x * PL_TILE < (uint32_t)PL_TILE ? (int)(a.n - blockIdx.x * PL_TILE) : PL_TILE; // planes of this tile
  PlaneEq mine;
  mine.a = mine.b = mine.c = mine.d = 0.0, mine.live = 0;
  if (i < a.n) plane_load(a.planes + (size_t)i * 4, mine);
  tile[lane] = mine;
  int32_t cnt = 0;   // FILL = false: the crossed triangles of lane p's plane in this slice
  long long row = 0; // FILL = true: the next row of lane p's plane
  if (FILL) {
#pragma unroll 1
    for (int p = 0; p < m; p++) {
      const size_t r = (size_t)(blockIdx.x * PL_TILE + (uint32_t)p) * (size_t)a.slices;
      int32_t sum = 0;
      for (int32_t l = lane; l < j; l += PL_BLOCK) sum += a.part[r + (size_t)l];
      if (j > 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      }
      if (lane == p) row = a.offsets[i] + (long long)sum;
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int32_t base = k0; base < k1; base += PL_BLOCK) {
    const int32_t k = base + lane;
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool fin = false;
    if (k < k1) fin = plane_tri(a.tri_geom + (size_t)k * 3, v);
#pragma unroll 1
    for (int p = 0; p < m; p++) {
      const PlaneEq pl = tile[p];
      const double s0 = plane_side(pl, v[0], v[1], v[2]), s1 = plane_side(pl, v[3], v[4], v[5]), s2 = plane_side(pl, v[6], v[7], v[8]);
      const bool crossed = fin && pl.live != 0 && plane_crossed(s0, s1, s2);
      const unsigned long long mask = __ballot(crossed);
      if (!FILL) {
        cnt += lane == p ? (int32_t)__popcll(mask) : 0;
      } else if (mask != 0ull) {
        const long long r0 = ((long long)__builtin_amdgcn_readlane((int)(row >> 32), p) << 32) |
                             (long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)row, p);
        if (crossed) {
          const long long r = r0 + (long long)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
          if ((unsigned long long)r < (unsigned long long)a.capacity) { // (a negative row -- offsets that no count call left -- is no row)
            a.tri_id[r] = k;
            if (a.seg) {
              f3 q0, q1;
              plane_segment(v, s0, s1, s2, q0, q1);
              float2* out = (float2*)(a.seg + (size_t)r * 6); // 24-byte rows: 8-byte aligned
              out[0] = make_float2(q0.x, q0.y), out[1] = make_float2(q0.z, q1.x), out[2] = make_float2(q1.y, q1.z);
            }
          }
        }
        if (lane == p) row += (long long)__popcll(mask);
      }
    }
  }
  if (!FILL && i < a.n) a.part[(size_t)i * (size_t)a.slices + (size_t)j] = cnt;
}
// n_cross[i] = the sum of part's row i: one WAVE per plane (four to a workgroup), the lanes stride over the row -- coalesced, and a
// call of few planes and thousands of slices is not one lane's chain of loads
__global__ __launch_bounds__(256) void plane_total_kernel(const int32_t* part, int32_t slices, uint32_t n, int32_t* n_cross) {
  const uint32_t i = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; // uniform across the wave
  const int lane = (int)(threadIdx.x & 63);
  if (i >= n) return;
  int32_t sum = 0;
  for (int32_t j = lane; j < slices; j += 64) sum += part[(size_t)i * (size_t)slices + (size_t)j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) n_cross[i] = sum;
}
// offsets = the exclusive prefix sum of n_cross, the total in offsets[n]: ONE workgroup -- every thread sums a contiguous chunk, the
// 1024 chunk sums are scanned in LDS, every thread writes its chunk.  Plain on purpose: n is the number of planes, and the sweep
// before it costs n * n_tri pair evaluations (profiles/r24/plane_rates.txt has its time).
constexpr int PL_SCAN = 1024;
__global__ __launch_bounds__(PL_SCAN) void plane_offsets_kernel(const int32_t* n_cross, uint32_t n, long long* offsets) {
  __shared__ long long sums[PL_SCAN];
  const uint32_t t = threadIdx.x;
  const unsigned long long chunk = ((unsigned long long)n + PL_SCAN - 1) / PL_SCAN;
  const unsigned long long lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  long long s = 0;
  for (unsigned long long i = lo; i < hi; i++) s += n_cross[i];
  sums[t] = s;
  __syncthreads();
  for (uint32_t o = 1; o < PL_SCAN; o <<= 1) {
    const long long add = t >= o ? sums[t - o] : 0;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  long long run = sums[t] - s;
  for (unsigned long long i = lo; i < hi; i++) {
    offsets[i] = run;
    run += n_cross[i];
  }
  if (t == PL_SCAN - 1) offsets[n] = sums[t];
}

// ezrt_plane_section_at_device: the rule for pairs the caller holds -- plane i against triangle tri_id[i].  An id outside the scene, a
// plane that is not live and a triangle with a non-finite coordinate write zeros.
__global__ __launch_bounds__(256) void plane_at_kernel(const float4* tri_geom, int32_t n_tri, const float* planes, const int32_t* tri_id,
                                                       uint32_t n, uint8_t* crosses, int8_t* side, float* seg) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t tri = tri_id[i];
  PlaneEq pl;
  plane_load(planes + (size_t)i * 4, pl);
  f3 q0 = mk(0.0f, 0.0f, 0.0f), q1 = q0;
  int8_t sd[3] = {0, 0, 0};
  bool crossed = false;
  if ((uint32_t)tri < (uint32_t)n_tri && pl.live) {
    double v[9];
    if (plane_tri(tri_geom + (size_t)tri * 3, v)) {
      const double s0 = plane_side(pl, v[0], v[1], v[2]), s1 = plane_side(pl, v[3], v[4], v[5]), s2 = plane_side(pl, v[6], v[7], v[8]);
      sd[0] = (int8_t)((s0 > 0.0) - (s0 < 0.0)), sd[1] = (int8_t)((s1 > 0.0) - (s1 < 0.0)), sd[2] = (int8_t)((s2 > 0.0) - (s2 < 0.0));
      crossed = plane_crossed(s0, s1, s2);
      if (crossed) plane_segment(v, s0, s1, s2, q0, q1);
    }
  }
  crosses[i] = crossed ? 1u : 0u;
  if (side) side[(size_t)i * 3] = sd[0], side[(size_t)i * 3 + 1] = sd[1], side[(size_t)i * 3 + 2] = sd[2];
  if (seg) {
    float* out = seg + (size_t)i * 6;
    out[0] = q0.x, out[1] = q0.y, out[2] = q0.z, out[3] = q1.x, out[4] = q1.y, out[5] = q1.z;
  }
}

// ---- plane loops (include/ezrt_plane_loops.h): the rows of a section chained into polylines, on bits alone.
//
// One workgroup per plane.  loops_plane is the whole of a plane's join (L4) and ranking (L5) on LOCAL row indices 0 .. m - 1 (int32:
// m <= n_tri) over a LoopsStore of arrays that loops_chain_kernel<true> places in LDS (planes of at most `tile` rows) and
// loops_chain_kernel<false> in the caller's `work`, at the plane's own rows of capacity-long arrays (2 x rows of the table's).  The
// workgroup leaves nxt, prd, hd (the head; -1 for a degenerate row), ps (pos) and hl (a head's number among its plane's heads) in
// `work` and the plane's number of loops in plane_loops[i], which scan_block_kernel then sums in place.  loops_length_kernel has the
// tail of every chain write its loop's length, scan_block_kernel sums those, and loops_scatter_kernel writes the outputs.
//
// Termination and bounds, whatever `offsets` holds (two chained planes of a garbage array may overlap, and then share rows of
// `work`): every probe loop runs at most T times, every list walk at most m times, every round loop K times, and every index read
// back from a store is used only if it is below m (loops_in); every store to an output is behind a check of its index.
// The LDS route's 512 threads are measured (profiles/r27/plane_loops_variants.txt): 256 lose 2 to 18 % on every set, 1024 lose 22 to
// 30 % at 10 000 planes.
constexpr int LP_TILE_MAX = 1024;                       // rows of a plane that is chained in LDS: 11 ints each, 44 KiB of the launch's 64
constexpr int LP_LDS_BLOCK = 512, LP_GLB_BLOCK = 1024;  // threads of the two routes' workgroups
constexpr int LP_BLOCK = 256;
struct LoopsArgs {
  const long long* offsets; // n + 1
  const uint32_t* seg;      // capacity x 6: the bits
  long long capacity;
  int32_t n_tri;
  uint32_t n;
  uint32_t tile;            // the effective tile_rows
  // work, capacity ints each (rep, oh, ih: 2 x capacity); lofs: capacity + 1
  int32_t *nxt, *prd, *hd, *ps, *hl, *lo, *li, *ro, *rep, *oh, *ih;
  long long* lofs;
  // outputs
  long long *next, *order, *plane_loops, *loop_offsets;
  long long loop_capacity;
  uint8_t* closed;
};
// the arrays of one plane: rep / oh / ih are the table (T = 2 m slots: representative row, head of the OUT list, head of the IN
// list), lo / li the links of the two lists, ro a row's rank among the OUT rows of its key.  The ranking's double buffers lie over
// the table, which is dead by then: {a, d} = {rep, rep + m} and {oh, oh + m}.
struct LoopsStore {
  int32_t *nxt, *prd, *lo, *li, *ro, *rep, *oh, *ih;
};
// L2: the rows [o0, o0 + m) of plane i, or false
__device__ inline bool loops_range(const LoopsArgs& a, uint32_t i, long long& o0, uint32_t& m) {
  const long long lo = a.offsets[i], hi = a.offsets[i + 1];
  if (lo < 0 || hi < lo || hi > a.capacity || hi - lo > (long long)a.n_tri) return false;
  o0 = lo, m = (uint32_t)(hi - lo);
  return true;
}
__device__ inline bool loops_in(int32_t x, uint32_t m) { return (uint32_t)x < m; }
// A load of a table word that atomics have written (rep, oh, ih): an atomic load itself, so that the global route does not read a
// line of the vector cache that the atomics, which are performed in L2, have gone past.  EVERY OTHER word of a LoopsStore on the
// global route (lo, li, ro, nxt, prd, and the ranking buffers, which reuse words of rep and oh that atomics modified last) is a plain
// store read by other waves with plain loads after __syncthreads.  That is sound for ONE reason: a plane is one workgroup, a
// workgroup's waves share their CU's vector cache, which sees its own CU's stores, and the barrier fences at workgroup scope.  It
// does not hold in threadgroup-split mode (the library is not built for it), and it would break silently if a plane were ever split
// over several workgroups: such a change has to make these loads and stores agent-scope atomics, or put launches between the phases.
__device__ inline int32_t loops_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// (the hash of the table's keys, loops_hash, is in ezrt_scan_kernels.h: the mesh processing's tables use it too)
// K rounds of doubling on the buffers {ac, dc} -> {an, dn} and back: a' = a[a], d' = MIN ? min(d, d[a]) : d + d[a].  Ends behind a
// barrier with the result in {ac, dc} (the pointers are swapped with the rounds).
template <int B, bool MIN>
__device__ inline void loops_rounds(int K, uint32_t m, int32_t*& ac, int32_t*& dc, int32_t*& an, int32_t*& dn) {
  for (int k = 0; k < K; k++) {
    for (uint32_t r = threadIdx.x; r < m; r += B) {
      int32_t x = ac[r];
      if (!loops_in(x, m)) x = (int32_t)r;
      const int32_t v = dc[r], w = dc[x], y = ac[x];
      an[r] = loops_in(y, m) ? y : (int32_t)r;
      dn[r] = MIN ? (w < v ? w : v) : (int32_t)((uint32_t)v + (uint32_t)w);
    }
    __syncthreads();
    int32_t* t0 = ac;
    ac = an, an = t0;
    int32_t* t1 = dc;
    dc = dn, dn = t1;
  }
}
template <int B>
__device__ inline void loops_plane(const LoopsArgs& a, const LoopsStore& s, uint32_t i, long long o0, uint32_t m, int32_t* sc /* LDS, B ints */) {
  const uint32_t t = threadIdx.x, T = 2 * m;
  const uint32_t* seg = a.seg + (size_t)o0 * 6;
  int32_t *hd = a.hd + o0, *ps = a.ps + o0, *hl = a.hl + o0;
  for (uint32_t e = t; e < T; e += B) s.rep[e] = -1, s.oh[e] = -1, s.ih[e] = -1;
  __syncthreads();
  // JOIN 1: every non-degenerate row claims or finds the slot of its q0 and pushes itself onto the slot's OUT list
  for (uint32_t r = t; r < m; r += B) {
    const uint32_t* q = seg + (size_t)r * 6;
    const uint32_t x0 = q[0], x1 = q[1], x2 = q[2];
    s.prd[r] = -1;
    if (x0 == q[3] && x1 == q[4] && x2 == q[5]) { // L3
      s.nxt[r] = -2;
      continue;
    }
    s.nxt[r] = -1;
    uint32_t p = loops_hash(x0, x1, x2) % T;
    int32_t slot = -1;
    for (uint32_t k = 0; k < T; k++) {
      const int32_t old = atomicCAS(&s.rep[p], -1, (int32_t)r);
      if (old == -1) {
        slot = (int32_t)p;
        break;
      }
      if (loops_in(old, m)) {
        const uint32_t* o = seg + (size_t)old * 6;
        if (o[0] == x0 && o[1] == x1 && o[2] == x2) {
          slot = (int32_t)p;
          break;
        }
      }
      p = p + 1 == T ? 0 : p + 1;
    }
    s.ro[r] = slot; // (the rank takes its place in the next phase)
    s.lo[r] = slot >= 0 ? atomicExch(&s.oh[slot], (int32_t)r) : -1;
  }
  __syncthreads();
  // JOIN 2: the rank among the OUT rows of the key; the slot of q1, if a q0 has it, and a push onto its IN list
  for (uint32_t r = t; r < m; r += B) {
    if (s.nxt[r] == -2) continue;
    const int32_t slot = s.ro[r];
    int32_t rank = 0;
    if (loops_in(slot, T)) {
      int32_t e = loops_ld(&s.oh[slot]);
      for (uint32_t k = 0; k < m && loops_in(e, m); k++) {
        rank += e < (int32_t)r;
        e = s.lo[e];
      }
    }
    s.ro[r] = rank;
    const uint32_t* q = seg + (size_t)r * 6;
    const uint32_t x3 = q[3], x4 = q[4], x5 = q[5];
    uint32_t p = loops_hash(x3, x4, x5) % T;
    int32_t found = -1;
    for (uint32_t k = 0; k < T; k++) {
      const int32_t v = loops_ld(&s.rep[p]);
      if (v == -1) break;
      if (loops_in(v, m)) {
        const uint32_t* o = seg + (size_t)v * 6;
        if (o[0] == x3 && o[1] == x4 && o[2] == x5) {
          found = (int32_t)p;
          break;
        }
      }
      p = p + 1 == T ? 0 : p + 1;
    }
    s.nxt[r] = found; // (the slot, until the next phase replaces it by the successor)
    s.li[r] = found >= 0 ? atomicExch(&s.ih[found], (int32_t)r) : -1;
  }
  __syncthreads();
  // JOIN 3: L4 -- the rank j among the IN rows of the key, and the OUT row of rank j
  for (uint32_t r = t; r < m; r += B) {
    const int32_t slot = s.nxt[r];
    if (slot < 0) continue; // degenerate, or no q0 has this q1
    int32_t o = -1;
    if (loops_in(slot, T)) {
      int32_t j = 0, e = loops_ld(&s.ih[slot]);
      for (uint32_t k = 0; k < m && loops_in(e, m); k++) {
        j += e < (int32_t)r;
        e = s.li[e];
      }
      e = loops_ld(&s.oh[slot]);
      for (uint32_t k = 0; k < m && loops_in(e, m); k++) {
        if (s.ro[e] == j) {
          o = e;
          break;
        }
        e = s.lo[e];
      }
    }
    s.nxt[r] = o;
    if (o >= 0) s.prd[o] = (int32_t)r;
  }
  __syncthreads();
  // RANKING 1: pointer jumping along the predecessor; a head points at itself with distance 0
  int K = 0;
  while ((1u << K) < m) K++;
  int32_t *ac = s.rep, *dc = s.rep + m, *an = s.oh, *dn = s.oh + m;
  for (uint32_t r = t; r < m; r += B) {
    const int32_t p = s.prd[r];
    ac[r] = loops_in(p, m) ? p : (int32_t)r;
    dc[r] = loops_in(p, m) ? 1 : 0;
  }
  __syncthreads();
  loops_rounds<B, false>(K, m, ac, dc, an, dn);
  // a row whose pointer has not reached a head lies on a cycle (hd = -2 until ranking 3); a degenerate row gets -1
  int cyc = 0;
  for (uint32_t r = t; r < m; r += B) {
    const int32_t h = ac[r];
    const bool on = s.nxt[r] != -2 && loops_in(h, m) && s.prd[h] >= 0;
    hd[r] = s.nxt[r] == -2 ? -1 : (on ? -2 : h);
    ps[r] = dc[r];
    cyc |= on;
  }
  if (__syncthreads_or(cyc)) {
    // RANKING 2: min-doubling along next gives every row of a cycle the cycle's lowest row; the others stand still
    for (uint32_t r = t; r < m; r += B) {
      const int32_t x = s.nxt[r];
      ac[r] = hd[r] == -2 && loops_in(x, m) ? x : (int32_t)r;
      dc[r] = (int32_t)r;
    }
    __syncthreads();
    loops_rounds<B, true>(K, m, ac, dc, an, dn);
    // RANKING 3: the cycle is cut before its lowest row and ranked like a path; the rows of paths are fixed points of the rounds
    for (uint32_t r = t; r < m; r += B) {
      const int32_t low = dc[r], p = s.prd[r];
      if (hd[r] == -2) {
        const bool head = low == (int32_t)r || !loops_in(p, m);
        ac[r] = head ? (int32_t)r : p;
        dc[r] = head ? 0 : 1;
      } else {
        ac[r] = hd[r] >= 0 ? hd[r] : (int32_t)r;
        dc[r] = hd[r] >= 0 ? ps[r] : 0;
      }
    }
    __syncthreads();
    loops_rounds<B, false>(K, m, ac, dc, an, dn);
    for (uint32_t r = t; r < m; r += B)
      if (hd[r] == -2) hd[r] = ac[r], ps[r] = dc[r];
  }
  // the links leave the store (the LDS route's is gone with the workgroup)
  for (uint32_t r = t; r < m; r += B) a.nxt[o0 + r] = s.nxt[r], a.prd[o0 + r] = s.prd[r];
  __syncthreads();
  // COMPACTION 1: the plane's heads numbered in ascending row -- every thread a contiguous chunk, the chunk sums scanned in LDS
  const uint32_t chunk = (m + B - 1) / B, c0 = t * chunk < m ? t * chunk : m, c1 = c0 + chunk < m ? c0 + chunk : m;
  int32_t cnt = 0;
  for (uint32_t r = c0; r < c1; r++) cnt += hd[r] == (int32_t)r;
  sc[t] = cnt;
  __syncthreads();
  for (uint32_t o = 1; o < (uint32_t)B; o <<= 1) {
    const int32_t add = t >= o ? sc[t - o] : 0;
    __syncthreads();
    sc[t] += add;
    __syncthreads();
  }
  int32_t run = sc[t] - cnt;
  for (uint32_t r = c0; r < c1; r++)
    if (hd[r] == (int32_t)r) hl[r] = run++;
  if (t == (uint32_t)B - 1) a.plane_loops[i] = sc[t];
}
// LDS: the planes of at most a.tile rows, and the planes without loops (not chained, or empty); otherwise the longer planes
template <bool LDS>
__global__ __launch_bounds__(LDS ? LP_LDS_BLOCK : LP_GLB_BLOCK) void loops_chain_kernel(LoopsArgs a) {
  constexpr int B = LDS ? LP_LDS_BLOCK : LP_GLB_BLOCK;
  __shared__ int32_t sc[B];
  __shared__ int32_t tile[LDS ? 11 * LP_TILE_MAX : 1];
  const uint32_t i = blockIdx.x;
  long long o0 = 0;
  uint32_t m = 0;
  const bool ok = loops_range(a, i, o0, m);
  if (!ok || m == 0) {
    if (LDS && threadIdx.x == 0) a.plane_loops[i] = 0;
    return;
  }
  if ((m <= a.tile) != LDS) return;
  LoopsStore s;
  if (LDS) {
    s.nxt = tile, s.prd = tile + m, s.lo = tile + 2 * m, s.li = tile + 3 * m, s.ro = tile + 4 * m;
    s.rep = tile + 5 * m, s.oh = tile + 7 * m, s.ih = tile + 9 * m;
  } else {
    s.nxt = a.nxt + o0, s.prd = a.prd + o0, s.lo = a.lo + o0, s.li = a.li + o0, s.ro = a.ro + o0;
    s.rep = a.rep + 2 * o0, s.oh = a.oh + 2 * o0, s.ih = a.ih + 2 * o0;
  }
  loops_plane<B>(a, s, i, o0, m, sc);
}
// the number of a row's loop, or -1: plane_loops[i] (summed by now) + the head's number in its plane
__device__ inline long long loops_id(const LoopsArgs& a, long long first, long long o0, uint32_t m, int32_t h) {
  if (!loops_in(h, m)) return -1;
  const long long l = first + a.hl[o0 + h];
  return l >= 0 && l < a.capacity ? l : -1;
}
// COMPACTION 2: the tail of a path (no successor) and of a cut cycle (its successor is its head) is at pos = length - 1
__global__ __launch_bounds__(LP_BLOCK) void loops_length_kernel(LoopsArgs a) {
  const uint32_t i = blockIdx.x;
  long long o0 = 0;
  uint32_t m = 0;
  if (!loops_range(a, i, o0, m)) return;
  const long long first = a.plane_loops[i];
  for (uint32_t r = threadIdx.x; r < m; r += LP_BLOCK) {
    const int32_t h = a.hd[o0 + r], x = a.nxt[o0 + r];
    if (h < 0 || (x >= 0 && x != h)) continue;
    const long long l = loops_id(a, first, o0, m, h);
    if (l >= 0) a.lofs[l] = (long long)a.ps[o0 + r] + 1;
  }
}
// COMPACTION 3: order, next, loop_offsets and closed
__global__ __launch_bounds__(LP_BLOCK) void loops_scatter_kernel(LoopsArgs a) {
  const uint32_t i = blockIdx.x;
  if (i == 0 && threadIdx.x == 0) {
    const long long L = a.plane_loops[a.n];
    if (L >= 0 && L <= a.loop_capacity && L <= a.capacity) a.loop_offsets[L] = a.lofs[L];
  }
  long long o0 = 0;
  uint32_t m = 0;
  if (!loops_range(a, i, o0, m)) return;
  const long long first = a.plane_loops[i];
  for (uint32_t r = threadIdx.x; r < m; r += LP_BLOCK) {
    const long long g = o0 + r;
    const int32_t h = a.hd[g], x = a.nxt[g];
    if (a.next) a.next[g] = loops_in(x, m) ? o0 + x : -1;
    if (h < 0) continue;
    const long long l = loops_id(a, first, o0, m, h);
    if (l < 0) continue;
    const long long at = a.lofs[l], k = at + a.ps[g];
    if (k >= 0 && k < a.capacity) a.order[k] = g;
    if (h == (int32_t)r && l < a.loop_capacity) {
      a.loop_offsets[l] = at;
      if (a.closed) a.closed[l] = a.prd[g] >= 0 ? 1 : 0;
    }
  }
}

} // namespace ezd
