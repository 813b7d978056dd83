// ezrt_refit.hip -- ezrt_scene_refit_device (include/ezrt_refit.h): new vertex positions into an existing scene, its topology kept.
//
// Every record a scene derives from its triangles is either a per-triangle function of the vertices (geometry and shading records,
// the pruning bound eta_T) or a bottom-up fold over a topology that a refit does not change (boxes, pruning flags), so the whole
// refit is data-parallel work on the device:
//   refit_tri_kernel       per triangle: tri_ref floats 0-17, the geometry and shading records, m_t and eta_T (ezi::tri_normal and
//                          ezi::prune_eta: the very functions ezrt_scene_create evaluates on the host), the maxima G and Z
//   refit_level_kernel     per node, one launch per height (leaves first): the builder's box fold over a leaf's triangle range or the
//                          union of the children's boxes, the largest eta_T below the node; for the caller's leaves also the check
//                          "every leaf box holds its triangles" that decides whether the scene prunes at all
//   (rocPRIM radix sorts)  of eta_T and of m_t: the exact selections create makes with std::nth_element
//   refit_finalize_kernel  one thread: create's cutoff, quantile branch, medians, a_max and counts, by binary search in the sorted arrays
//   refit_bin_kernel       the binary records' child boxes and prune flags (q3.z / q3.w)
//   refit_wide_kernel      the 4-wide records' slot boxes and REF_NOPRUNE bits (cleared, then set again), and the root's flag
// The scalars the trace launches take as arguments (prune_a, root4, prunable) are read back once at the end: the call is synchronous.
#include <rocprim/device/device_radix_sort.hpp>

#include "ezrt_internal.h"
#include "ezrt_refit.h"

namespace {

// RefitState::ctl words
enum : int {
  RCTL_G = 0,       // max 1 / smin (double bits; atomic max: the values are >= 0)
  RCTL_Z,           // max zeta (double bits, -0 taken as +0)
  RCTL_NOT_HOLD,    // a caller leaf whose box does not hold one of its triangles
  RCTL_FLAGGED,     // 4-wide references that got REF_NOPRUNE
  RCTL_PRUNABLE,    // refit_finalize_kernel: 1 if the scene prunes
  RCTL_CUTOFF,      // ... cutoff (double bits): a node is flagged iff the largest eta_T below it exceeds it
  RCTL_M,           // ... prune_M, prune_A_med (double bits), prune_a (float bits), prune_bad
  RCTL_A_MED,
  RCTL_A,
  RCTL_BAD,
  RCTL_ROOT4,       // refit_wide_kernel: 1 if the root reference is flagged
  RCTL_WORDS
};

__device__ __forceinline__ float glm_min(float a, float b) { return (b < a) ? b : a; } // glm::min: the first operand wins ties and NaN
__device__ __forceinline__ float glm_max(float a, float b) { return (a < b) ? b : a; } // glm::max
__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ double bitsd(unsigned long long u) { return __longlong_as_double((long long)u); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}

__global__ void __launch_bounds__(256) refit_tri_kernel(const float* __restrict__ in, int n_tri, float* __restrict__ tri_ref,
                                                        float4* __restrict__ geom, float4* __restrict__ shade, double* __restrict__ eta,
                                                        double* __restrict__ m_t, unsigned long long* __restrict__ ctl) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  unsigned long long g = 0ull, z = 0ull; // (all lanes reach the wave reductions below)
  if (i < n_tri) {
    const float* src = in + (size_t)i * EZRT_TRI_FLOATS;
    float t[18];
#pragma unroll
    for (int k = 0; k < 18; k++) t[k] = src[k];
    float* dst = tri_ref + (size_t)i * EZRT_TRI_FLOATS;
#pragma unroll
    for (int k = 0; k < 18; k++) dst[k] = t[k];
    float nx, ny, nz;
    ezi::tri_normal(t, nx, ny, nz);
    geom[(size_t)i * 3 + 0] = make_float4(t[0], t[1], t[2], nx);
    geom[(size_t)i * 3 + 1] = make_float4(t[3], t[4], t[5], ny);
    geom[(size_t)i * 3 + 2] = make_float4(t[6], t[7], t[8], nz);
    const ShadeDen dn = shade_denominators(f3{t[0], t[1], t[2]}, f3{t[3], t[4], t[5]}, f3{t[6], t[7], t[8]});
    float4* o = shade + (size_t)i * SHADE_REC_FLOAT4;
    o[0] = make_float4(t[9], t[10], t[11], t[12]);
    o[1] = make_float4(t[13], t[14], t[15], t[16]);
    float4 o2 = o[2]; // (.y = the triangle's material: kept)
    o2.x = t[17];
    o[2] = o2;
    o[3] = make_float4(dn.a5, dn.b5, dn.a34, dn.b34);
    const ezi::PruneEta e = ezi::prune_eta(t, nx, ny, nz);
    m_t[i] = e.m_t;
    eta[i] = e.eta; // (0 when no hit can be accepted, +inf without a bound)
    if (e.kind == 2) {
      g = dbits(e.inv_smin);
      z = dbits(e.zeta + 0.0);
    }
  }
  g = wave_max_u64(g);
  z = wave_max_u64(z);
  if ((threadIdx.x & 63) == 0) {
    if (g) atomicMax(&ctl[RCTL_G], g);
    if (z) atomicMax(&ctl[RCTL_Z], z);
  }
}

// nodes (left, right, n, index); box[2 id] = (AA, 0), box[2 id + 1] = (BB, 0)
__global__ void __launch_bounds__(256) refit_level_kernel(const int4* __restrict__ nodes, const int32_t* __restrict__ order, int begin,
                                                          int end, const float* __restrict__ tri_ref, const double* __restrict__ eta,
                                                          float4* __restrict__ box, double* __restrict__ eta_max,
                                                          unsigned long long* __restrict__ not_hold) {
  const int k = begin + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= end) return;
  const int id = order[k];
  const int4 nd = nodes[id];
  float lo[3], hi[3];
  double em = 0.0;
  if (nd.z > 0) { // a leaf: buildBVH's fold over [index, index + n) (P5/main.cpp:405-423)
    for (int c = 0; c < 3; c++) {
      lo[c] = (float)1145141919;
      hi[c] = (float)-1145141919;
    }
    for (int j = nd.w; j < nd.w + nd.z; j++) {
      const float* t = tri_ref + (size_t)j * EZRT_TRI_FLOATS;
      for (int c = 0; c < 3; c++) {
        lo[c] = glm_min(lo[c], glm_min(t[c], glm_min(t[3 + c], t[6 + c])));
        hi[c] = glm_max(hi[c], glm_max(t[c], glm_max(t[3 + c], t[6 + c])));
      }
      const double e = eta[j];
      em = e > em ? e : em;
    }
    if (not_hold) {
      bool hold = true;
      for (int j = nd.w; j < nd.w + nd.z; j++) {
        const float* t = tri_ref + (size_t)j * EZRT_TRI_FLOATS;
        for (int v = 0; v < 9; v++)
          if (!(t[v] >= lo[v % 3] && t[v] <= hi[v % 3])) hold = false; // (false on NaN)
      }
      if (!hold) atomicOr(not_hold, 1ull);
    }
  } else { // an inner node: the union of its children's boxes, left then right
    const float4 la = box[2 * (size_t)nd.x], lb = box[2 * (size_t)nd.x + 1];
    const float4 ra = box[2 * (size_t)nd.y], rb = box[2 * (size_t)nd.y + 1];
    lo[0] = glm_min(la.x, ra.x);
    lo[1] = glm_min(la.y, ra.y);
    lo[2] = glm_min(la.z, ra.z);
    hi[0] = glm_max(lb.x, rb.x);
    hi[1] = glm_max(lb.y, rb.y);
    hi[2] = glm_max(lb.z, rb.z);
    const double el = eta_max[nd.x], er = eta_max[nd.y];
    em = er > el ? er : el;
  }
  box[2 * (size_t)id] = make_float4(lo[0], lo[1], lo[2], 0.0f);
  box[2 * (size_t)id + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  eta_max[id] = em;
}

// number of entries <= x of the ascending array a[0, n)
__device__ size_t count_le(const double* a, size_t n, double x) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (a[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ezrt_scene_create's pruning scalars (ezrt_scene_build.hip "distance pruning") from the sorted eta_T and m_t: the nth_element
// selections there are the same ranks here.  eta_T is 0 (no hit can be accepted), finite > 0 (a bound) or +inf (none).
__global__ void refit_finalize_kernel(const double* __restrict__ eta_s, const double* __restrict__ mt_s, int n_tri, int has_wide,
                                      unsigned long long* __restrict__ ctl) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const size_t n = (size_t)n_tri;
  if (!has_wide || ctl[RCTL_NOT_HOLD] != 0ull) {
    for (int w = RCTL_PRUNABLE; w <= RCTL_BAD; w++) ctl[w] = 0ull;
    return;
  }
  const double M = __builtin_fmax(0.0, mt_s[n - 1]);
  const size_t n_zero = count_le(eta_s, n, 0.0);                // eta == 0
  const size_t n_fin = count_le(eta_s, n, 1.7976931348623157e308); // eta < +inf
  double cutoff = M / 8192.0;
  size_t c = count_le(eta_s, n, cutoff);
  const double a_glob = c > 0 ? __builtin_fmax(0.0, eta_s[c - 1]) : 0.0;
  const double scale = mt_s[n / 2];
  const size_t n_all = n_fin - n_zero; // 0 < eta < +inf
  if (a_glob > scale / 16384.0 && n_all >= 2048) {
    const size_t k = n_all - 1 - n_all / 1024;
    cutoff = __builtin_fmin(cutoff, eta_s[n_zero + k]);
  }
  c = count_le(eta_s, n, cutoff);
  const double a_max = c > 0 ? __builtin_fmax(0.0, eta_s[c - 1]) : 0.0;
  const size_t n_med = c - n_zero; // 0 < eta <= cutoff
  const double a_med = n_med > 0 ? 2.0 * eta_s[n_zero + n_med / 2] : 0.0;
  const unsigned long long bad = (unsigned long long)((n - n_fin) + (n_fin > c ? n_fin - c : 0));
  const float a = nextafterf((float)(2.0 * a_max), __builtin_inff());
  ctl[RCTL_PRUNABLE] = 1ull;
  ctl[RCTL_CUTOFF] = dbits(cutoff);
  ctl[RCTL_M] = dbits(M);
  ctl[RCTL_A_MED] = dbits(a_med);
  ctl[RCTL_A] = (unsigned long long)__float_as_uint(a);
  ctl[RCTL_BAD] = bad;
}

__device__ __forceinline__ bool node_flagged(const double* eta_max, int id, const unsigned long long* ctl) {
  return ctl[RCTL_PRUNABLE] != 0ull && eta_max[id] > bitsd(ctl[RCTL_CUTOFF]);
}

// recs: (binary record, left, right, -) per inner node of the caller's tree
__global__ void __launch_bounds__(256) refit_bin_kernel(const int4* __restrict__ recs, int n, const float4* __restrict__ box,
                                                        const double* __restrict__ eta_max, const unsigned long long* __restrict__ ctl,
                                                        float4* __restrict__ inner) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int4 r = recs[i];
  const float4 la = box[2 * (size_t)r.y], lb = box[2 * (size_t)r.y + 1];
  const float4 ra = box[2 * (size_t)r.z], rb = box[2 * (size_t)r.z + 1];
  float4* q = inner + (size_t)r.x * 4;
  q[0] = make_float4(la.x, la.y, la.z, lb.x);
  q[1] = make_float4(lb.y, lb.z, ra.x, ra.y);
  q[2] = make_float4(ra.z, rb.x, rb.y, rb.z);
  float4 q3 = q[3]; // (.x / .y: the child references, kept)
  q3.z = __uint_as_float(node_flagged(eta_max, r.y, ctl) ? 1u : 0u);
  q3.w = __uint_as_float(node_flagged(eta_max, r.z, ctl) ? 1u : 0u);
  q[3] = q3;
}

__device__ __forceinline__ float& lane_of(float4& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }

// slots: the tree node of each slot of each 4-wide record (0 = unused: its NaN boxes and REF_EMPTY stay)
__global__ void __launch_bounds__(256) refit_wide_kernel(const int4* __restrict__ slots, int n_rec, const float4* __restrict__ box,
                                                         const double* __restrict__ eta_max, unsigned long long* __restrict__ ctl,
                                                         float4* __restrict__ inner4) {
  const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (q == 0) ctl[RCTL_ROOT4] = node_flagged(eta_max, 1, ctl) ? 1ull : 0ull;
  if (q >= n_rec) return;
  const int4 sl = slots[q];
  const int nd[4] = {sl.x, sl.y, sl.z, sl.w};
  float4* o = inner4 + (size_t)q * N4_FLOAT4;
  float4 aa[3], bb[3], ref = o[N4_ROW_REF];
  for (int c = 0; c < 3; c++) {
    aa[c] = o[N4_ROW_AA + c];
    bb[c] = o[N4_ROW_BB + c];
  }
  unsigned long long flagged = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (nd[k] <= 0) continue;
    const float4 lo = box[2 * (size_t)nd[k]], hi = box[2 * (size_t)nd[k] + 1];
    lane_of(aa[0], k) = lo.x;
    lane_of(aa[1], k) = lo.y;
    lane_of(aa[2], k) = lo.z;
    lane_of(bb[0], k) = hi.x;
    lane_of(bb[1], k) = hi.y;
    lane_of(bb[2], k) = hi.z;
    uint32_t rf = __float_as_uint(lane_of(ref, k));
    if ((int32_t)rf >= 0) { // an inner reference (leaf references and REF_EMPTY have the top bit set)
      rf &= ~REF_NOPRUNE;
      if (node_flagged(eta_max, nd[k], ctl)) {
        rf |= REF_NOPRUNE;
        flagged++;
      }
      lane_of(ref, k) = __uint_as_float(rf);
    }
  }
  for (int c = 0; c < 3; c++) {
    o[N4_ROW_AA + c] = aa[c];
    o[N4_ROW_BB + c] = bb[c];
  }
  o[N4_ROW_REF] = ref;
  if (flagged) atomicAdd(&ctl[RCTL_FLAGGED], flagged);
}

// ---- host side

// the caller's arrays are a DAG when a node has two parents (ezrt_scene_create keeps the binary kernel for them; a refit refuses them)
bool topology_is_dag(const EzrtScene* s) {
  const std::vector<ezi::HostNode>& hn = s->topo_nodes;
  std::vector<unsigned char> parents(hn.size(), 0);
  for (size_t i = 1; i < hn.size(); i++) {
    if (s->topo_inner_id[i] < 0) continue;
    const int kids[2] = {hn[i].left, hn[i].right};
    for (int k : kids)
      if (++parents[(size_t)k] > 1) return true;
  }
  return false;
}

// node ids 1 .. size-1 of a tree whose children carry larger ids than their parents, grouped by height (leaves = 0)
int upload_tree(RefitTree& T, const std::vector<ezi::HostNode>& hn) {
  const size_t n = hn.size();
  std::vector<int> height(n, 0);
  std::vector<int4> nodes(n, make_int4(0, 0, 0, 0));
  int max_h = 0;
  for (size_t i = n; i-- > 1;) {
    const ezi::HostNode& h = hn[i];
    if (h.n > 0) {
      nodes[i] = make_int4(0, 0, h.n, h.index);
    } else {
      nodes[i] = make_int4(h.left, h.right, 0, 0);
      height[i] = 1 + std::max(height[(size_t)h.left], height[(size_t)h.right]);
      max_h = std::max(max_h, height[i]);
    }
  }
  T.level_off.assign((size_t)max_h + 2, 0);
  for (size_t i = 1; i < n; i++) T.level_off[(size_t)height[i] + 1]++;
  for (int k = 0; k <= max_h; k++) T.level_off[(size_t)k + 1] += T.level_off[(size_t)k];
  std::vector<int32_t> order(n > 1 ? n - 1 : 1, 0);
  std::vector<int> fill(T.level_off.begin(), T.level_off.end() - 1);
  for (size_t i = 1; i < n; i++) order[(size_t)fill[(size_t)height[i]]++] = (int32_t)i;
  HIP_TRY(T.nodes.ensure(n));
  HIP_TRY(T.order.ensure(order.size()));
  HIP_TRY(T.box.ensure(2 * n));
  HIP_TRY(T.eta_max.ensure(n));
  HIP_TRY(hipMemcpy(T.nodes.p, nodes.data(), n * sizeof(int4), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(T.order.p, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return 0;
}

// the first refit of a scene: its topology on the device, and all the scratch later refits reuse
int refit_prepare(EzrtScene* s) {
  RefitState& R = *s->refit;
  const size_t n_tri = (size_t)s->n_tri;
  int rc = upload_tree(R.caller, s->topo_nodes);
  if (rc) return rc;
  if (s->retreed) {
    rc = upload_tree(R.own, s->topo_tree4);
    if (rc) return rc;
  }
  std::vector<int4> bin;
  bin.reserve((size_t)s->n_inner);
  for (size_t i = 1; i < s->topo_nodes.size(); i++)
    if (s->topo_inner_id[i] >= 0) bin.push_back(make_int4(s->topo_inner_id[i], s->topo_nodes[i].left, s->topo_nodes[i].right, 0));
  if (!bin.empty()) {
    HIP_TRY(R.bin_recs.ensure(bin.size()));
    HIP_TRY(hipMemcpy(R.bin_recs.p, bin.data(), bin.size() * sizeof(int4), hipMemcpyHostToDevice));
  }
  if (s->n_inner4 > 0) {
    std::vector<int4> sl((size_t)s->n_inner4);
    for (size_t q = 0; q < sl.size(); q++) {
      const std::array<int, 4>& a = s->topo_rec_slots[q];
      sl[q] = make_int4(a[0], a[1], a[2], a[3]);
    }
    HIP_TRY(R.rec4_slots.ensure(sl.size()));
    HIP_TRY(hipMemcpy(R.rec4_slots.p, sl.data(), sl.size() * sizeof(int4), hipMemcpyHostToDevice));
  }
  HIP_TRY(R.eta.ensure(n_tri));
  HIP_TRY(R.m_t.ensure(n_tri));
  HIP_TRY(R.sorted.ensure(2 * n_tri));
  size_t bytes = 0;
  HIP_TRY(rocprim::radix_sort_keys(nullptr, bytes, R.eta.p, R.sorted.p, n_tri));
  HIP_TRY(R.sort_tmp.ensure(bytes > 0 ? bytes : 1));
  R.sort_tmp_bytes = bytes;
  HIP_TRY(R.ctl.ensure(RCTL_WORDS));
  if (!R.ctl_host) HIP_TRY(hipHostMalloc((void**)&R.ctl_host, RCTL_WORDS * sizeof(unsigned long long)));
  for (hipEvent_t& e : R.ev_pipe)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  R.ready = true;
  return 0;
}

void launch_tree(const RefitTree& T, const float* tri_ref, const double* eta, unsigned long long* not_hold, hipStream_t st) {
  for (size_t k = 0; k + 1 < T.level_off.size(); k++) {
    const int b = T.level_off[k], e = T.level_off[k + 1];
    if (e <= b) continue;
    hipLaunchKernelGGL(refit_level_kernel, dim3((unsigned)((e - b + 255) / 256)), dim3(256), 0, st, T.nodes.p, T.order.p, b, e, tri_ref,
                       eta, T.box.p, T.eta_max.p, not_hold);
  }
}

int refit_body(EzrtScene* s, const float* tri36, int n_tri, hipStream_t st) {
  if (!s || !tri36) return fail(EZRT_ERR_INVALID, "NULL scene or triangles");
  if (n_tri != s->n_tri) return fail(EZRT_ERR_INVALID, "n_tri = %d, the scene has %d triangles", n_tri, s->n_tri);
  hipPointerAttribute_t sat;
  if (!s->tri_geom.p || hipPointerGetAttributes(&sat, s->tri_geom.p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(EZRT_ERR_INVALID, "the scene has no device records");
  }
  const int dev = sat.device;
  if (!ezi::device_buffer_of(tri36, (size_t)n_tri * EZRT_TRI_FLOATS * sizeof(float), dev))
    return fail(EZRT_ERR_INVALID, "tri36 must be device memory of the scene's device (%d), %d x 36 floats", dev, n_tri);
  if (s->topo_nodes.size() != (size_t)s->n_nodes) return fail(EZRT_ERR_UNSUPPORTED, "the scene kept no topology");
  if (!s->refit) {
    s->refit = new RefitState();
    s->refit->is_dag = topology_is_dag(s) ? 1 : 0;
  }
  RefitState& R = *s->refit;
  if (R.is_dag) return fail(EZRT_ERR_UNSUPPORTED, "the scene's node arrays are not a tree (a node has two parents): rebuild it instead");
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  struct Restore {
    int d;
    ~Restore() { (void)hipSetDevice(d); }
  } restore{prev};
  if (dev != prev) HIP_TRY(hipSetDevice(dev));
  if (!R.ready) {
    const int rc = refit_prepare(s);
    if (rc) return rc;
  }

  // after everything already issued on the scene: the last render call (its end event follows every chunk it accumulated), the two
  // pipelined streams (chunks there do not wait for the caller's stream), the last device query, the last shading query
  if (s->ev_end) HIP_TRY(hipStreamWaitEvent(st, s->ev_end, 0));
  for (int i = 0; i < ezh::SHARED_STREAMS; i++)
    if (s->pipe[i].stream) {
      HIP_TRY(hipEventRecord(R.ev_pipe[i], s->pipe[i].stream));
      HIP_TRY(hipStreamWaitEvent(st, R.ev_pipe[i], 0));
    }
  if (s->query.ev_end) HIP_TRY(hipStreamWaitEvent(st, s->query.ev_end, 0));
  if (s->query.ev_shade_end) HIP_TRY(hipStreamWaitEvent(st, s->query.ev_shade_end, 0));

  const int n = s->n_tri;
  const bool wide = s->n_inner4 > 0;
  HIP_TRY(hipMemsetAsync(R.ctl.p, 0, RCTL_WORDS * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(refit_tri_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tri36, n, s->tri_ref.p, s->tri_geom.p,
                     s->tri_shade.p, R.eta.p, R.m_t.p, R.ctl.p);
  launch_tree(R.caller, s->tri_ref.p, R.eta.p, wide ? R.ctl.p + RCTL_NOT_HOLD : nullptr, st);
  if (s->retreed) launch_tree(R.own, s->tri_ref.p, R.eta.p, nullptr, st);
  double* eta_s = R.sorted.p;
  double* mt_s = R.sorted.p + n;
  if (wide) {
    size_t bytes = R.sort_tmp_bytes;
    HIP_TRY(rocprim::radix_sort_keys(R.sort_tmp.p, bytes, R.eta.p, eta_s, (size_t)n, 0, 64, st));
    bytes = R.sort_tmp_bytes;
    HIP_TRY(rocprim::radix_sort_keys(R.sort_tmp.p, bytes, R.m_t.p, mt_s, (size_t)n, 0, 64, st));
  }
  hipLaunchKernelGGL(refit_finalize_kernel, dim3(1), dim3(64), 0, st, eta_s, mt_s, n, wide ? 1 : 0, R.ctl.p);
  if (R.bin_recs.p && s->n_inner > 0)
    hipLaunchKernelGGL(refit_bin_kernel, dim3((unsigned)((s->n_inner + 255) / 256)), dim3(256), 0, st, R.bin_recs.p, s->n_inner,
                       R.caller.box.p, R.caller.eta_max.p, R.ctl.p, s->inner.p);
  if (wide) {
    const RefitTree& T = s->retreed ? R.own : R.caller;
    hipLaunchKernelGGL(refit_wide_kernel, dim3((unsigned)((s->n_inner4 + 255) / 256)), dim3(256), 0, st, R.rec4_slots.p, s->n_inner4,
                       T.box.p, T.eta_max.p, R.ctl.p, s->inner4.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(R.ctl_host, R.ctl.p, RCTL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  const unsigned long long* c = R.ctl_host;
  auto d = [](unsigned long long u) {
    double x;
    memcpy(&x, &u, sizeof x);
    return x;
  };
  s->prunable = c[RCTL_PRUNABLE] != 0ull;
  if (s->prunable) {
    const uint32_t ab = (uint32_t)c[RCTL_A];
    s->prune_G = d(c[RCTL_G]);
    s->prune_Z = d(c[RCTL_Z]);
    s->prune_M = d(c[RCTL_M]);
    s->prune_A_med = d(c[RCTL_A_MED]);
    memcpy(&s->prune_a, &ab, sizeof ab);
    s->prune_bad = (int64_t)c[RCTL_BAD];
    const bool root = c[RCTL_ROOT4] != 0ull;
    s->prune_flagged = (int64_t)c[RCTL_FLAGGED] + (root ? 1 : 0);
    s->root4 = root ? REF_NOPRUNE : 0u;
  } else {
    s->prune_G = s->prune_Z = s->prune_M = s->prune_A_med = 0.0;
    s->prune_a = 0.0f;
    s->prune_bad = s->prune_flagged = 0;
    s->root4 = wide ? 0u : s->root_ref;
  }
  return 0;
}

} // namespace

extern "C" int ezrt_scene_refit_device(EzrtScene* s, const float* tri36, int n_tri, void* stream) {
  return ezi::guarded("ezrt_scene_refit_device", [&]() -> int { return refit_body(s, tri36, n_tri, (hipStream_t)stream); });
}
