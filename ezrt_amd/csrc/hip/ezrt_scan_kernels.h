// ezrt_scan_kernels.h -- what the plane loops (ezrt_point_queries.h) and the mesh processing (the ezrt_*_kernels.h of ezrt_mesh.hip)
// share: the hash of their tables, and the exclusive prefix sum in its two forms, each with the host call that launches it.
//
//   scan_block_kernel                          ONE workgroup of SCAN_ONE lanes: a number of planes, of loops, of tiles
//   scan_tile_sums_kernel, scan_tiles_kernel   many workgroups, a tile of SCAN_TILE entries each, with scan_block_kernel between them
//   scan_small, scan_tiled                     the launches of the two forms on a stream
//
// Both translation units launch scan_block_kernel, so the kernels are `static`: their host stubs do not collide at link time, and the
// small one is compiled twice (a few hundred bytes of code).  A unit compiles every static kernel it sees, launched or not, so the tiled
// form is behind EZRT_SCAN_TILED, which ezrt_mesh.hip, its only user, defines before the include.
#pragma once

constexpr int SCAN_ONE = 1024; // lanes of the one-workgroup scan

// a mix of the 12 bytes (the finaliser of MurmurHash3): coordinates on a coarse grid differ in few, high bits
__device__ inline uint32_t loops_hash(uint32_t x, uint32_t y, uint32_t z) {
  uint32_t h = x * 0x9E3779B1u;
  h = (h << 13 | h >> 19) ^ (y * 0x85EBCA77u);
  h = (h << 13 | h >> 19) ^ (z * 0xC2B2AE3Du);
  h ^= h >> 16, h *= 0x85EBCA6Bu, h ^= h >> 13, h *= 0xC2B2AE35u, h ^= h >> 16;
  return h;
}

// x[0 .. n) -> its exclusive prefix sum IN PLACE, the total in x[n]; n = min(*n_dev, n_max) where n_dev is given, else n_max.  ONE
// workgroup, as plane_offsets_kernel: n is a number of planes, of loops or of tiles, small beside the rows.
static __global__ __launch_bounds__(SCAN_ONE) void scan_block_kernel(long long* x, const long long* n_dev, long long n_max) {
  __shared__ long long sums[SCAN_ONE];
  const uint32_t t = threadIdx.x;
  long long nn = n_dev ? *n_dev : n_max;
  nn = nn < 0 ? 0 : (nn > n_max ? n_max : nn);
  const unsigned long long n = (unsigned long long)nn, chunk = (n + SCAN_ONE - 1) / SCAN_ONE;
  const unsigned long long lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  long long s = 0;
  for (unsigned long long i = lo; i < hi; i++) s += x[i];
  sums[t] = s;
  __syncthreads();
  for (uint32_t o = 1; o < SCAN_ONE; o <<= 1) {
    const long long add = t >= o ? sums[t - o] : 0;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  long long run = sums[t] - s;
  for (unsigned long long i = lo; i < hi; i++) {
    const long long v = x[i];
    x[i] = run;
    run += v;
  }
  if (t == SCAN_ONE - 1) x[n] = sums[t];
}
// the exclusive prefix sum of x[0 .. n) in place on `st`, the total in x[n]; n = min(*n_dev, n_max), n_dev read on the device, or
// n_max where it is null.  One launch of one workgroup.
static inline void scan_small(hipStream_t st, long long* x, const long long* n_dev, long long n_max) {
  hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(SCAN_ONE), 0, st, x, n_dev, n_max);
}

#ifdef EZRT_SCAN_TILED
constexpr int SCAN_BLOCK = 256;                  // lanes of a tile's workgroup
constexpr int SCAN_PER = 8;                      // entries per lane of a tile
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_PER; // 2048
// scan_block_kernel's contract, but over ceil(n_max / SCAN_TILE) workgroups (one workgroup took 5.3 of the weld's 6.2 ms per 10^6
// corners).  scan_tile_sums_kernel: tile b's sum into tiles[b] (0 behind n); scan_block_kernel over tiles; scan_tiles_kernel: the
// tile's own exclusive scan plus tiles[b].  A tile is SCAN_BLOCK lanes of SCAN_PER consecutive entries; tiles cross launch boundaries.
__device__ inline unsigned long long scan_n(const long long* n_dev, long long n_max) {
  long long nn = n_dev ? *n_dev : n_max;
  nn = nn < 0 ? 0 : (nn > n_max ? n_max : nn);
  return (unsigned long long)nn;
}
static __global__ __launch_bounds__(SCAN_BLOCK) void scan_tile_sums_kernel(const long long* x, long long* tiles, const long long* n_dev, long long n_max) {
  __shared__ long long part[SCAN_BLOCK / 64];
  const unsigned long long n = scan_n(n_dev, n_max), base = (unsigned long long)blockIdx.x * SCAN_TILE;
  long long s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_PER; j++) { // coalesced: the order of an integer sum does not matter
    const unsigned long long i = base + (unsigned long long)j * SCAN_BLOCK + threadIdx.x;
    s += i < n ? x[i] : 0;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
    for (int w = 0; w < SCAN_BLOCK / 64; w++) t += part[w];
    tiles[blockIdx.x] = t;
  }
}
static __global__ __launch_bounds__(SCAN_BLOCK) void scan_tiles_kernel(long long* x, const long long* tiles, const long long* n_dev, long long n_max) {
  __shared__ long long sums[SCAN_BLOCK];
  const unsigned long long n = scan_n(n_dev, n_max), lo = (unsigned long long)blockIdx.x * SCAN_TILE + (unsigned long long)threadIdx.x * SCAN_PER;
  const uint32_t t = threadIdx.x;
  long long v[SCAN_PER], s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_PER; j++) {
    v[j] = lo + j < n ? x[lo + j] : 0;
    s += v[j];
  }
  sums[t] = s;
  __syncthreads();
  for (uint32_t o = 1; o < SCAN_BLOCK; o <<= 1) {
    const long long add = t >= o ? sums[t - o] : 0;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  long long run = tiles[blockIdx.x] + sums[t] - s;
#pragma unroll
  for (int j = 0; j < SCAN_PER; j++) {
    if (lo + j < n) x[lo + j] = run;
    run += v[j];
  }
  if (blockIdx.x == 0 && t == 0) x[n] = tiles[gridDim.x]; // the total: scan_block_kernel left it behind the tiles' sums
}
// the tiles of a scan of n entries
inline uint64_t scan_tile_count(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
// scan_small's contract over n_tiles = scan_tile_count(n_max) workgroups, in three launches; `tiles` is n_tiles + 1 words of scratch
static inline void scan_tiled(hipStream_t st, long long* x, long long* tiles, uint64_t n_tiles, const long long* n_dev, long long n_max) {
  const dim3 g((unsigned)n_tiles), b(SCAN_BLOCK);
  hipLaunchKernelGGL(scan_tile_sums_kernel, g, b, 0, st, (const long long*)x, tiles, n_dev, n_max);
  scan_small(st, tiles, nullptr, (long long)n_tiles);
  hipLaunchKernelGGL(scan_tiles_kernel, g, b, 0, st, x, (const long long*)tiles, n_dev, n_max);
}
#endif // EZRT_SCAN_TILED
