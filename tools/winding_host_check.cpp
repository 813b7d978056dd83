// tools/winding_host_check.cpp -- winding_tri / winding_term / winding_pair / winding_of (ezrt_amd/csrc/hip/ezrt_device.h) compiled for
// the host and held against the numpy restatement: the term q_k of every pair of points x triangles, by the kernel's split
// (winding_tri once per triangle, winding_term per pair) and by winding_pair, every point's int64 sum and its float, on the bits.
// Built and run by tools/winding_host_check.py, which cuts the rule's section out of ezrt_device.h into winding_rule.inc and writes
// <dir>/<scene>_*.bin; meant for -fsanitize=address,undefined.  usage: winding_host_check <dir> <scene> ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ezrt_detmath.h"
#define EZD static inline
#define __restrict__
struct float4 {
  float x, y, z, w;
};
namespace ezd {
struct f3 {
  float x, y, z;
};
EZD f3 mk(float x, float y, float z) { return f3{x, y, z}; }
#include "winding_rule.inc"
} // namespace ezd

template <class T>
static std::vector<T> load(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    perror(path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)bytes / sizeof(T));
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  using namespace ezd;
  if (argc < 3) return 2;
  size_t total = 0, total_live = 0;
  for (int s = 2; s < argc; s++) {
    const std::string base = std::string(argv[1]) + "/" + argv[s];
    const std::vector<float> tri = load<float>(base + "_tri.bin"), pts = load<float>(base + "_points.bin");
    const std::vector<int64_t> want = load<int64_t>(base + "_terms.bin"), want_sum = load<int64_t>(base + "_fixed.bin");
    const std::vector<uint32_t> want_w = load<uint32_t>(base + "_winding.bin");
    const size_t m = tri.size() / 9, n = pts.size() / 3;
    if (want.size() != n * m || want_sum.size() != n || want_w.size() != n) return 2;
    std::vector<float4> tg(m * 3); // the device's tri_geom rows: (p.xyz, unused)
    for (size_t k = 0; k < m; k++)
      for (int v = 0; v < 3; v++) tg[k * 3 + v] = float4{tri[k * 9 + v * 3], tri[k * 9 + v * 3 + 1], tri[k * 9 + v * 3 + 2], 0.0f};
    std::vector<WindingTri> sorted(m);
    size_t dead = 0;
    for (size_t k = 0; k < m; k++) {
      winding_tri(&tg[k * 3], sorted[k]);
      dead += sorted[k].sgn == 0.0f;
    }
    size_t pairs = 0, nonzero = 0, wrong = 0, wrong_pair = 0, wrong_sum = 0, wrong_w = 0;
    const float inf = __builtin_inff();
    for (size_t i = 0; i < n; i++) {
      const f3 p = mk(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]);
      const bool live = ez_abs(p.x) < inf && ez_abs(p.y) < inf && ez_abs(p.z) < inf; // as winding_kernel has it
      long long S = 0;
      for (size_t k = 0; k < m; k++) {
        long long q = 0;
        if (live && sorted[k].sgn != 0.0f) q = winding_term(sorted[k], (double)p.x, (double)p.y, (double)p.z);
        S += q;
        pairs++, nonzero += q != 0;
        wrong += q != want[i * m + k];
        wrong_pair += winding_pair(&tg[k * 3], p) != want[i * m + k];
      }
      wrong_sum += S != want_sum[i];
      const float w = winding_of(S);
      uint32_t bits;
      memcpy(&bits, &w, 4);
      wrong_w += bits != want_w[i];
    }
    printf("%s: %zu points x %zu triangles (%zu without a term) = %zu pairs, %zu non-zero terms; %zu terms, %zu terms by winding_pair, "
           "%zu sums and %zu floats differ from the restatement\n", argv[s], n, m, dead, pairs, nonzero, wrong, wrong_pair, wrong_sum, wrong_w);
    total += pairs, total_live += nonzero;
    if (wrong || wrong_pair || wrong_sum || wrong_w) return 1;
  }
  printf("%zu pairs in all, %zu non-zero: 0 differences\n", total, total_live);
  return 0;
}
