// tools/tri_distance_host_check.cpp -- segment_segment_closest / tri_distance_box / tri_distance_pair / tri_distance_candidate
// (ezrt_amd/csrc/hip/ezrt_device.h) compiled for the host and held against the numpy restatement on every pair of queries x triangles:
// candidate, dist2 and crosses of each pair, lb <= dist2 against the triangle's own bounding box, and the answer of each query (winner,
// dist2, both points, crosses).  Built and run by tools/tri_distance_host_check.py, which cuts the rule's sections out of ezrt_device.h
// into tri_distance_rule.inc and writes <dir>/<scene>_{tri,q,cand,d2,cross,win,wd2,wx,wy,wc}.bin; meant for
// -fsanitize=address,undefined.  usage: tri_distance_host_check <dir> <scene> ...
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
EZD f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
EZD f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
EZD f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
EZD float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
#include "tri_distance_rule.inc"
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
static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0; }
static bool same3(ezd::f3 a, const float* b) { return same(a.x, b[0]) && same(a.y, b[1]) && same(a.z, b[2]); }

int main(int argc, char** argv) {
  using namespace ezd;
  if (argc < 3) return 2;
  for (int s = 2; s < argc; s++) {
    const std::string base = std::string(argv[1]) + "/" + argv[s];
    const std::vector<float> tri = load<float>(base + "_tri.bin"), q = load<float>(base + "_q.bin"), want_d2 = load<float>(base + "_d2.bin");
    const std::vector<uint8_t> want_cand = load<uint8_t>(base + "_cand.bin"), want_cross = load<uint8_t>(base + "_cross.bin");
    const std::vector<int32_t> win = load<int32_t>(base + "_win.bin");
    const std::vector<float> wd2 = load<float>(base + "_wd2.bin"), wx = load<float>(base + "_wx.bin"), wy = load<float>(base + "_wy.bin");
    const std::vector<uint8_t> wc = load<uint8_t>(base + "_wc.bin");
    const size_t m = tri.size() / 9, n = q.size() / 9;
    if (want_d2.size() != n * m || want_cand.size() != n * m || want_cross.size() != n * m || win.size() != n) return 2;
    size_t pairs = 0, cands = 0, crossing = 0, wrong = 0, above = 0, dead = 0, wrong_answers = 0;
    std::vector<float4> tg(m * 3); // the device's tri_geom rows: (p.xyz, unused)
    for (size_t k = 0; k < m; k++)
      for (int v = 0; v < 3; v++) tg[k * 3 + v] = float4{tri[k * 9 + v * 3], tri[k * 9 + v * 3 + 1], tri[k * 9 + v * 3 + 2], 0.0f};
    for (size_t i = 0; i < n; i++) {
      const float* t = &q[i * 9];
      const f3 p1 = mk(t[0], t[1], t[2]), p2 = mk(t[3], t[4], t[5]), p3 = mk(t[6], t[7], t[8]);
      TriQuery Q;
      const bool live = tri_query(p1, p2, p3, Q);
      dead += !live;
      TriDistanceBest r;
      r.tri = -1, r.best = __builtin_inff(), r.x = r.y = mk(0.0f, 0.0f, 0.0f), r.crosses = false;
      for (size_t k = 0; k < m; k++) {
        float d2 = __builtin_inff();
        f3 x, y;
        bool crosses = false;
        const bool cand = live && tri_distance_pair(&tg[k * 3], Q, p1, p2, p3, d2, x, y, crosses);
        if (!cand) d2 = __builtin_inff(), crosses = false;
        pairs++, cands += cand, crossing += crosses;
        wrong += cand != (want_cand[i * m + k] != 0) || !same(d2, want_d2[i * m + k]) || crosses != (want_cross[i * m + k] != 0);
        if (cand) { // the pair gate and the walk's bound on the triangle's own bounding box
          const float4 a = tg[k * 3], b = tg[k * 3 + 1], c = tg[k * 3 + 2];
          const f3 lo = mk(ez_min(ez_min(a.x, b.x), c.x), ez_min(ez_min(a.y, b.y), c.y), ez_min(ez_min(a.z, b.z), c.z));
          const f3 hi = mk(ez_max(ez_max(a.x, b.x), c.x), ez_max(ez_max(a.y, b.y), c.y), ez_max(ez_max(a.z, b.z), c.z));
          above += !(tri_distance_box(Q.lo, Q.hi, lo, hi) <= d2);
        }
        if (live) tri_distance_candidate(r, tg.data(), (int32_t)k, Q, p1, p2, p3);
      }
      const float best = r.tri >= 0 ? r.best : __builtin_inff();
      wrong_answers += r.tri != win[i] || !same(best, wd2[i]) || !same3(r.x, &wx[i * 3]) || !same3(r.y, &wy[i * 3]) || (r.crosses ? 1 : 0) != wc[i];
    }
    printf("%s: %zu queries (%zu not live) x %zu triangles = %zu pairs, %zu candidates, %zu crossing; %zu pairs and %zu answers differ from "
           "the restatement, %zu pairs with lb > dist2\n", argv[s], n, dead, m, pairs, cands, crossing, wrong, wrong_answers, above);
    if (wrong || wrong_answers || above) return 1;
  }
  return 0;
}
