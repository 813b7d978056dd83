// tools/segment_host_check.cpp -- segment_pair / segment_query / segment_gate / segment_candidate (ezrt_amd/csrc/hip/ezrt_device.h)
// compiled for the host and held against the numpy restatement on every pair of segments x triangles: candidate, dist2, (x, y) and
// crosses of each pair, lb <= dist2 against the triangle's own bounding box, and the answers of each query -- winner, dist2, both
// points and crosses without and with d_max (found as the kernel finds them: the pair gate before the pair rule), the capsule's row
// and count.  Built and run by tools/segment_host_check.py, which cuts the rule's sections out of ezrt_device.h into segment_rule.inc and
// writes <dir>/<scene>_*.bin; meant for -fsanitize=address,undefined.  usage: segment_host_check <dir> <K> <scene> ...
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
#include "segment_rule.inc"
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
  if (argc < 4) return 2;
  const int K = atoi(argv[2]);
  size_t total = 0;
  for (int s = 3; s < argc; s++) {
    const std::string base = std::string(argv[1]) + "/" + argv[s];
    const std::vector<float> tri = load<float>(base + "_tri.bin"), q = load<float>(base + "_q.bin"), want_d2 = load<float>(base + "_d2.bin");
    const std::vector<float> want_x = load<float>(base + "_x.bin"), want_y = load<float>(base + "_y.bin");
    const std::vector<float> dmax = load<float>(base + "_dmax.bin"), radius = load<float>(base + "_radius.bin");
    const std::vector<uint8_t> want_cand = load<uint8_t>(base + "_cand.bin"), want_cross = load<uint8_t>(base + "_cross.bin");
    const std::vector<int32_t> rows = load<int32_t>(base + "_rows.bin"), count = load<int32_t>(base + "_count.bin");
    const size_t m = tri.size() / 9, n = q.size() / 6;
    if (want_d2.size() != n * m || want_cand.size() != n * m || want_cross.size() != n * m || want_x.size() != n * m * 3 ||
        want_y.size() != n * m * 3 || rows.size() != n * (size_t)K || count.size() != n || dmax.size() != n || radius.size() != n)
      return 2;
    size_t pairs = 0, cands = 0, crossing = 0, wrong = 0, above = 0, dead = 0, wrong_answers = 0, wrong_rows = 0;
    std::vector<float4> tg(m * 3); // the device's tri_geom rows: (p.xyz, unused)
    for (size_t k = 0; k < m; k++)
      for (int v = 0; v < 3; v++) tg[k * 3 + v] = float4{tri[k * 9 + v * 3], tri[k * 9 + v * 3 + 1], tri[k * 9 + v * 3 + 2], 0.0f};
    for (size_t i = 0; i < n; i++) { // every pair
      const float* t = &q[i * 6];
      SegQuery Q;
      const bool live = segment_query(mk(t[0], t[1], t[2]), mk(t[3], t[4], t[5]), Q);
      dead += !live;
      for (size_t k = 0; k < m; k++) {
        float d2 = __builtin_inff();
        f3 x = mk(0.0f, 0.0f, 0.0f), y = x;
        bool crosses = false;
        const bool cand = live && segment_pair(&tg[k * 3], Q.a, Q.b, Q.lo, Q.hi, d2, x, y, crosses);
        if (!cand) d2 = __builtin_inff(), crosses = false, x = y = mk(0.0f, 0.0f, 0.0f);
        pairs++, cands += cand, crossing += crosses;
        const size_t p = i * m + k;
        wrong += cand != (want_cand[p] != 0) || !same(d2, want_d2[p]) || crosses != (want_cross[p] != 0) || !same3(x, &want_x[p * 3]) ||
                 !same3(y, &want_y[p * 3]);
        if (cand) above += !(segment_gate(&tg[k * 3], Q) <= d2); // the pair gate and the walk's bound on the triangle's own bounding box
      }
    }
    for (int pass = 0; pass < 2; pass++) { // every query's answer as the sweep finds it, without and with d_max
      const std::string tag = base + (pass ? "_lim" : "_free");
      const std::vector<int32_t> win = load<int32_t>(tag + "_win.bin");
      const std::vector<float> wd2 = load<float>(tag + "_wd2.bin"), wx = load<float>(tag + "_wx.bin"), wy = load<float>(tag + "_wy.bin");
      const std::vector<uint8_t> wc = load<uint8_t>(tag + "_wc.bin");
      if (win.size() != n || wd2.size() != n || wx.size() != n * 3 || wy.size() != n * 3 || wc.size() != n) return 2;
      for (size_t i = 0; i < n; i++) {
        const float* t = &q[i * 6];
        TriDistanceBest r;
        r.tri = -1, r.best = __builtin_inff(), r.x = r.y = mk(0.0f, 0.0f, 0.0f), r.crosses = false;
        bool live = true;
        if (pass) {
          if (dmax[i] >= 0.0f) r.best = dmax[i] * dmax[i];
          else live = false;
        }
        SegQuery Q;
        if (live && segment_query(mk(t[0], t[1], t[2]), mk(t[3], t[4], t[5]), Q))
          for (size_t k = 0; k < m; k++) {
            if (segment_gate(&tg[k * 3], Q) > r.best) continue;
            segment_candidate(r, tg.data(), (int32_t)k, Q);
          }
        const float best = r.tri >= 0 ? r.best : __builtin_inff();
        wrong_answers += r.tri != win[i] || !same(best, wd2[i]) || !same3(r.x, &wx[i * 3]) || !same3(r.y, &wy[i * 3]) || (r.crosses ? 1 : 0) != wc[i];
      }
    }
    for (size_t i = 0; i < n; i++) { // the capsule's row and count
      const float* t = &q[i * 6];
      const float rad = radius[i], R2 = rad * rad;
      SegQuery Q;
      std::vector<int32_t> row((size_t)K, -1);
      int32_t c = 0;
      if (rad >= 0.0f && rad < __builtin_inff() && segment_query(mk(t[0], t[1], t[2]), mk(t[3], t[4], t[5]), Q))
        for (size_t k = 0; k < m; k++) {
          if (segment_gate(&tg[k * 3], Q) > R2) continue;
          f3 x, y;
          float d2;
          bool crosses;
          if (!segment_pair(&tg[k * 3], Q.a, Q.b, Q.lo, Q.hi, d2, x, y, crosses) || !(d2 <= R2)) continue;
          if (c < K) row[(size_t)c] = (int32_t)k;
          c++;
        }
      wrong_rows += c != count[i] || memcmp(row.data(), &rows[i * (size_t)K], sizeof(int32_t) * (size_t)K) != 0;
    }
    printf("%s: %zu queries (%zu not live) x %zu triangles = %zu pairs, %zu candidates, %zu crossing; %zu pairs, %zu answers and %zu rows "
           "differ from the restatement, %zu pairs with lb > dist2\n", argv[s], n, dead, m, pairs, cands, crossing, wrong, wrong_answers,
           wrong_rows, above);
    total += pairs;
    if (wrong || wrong_answers || wrong_rows || above) return 1;
  }
  printf("%zu pairs in all: 0 differences\n", total);
  return 0;
}
