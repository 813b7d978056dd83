// tools/sphere_cast_host_check.cpp -- sphere_cast_live / sphere_cast_slab / sphere_cast_pair / sphere_cast_candidate / sphere_cast_at
// (ezrt_amd/csrc/hip/ezrt_device.h) compiled for the host and held against the numpy restatement on every pair of queries x triangles:
// gate, tnear, candidate, t, sub-candidate and contact point of each pair, tnear <= t, and the answer of each query (winner, t, point, touching;
// the touching step by closest_point_candidate over all triangles, as the kernel's search finds it).  Built and run by
// tools/sphere_cast_host_check.py, which cuts the rule's sections out of ezrt_device.h into sphere_cast_rule.inc and writes
// <dir>/<scene>_{tri,ray,rad,gate,tnear,cand,t,sub,px,win,wt,wx,wtouch}.bin; meant for -fsanitize=address,undefined.
// usage: sphere_cast_host_check <dir> <scene> ...
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
EZD f3 operator-(f3 a) { return mk(-a.x, -a.y, -a.z); }
EZD float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
EZD f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
#include "sphere_cast_rule.inc"
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
  const float inf = __builtin_inff();
  for (int s = 2; s < argc; s++) {
    const std::string base = std::string(argv[1]) + "/" + argv[s];
    const std::vector<float> tri = load<float>(base + "_tri.bin"), ray = load<float>(base + "_ray.bin"), rad = load<float>(base + "_rad.bin");
    const std::vector<uint8_t> want_gate = load<uint8_t>(base + "_gate.bin"), want_cand = load<uint8_t>(base + "_cand.bin");
    const std::vector<float> want_tnear = load<float>(base + "_tnear.bin"), want_t = load<float>(base + "_t.bin");
    const std::vector<int8_t> want_sub = load<int8_t>(base + "_sub.bin");
    const std::vector<float> want_px = load<float>(base + "_px.bin");
    const std::vector<int32_t> win = load<int32_t>(base + "_win.bin");
    const std::vector<float> wt = load<float>(base + "_wt.bin"), wx = load<float>(base + "_wx.bin");
    const std::vector<uint8_t> wtouch = load<uint8_t>(base + "_wtouch.bin");
    const size_t m = tri.size() / 9, n = rad.size();
    if (ray.size() != n * 6 || want_t.size() != n * m || want_cand.size() != n * m || want_gate.size() != n * m || want_px.size() != n * m * 3 || win.size() != n) return 2;
    size_t pairs = 0, gates = 0, cands = 0, wrong = 0, above = 0, dead = 0, wrong_answers = 0, touching = 0;
    std::vector<float4> tg(m * 3); // the device's tri_geom rows: (p.xyz, unused)
    for (size_t k = 0; k < m; k++)
      for (int v = 0; v < 3; v++) tg[k * 3 + v] = float4{tri[k * 9 + v * 3], tri[k * 9 + v * 3 + 1], tri[k * 9 + v * 3 + 2], 0.0f};
    for (size_t i = 0; i < n; i++) {
      const float* r6 = &ray[i * 6];
      SphereRay q;
      const bool live = sphere_cast_live(mk(r6[0], r6[1], r6[2]), mk(r6[3], r6[4], r6[5]), rad[i], q);
      dead += !live;
      SphereBest r;
      r.tri = -1, r.t = inf, r.point = mk(0.0f, 0.0f, 0.0f), r.touching = false;
      ClosestBest c;
      c.tri = -1, c.best = q.rr, c.v = c.w = 0.0f, c.q = mk(0.0f, 0.0f, 0.0f);
      for (size_t k = 0; k < m; k++) {
        float t = inf, tnear = 0.0f;
        f3 x;
        int sub = -1;
        const float4 a = tg[k * 3], b = tg[k * 3 + 1], cc = tg[k * 3 + 2];
        const f3 lo = mk(ez_min(ez_min(a.x, b.x), cc.x), ez_min(ez_min(a.y, b.y), cc.y), ez_min(ez_min(a.z, b.z), cc.z));
        const f3 hi = mk(ez_max(ez_max(a.x, b.x), cc.x), ez_max(ez_max(a.y, b.y), cc.y), ez_max(ez_max(a.z, b.z), cc.z));
        float tn_box = 0.0f;
        const bool finite = ez_abs(lo.x) < inf && ez_abs(lo.y) < inf && ez_abs(lo.z) < inf && ez_abs(hi.x) < inf && ez_abs(hi.y) < inf && ez_abs(hi.z) < inf;
        const bool gate = live && finite && sphere_cast_slab(q, lo, hi, tn_box);
        const bool cand = live && sphere_cast_pair(&tg[k * 3], q, inf, t, x, sub, tnear);
        if (!cand) t = inf, sub = -1, x = mk(0.0f, 0.0f, 0.0f);
        pairs++, gates += gate, cands += cand;
        wrong += gate != (want_gate[i * m + k] != 0) || (gate && !same(tn_box, want_tnear[i * m + k])) || cand != (want_cand[i * m + k] != 0) ||
                 !same(t, want_t[i * m + k]) || sub != want_sub[i * m + k] || !same3(x, &want_px[(i * m + k) * 3]);
        above += cand && !(tnear <= t && sphere_cast_box(q, lo, hi) <= t);
        if (live) {
          closest_point_candidate(c, tg.data(), (int32_t)k, q.o);
          sphere_cast_candidate(r, tg.data(), (int32_t)k, q);
        }
      }
      if (live && c.tri >= 0) r.tri = c.tri, r.t = 0.0f, r.point = c.q, r.touching = true;
      touching += r.touching;
      const float best = r.tri >= 0 ? r.t : inf;
      wrong_answers += r.tri != win[i] || !same(best, wt[i]) || !same3(r.point, &wx[i * 3]) || (r.touching ? 1 : 0) != wtouch[i];
      if (live && r.tri >= 0) { // the pair rule for a held pair reproduces the winner
        SphereBest h;
        h.tri = -1, h.t = inf, h.point = mk(0.0f, 0.0f, 0.0f), h.touching = false;
        sphere_cast_at(h, tg.data(), r.tri, q);
        wrong_answers += h.tri != r.tri || !same(h.t, r.t) || !same3(h.point, &wx[i * 3]) || h.touching != r.touching;
      }
    }
    printf("%s: %zu queries (%zu not live, %zu touching) x %zu triangles = %zu pairs, %zu pass the gate, %zu candidates; %zu pairs and %zu "
           "answers differ from the restatement, %zu pairs with tnear > t\n", argv[s], n, dead, touching, m, pairs, gates, cands, wrong,
           wrong_answers, above);
    if (wrong || wrong_answers || above) return 1;
  }
  return 0;
}
