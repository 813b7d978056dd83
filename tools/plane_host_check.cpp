// tools/plane_host_check.cpp -- plane_load / plane_side / plane_tri / plane_crossed / plane_coord / plane_point / plane_segment
// (ezrt_amd/csrc/hip/ezrt_device.h) compiled for the host and held against the numpy restatement: of every pair of planes x triangles
// whether it is crossed, every plane's count, and of every crossed pair the row (q0, q1), on the bits, in the restatement's CSR order.
// Built and run by tools/plane_host_check.py, which cuts the rule's section out of ezrt_device.h into plane_rule.inc and writes
// <dir>/<scene>_*.bin; meant for -fsanitize=address,undefined.  usage: plane_host_check <dir> <scene> ...
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
#include "plane_rule.inc"
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
  size_t total = 0, total_rows = 0;
  for (int s = 2; s < argc; s++) {
    const std::string base = std::string(argv[1]) + "/" + argv[s];
    const std::vector<float> tri = load<float>(base + "_tri.bin"), planes = load<float>(base + "_planes.bin");
    const std::vector<int64_t> want_off = load<int64_t>(base + "_offsets.bin");
    const std::vector<int32_t> want_id = load<int32_t>(base + "_ids.bin");
    const std::vector<uint32_t> want_seg = load<uint32_t>(base + "_seg.bin");
    const size_t m = tri.size() / 9, n = planes.size() / 4;
    if (want_off.size() != n + 1 || want_seg.size() != want_id.size() * 6 || (size_t)want_off[n] != want_id.size()) return 2;
    std::vector<float4> tg(m * 3); // the device's tri_geom rows: (p.xyz, unused)
    for (size_t k = 0; k < m; k++)
      for (int v = 0; v < 3; v++) tg[k * 3 + v] = float4{tri[k * 9 + v * 3], tri[k * 9 + v * 3 + 1], tri[k * 9 + v * 3 + 2], 0.0f};
    size_t pairs = 0, rows = 0, dead = 0, wrong_count = 0, wrong_id = 0, wrong_seg = 0, zero_len = 0;
    for (size_t i = 0; i < n; i++) {
      PlaneEq pl;
      plane_load(&planes[i * 4], pl);
      dead += !pl.live;
      size_t row = (size_t)want_off[i];
      const size_t end = (size_t)want_off[i + 1];
      for (size_t k = 0; k < m; k++) {
        double v[9];
        const bool fin = plane_tri(&tg[k * 3], v);
        pairs++;
        if (!fin || !pl.live) continue; // as plane_kernel has it: the sides are not looked at
        const double s0 = plane_side(pl, v[0], v[1], v[2]), s1 = plane_side(pl, v[3], v[4], v[5]), s2 = plane_side(pl, v[6], v[7], v[8]);
        if (!plane_crossed(s0, s1, s2)) continue;
        if (row >= end || want_id[row] != (int32_t)k) {
          wrong_id++;
          continue;
        }
        f3 q0, q1;
        plane_segment(v, s0, s1, s2, q0, q1);
        const float q[6] = {q0.x, q0.y, q0.z, q1.x, q1.y, q1.z};
        uint32_t bits[6];
        memcpy(bits, q, sizeof bits);
        wrong_seg += memcmp(bits, &want_seg[row * 6], sizeof bits) != 0;
        zero_len += memcmp(bits, bits + 3, 12) == 0;
        row++, rows++;
      }
      wrong_count += row != end;
    }
    printf("%s: %zu planes (%zu not live) x %zu triangles = %zu pairs, %zu crossed (%zu in a zero-length segment); %zu counts, %zu ids "
           "and %zu rows differ from the restatement\n", argv[s], n, dead, m, pairs, rows, zero_len, wrong_count, wrong_id, wrong_seg);
    total += pairs, total_rows += rows;
    if (wrong_count || wrong_id || wrong_seg) return 1;
  }
  printf("%zu pairs in all, %zu crossed: 0 differences\n", total, total_rows);
  return 0;
}
