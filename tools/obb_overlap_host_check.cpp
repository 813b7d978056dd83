// tools/obb_overlap_host_check.cpp -- obb_query / obb_hull_gate / obb_face_gate / obb_overlaps (ezrt_amd/csrc/hip/ezrt_device.h)
// compiled for the host and held against the numpy restatement: liveness of every box, overlaps of every pair of boxes x triangles,
// every box's row and count (found as the sweep finds them), each of the two gates on every node box of the caller's tree on the bits
// of the restatement's, and no overlapping triangle below a node that the gates reject.  Built and run by
// tools/obb_overlap_host_check.py, which cuts the rule's section out of ezrt_device.h into obb_rule.inc and writes
// <dir>/<scene>_*.bin; meant for -fsanitize=address,undefined.  usage: obb_overlap_host_check <dir> <K> <scene> ...
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
#include "obb_rule.inc"
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
  if (argc < 4) return 2;
  const int K = atoi(argv[2]);
  size_t total = 0, total_over = 0;
  for (int s = 3; s < argc; s++) {
    const std::string base = std::string(argv[1]) + "/" + argv[s];
    const std::vector<float> tri = load<float>(base + "_tri.bin"), centre = load<float>(base + "_centre.bin"), axes = load<float>(base + "_axes.bin");
    const std::vector<float> nodebox = load<float>(base + "_nodebox.bin");
    const std::vector<uint8_t> want_live = load<uint8_t>(base + "_live.bin"), want = load<uint8_t>(base + "_over.bin");
    const std::vector<uint8_t> want_hull = load<uint8_t>(base + "_hull.bin"), want_face = load<uint8_t>(base + "_face.bin");
    const std::vector<int32_t> rows = load<int32_t>(base + "_rows.bin"), count = load<int32_t>(base + "_count.bin");
    const std::vector<int32_t> start = load<int32_t>(base + "_start.bin"), ids = load<int32_t>(base + "_ids.bin");
    const size_t m = tri.size() / 9, n = centre.size() / 3, nodes = nodebox.size() / 6;
    if (axes.size() != n * 9 || want_live.size() != n || want.size() != n * m || rows.size() != n * (size_t)K || count.size() != n ||
        want_hull.size() != n * nodes || want_face.size() != n * nodes || start.size() != nodes + 1 || (size_t)start[nodes] != ids.size())
      return 2;
    std::vector<float4> tg(m * 3); // the device's tri_geom rows: (p.xyz, unused)
    for (size_t k = 0; k < m; k++)
      for (int v = 0; v < 3; v++) tg[k * 3 + v] = float4{tri[k * 9 + v * 3], tri[k * 9 + v * 3 + 1], tri[k * 9 + v * 3 + 2], 0.0f};
    size_t pairs = 0, overlapping = 0, dead = 0, wrong_live = 0, wrong = 0, wrong_rows = 0;
    size_t slots = 0, rejected = 0, by_face = 0, wrong_gate = 0, lost = 0;
    for (size_t i = 0; i < n; i++) {
      const float *c = &centre[i * 3], *u = &axes[i * 9];
      ObbQuery q;
      const bool live = obb_query(mk(c[0], c[1], c[2]), mk(u[0], u[1], u[2]), mk(u[3], u[4], u[5]), mk(u[6], u[7], u[8]), q);
      dead += !live;
      wrong_live += live != (want_live[i] != 0);
      std::vector<int32_t> row((size_t)K, -1);
      int32_t found = 0;
      for (size_t k = 0; k < m; k++) { // every pair, and the row and count as the sweep finds them
        const bool o = live && obb_overlaps(&tg[k * 3], q);
        pairs++, overlapping += o;
        wrong += o != (want[i * m + k] != 0);
        if (o) {
          if (found < K) row[(size_t)found] = (int32_t)k;
          found++;
        }
      }
      wrong_rows += found != count[i] || memcmp(row.data(), &rows[i * (size_t)K], sizeof(int32_t) * (size_t)K) != 0;
      for (size_t j = 1; j < nodes; j++) { // the two gates on every node box of the caller's tree
        const float* b = &nodebox[j * 6];
        const f3 lo = mk(b[0], b[1], b[2]), hi = mk(b[3], b[4], b[5]);
        const bool hull = live && obb_hull_gate(q, lo, hi), face = live && obb_face_gate(q, lo, hi);
        wrong_gate += hull != (want_hull[i * nodes + j] != 0) || face != (want_face[i * nodes + j] != 0);
        slots++;
        if (hull && face) continue;
        rejected++, by_face += hull;
        for (int32_t t = start[j]; t < start[j + 1]; t++) lost += want[i * m + (size_t)ids[(size_t)t]] != 0;
      }
    }
    printf("%s: %zu boxes (%zu not live) x %zu triangles = %zu pairs, %zu overlapping; %zu boxes' liveness, %zu pairs and %zu rows differ "
           "from the restatement; %zu node boxes x boxes, %zu rejected (%zu by the face gate behind a hull that passes), %zu gates differ, "
           "%zu overlapping triangles below a rejected node\n", argv[s], n, dead, m, pairs, overlapping, wrong_live, wrong, wrong_rows, slots,
           rejected, by_face, wrong_gate, lost);
    total += pairs, total_over += overlapping;
    if (wrong_live || wrong || wrong_rows || wrong_gate || lost) return 1;
  }
  printf("%zu pairs in all, %zu overlapping: 0 differences\n", total, total_over);
  return 0;
}
