// tools/self_overlap_host_check.cpp -- self_crosses (ezrt_amd/csrc/hip/ezrt_device.h) compiled for the host and held against the
// numpy restatement on every pair of triangles of a scene.  Built and run by tools/self_overlap_host_check.py, which cuts the rules'
// sections out of ezrt_device.h into tri_rule.inc and writes <dir>/<scene>_{tri,cross}.bin; meant for -fsanitize=address,undefined.
// usage: self_overlap_host_check <dir> <scene> ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
#include "tri_rule.inc"
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
  for (int a = 2; a < argc; a++) {
    const std::string base = std::string(argv[1]) + "/" + argv[a];
    const std::vector<float> tri = load<float>(base + "_tri.bin");
    const std::vector<uint8_t> want = load<uint8_t>(base + "_cross.bin");
    const size_t m = tri.size() / 9;
    size_t pairs = 0, cross = 0, wrong = 0, dead = 0;
    if (want.size() != m * m) return 2;
    std::vector<float4> tg(m * 3); // the device's tri_geom rows: (p.xyz, unused)
    for (size_t k = 0; k < m; k++)
      for (int v = 0; v < 3; v++) tg[k * 3 + v] = float4{tri[k * 9 + v * 3], tri[k * 9 + v * 3 + 1], tri[k * 9 + v * 3 + 2], 0.0f};
    for (size_t i = 0; i < m; i++) {
      const float* t = &tri[i * 9];
      TriQuery Q;
      const bool live = tri_query(mk(t[0], t[1], t[2]), mk(t[3], t[4], t[5]), mk(t[6], t[7], t[8]), Q);
      dead += !live;
      for (size_t k = 0; k < m; k++) {
        const bool o = live && k != i && self_crosses(&tg[k * 3], Q);
        pairs++, cross += o, wrong += (o != (want[i * m + k] != 0));
      }
    }
    printf("%s: %zu triangles (%zu not live), %zu pairs, %zu crossings, %zu differ from the restatement\n", argv[a], m, dead, pairs, cross,
           wrong);
    if (wrong) return 1;
  }
  return 0;
}
