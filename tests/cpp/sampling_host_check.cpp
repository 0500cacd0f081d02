// sampling_host_check.cpp -- icp_sampling.h (the cropping and sampling filters' arithmetic, shared by the kernels and the host)
// compiled by a plain C++ compiler, for tests/test_sampling_host.py to hold against tests/sampling_restated.py.
//   sampling_host_check MODE FILE     FILE: float32 records; one line of output per record
//     pass   x y z field lo hi negative                  -> keep
//     crop   T[12] x y z min[3] max[3] negative has_T    -> keep q.x q.y q.z (bits, hex)
//     cell   x y z leaf                                  -> cell.x cell.y cell.z d2 (bits, hex) uniform_key(d2, record number) (hex)
//     far    qx qy qz px py pz                            -> d2 (bits, hex) fps_key(d2, record number) (hex) and the key's two halves back
//   sampling_host_check seed SEED N                      -> the generator's draw over N rows
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../icpslam_amd/csrc/icp_sampling.h"

using namespace icpgpu;

static std::vector<float> read_all(const char* path) {
  std::vector<float> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  float buf[1024];
  size_t got;
  while ((got = std::fread(buf, sizeof(float), 1024, f)) > 0) v.insert(v.end(), buf, buf + got);
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const char* mode = argv[1];
  if (!std::strcmp(mode, "seed")) {
    if (argc < 4) return 2;
    std::printf("%llu\n", sampling_seed_draw(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10)));
    return 0;
  }
  const std::vector<float> v = read_all(argv[2]);
  const size_t width = !std::strcmp(mode, "pass") ? 7 : !std::strcmp(mode, "crop") ? 23 : !std::strcmp(mode, "cell") ? 4 : !std::strcmp(mode, "far") ? 6 : 0;
  if (!width || v.size() % width) return 2;
  for (size_t r = 0; r < v.size() / width; ++r) {
    const float* p = v.data() + r * width;
    if (width == 7) {
      std::printf("%d\n", pass_through_keep(p[0], p[1], p[2], (int)p[3], p[4], p[5], (int)p[6]));
    } else if (width == 23) {
      float q[3] = {p[12], p[13], p[14]};
      if (p[22] != 0.f) sampling_xform(p, p[12], p[13], p[14], q);
      std::printf("%d %08x %08x %08x\n", crop_box_keep(p[12], p[13], p[14], q, p + 15, p + 18, (int)p[21]), sampling_float_bits(q[0]),
                  sampling_float_bits(q[1]), sampling_float_bits(q[2]));
    } else if (width == 4) {
      int cell[3];
      const float d2 = uniform_cell(p[0], p[1], p[2], 1.0f / p[3], p[3], cell);
      std::printf("%d %d %d %08x %016llx\n", cell[0], cell[1], cell[2], sampling_float_bits(d2), uniform_key(d2, (int)r));
    } else {
      const float d2 = fps_d2(p[0], p[1], p[2], p[3], p[4], p[5]);
      const unsigned long long key = fps_key(d2, (int)r);
      std::printf("%08x %016llx %d %08x\n", sampling_float_bits(d2), key, fps_key_index(key), sampling_float_bits(fps_key_measure(key)));
    }
  }
  return 0;
}
