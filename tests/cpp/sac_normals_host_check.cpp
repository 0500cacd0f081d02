// sac_normals_host_check.cpp -- icp_angle.h and icp_sac_normals.h compiled for the HOST (no HIP: a plain C++ compiler with
// -ffp-contract=off), so that tests/test_sac_normals_host.py can hold the expressions the kernels are built from against
// tests/sac_normals_restated.py bit for bit.
// usage: sac_normals_host_check <mode> <input.bin>      records of float32 (float64 for `terms`) in, hex words out, one line a record
//   angle   y x                                   -> A(y, x)
//   plane   coeff[4] q[3] m[3] w                  -> val
//   cyl     coeff[7] q[3] m[3] w                  -> val, on_axis
//   model   p1[3] n1[3] p2[3] n2[3]               -> ok, coeff[7]
//   terms   P[3] D[3] r ia ib q[3] (float64)      -> the 21 terms (float64)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../icpslam_amd/csrc/icp_sac_normals.h"

template <class T>
static std::vector<T> read_all(const char* path) {
  std::vector<T> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  T x;
  while (std::fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}
static void hex32(float v) {
  std::uint32_t w;
  std::memcpy(&w, &v, 4);
  std::printf(" %08x", w);
}
static void hex64(double v) {
  std::uint64_t w;
  std::memcpy(&w, &v, 8);
  std::printf(" %016llx", (unsigned long long)w);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  if (mode == "terms") {
    const std::vector<double> in = read_all<double>(argv[2]);
    for (std::size_t k = 0; k + 12 <= in.size(); k += 12) {
      double out[21];
      icpgpu::sacn_cyl_terms(&in[k], &in[k + 3], (int)in[k + 7], (int)in[k + 8], in[k + 6], (float)in[k + 9], (float)in[k + 10], (float)in[k + 11], out);
      for (double v : out) hex64(v);
      std::printf("\n");
    }
    return 0;
  }
  const std::vector<float> in = read_all<float>(argv[2]);
  const std::size_t width = mode == "angle" ? 2 : mode == "plane" ? 11 : mode == "cyl" ? 14 : mode == "model" ? 12 : 0;
  if (!width) return 2;
  for (std::size_t k = 0; k + width <= in.size(); k += width) {
    const float* r = &in[k];
    if (mode == "angle") {
      hex32(icpgpu::folded_angle(r[0], r[1]));
    } else if (mode == "plane") {
      hex32(icpgpu::sacn_plane_value(r, r[4], r[5], r[6], r[7], r[8], r[9], r[10]));
    } else if (mode == "cyl") {
      bool on_axis = false;
      hex32(icpgpu::sacn_cyl_value(r, r[7], r[8], r[9], r[10], r[11], r[12], r[13], &on_axis));
      std::printf(" %d", on_axis ? 1 : 0);
    } else {
      float co[7] = {0, 0, 0, 0, 0, 0, 0};
      const bool ok = icpgpu::sacn_cylinder_model(r, r + 3, r + 6, r + 9, co);
      std::printf(" %d", ok ? 1 : 0);
      for (float v : co) hex32(ok ? v : 0.f);
    }
    std::printf("\n");
  }
  return 0;
}
