// ndt_demo.cpp -- the reference's call site (icp_odometer.cpp:186-201) with the registration class swapped for
// icpgpu::NormalDistributionsTransform, PCL's NDT defaults otherwise.
// usage: ndt_demo <src.bin> <n_src> <tgt.bin> <n_tgt> <resolution> [<guess.bin>]
//        (clouds: raw float32 records of four; guess: 16 float32, column-major)
// prints: converged iterations transformation_probability fitness T[16] (column-major, %.9g: every float round-trips)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-in with the memory layout of pcl::PointXYZ / pcl::PointCloud (PCL is not in this image)
struct alignas(16) PointXYZ {
  float x, y, z, pad;
};
struct PointCloud {
  std::vector<PointXYZ> points;
  std::size_t size() const { return points.size(); }
  using Ptr = std::shared_ptr<PointCloud>;
};
}  // namespace mock_pcl

static void read_floats(const char* path, void* dst, std::size_t bytes) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  if (bytes && std::fread(dst, 1, bytes, f) != bytes) { std::fprintf(stderr, "short read\n"); std::exit(2); }
  std::fclose(f);
}

static mock_pcl::PointCloud::Ptr load(const char* path, std::size_t n) {
  auto c = std::make_shared<mock_pcl::PointCloud>();
  c->points.resize(n);
  read_floats(path, c->points.data(), n * sizeof(mock_pcl::PointXYZ));
  return c;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  auto curr_cloud_ = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  auto prev_cloud_ = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  try {
    icpgpu::NormalDistributionsTransform<mock_pcl::PointCloud> ndt;
    if (ndt.getMaximumIterations() != 35 || ndt.getTransformationEpsilon() != 0.1 || ndt.getStepSize() != 0.1 ||
        ndt.getOulierRatio() != 0.55 || ndt.getResolution() != 1.0f) {
      std::fprintf(stderr, "not PCL's NDT defaults\n");
      return 4;
    }
    ndt.setResolution(static_cast<float>(std::atof(argv[5])));
    ndt.setInputSource(curr_cloud_);
    ndt.setInputTarget(prev_cloud_);
    mock_pcl::PointCloud::Ptr out(new mock_pcl::PointCloud());
    if (argc > 6) {
      float g[16];
      read_floats(argv[6], g, sizeof g);
      ndt.align(*out, icpgpu::make_matrix4(g));
    } else {
      ndt.align(*out);
    }
    const auto T = ndt.getFinalTransformation();
    std::printf("%d %d %.17g %.17g", ndt.hasConverged() ? 1 : 0, ndt.getFinalNumIteration(), ndt.getTransformationProbability(),
                ndt.getFitnessScore());
    for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
