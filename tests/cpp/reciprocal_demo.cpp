// reciprocal_demo.cpp -- a PCL call site that turns reciprocal correspondences on, with the registration classes swapped for the
// shim's: setUseReciprocalCorrespondences(true) followed by a trimmed rejector, PCL's spelling of every call.
// usage: reciprocal_demo <src.bin> <n_src> <tgt.bin> <n_tgt> <max_iters> [p2plane]     (clouds: raw float32 records of four)
// prints: converged iterations n_correspondences T[16] (column-major, %.9g: every float round-trips), then on a second line the
// same for a GeneralizedIterativeClosestPoint with the flag on and with it off (the flag is stored and changes nothing)
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

static mock_pcl::PointCloud::Ptr load(const char* path, std::size_t n) {
  auto c = std::make_shared<mock_pcl::PointCloud>();
  c->points.resize(n);
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  if (n && std::fread(c->points.data(), sizeof(mock_pcl::PointXYZ), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
  std::fclose(f);
  return c;
}

template <class Icp>
static void print(Icp& icp) {
  const auto T = icp.getFinalTransformation();
  std::printf("%d %d %u", icp.hasConverged() ? 1 : 0, icp.getResult().iterations, icp.getResult().n_correspondences);
  for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
}

template <class Icp>
static int run(const mock_pcl::PointCloud::Ptr& curr_cloud_, const mock_pcl::PointCloud::Ptr& prev_cloud_, double max_iters) {
  Icp icp;
  icp.setMaximumIterations(max_iters);
  icp.setTransformationEpsilon(1e-06);
  icp.setMaxCorrespondenceDistance(1.0);
  icp.setRANSACIterations(0);
  if (icp.getUseReciprocalCorrespondences()) return 4;  // PCL's default: off
  icp.setUseReciprocalCorrespondences(true);
  if (!icp.getUseReciprocalCorrespondences()) return 4;
  icpgpu::registration::CorrespondenceRejectorTrimmed::Ptr rej_trim(new icpgpu::registration::CorrespondenceRejectorTrimmed);
  rej_trim->setOverlapRatio(0.9f);
  icp.addCorrespondenceRejector(rej_trim);
  icp.setInputSource(curr_cloud_);
  icp.setInputTarget(prev_cloud_);
  mock_pcl::PointCloud::Ptr out(new mock_pcl::PointCloud());
  icp.align(*out);
  print(icp);
  std::printf("\n");
  // the flag on the classes that never read it
  for (int on = 1; on >= 0; --on) {
    icpgpu::GeneralizedIterativeClosestPoint<mock_pcl::PointCloud> gicp;
    gicp.setMaximumIterations(3);
    gicp.setUseReciprocalCorrespondences(on != 0);
    if (gicp.getUseReciprocalCorrespondences() != (on != 0)) return 4;
    gicp.setInputSource(curr_cloud_);
    gicp.setInputTarget(prev_cloud_);
    gicp.align(*out);
    print(gicp);
    std::printf(on ? " " : "\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  auto curr_cloud_ = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  auto prev_cloud_ = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  try {
    if (argc > 6) return run<icpgpu::IterativeClosestPointWithNormals<mock_pcl::PointCloud>>(curr_cloud_, prev_cloud_, std::atof(argv[5]));
    return run<icpgpu::IterativeClosestPoint<mock_pcl::PointCloud>>(curr_cloud_, prev_cloud_, std::atof(argv[5]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
