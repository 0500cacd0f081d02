// rejectors_demo.cpp -- a PCL call site that adds correspondence rejectors, with the registration and rejector classes swapped for
// the shim's: median distance (factor 2) followed by one-to-one, PCL's spelling of every call.
// usage: rejectors_demo <src.bin> <n_src> <tgt.bin> <n_tgt> <max_iters> [p2plane]     (clouds: raw float32 records of four)
// prints: converged iterations n_correspondences median_distance T[16] (column-major, %.9g: every float round-trips)
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
static int run(const mock_pcl::PointCloud::Ptr& curr_cloud_, const mock_pcl::PointCloud::Ptr& prev_cloud_, double max_iters) {
  Icp icp;
  icp.setMaximumIterations(max_iters);
  icp.setTransformationEpsilon(1e-06);
  icp.setMaxCorrespondenceDistance(1.0);
  icp.setRANSACIterations(0);
  icpgpu::registration::CorrespondenceRejectorMedianDistance::Ptr rej_med(new icpgpu::registration::CorrespondenceRejectorMedianDistance);
  rej_med->setMedianFactor(2.0);
  icp.addCorrespondenceRejector(rej_med);
  icpgpu::registration::CorrespondenceRejectorOneToOne::Ptr rej_one(new icpgpu::registration::CorrespondenceRejectorOneToOne);
  icp.addCorrespondenceRejector(rej_one);
  icpgpu::registration::CorrespondenceRejectorTrimmed::Ptr rej_trim(new icpgpu::registration::CorrespondenceRejectorTrimmed);
  rej_trim->setOverlapRatio(0.5f);
  rej_trim->setMinCorrespondences(3);
  icp.addCorrespondenceRejector(rej_trim);
  if (icp.getCorrespondenceRejectors().size() != 3 || !icp.removeCorrespondenceRejector(2) || icp.removeCorrespondenceRejector(2)) return 4;
  icp.setInputSource(curr_cloud_);
  icp.setInputTarget(prev_cloud_);
  mock_pcl::PointCloud::Ptr out(new mock_pcl::PointCloud());
  icp.align(*out);
  const auto T = icp.getFinalTransformation();
  std::printf("%d %d %u %.9g", icp.hasConverged() ? 1 : 0, icp.getResult().iterations, icp.getResult().n_correspondences,
              rej_med->getMedianDistance());
  for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
  std::printf("\n");
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
