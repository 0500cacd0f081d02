// outlier_demo.cpp -- the chain a LIDAR front end writes with PCL, the filter and registration classes swapped for the shim's
// (INTEGRATION.md): VoxelGrid -> StatisticalOutlierRemoval -> GICP, and a RadiusOutlierRemoval over the same down-sampled cloud.
// usage: outlier_demo <scan.bin> <n_scan> <tgt.bin> <n_tgt> <leaf> <mean_k> <stddev_mult> <radius> <min_pts> <filtered_out.bin>
// (clouds: raw float32 records of four).  Writes the statistical filter's output cloud to <filtered_out.bin> and prints
//   line 1: n_voxel n_kept_sor n_kept_ror is_dense_width_ok
//   line 2: the statistical filter's removed indices      line 3: the radius filter's removed indices
//   line 4: converged iterations T[16] (column-major, %.9g: every float round-trips)
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
  unsigned width = 0, height = 0;
  bool is_dense = false;
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

static void print_indices(const std::vector<int>& v) {
  for (std::size_t i = 0; i < v.size(); ++i) std::printf(i ? " %d" : "%d", v[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  auto scan = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  auto prev_cloud_ = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  const float leaf = (float)std::atof(argv[5]);
  try {
    mock_pcl::PointCloud::Ptr down(new mock_pcl::PointCloud()), curr_cloud_(new mock_pcl::PointCloud()), by_radius(new mock_pcl::PointCloud());
    icpgpu::VoxelGrid<mock_pcl::PointCloud> voxel_filter;
    voxel_filter.setInputCloud(scan);
    voxel_filter.setLeafSize(leaf, leaf, leaf);
    voxel_filter.filter(*down);

    icpgpu::StatisticalOutlierRemoval<mock_pcl::PointCloud> sor;
    sor.setInputCloud(down);
    sor.setMeanK(std::atoi(argv[6]));
    sor.setStddevMulThresh(std::atof(argv[7]));
    sor.filter(*curr_cloud_);

    icpgpu::RadiusOutlierRemoval<mock_pcl::PointCloud> ror;
    ror.setInputCloud(down);
    ror.setRadiusSearch(std::atof(argv[8]));
    ror.setMinNeighborsInRadius(std::atoi(argv[9]));
    ror.filter(*by_radius);

    const bool shape_ok = curr_cloud_->width == curr_cloud_->points.size() && curr_cloud_->height == 1 && curr_cloud_->is_dense;
    std::printf("%zu %zu %zu %d\n", down->size(), curr_cloud_->size(), by_radius->size(), shape_ok ? 1 : 0);
    print_indices(sor.getRemovedIndices());
    print_indices(ror.getRemovedIndices());
    FILE* f = std::fopen(argv[10], "wb");
    if (!f) { std::perror(argv[10]); return 2; }
    if (curr_cloud_->size()) std::fwrite(curr_cloud_->points.data(), sizeof(mock_pcl::PointXYZ), curr_cloud_->size(), f);
    std::fclose(f);

    icpgpu::GeneralizedIterativeClosestPoint<mock_pcl::PointCloud> icp;
    icp.setMaximumIterations(8);
    icp.setTransformationEpsilon(1e-06);
    icp.setMaxCorrespondenceDistance(1.0);
    icp.setRANSACIterations(0);
    icp.setInputSource(curr_cloud_);
    icp.setInputTarget(prev_cloud_);
    mock_pcl::PointCloud::Ptr out(new mock_pcl::PointCloud());
    icp.align(*out);
    const auto T = icp.getFinalTransformation();
    std::printf("%d %d", icp.hasConverged() ? 1 : 0, icp.getResult().iterations);
    for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
    std::printf("\n");
    // a refused call leaves the output empty, as PCL's error path does
    sor.setMeanK(0);
    sor.filter(*curr_cloud_);
    return curr_cloud_->size() == 0 && sor.getRemovedIndices().empty() ? 0 : 5;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
