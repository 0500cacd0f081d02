// region_demo.cpp -- pcl::RegionGrowing's calls with the shim's class in its place, behind the VoxelGrid and the
// NormalEstimation of PCL's region growing tutorial: VoxelGrid -> NormalEstimation -> RegionGrowing -> extract, and beside it the
// EuclideanClusterExtraction of the same filtered cloud.
// usage: region_demo <cloud.bin> <n> <leaf> <k_normals> <k> <theta_degrees> <curvature> <min_size> <tolerance>
//   (cloud: raw float32 records of four).  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the normals: every point's nx, ny, nz, curvature as hex words
//   line 3: the number of regions
//   then one line per region: its indices ("-" for none)
//   then: every filtered point's label
//   then: for every 97th point, "index: getSegmentFromPoint's indices"
//   last line: the sizes of the euclidean clusters at <tolerance>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-ins with the members of pcl::PointXYZ / pcl::Normal / pcl::PointCloud (PCL is not in this image)
struct alignas(16) PointXYZ {
  float x, y, z, pad;
};
struct alignas(16) Normal {
  float normal_x, normal_y, normal_z, pad, curvature, pad2[3];
};
template <class PointT>
struct PointCloud {
  std::vector<PointT> points;
  unsigned width = 0, height = 0;
  bool is_dense = true;
  std::size_t size() const { return points.size(); }
  using Ptr = std::shared_ptr<PointCloud>;
};
}  // namespace mock_pcl
typedef mock_pcl::PointCloud<mock_pcl::PointXYZ> Cloud;
typedef mock_pcl::PointCloud<mock_pcl::Normal> Normals;

static Cloud::Ptr load(const char* path, std::size_t n) {
  auto c = std::make_shared<Cloud>();
  c->points.resize(n);
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  if (n && std::fread(c->points.data(), sizeof(mock_pcl::PointXYZ), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
  std::fclose(f);
  return c;
}

static void print_hex(const float* v, int count) {
  for (int e = 0; e < count; ++e) {
    std::uint32_t w;
    std::memcpy(&w, &v[e], 4);
    std::printf(" %08x", w);
  }
}

static void print_indices(const std::vector<int>& indices) {
  if (indices.empty()) std::printf("-");
  for (std::vector<int>::const_iterator pit = indices.begin(); pit != indices.end(); ++pit) std::printf(pit == indices.begin() ? "%d" : " %d", *pit);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const int k_normals = std::atoi(argv[4]), k = std::atoi(argv[5]);
  const float theta = (float)(std::atof(argv[6]) / 180.0 * M_PI), curvature = (float)std::atof(argv[7]);
  const int min_size = std::atoi(argv[8]);
  const double tolerance = std::atof(argv[9]);
  try {
    Cloud::Ptr cloud(new Cloud);
    icpgpu::VoxelGrid<Cloud> vg;
    vg.setInputCloud(raw);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*cloud);
    std::printf("%zu", cloud->points.size());
    for (const auto& p : cloud->points) {
      const float v[4] = {p.x, p.y, p.z, p.pad};
      print_hex(v, 4);
    }
    std::printf("\n");

    icpgpu::search::KdTree<Cloud>::Ptr tree(new icpgpu::search::KdTree<Cloud>);
    Normals::Ptr normals(new Normals);
    icpgpu::NormalEstimation<Cloud, Normals> normal_estimator;
    normal_estimator.setSearchMethod(tree);
    normal_estimator.setInputCloud(cloud);
    normal_estimator.setKSearch(k_normals);
    normal_estimator.compute(*normals);
    std::printf("%zu", normals->points.size());
    for (const auto& p : normals->points) {
      const float v[4] = {p.normal_x, p.normal_y, p.normal_z, p.curvature};
      print_hex(v, 4);
    }
    std::printf("\n");

    icpgpu::RegionGrowing<Cloud, Normals> reg;
    if (reg.getNumberOfNeighbours() != 30 || reg.getCurvatureThreshold() != 0.05f || reg.getMinClusterSize() != 1 ||
        reg.getMaxClusterSize() != 2147483647 || reg.getSmoothnessThreshold() != 30.0f / 180.0f * static_cast<float>(M_PI) ||
        !reg.getCurvatureTestFlag() || !reg.getSmoothModeFlag() || reg.getResidualTestFlag())
      return 4;
    reg.setMinClusterSize(min_size);
    reg.setMaxClusterSize(1000000);
    reg.setSearchMethod(tree);
    reg.setNumberOfNeighbours(k);
    reg.setInputCloud(cloud);
    reg.setInputNormals(normals);
    reg.setSmoothnessThreshold(theta);
    reg.setCurvatureThreshold(curvature);
    int thrown = 0;
    try { reg.setSmoothModeFlag(false); } catch (const std::invalid_argument&) { ++thrown; }
    try { reg.setResidualTestFlag(true); } catch (const std::invalid_argument&) { ++thrown; }
    if (thrown != 2) return 4;

    std::vector<icpgpu::PointIndices> clusters;
    reg.extract(clusters);
    std::printf("%zu\n", clusters.size());
    for (std::vector<icpgpu::PointIndices>::const_iterator it = clusters.begin(); it != clusters.end(); ++it) print_indices(it->indices);
    print_indices(reg.getLabels());
    for (std::size_t i = 0; i < cloud->points.size(); i += 97) {
      icpgpu::PointIndices segment;
      reg.getSegmentFromPoint((int)i, segment);
      std::printf("%zu: ", i);
      print_indices(segment.indices);
    }

    std::vector<icpgpu::PointIndices> components;
    icpgpu::EuclideanClusterExtraction<Cloud> ec;
    ec.setClusterTolerance(tolerance);
    ec.setInputCloud(cloud);
    ec.extract(components);
    std::vector<int> sizes;
    for (std::size_t r = 0; r < components.size(); ++r) sizes.push_back((int)components[r].indices.size());
    print_indices(sizes);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  return 0;
}
