// sac_demo.cpp -- the ground removal of a LIDAR pipeline with the shim's classes in PCL's places:
// VoxelGrid -> SACSegmentation(SACMODEL_PLANE, SAC_RANSAC) -> ExtractIndices(setNegative(true)) -> EuclideanClusterExtraction, and
// beside it the same clustering WITHOUT the ground removal.
// usage: sac_demo <cloud.bin> <n> <leaf> <distance_threshold> <seed> <tolerance> <min_size> <n_objects>   (cloud: raw float32 records of
// four).  Exit status 5 unless the objects come out as n_objects separate clusters and, without the ground removal, everything is ONE
// component larger than the largest object.  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the plane: the four coefficients as hex words, the iterations, the number of inliers
//   line 3: the inliers ("-" for none)
//   line 4: the number of points left, the number of clusters among them
//   then one line per cluster: its size and its bounding box in x and y (min x, max x, min y, max y)
//   last line: the cluster sizes without the ground removal
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-ins with the members of pcl::PointXYZ / pcl::PointCloud (PCL is not in this image)
struct alignas(16) PointXYZ {
  float x, y, z, pad;
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

static Cloud::Ptr load(const char* path, std::size_t n) {
  auto c = std::make_shared<Cloud>();
  c->points.resize(n);
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  if (n && std::fread(c->points.data(), sizeof(mock_pcl::PointXYZ), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
  std::fclose(f);
  return c;
}

static void print_hex(const float* v, int n) {
  for (int e = 0; e < n; ++e) {
    std::uint32_t w;
    std::memcpy(&w, &v[e], 4);
    std::printf(" %08x", w);
  }
}

static std::vector<icpgpu::PointIndices> clusters_of(const Cloud::Ptr& cloud, double tolerance, int min_size) {
  icpgpu::search::KdTree<Cloud>::Ptr tree(new icpgpu::search::KdTree<Cloud>);
  tree->setInputCloud(cloud);
  std::vector<icpgpu::PointIndices> cluster_indices;
  icpgpu::EuclideanClusterExtraction<Cloud> ec;
  ec.setClusterTolerance(tolerance);
  ec.setMinClusterSize(min_size);
  ec.setMaxClusterSize(2147483647);
  ec.setSearchMethod(tree);
  ec.setInputCloud(cloud);
  ec.extract(cluster_indices);
  return cluster_indices;
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const double threshold = std::atof(argv[4]);
  const unsigned long long seed = std::strtoull(argv[5], nullptr, 10);
  const double tolerance = std::atof(argv[6]);
  const int min_size = std::atoi(argv[7]);
  const std::size_t n_objects = std::strtoull(argv[8], nullptr, 10);
  try {
    Cloud::Ptr filtered(new Cloud);
    icpgpu::VoxelGrid<Cloud> vg;
    vg.setInputCloud(raw);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*filtered);
    std::printf("%zu", filtered->points.size());
    for (const auto& p : filtered->points) {
      const float v[4] = {p.x, p.y, p.z, p.pad};
      print_hex(v, 4);
    }
    std::printf("\n");

    icpgpu::ModelCoefficients::Ptr coefficients(new icpgpu::ModelCoefficients);
    icpgpu::PointIndices::Ptr inliers(new icpgpu::PointIndices);
    icpgpu::SACSegmentation<Cloud> seg;
    if (seg.getDistanceThreshold() != 0.0 || seg.getMaxIterations() != 50 || seg.getProbability() != 0.99 || !seg.getOptimizeCoefficients() ||
        seg.getModelType() != icpgpu::SACMODEL_PLANE || seg.getMethodType() != icpgpu::SAC_RANSAC)
      return 4;  // PCL's defaults
    seg.setOptimizeCoefficients(true);
    seg.setModelType(icpgpu::SACMODEL_PLANE);
    seg.setMethodType(icpgpu::SAC_RANSAC);
    seg.setMaxIterations(100);
    seg.setDistanceThreshold(threshold);
    seg.setSeed(seed);
    seg.setInputCloud(filtered);
    seg.segment(*inliers, *coefficients);
    if (coefficients->values.size() != 4 || inliers->indices.empty()) return 4;
    print_hex(coefficients->values.data(), 4);
    std::printf(" %d %zu\n", seg.getIterations(), inliers->indices.size());
    for (std::size_t k = 0; k < inliers->indices.size(); ++k) std::printf(k ? " %d" : "%d", inliers->indices[k]);
    std::printf("\n");

    Cloud::Ptr objects(new Cloud);
    icpgpu::ExtractIndices<Cloud> extract;
    extract.setInputCloud(filtered);
    extract.setIndices(inliers);
    extract.setNegative(true);
    extract.filter(*objects);
    if (objects->points.size() + inliers->indices.size() != filtered->points.size()) return 4;

    const std::vector<icpgpu::PointIndices> with = clusters_of(objects, tolerance, min_size);
    std::printf("%zu %zu\n", objects->points.size(), with.size());
    std::size_t largest_object = 0;
    for (const auto& cl : with) {
      float bx[4] = {1e30f, -1e30f, 1e30f, -1e30f};
      for (int i : cl.indices) {
        const auto& p = objects->points[(std::size_t)i];
        bx[0] = std::min(bx[0], p.x), bx[1] = std::max(bx[1], p.x), bx[2] = std::min(bx[2], p.y), bx[3] = std::max(bx[3], p.y);
      }
      std::printf("%zu %.3f %.3f %.3f %.3f\n", cl.indices.size(), bx[0], bx[1], bx[2], bx[3]);
      largest_object = std::max(largest_object, cl.indices.size());
    }
    const std::vector<icpgpu::PointIndices> without = clusters_of(filtered, tolerance, min_size);
    for (std::size_t k = 0; k < without.size(); ++k) std::printf(k ? " %zu" : "%zu", without[k].indices.size());
    std::printf("\n");
    if (with.size() != n_objects) return 5;                                           // the objects, each on its own
    if (without.size() != 1 || without[0].indices.size() <= largest_object) return 5;  // the ground joins them all
    if (without[0].indices.size() != filtered->points.size()) return 5;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  return 0;
}
