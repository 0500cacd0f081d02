// pmf_demo.cpp -- the ground removal of a LIDAR pipeline where the ground is no plane, with the shim's classes in PCL's places
// (INTEGRATION.md): VoxelGrid -> ProgressiveMorphologicalFilter -> ExtractIndices(setNegative(true)) -> EuclideanClusterExtraction, and
// beside it the same chain with SACSegmentation(SACMODEL_PLANE) in the filter's place at the filter's initial distance.
// usage: pmf_demo <cloud.bin> <n> <leaf> <threshold> <seed> <tolerance> <min_size> <n_objects>   (cloud: raw float32 records of four).
// Exit status 5 unless the filter's chain ends in n_objects clusters and the plane's chain does not.  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the passes, the number of ground points
//   line 3: the ground's indices ("-" for none)
//   line 4: the OPEN of the filtered cloud at a window of 3 (icpgpu::applyMorphologicalOperator): every z as a hex word
//   line 5: the number of points left, the number of clusters among them
//   then one line per cluster: its size and its bounding box in x and y (min x, max x, min y, max y)
//   last line: the plane's chain: its inliers, the points left, the cluster sizes among them
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

static Cloud::Ptr without(const Cloud::Ptr& cloud, const icpgpu::PointIndices::Ptr& indices) {
  Cloud::Ptr rest(new Cloud);
  icpgpu::ExtractIndices<Cloud> extract;
  extract.setInputCloud(cloud);
  extract.setIndices(indices);
  extract.setNegative(true);
  extract.filter(*rest);
  return rest;
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

    icpgpu::PointIndices::Ptr ground(new icpgpu::PointIndices);
    icpgpu::ProgressiveMorphologicalFilter<Cloud> pmf;
    if (pmf.getMaxWindowSize() != 33 || pmf.getSlope() != 0.7f || pmf.getMaxDistance() != 10.0f || pmf.getInitialDistance() != 0.15f ||
        pmf.getCellSize() != 1.0f || pmf.getBase() != 2.0f || !pmf.getExponential())
      return 4;  // PCL's defaults
    pmf.setInputCloud(filtered);
    pmf.setMaxWindowSize(33);
    pmf.setSlope(0.7f);
    pmf.setInitialDistance((float)threshold);
    pmf.setMaxDistance(10.0f);
    pmf.setCellSize(1.0f);
    pmf.setBase(2.0f);
    pmf.setExponential(true);
    pmf.extract(ground->indices);
    if (ground->indices.empty()) return 4;
    std::printf("%d %zu\n", pmf.getPasses(), ground->indices.size());
    for (std::size_t k = 0; k < ground->indices.size(); ++k) std::printf(k ? " %d" : "%d", ground->indices[k]);
    std::printf("\n");

    Cloud opened;
    icpgpu::applyMorphologicalOperator(filtered, 3.0f, icpgpu::MORPH_OPEN, opened);
    if (opened.points.size() != filtered->points.size()) return 4;
    for (const auto& p : opened.points) print_hex(&p.z, 1);
    std::printf("\n");

    Cloud::Ptr objects = without(filtered, ground);
    if (objects->points.size() + ground->indices.size() != filtered->points.size()) return 4;
    const std::vector<icpgpu::PointIndices> with = clusters_of(objects, tolerance, min_size);
    std::printf("%zu %zu\n", objects->points.size(), with.size());
    for (const auto& cl : with) {
      float bx[4] = {1e30f, -1e30f, 1e30f, -1e30f};
      for (int i : cl.indices) {
        const auto& p = objects->points[(std::size_t)i];
        bx[0] = std::min(bx[0], p.x), bx[1] = std::max(bx[1], p.x), bx[2] = std::min(bx[2], p.y), bx[3] = std::max(bx[3], p.y);
      }
      std::printf("%zu %.3f %.3f %.3f %.3f\n", cl.indices.size(), bx[0], bx[1], bx[2], bx[3]);
    }

    // the same chain with the plane in the filter's place
    icpgpu::ModelCoefficients::Ptr coefficients(new icpgpu::ModelCoefficients);
    icpgpu::PointIndices::Ptr inliers(new icpgpu::PointIndices);
    icpgpu::SACSegmentation<Cloud> seg;
    seg.setModelType(icpgpu::SACMODEL_PLANE);
    seg.setMethodType(icpgpu::SAC_RANSAC);
    seg.setMaxIterations(100);
    seg.setDistanceThreshold(threshold);
    seg.setSeed(seed);
    seg.setInputCloud(filtered);
    seg.segment(*inliers, *coefficients);
    Cloud::Ptr rest = without(filtered, inliers);
    const std::vector<icpgpu::PointIndices> plane = clusters_of(rest, tolerance, min_size);
    std::printf("%zu %zu", inliers->indices.size(), rest->points.size());
    for (const auto& cl : plane) std::printf(" %zu", cl.indices.size());
    std::printf("\n");
    if (with.size() != n_objects) return 5;    // the objects, each on its own
    if (plane.size() == n_objects) return 5;   // the plane leaves ground behind that joins or outnumbers them
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  return 0;
}
