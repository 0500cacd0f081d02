// cluster_demo.cpp -- pcl::EuclideanClusterExtraction's calls with the shim's class in its place, behind the
// VoxelGrid of every PCL scan pipeline: VoxelGrid -> EuclideanClusterExtraction -> extract.
// usage: cluster_demo <cloud.bin> <n> <leaf> <tolerance> <min_size> <max_size>     (cloud: raw float32 records of four).  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the number of clusters
//   then one line per cluster: its indices ("-" for none)
//   last line: every filtered point's label
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-ins with the members of pcl::PointXYZ / pcl::PointCloud / pcl::search::KdTree (PCL is not in this image)
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

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const double tolerance = std::atof(argv[4]);
  const int min_size = std::atoi(argv[5]), max_size = std::atoi(argv[6]);
  try {
    Cloud::Ptr filtered(new Cloud);
    icpgpu::VoxelGrid<Cloud> vg;
    vg.setInputCloud(raw);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*filtered);
    std::printf("%zu", filtered->points.size());
    for (const auto& p : filtered->points) {
      const float v[4] = {p.x, p.y, p.z, p.pad};
      for (int e = 0; e < 4; ++e) {
        std::uint32_t w;
        std::memcpy(&w, &v[e], 4);
        std::printf(" %08x", w);
      }
    }
    std::printf("\n");

    icpgpu::search::KdTree<Cloud>::Ptr tree(new icpgpu::search::KdTree<Cloud>);
    tree->setInputCloud(filtered);
    std::vector<icpgpu::PointIndices> cluster_indices;
    icpgpu::EuclideanClusterExtraction<Cloud> ec;
    if (ec.getClusterTolerance() != 0.0 || ec.getMinClusterSize() != 1 || ec.getMaxClusterSize() != 2147483647) return 4;
    ec.setClusterTolerance(tolerance);
    ec.setMinClusterSize(min_size);
    ec.setMaxClusterSize(max_size);
    ec.setSearchMethod(tree);
    ec.setInputCloud(filtered);
    ec.extract(cluster_indices);
    if (ec.getClusterTolerance() != tolerance || ec.getMinClusterSize() != min_size || ec.getMaxClusterSize() != max_size) return 4;

    std::printf("%zu\n", cluster_indices.size());
    for (std::vector<icpgpu::PointIndices>::const_iterator it = cluster_indices.begin(); it != cluster_indices.end(); ++it) {
      if (it->indices.empty()) std::printf("-");
      for (std::vector<int>::const_iterator pit = it->indices.begin(); pit != it->indices.end(); ++pit)
        std::printf(pit == it->indices.begin() ? "%d" : " %d", *pit);
      std::printf("\n");
    }
    const std::vector<int>& labels = ec.getLabels();
    if (labels.empty()) std::printf("-");
    for (std::size_t i = 0; i < labels.size(); ++i) std::printf(i ? " %d" : "%d", labels[i]);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  return 0;
}
