// search_demo.cpp -- pcl::search::KdTree's calls with the shim's class in its place: single-point, by-index and
// batched k-nearest and radius searches over one cloud.
// usage: search_demo <cloud.bin> <n> <queries.bin> <n_q> <k> <radius> <max_nn> <index>
// (clouds: raw float32 records of four).  Prints, one list per line ("-" for an empty one; distances as %.9g: every float round-trips)
//   lines 1-2: indices, squared distances of nearestKSearch(queries[0], k)       lines 3-4: of nearestKSearch(index, k)
//   lines 5-6: of radiusSearch(queries[0], radius)                               lines 7-8: of radiusSearch(index, radius, max_nn)
//   line 9: the four return values
//   lines 10-12: the batched nearestKSearch(queries, k): n_found, indices, squared distances (row-major)
//   lines 13-15: the batched radiusSearch(queries, radius, max_nn): row_start, indices, squared distances
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

template <class T>
static void print_list(const std::vector<T>& v, const char* fmt) {
  if (v.empty()) std::printf("-");
  for (std::size_t i = 0; i < v.size(); ++i) {
    if (i) std::printf(" ");
    std::printf(fmt, v[i]);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  auto cloud = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  auto queries = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  const int k = std::atoi(argv[5]);
  const double radius = std::atof(argv[6]);
  const unsigned max_nn = (unsigned)std::atoi(argv[7]);
  const int index = std::atoi(argv[8]);
  try {
    icpgpu::search::KdTree<mock_pcl::PointCloud> tree;
    tree.setInputCloud(cloud);
    std::vector<int> indices;
    std::vector<float> sqr_distances;
    int found[4];
    found[0] = tree.nearestKSearch(queries->points[0], k, indices, sqr_distances);
    print_list(indices, "%d"), print_list(sqr_distances, "%.9g");
    found[1] = tree.nearestKSearch(index, k, indices, sqr_distances);
    print_list(indices, "%d"), print_list(sqr_distances, "%.9g");
    found[2] = tree.radiusSearch(queries->points[0], radius, indices, sqr_distances);
    print_list(indices, "%d"), print_list(sqr_distances, "%.9g");
    found[3] = tree.radiusSearch(index, radius, indices, sqr_distances, max_nn);
    print_list(indices, "%d"), print_list(sqr_distances, "%.9g");
    std::printf("%d %d %d %d\n", found[0], found[1], found[2], found[3]);

    icpgpu::KdTreeFLANN<mock_pcl::PointCloud> flann;  // (the alias: the same class)
    flann.setInputCloud(cloud);
    std::vector<int> n_found;
    if (flann.nearestKSearch(*queries, k, indices, sqr_distances, n_found) != (int)queries->size()) return 4;
    print_list(n_found, "%d"), print_list(indices, "%d"), print_list(sqr_distances, "%.9g");
    std::vector<long long> row_start;
    if (flann.radiusSearch(*queries, radius, row_start, indices, sqr_distances, max_nn) != (int)queries->size()) return 4;
    print_list(row_start, "%lld"), print_list(indices, "%d"), print_list(sqr_distances, "%.9g");
    // a refused call finds nothing, and the tree goes on answering
    if (tree.nearestKSearch(index, 65, indices, sqr_distances) != 0 || !indices.empty()) return 5;
    if (tree.radiusSearch(index, -1.0, indices, sqr_distances) != 0 || !indices.empty()) return 5;
    return tree.nearestKSearch(index, 1, indices, sqr_distances) == 1 && indices[0] == index ? 0 : 5;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
