// segment_demo.cpp -- "where are the objects and how big are they" at the end of a LIDAR pipeline, with the shim's classes in PCL's
// places: VoxelGrid -> ProgressiveMorphologicalFilter -> ExtractIndices(setNegative(true)) ->
// EuclideanClusterExtraction -> MomentOfInertiaEstimation::computeClusters, which reads the clusters where the extraction left them on
// the device; then the PCL-spelled one-segment calls on the first cluster.
// usage: segment_demo <cloud.bin> <n> <leaf> <initial_distance> <tolerance> <min_size> <n_objects>   (cloud: raw float32 records of four).
// Exit status 5 unless the chain ends in n_objects clusters, 4 when the one-segment calls disagree with the first record.  Prints
//   line 1: the cloud the clusters index (voxel-filtered, ground removed): its size, then every point's x, y, z, w as hex words
//   line 2: the number of clusters
//   then one line per cluster: its indices
//   then one line per cluster: its icpgpu_segment_record as 100 hex words
//   last line: "one-segment calls agree"
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
struct Vector3f {  // Eigen::Vector3f's and Eigen::Vector4f's operator[]
  float v[3];
  float& operator[](int i) { return v[i]; }
};
struct Vector4f {
  float v[4];
  float& operator[](int i) { return v[i]; }
};
struct Matrix3f {  // Eigen::Matrix3f's operator()
  float m[9];
  float& operator()(int r, int c) { return m[3 * r + c]; }
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
  if (argc < 8) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const float initial_distance = (float)std::atof(argv[4]);
  const double tolerance = std::atof(argv[5]);
  const int min_size = std::atoi(argv[6]);
  const std::size_t n_objects = std::strtoull(argv[7], nullptr, 10);
  try {
    Cloud::Ptr filtered(new Cloud);
    icpgpu::VoxelGrid<Cloud> vg;
    vg.setInputCloud(raw);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*filtered);

    icpgpu::PointIndices::Ptr ground(new icpgpu::PointIndices);
    icpgpu::ProgressiveMorphologicalFilter<Cloud> pmf;
    pmf.setInputCloud(filtered);
    pmf.setInitialDistance(initial_distance);
    pmf.extract(ground->indices);
    if (ground->indices.empty()) return 4;

    Cloud::Ptr objects(new Cloud);
    icpgpu::ExtractIndices<Cloud> extract;
    extract.setInputCloud(filtered);
    extract.setIndices(ground);
    extract.setNegative(true);
    extract.filter(*objects);
    std::printf("%zu", objects->points.size());
    for (const auto& p : objects->points) {
      const float v[4] = {p.x, p.y, p.z, p.pad};
      for (int e = 0; e < 4; ++e) {
        std::uint32_t w;
        std::memcpy(&w, &v[e], 4);
        std::printf(" %08x", w);
      }
    }
    std::printf("\n");

    std::vector<icpgpu::PointIndices> cluster_indices;
    icpgpu::EuclideanClusterExtraction<Cloud> ec;
    ec.setClusterTolerance(tolerance);
    ec.setMinClusterSize(min_size);
    ec.setMaxClusterSize(2147483647);
    ec.setInputCloud(objects);
    ec.extract(cluster_indices);
    std::printf("%zu\n", cluster_indices.size());
    for (const auto& cl : cluster_indices) {
      for (std::size_t k = 0; k < cl.indices.size(); ++k) std::printf(k ? " %d" : "%d", cl.indices[k]);
      std::printf("\n");
    }

    icpgpu::MomentOfInertiaEstimation<Cloud> boxes;
    boxes.computeClusters(ec);   // no indices travel: the clusters are read where ec left them
    const std::vector<icpgpu_segment_record>& records = boxes.getRecords();
    if (records.size() != cluster_indices.size()) return 4;
    for (const icpgpu_segment_record& r : records) {
      std::uint32_t w[sizeof(icpgpu_segment_record) / 4];
      std::memcpy(w, &r, sizeof r);
      for (std::size_t e = 0; e < sizeof w / sizeof w[0]; ++e) std::printf(e ? " %08x" : "%08x", w[e]);
      std::printf("\n");
    }
    if (records.size() != n_objects) return 5;

    // PCL's spelling for one cluster, and the per-cluster functions that usually follow a clustering
    const icpgpu_segment_record& first = records[0];
    icpgpu::PointIndices::Ptr one(new icpgpu::PointIndices(cluster_indices[0]));
    icpgpu::MomentOfInertiaEstimation<Cloud> feature_extractor;
    feature_extractor.setInputCloud(objects);
    feature_extractor.setIndices(one);
    feature_extractor.compute();
    mock_pcl::PointXYZ min_point_AABB, max_point_AABB, min_point_OBB, max_point_OBB, position_OBB;
    mock_pcl::Matrix3f rotational_matrix_OBB, covariance;
    mock_pcl::Vector3f major_vector, middle_vector, minor_vector, mass_center;
    mock_pcl::Vector4f lo, hi, centroid, centroid2;
    float major_value, middle_value, minor_value;
    if (!feature_extractor.getAABB(min_point_AABB, max_point_AABB) ||
        !feature_extractor.getOBB(min_point_OBB, max_point_OBB, position_OBB, rotational_matrix_OBB) ||
        !feature_extractor.getEigenValues(major_value, middle_value, minor_value) ||
        !feature_extractor.getEigenVectors(major_vector, middle_vector, minor_vector) || !feature_extractor.getMassCenter(mass_center))
      return 4;
    if (std::memcmp(&feature_extractor.getRecords()[0], &first, sizeof first) != 0) return 4;   // the HOST source gives the device source's bits
    icpgpu::getMinMax3D(*objects, one->indices, lo, hi);
    const unsigned m = icpgpu::compute3DCentroid(*objects, one->indices, centroid);
    const unsigned m2 = icpgpu::computeMeanAndCovarianceMatrix(*objects, one->indices, covariance, centroid2);
    bool same = m == (unsigned)first.count && m2 == m && max_point_OBB.x == (float)(first.obb_dims[0] / 2.0) && min_point_OBB.z == -(float)(first.obb_dims[2] / 2.0) &&
                position_OBB.y == (float)first.obb_position[1] && major_value == (float)first.eigenvalues[0] && minor_value == (float)first.eigenvalues[2];
    for (int k = 0; k < 3; ++k) {
      same = same && lo[k] == first.aabb_min[k] && hi[k] == first.aabb_max[k] && centroid[k] == (float)first.centroid[k] && centroid2[k] == centroid[k] &&
             mass_center[k] == centroid[k] && major_vector[k] == (float)first.axes[k] && middle_vector[k] == (float)first.axes[3 + k] &&
             minor_vector[k] == (float)first.axes[6 + k] && rotational_matrix_OBB(k, 0) == major_vector[k] && rotational_matrix_OBB(k, 2) == minor_vector[k];
    }
    same = same && min_point_AABB.z == first.aabb_min[2] && max_point_AABB.x == first.aabb_max[0] && covariance(0, 1) == (float)first.cov[1] &&
           covariance(2, 2) == (float)first.cov[5] && covariance(1, 0) == covariance(0, 1) && centroid[3] == 1.f && lo[3] == 0.f;
    if (!same) return 4;
    bool threw = false;
    try {
      std::vector<float> moment;
      feature_extractor.getMomentOfInertia(moment);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    if (!threw) return 4;
    std::printf("one-segment calls agree\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  return 0;
}
