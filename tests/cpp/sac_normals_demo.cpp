// sac_normals_demo.cpp -- PCL's cylinder segmentation recipe with the shim's classes in PCL's places:
// VoxelGrid -> NormalEstimation -> SACSegmentationFromNormals(SACMODEL_NORMAL_PLANE) -> ExtractIndices(setNegative(true)) ->
// NormalEstimation -> SACSegmentationFromNormals(SACMODEL_CYLINDER, a vertical axis, radius limits).
// usage: sac_normals_demo <cloud.bin> <n> <leaf> <k_normals> <plane_threshold> <cylinder_threshold> <radius_min> <radius_max> <eps_angle> <seed>
// (cloud: raw float32 records of four).  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the plane: the four coefficients as hex words, the iterations, the number of inliers
//   line 3: the plane's inliers
//   line 4: the cylinder: the seven coefficients as hex words, the iterations, the number of inliers
//   line 5: the cylinder's inliers (indices into the cloud without the plane)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

static void print_hex(const float* v, int n) {
  for (int e = 0; e < n; ++e) {
    std::uint32_t w;
    std::memcpy(&w, &v[e], 4);
    std::printf(" %08x", w);
  }
}

static Normals::Ptr normals_of(const Cloud::Ptr& cloud, int k) {
  icpgpu::search::KdTree<Cloud>::Ptr tree(new icpgpu::search::KdTree<Cloud>);
  Normals::Ptr normals(new Normals);
  icpgpu::NormalEstimation<Cloud, Normals> ne;
  ne.setSearchMethod(tree);
  ne.setInputCloud(cloud);
  ne.setKSearch(k);
  ne.setViewPoint(0.f, 0.f, 3.f);
  ne.compute(*normals);
  return normals;
}

static void print_result(const icpgpu::ModelCoefficients& co, int iterations, const icpgpu::PointIndices& in) {
  print_hex(co.values.data(), (int)co.values.size());
  std::printf(" %d %zu\n", iterations, in.indices.size());
  for (std::size_t k = 0; k < in.indices.size(); ++k) std::printf(k ? " %d" : "%d", in.indices[k]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const int k_normals = std::atoi(argv[4]);
  const double plane_threshold = std::atof(argv[5]), cylinder_threshold = std::atof(argv[6]);
  const double radius_min = std::atof(argv[7]), radius_max = std::atof(argv[8]), eps_angle = std::atof(argv[9]);
  const unsigned long long seed = std::strtoull(argv[10], nullptr, 10);
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

    Normals::Ptr normals = normals_of(filtered, k_normals);
    icpgpu::ModelCoefficients::Ptr plane(new icpgpu::ModelCoefficients), cylinder(new icpgpu::ModelCoefficients);
    icpgpu::PointIndices::Ptr plane_inliers(new icpgpu::PointIndices), cylinder_inliers(new icpgpu::PointIndices);
    icpgpu::SACSegmentationFromNormals<Cloud, Normals> seg;
    double r0 = -1.0, r1 = -1.0;
    seg.getRadiusLimits(r0, r1);
    if (seg.getDistanceThreshold() != 0.0 || seg.getMaxIterations() != 50 || seg.getProbability() != 0.99 || !seg.getOptimizeCoefficients() ||
        seg.getModelType() != icpgpu::SACMODEL_NORMAL_PLANE || seg.getMethodType() != icpgpu::SAC_RANSAC || seg.getNormalDistanceWeight() != 0.1 ||
        r0 != 0.0 || r1 != 0.0)
      return 4;  // PCL's defaults
    seg.setOptimizeCoefficients(true);
    seg.setModelType(icpgpu::SACMODEL_NORMAL_PLANE);
    seg.setNormalDistanceWeight(0.1);
    seg.setMethodType(icpgpu::SAC_RANSAC);
    seg.setMaxIterations(100);
    seg.setDistanceThreshold(plane_threshold);
    seg.setSeed(seed);
    seg.setInputCloud(filtered);
    seg.setInputNormals(normals);
    seg.segment(*plane_inliers, *plane);
    if (plane->values.size() != 4 || plane_inliers->indices.empty()) return 4;
    print_result(*plane, seg.getIterations(), *plane_inliers);

    Cloud::Ptr rest(new Cloud);
    icpgpu::ExtractIndices<Cloud> extract;
    extract.setInputCloud(filtered);
    extract.setIndices(plane_inliers);
    extract.setNegative(true);
    extract.filter(*rest);
    if (rest->points.size() + plane_inliers->indices.size() != filtered->points.size()) return 4;

    Normals::Ptr rest_normals = normals_of(rest, k_normals);
    const float up[3] = {0.f, 0.f, 1.f};
    seg.setModelType(icpgpu::SACMODEL_CYLINDER);
    seg.setMaxIterations(1000);
    seg.setDistanceThreshold(cylinder_threshold);
    seg.setRadiusLimits(radius_min, radius_max);
    seg.setAxis(up);
    seg.setEpsAngle(eps_angle);
    seg.setInputCloud(rest);
    seg.setInputNormals(rest_normals);
    seg.segment(*cylinder_inliers, *cylinder);
    if (cylinder->values.size() != 7 || cylinder_inliers->indices.empty()) return 5;
    print_result(*cylinder, seg.getIterations(), *cylinder_inliers);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  return 0;
}
