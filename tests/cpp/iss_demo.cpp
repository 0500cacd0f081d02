// iss_demo.cpp -- pcl::ISSKeypoint3D's calls with the shim's class in its place, inside the front end of a global
// registration: VoxelGrid -> ISSKeypoint3D -> NormalEstimation -> FPFHEstimation at the keypoints over the filtered surface.
// usage: iss_demo <raw.bin> <n> <leaf> <salient_radius> <non_max_radius> <gamma_21> <gamma_32> <min_neighbors> <normals_k> <fpfh_radius>
// (the cloud: raw float32 records of four).  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the keypoints' indices into the filtered cloud: their number, then the indices
//   line 3: the keypoint cloud: its width, then every point's x, y, z, w as hex words
//   line 4: the filtered cloud's normals (setKSearch(normals_k), viewpoint at the origin): is_dense, then normal_x, normal_y, normal_z,
//           curvature as hex words
//   line 5: the keypoints' signatures over the filtered surface: is_dense, then 33 hex words per keypoint
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-ins with the members of pcl::PointXYZ / pcl::Normal / pcl::FPFHSignature33 / pcl::PointCloud (PCL is not in this image)
struct alignas(16) PointXYZ {
  float x, y, z, pad;
};
struct alignas(16) Normal {  // (pcl::Normal's layout: the normal in four floats, then the curvature)
  float normal_x, normal_y, normal_z, pad0;
  float curvature, pad1[3];
};
struct FPFHSignature33 {
  float histogram[33];
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
typedef mock_pcl::PointCloud<mock_pcl::FPFHSignature33> Signatures;

static Cloud::Ptr load(const char* path, std::size_t n) {
  auto c = std::make_shared<Cloud>();
  c->points.resize(n);
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  if (n && std::fread(c->points.data(), sizeof(mock_pcl::PointXYZ), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
  std::fclose(f);
  return c;
}

static void print_words(const float* v, int count) {
  for (int e = 0; e < count; ++e) {
    std::uint32_t w;
    std::memcpy(&w, &v[e], 4);
    std::printf(" %08x", w);
  }
}

static void print_cloud(const Cloud& c, std::size_t head) {
  std::printf("%zu", head);
  for (const auto& p : c.points) {
    const float v[4] = {p.x, p.y, p.z, p.pad};
    print_words(v, 4);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const double salient = std::atof(argv[4]), non_max = std::atof(argv[5]), gamma_21 = std::atof(argv[6]), gamma_32 = std::atof(argv[7]);
  const int min_neighbors = std::atoi(argv[8]), normals_k = std::atoi(argv[9]);
  const double fpfh_radius = std::atof(argv[10]);
  try {
    Cloud::Ptr filtered(new Cloud);
    icpgpu::VoxelGrid<Cloud> vg;                                   // was: pcl::VoxelGrid<pcl::PointXYZ>
    vg.setInputCloud(raw);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*filtered);
    print_cloud(*filtered, filtered->points.size());

    Cloud::Ptr keypoints(new Cloud);
    icpgpu::ISSKeypoint3D<Cloud> iss;                               // was: pcl::ISSKeypoint3D<pcl::PointXYZ, pcl::PointXYZ>
    iss.setSearchMethod(std::shared_ptr<int>());                    // (pcl::search::KdTree: accepted)
    iss.setInputCloud(filtered);
    iss.compute(*keypoints);                                        // PCL's default radii are 0: nothing comes out
    if (!keypoints->points.empty() || !iss.getKeypointsIndices()->indices.empty()) return 3;
    iss.setSalientRadius(salient);
    iss.setNonMaxRadius(non_max);
    iss.setThreshold21(gamma_21);
    iss.setThreshold32(gamma_32);
    iss.setMinNeighbors(min_neighbors);
    iss.setNormalRadius(4 * leaf);                                  // stored, without effect
    iss.setNumberOfThreads(4);
    iss.setBorderRadius(0.0);
    bool threw = false;
    try {
      iss.setBorderRadius(2 * leaf);                                // border estimation is not provided
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    if (!threw) return 4;
    iss.compute(*keypoints);
    icpgpu::PointIndices::ConstPtr indices = iss.getKeypointsIndices();
    if (indices->indices.size() != keypoints->points.size() || keypoints->width != keypoints->points.size()) return 5;
    std::printf("%zu", indices->indices.size());
    for (int i : indices->indices) std::printf(" %d", i);
    std::printf("\n");
    print_cloud(*keypoints, keypoints->width);

    Normals::Ptr normals(new Normals);
    icpgpu::NormalEstimation<Cloud, Normals> ne;                    // was: pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal>
    ne.setInputCloud(filtered);
    ne.setKSearch(normals_k);
    ne.compute(*normals);
    std::printf("%d", normals->is_dense ? 1 : 0);
    for (const auto& p : normals->points) {
      const float v[4] = {p.normal_x, p.normal_y, p.normal_z, p.curvature};
      print_words(v, 4);
    }
    std::printf("\n");

    Signatures at_keypoints;
    icpgpu::FPFHEstimation<Cloud, Normals, Signatures> fpfh;        // was: pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33>
    fpfh.setInputCloud(keypoints);                                  // ISSKeypoint3D's output cloud, as it is
    fpfh.setSearchSurface(filtered);
    fpfh.setInputNormals(normals);
    fpfh.setRadiusSearch(fpfh_radius);
    fpfh.compute(at_keypoints);
    if (at_keypoints.points.size() != keypoints->points.size()) return 6;
    std::printf("%d", at_keypoints.is_dense ? 1 : 0);
    for (const auto& p : at_keypoints.points) print_words(p.histogram, 33);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "iss_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
