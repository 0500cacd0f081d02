// fpfh_demo.cpp -- pcl::FPFHEstimation's calls with the shim's class in its place, behind the front end every PCL
// feature pipeline has: VoxelGrid -> NormalEstimation -> FPFHEstimation at keypoints over the denser, filtered surface.
// usage: fpfh_demo <raw.bin> <n> <leaf> <normals_k> <keypoints.bin> <n_key> <k> <radius>   (clouds: raw float32 records of four;
// exactly one of k and radius is not 0).  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: its normals (setKSearch(normals_k), viewpoint at the origin): is_dense, then normal_x, normal_y, normal_z, curvature as hex words
//   line 3: the keypoints' signatures over the filtered surface: is_dense, then 33 hex words per keypoint
//   line 4: the filtered cloud's own signatures (no search surface), the same way
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

static void print_signatures(const Signatures& out) {
  std::printf("%d", out.is_dense ? 1 : 0);
  for (const auto& p : out.points) print_words(p.histogram, 33);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const int normals_k = std::atoi(argv[4]);
  auto keypoints = load(argv[5], std::strtoull(argv[6], nullptr, 10));
  const int k = std::atoi(argv[7]);
  const double radius = std::atof(argv[8]);
  static_assert(sizeof(icpgpu::FPFHSignature33) == 33 * sizeof(float), "icpgpu::FPFHSignature33 is pcl::FPFHSignature33's histogram");
  try {
    Cloud::Ptr filtered(new Cloud);
    icpgpu::VoxelGrid<Cloud> vg;                                   // was: pcl::VoxelGrid<pcl::PointXYZ>
    vg.setInputCloud(raw);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*filtered);
    std::printf("%zu", filtered->points.size());
    for (const auto& p : filtered->points) {
      const float v[4] = {p.x, p.y, p.z, p.pad};
      print_words(v, 4);
    }
    std::printf("\n");

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

    Signatures at_keypoints, own;
    icpgpu::FPFHEstimation<Cloud, Normals, Signatures> fpfh;        // was: pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33>
    fpfh.setInputCloud(keypoints);
    fpfh.setSearchSurface(filtered);
    fpfh.setInputNormals(normals);                                  // NormalEstimation's output cloud, as it is
    fpfh.setSearchMethod(std::shared_ptr<int>());                   // (pcl::search::KdTree: accepted)
    if (k) fpfh.setKSearch(k);
    if (radius != 0.0) fpfh.setRadiusSearch(radius);
    fpfh.compute(at_keypoints);
    if (at_keypoints.points.size() != keypoints->points.size() || at_keypoints.width != keypoints->points.size()) return 3;
    print_signatures(at_keypoints);

    icpgpu::FPFHEstimation<Cloud, Normals, mock_pcl::PointCloud<icpgpu::FPFHSignature33>> self;
    mock_pcl::PointCloud<icpgpu::FPFHSignature33> own_sig;
    self.setInputCloud(filtered);
    self.setInputNormals(normals);
    if (k) self.setKSearch(k);
    if (radius != 0.0) self.setRadiusSearch(radius);
    self.compute(own_sig);
    own.is_dense = own_sig.is_dense;
    own.points.resize(own_sig.points.size());
    for (std::size_t i = 0; i < own_sig.points.size(); ++i) std::memcpy(own.points[i].histogram, own_sig.points[i].histogram, sizeof own.points[i].histogram);
    print_signatures(own);

    self.setKSearch(5);                                             // both set (or, with k given, a radius on top): refused, the output is empty
    self.setRadiusSearch(0.5);
    self.compute(own_sig);
    if (!own_sig.points.empty()) return 4;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fpfh_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
