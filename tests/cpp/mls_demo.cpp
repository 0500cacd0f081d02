// mls_demo.cpp -- pcl::MovingLeastSquares's calls with the shim's class in its place, in front of the descriptors of a
// global registration: VoxelGrid -> MovingLeastSquares -> NormalEstimation -> FPFHEstimation over the smoothed cloud, and the same
// chain without the smoothing beside it.
// usage: mls_demo <raw.bin> <n> <leaf> <search_radius> <order> <normals_radius> <fpfh_radius>
// (the cloud: raw float32 records of four).  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the kept points' indices into the filtered cloud: their number, then the indices
//   line 3: the smoothed cloud: its width, then every point's x, y, z, normal_x, normal_y, normal_z, curvature as hex words
//   line 4: the smoothed cloud's normals (setRadiusSearch(normals_radius), viewpoint at the origin): is_dense, then normal_x, normal_y,
//           normal_z, curvature as hex words
//   line 5: the smoothed cloud's signatures: is_dense, then 33 hex words per point
//   line 6: the filtered cloud's signatures, from its own normals, without MovingLeastSquares: is_dense, then 33 hex words per point
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-ins with the members of pcl::PointXYZ / pcl::Normal / pcl::PointNormal / pcl::FPFHSignature33 / pcl::PointCloud
struct alignas(16) PointXYZ {
  float x, y, z, pad;
};
struct alignas(16) Normal {
  float normal_x, normal_y, normal_z, pad0;
  float curvature, pad1[3];
};
struct alignas(16) PointNormal {  // (pcl::PointNormal's layout)
  float x, y, z, pad0;
  float normal_x, normal_y, normal_z, pad1;
  float curvature, pad2[3];
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
typedef mock_pcl::PointCloud<mock_pcl::PointNormal> Smoothed;
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

// NormalEstimation -> FPFHEstimation over a cloud's own points; prints the normals when asked, then the signatures
static int describe(const Cloud::Ptr& cloud, double normals_radius, double fpfh_radius, bool print_normals) {
  Normals::Ptr normals(new Normals);
  icpgpu::NormalEstimation<Cloud, Normals> ne;                      // was: pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal>
  ne.setInputCloud(cloud);
  ne.setRadiusSearch(normals_radius);
  ne.compute(*normals);
  if (normals->points.size() != cloud->points.size()) return 7;
  if (print_normals) {
    std::printf("%d", normals->is_dense ? 1 : 0);
    for (const auto& p : normals->points) {
      const float v[4] = {p.normal_x, p.normal_y, p.normal_z, p.curvature};
      print_words(v, 4);
    }
    std::printf("\n");
  }
  Signatures signatures;
  icpgpu::FPFHEstimation<Cloud, Normals, Signatures> fpfh;          // was: pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33>
  fpfh.setInputCloud(cloud);
  fpfh.setInputNormals(normals);
  fpfh.setRadiusSearch(fpfh_radius);
  fpfh.compute(signatures);
  if (signatures.points.size() != cloud->points.size()) return 8;
  std::printf("%d", signatures.is_dense ? 1 : 0);
  for (const auto& p : signatures.points) print_words(p.histogram, 33);
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const double search_radius = std::atof(argv[4]);
  const int order = std::atoi(argv[5]);
  const double normals_radius = std::atof(argv[6]), fpfh_radius = std::atof(argv[7]);
  try {
    Cloud::Ptr filtered(new Cloud);
    icpgpu::VoxelGrid<Cloud> vg;                                    // was: pcl::VoxelGrid<pcl::PointXYZ>
    vg.setInputCloud(raw);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*filtered);
    std::printf("%zu", filtered->points.size());
    for (const auto& p : filtered->points) {
      const float v[4] = {p.x, p.y, p.z, p.pad};
      print_words(v, 4);
    }
    std::printf("\n");

    Smoothed smoothed;
    icpgpu::MovingLeastSquares<Cloud, Smoothed> mls;                // was: pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal>
    mls.setSearchMethod(std::shared_ptr<int>());                    // (pcl::search::KdTree: accepted)
    mls.setInputCloud(filtered);
    mls.setComputeNormals(true);
    mls.process(smoothed);                                          // PCL's default radius is 0: nothing comes out
    if (!smoothed.points.empty() || !mls.getCorrespondingIndices()->indices.empty()) return 3;
    mls.setSearchRadius(search_radius);
    mls.setPolynomialFit(true);
    mls.setPolynomialOrder(order);
    mls.setSqrGaussParam(search_radius * search_radius);            // PCL's default, spelled out
    mls.setUpsamplingMethod(icpgpu::MovingLeastSquares<Cloud, Smoothed>::NONE);
    bool threw = false;
    try {
      mls.setUpsamplingMethod(icpgpu::MovingLeastSquares<Cloud, Smoothed>::SAMPLE_LOCAL_PLANE);   // upsampling is not provided
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    if (!threw) return 4;
    mls.process(smoothed);
    icpgpu::PointIndices::ConstPtr indices = mls.getCorrespondingIndices();
    if (indices->indices.size() != smoothed.points.size() || smoothed.width != smoothed.points.size()) return 5;
    std::printf("%zu", indices->indices.size());
    for (int i : indices->indices) std::printf(" %d", i);
    std::printf("\n%u", smoothed.width);
    for (const auto& p : smoothed.points) {
      const float v[7] = {p.x, p.y, p.z, p.normal_x, p.normal_y, p.normal_z, p.curvature};
      print_words(v, 7);
    }
    std::printf("\n");

    Cloud::Ptr surface(new Cloud);                                  // (pcl::copyPointCloud(smoothed, *surface))
    surface->points.resize(smoothed.points.size());
    for (std::size_t i = 0; i < smoothed.points.size(); ++i) surface->points[i] = mock_pcl::PointXYZ{smoothed.points[i].x, smoothed.points[i].y, smoothed.points[i].z, 1.f};
    surface->width = smoothed.width, surface->height = 1;
    int rc = describe(surface, normals_radius, fpfh_radius, true);
    if (rc) return rc;
    rc = describe(filtered, normals_radius, fpfh_radius, false);
    if (rc) return rc;

    Cloud bare;                                                     // an output type without normals takes x, y, z alone
    icpgpu::MovingLeastSquares<Cloud, Cloud> plain;
    plain.setInputCloud(filtered);
    plain.setSearchRadius(search_radius);
    plain.setPolynomialOrder(order);
    plain.setComputeNormals(true);
    plain.process(bare);
    if (bare.points.size() != smoothed.points.size()) return 6;
    for (std::size_t i = 0; i < bare.points.size(); ++i)
      if (std::memcmp(&bare.points[i], &smoothed.points[i], 12) != 0) return 6;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mls_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
