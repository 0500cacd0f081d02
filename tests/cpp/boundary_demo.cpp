// boundary_demo.cpp -- pcl::BoundaryEstimation's and pcl::ISSKeypoint3D's border-estimation calls with the shim's classes in their
// place, inside the front end of a global registration: VoxelGrid -> NormalEstimation -> BoundaryEstimation ->
// ISSKeypoint3DBorder -> FPFHEstimation at the keypoints over the filtered surface.
// usage: boundary_demo <raw.bin> <n> <leaf> <salient_radius> <non_max_radius> <gamma_21> <gamma_32> <min_neighbors> <normals_k>
//                      <border_radius> <fpfh_radius>
// (the cloud: raw float32 records of four).  Prints
//   line 1: the voxel-filtered cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the filtered cloud's normals (setKSearch(normals_k), viewpoint at the origin): is_dense, then normal_x, normal_y, normal_z,
//           curvature as hex words
//   line 3: BoundaryEstimation (setRadiusSearch(border_radius), the default threshold): the size, then boundary_point per point
//   line 4: plain ISSKeypoint3D's keypoint indices: their number, then the indices
//   line 5: ISSKeypoint3DBorder's keypoint indices (setBorderRadius(border_radius), setNormals): their number, then the indices
//   line 6: its edge points, line 7: its border points, in the same form
//   line 8: the same class with setNormalRadius instead of setNormals and the border radius 0: its keypoint indices
//   line 9: the signatures at line 5's keypoints over the filtered surface: is_dense, then 33 hex words per keypoint
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-ins with the members of pcl::PointXYZ / pcl::Normal / pcl::Boundary / pcl::FPFHSignature33 / pcl::PointCloud
struct alignas(16) PointXYZ {
  float x, y, z, pad;
};
struct alignas(16) Normal {  // (pcl::Normal's layout: the normal in four floats, then the curvature)
  float normal_x, normal_y, normal_z, pad0;
  float curvature, pad1[3];
};
struct Boundary {
  std::uint8_t boundary_point;
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
typedef mock_pcl::PointCloud<mock_pcl::Boundary> Boundaries;
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

static void print_indices(const std::vector<int>& indices) {
  std::printf("%zu", indices.size());
  for (int i : indices) std::printf(" %d", i);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 12) return 2;
  auto raw = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  const float leaf = (float)std::atof(argv[3]);
  const double salient = std::atof(argv[4]), non_max = std::atof(argv[5]), gamma_21 = std::atof(argv[6]), gamma_32 = std::atof(argv[7]);
  const int min_neighbors = std::atoi(argv[8]), normals_k = std::atoi(argv[9]);
  const double border_radius = std::atof(argv[10]), fpfh_radius = std::atof(argv[11]);
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

    Boundaries boundaries;
    icpgpu::BoundaryEstimation<Cloud, Normals> be;                  // was: pcl::BoundaryEstimation<pcl::PointXYZ, pcl::Normal, pcl::Boundary>
    be.setSearchMethod(std::shared_ptr<int>());                     // (pcl::search::KdTree: accepted)
    be.setInputCloud(filtered);
    be.compute(boundaries);                                         // no normals yet: nothing comes out
    if (!boundaries.points.empty()) return 3;
    be.setInputNormals(normals);
    be.compute(boundaries);                                         // neither k nor a radius: refused, nothing comes out
    if (!boundaries.points.empty()) return 4;
    be.setRadiusSearch(border_radius);
    if (be.getAngleThreshold() != 1.57079632679489661923f) return 5;
    be.compute(boundaries);
    if (boundaries.points.size() != filtered->points.size() || boundaries.width != filtered->points.size()) return 6;
    std::printf("%zu", boundaries.points.size());
    for (const auto& b : boundaries.points) std::printf(" %d", (int)b.boundary_point);
    std::printf("\n");

    Cloud::Ptr plain_keypoints(new Cloud), keypoints(new Cloud), again(new Cloud);
    icpgpu::ISSKeypoint3D<Cloud> plain;                             // was: pcl::ISSKeypoint3D<pcl::PointXYZ, pcl::PointXYZ>
    icpgpu::ISSKeypoint3DBorder<Cloud, Normals> iss;                // was: the same, with setBorderRadius above 0
    plain.setInputCloud(filtered);
    iss.setInputCloud(filtered);
    for (icpgpu::ISSKeypoint3D<Cloud>* k : {&plain, static_cast<icpgpu::ISSKeypoint3D<Cloud>*>(&iss)}) {
      k->setSalientRadius(salient);
      k->setNonMaxRadius(non_max);
      k->setThreshold21(gamma_21);
      k->setThreshold32(gamma_32);
      k->setMinNeighbors(min_neighbors);
    }
    plain.compute(*plain_keypoints);
    print_indices(plain.getKeypointsIndices()->indices);
    iss.setBorderRadius(border_radius);
    iss.compute(*keypoints);                                        // neither normals nor a normal radius: refused, nothing comes out
    if (!keypoints->points.empty() || !iss.getEdgePoints()->indices.empty()) return 7;
    iss.setNormals(normals);
    iss.setAngleThreshold(1.57079632679489661923f);
    iss.compute(*keypoints);
    if (iss.getKeypointsIndices()->indices.size() != keypoints->points.size() || keypoints->width != keypoints->points.size()) return 8;
    print_indices(iss.getKeypointsIndices()->indices);
    print_indices(iss.getEdgePoints()->indices);
    print_indices(iss.getBorderPoints()->indices);

    icpgpu::ISSKeypoint3DBorder<Cloud, Normals> off;                // border radius 0: plain ISS, whatever the normal radius
    off.setInputCloud(filtered);
    off.setSalientRadius(salient);
    off.setNonMaxRadius(non_max);
    off.setThreshold21(gamma_21);
    off.setThreshold32(gamma_32);
    off.setMinNeighbors(min_neighbors);
    off.setNormalRadius(4 * leaf);
    off.setBorderRadius(0.0);
    off.compute(*again);
    if (!off.getEdgePoints()->indices.empty() || !off.getBorderPoints()->indices.empty()) return 9;
    print_indices(off.getKeypointsIndices()->indices);

    Signatures at_keypoints;
    icpgpu::FPFHEstimation<Cloud, Normals, Signatures> fpfh;        // was: pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33>
    fpfh.setInputCloud(keypoints);
    fpfh.setSearchSurface(filtered);
    fpfh.setInputNormals(normals);
    fpfh.setRadiusSearch(fpfh_radius);
    fpfh.compute(at_keypoints);
    if (at_keypoints.points.size() != keypoints->points.size()) return 10;
    std::printf("%d", at_keypoints.is_dense ? 1 : 0);
    for (const auto& p : at_keypoints.points) print_words(p.histogram, 33);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "boundary_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
