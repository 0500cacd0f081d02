// normals_demo.cpp -- pcl::NormalEstimation's calls with the shim's class in its place, in both modes and with a
// search surface, and the chain NormalEstimation -> IterativeClosestPointWithNormals::setTargetNormals -> align.
// usage: normals_demo <cloud.bin> <n> <surface.bin> <n_s> <k> <radius> <vpx> <vpy> <vpz> <src.bin> <n_src> <max_iters>
// (clouds: raw float32 records of four).  Prints
//   line 1: setKSearch(k) over the cloud itself: is_dense, then every point's normal_x, normal_y, normal_z, curvature as hex words
//   line 2: setRadiusSearch(radius) over the cloud itself, the same way
//   line 3: setKSearch(k) with setSearchSurface(surface), the same way
//   line 4: the chain: the cloud is the target, its line-1 normals go to setTargetNormals, <src> is aligned to it:
//           converged iterations T[16] (column-major, %.9g: every float round-trips)
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
struct alignas(16) Normal {  // (pcl::Normal's layout: the normal in four floats, then the curvature)
  float normal_x, normal_y, normal_z, pad0;
  float curvature, pad1[3];
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

static void print_normals(const Normals& out) {
  std::printf("%d", out.is_dense ? 1 : 0);
  for (const auto& p : out.points) {
    const float v[4] = {p.normal_x, p.normal_y, p.normal_z, p.curvature};
    for (int e = 0; e < 4; ++e) {
      std::uint32_t w;
      std::memcpy(&w, &v[e], 4);
      std::printf(" %08x", w);
    }
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 13) return 2;
  auto cloud = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  auto surface = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  const int k = std::atoi(argv[5]);
  const double radius = std::atof(argv[6]);
  const float vp[3] = {(float)std::atof(argv[7]), (float)std::atof(argv[8]), (float)std::atof(argv[9])};
  auto src = load(argv[10], std::strtoull(argv[11], nullptr, 10));
  const double max_iters = std::atof(argv[12]);
  try {
    Normals normals;
    icpgpu::NormalEstimation<Cloud, Normals> ne;
    ne.setInputCloud(cloud);
    ne.setSearchMethod(std::shared_ptr<int>());  // (a pcl::search::KdTree in PCL: accepted and ignored)
    ne.setViewPoint(vp[0], vp[1], vp[2]);
    float x, y, z;
    ne.getViewPoint(x, y, z);
    if (x != vp[0] || y != vp[1] || z != vp[2]) return 4;
    ne.setKSearch(k);
    ne.compute(normals);
    if (normals.size() != cloud->size() || normals.width != cloud->size() || normals.height != 1) return 4;
    print_normals(normals);
    const std::vector<float> target_normals = ne.getNormalsXYZC();

    ne.setRadiusSearch(radius);  // both set: refused, as in PCL -- the output stays empty
    ne.compute(normals);
    if (normals.size() != 0 || !ne.getNormalsXYZC().empty()) return 5;
    ne.setKSearch(0);
    ne.compute(normals);
    print_normals(normals);

    icpgpu::NormalEstimation<Cloud, Normals> over_surface;
    over_surface.setInputCloud(cloud);
    over_surface.setSearchSurface(surface);
    over_surface.setViewPoint(vp[0], vp[1], vp[2]);
    over_surface.setKSearch(k);
    over_surface.compute(normals);
    print_normals(normals);

    icpgpu::IterativeClosestPointWithNormals<Cloud> icp;
    icp.setMaximumIterations(max_iters);
    icp.setTransformationEpsilon(1e-06);
    icp.setMaxCorrespondenceDistance(1.0);
    icp.setInputSource(src);
    icp.setInputTarget(cloud);
    icp.setTargetNormals(target_normals.data(), target_normals.size() / 4);
    Cloud::Ptr out(new Cloud());
    icp.align(*out);
    const auto T = icp.getFinalTransformation();
    std::printf("%d %d", icp.hasConverged() ? 1 : 0, icp.getResult().iterations);
    for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
