// symmetric_demo.cpp -- the chain a PCL user writes once both clouds carry normals, with the shim's classes in PCL's places
// (INTEGRATION.md): NormalEstimation on both clouds -> setSourceNormals / setTargetNormals -> IterativeClosestPointWithNormals with
// setUseSymmetricObjective(true) and a CorrespondenceRejectorSurfaceNormal in its chain -> align.
// usage: symmetric_demo <src.bin> <n_src> <tgt.bin> <n_tgt> <max_iters> <k> <threshold>   (clouds: raw float32 records of four)
// prints: converged iterations T[16] (column-major, %.9g: every float round-trips)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-ins with the members of pcl::PointXYZ / pcl::Normal / pcl::PointCloud (PCL is not in this image)
struct alignas(16) PointXYZ {
  float x, y, z, pad;
};
struct alignas(16) Normal {
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

static std::vector<float> normals_of(const Cloud::Ptr& cloud, int k) {
  Normals normals;
  icpgpu::NormalEstimation<Cloud, Normals> ne;
  ne.setInputCloud(cloud);
  ne.setKSearch(k);
  ne.compute(normals);
  if (normals.size() != cloud->size()) std::exit(4);
  return ne.getNormalsXYZC();
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  auto src = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  auto tgt = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  const double max_iters = std::atof(argv[5]);
  const int k = std::atoi(argv[6]);
  const double threshold = std::atof(argv[7]);
  try {
    const std::vector<float> src_normals = normals_of(src, k), tgt_normals = normals_of(tgt, k);
    icpgpu::IterativeClosestPointWithNormals<Cloud> icp;
    icp.setMaximumIterations(max_iters);
    icp.setTransformationEpsilon(1e-06);
    icp.setMaxCorrespondenceDistance(1.0);
    icp.setInputSource(src);
    icp.setInputTarget(tgt);
    icp.setSourceNormals(src_normals.data(), src_normals.size() / 4);
    icp.setTargetNormals(tgt_normals.data(), tgt_normals.size() / 4);
    if (icp.getUseSymmetricObjective() || !icp.getEnforceSameDirectionNormals()) return 4;  // PCL's defaults
    icp.setUseSymmetricObjective(true);
    icp.setEnforceSameDirectionNormals(true);
    icpgpu::registration::CorrespondenceRejectorSurfaceNormal::Ptr rej(new icpgpu::registration::CorrespondenceRejectorSurfaceNormal);
    if (rej->getThreshold() != 1.0) return 4;
    rej->setThreshold(threshold);
    icp.addCorrespondenceRejector(rej);
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
