// rsac_demo.cpp -- two PCL call sites of CorrespondenceRejectorSampleConsensus with the classes swapped for the shim's
// (INTEGRATION.md), PCL's spelling of every call:
//   chain: rsac_demo chain <src.bin> <n_src> <tgt.bin> <n_tgt> <max_iters> <inlier_threshold> <ransac_iterations>
//          the rejector in an IterativeClosestPoint's chain; prints converged iterations n_correspondences T[16] bestT[16]
//   alone: rsac_demo alone <src.bin> <n_src> <tgt.bin> <n_tgt> <pairs.bin> <n_pairs> <inlier_threshold> <ransac_iterations>
//          (pairs: raw int32 records of two) the rejector behind feature matches; prints n_remaining bestT[16], then the
//          remaining pairs' positions in the input
// (clouds: raw float32 records of four; matrices column-major, %.9g: every float round-trips)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "icpgpu_registration.hpp"

namespace mock_pcl {  // stand-in with the memory layout of pcl::PointXYZ / pcl::PointCloud (PCL is not in this image)
struct alignas(16) PointXYZ {
  float x, y, z, pad;
};
struct PointCloud {
  std::vector<PointXYZ> points;
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

template <class M>
static void print16(const M& T) {
  for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
}

static int chain(int argc, char** argv) {
  if (argc < 9) return 2;
  auto curr_cloud_ = load(argv[2], std::strtoull(argv[3], nullptr, 10));
  auto prev_cloud_ = load(argv[4], std::strtoull(argv[5], nullptr, 10));
  icpgpu::IterativeClosestPoint<mock_pcl::PointCloud> icp;
  icp.setMaximumIterations(std::atoi(argv[6]));
  icp.setTransformationEpsilon(1e-09);
  icp.setMaxCorrespondenceDistance(1.0);
  icp.setRANSACIterations(0);
  icpgpu::registration::CorrespondenceRejectorSampleConsensus::Ptr rej(new icpgpu::registration::CorrespondenceRejectorSampleConsensus);
  rej->setInlierThreshold(std::atof(argv[7]));
  rej->setMaximumIterations(std::atoi(argv[8]));
  rej->setRefineModel(false);
  bool threw = false;
  try {
    rej->setRefineModel(true);
  } catch (const std::exception&) {
    threw = true;
  }
  if (!threw || rej->getInlierThreshold() != std::atof(argv[7]) || rej->getMaximumIterations() != std::atoi(argv[8])) return 4;
  icp.addCorrespondenceRejector(rej);
  icp.setInputSource(curr_cloud_);
  icp.setInputTarget(prev_cloud_);
  mock_pcl::PointCloud::Ptr out(new mock_pcl::PointCloud());
  icp.align(*out);
  std::printf("%d %d %u", icp.hasConverged() ? 1 : 0, icp.getResult().iterations, icp.getResult().n_correspondences);
  print16(icp.getFinalTransformation());
  print16(rej->getBestTransformation());
  std::printf("\n");
  return 0;
}

static int alone(int argc, char** argv) {
  if (argc < 10) return 2;
  auto source = load(argv[2], std::strtoull(argv[3], nullptr, 10));
  auto target = load(argv[4], std::strtoull(argv[5], nullptr, 10));
  const std::size_t n_pairs = std::strtoull(argv[7], nullptr, 10);
  std::vector<int32_t> raw(2 * n_pairs);
  FILE* f = std::fopen(argv[6], "rb");
  if (!f) { std::perror(argv[6]); return 2; }
  if (n_pairs && std::fread(raw.data(), 2 * sizeof(int32_t), n_pairs, f) != n_pairs) { std::fprintf(stderr, "short read\n"); return 2; }
  std::fclose(f);
  std::shared_ptr<icpgpu::Correspondences> correspondences(new icpgpu::Correspondences);
  for (std::size_t r = 0; r < n_pairs; ++r) correspondences->push_back(icpgpu::Correspondence{raw[2 * r], raw[2 * r + 1], (float)r});
  icpgpu::registration::CorrespondenceRejectorSampleConsensus rejector_sac;
  rejector_sac.setInputSource(source);
  rejector_sac.setInputTarget(target);
  rejector_sac.setInlierThreshold(std::atof(argv[8]));
  rejector_sac.setMaximumIterations(std::atoi(argv[9]));
  rejector_sac.setInputCorrespondences(correspondences);
  icpgpu::Correspondences remaining;
  rejector_sac.getCorrespondences(remaining);
  std::printf("%zu", remaining.size());
  print16(rejector_sac.getBestTransformation());
  std::printf("\n");
  for (const auto& c : remaining) std::printf("%d ", (int)c.distance);  // (the demo stored each pair's position there)
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    return std::strcmp(argv[1], "chain") == 0 ? chain(argc, argv) : alone(argc, argv);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
