// scp_demo.cpp -- pcl::SampleConsensusPrerejective's calls with the shim's classes in their place: the global
// registration chain NormalEstimation -> FPFHEstimation -> SampleConsensusPrerejective -> IterativeClosestPoint, and the feature tree.
// usage: scp_demo <source.bin> <n_s> <target.bin> <n> <normals_k> <fpfh_radius> <nr_samples> <randomness> <similarity> <distance>
//                 <inlier_fraction> <iterations> <seed>        (clouds: raw float32 records of four).  Prints
//   line 1: the source's signatures: is_dense, then 33 hex words per point
//   line 2: the target's signatures, the same way
//   line 3: hasConverged, the number of inliers, the fitness as a hex word, then the 16 entries of the transformation, column-major, as hex words
//   line 4: the inliers
//   line 5: the aligned source: x, y, z, w as hex words
//   line 6: the feature tree's batched search of the source's signatures in the target's, k = <randomness>: the indices, row after row
//   line 7: the first source signature's single search, the same k: the number found, then the indices
//   line 8: ICP started from the alignment: hasConverged, then its transformation as hex words
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
struct alignas(16) Normal {
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

static Signatures::Ptr describe(const Cloud::Ptr& cloud, int normals_k, double radius) {
  Normals::Ptr normals(new Normals);
  icpgpu::NormalEstimation<Cloud, Normals> ne;                      // was: pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal>
  ne.setInputCloud(cloud);
  ne.setKSearch(normals_k);
  ne.compute(*normals);
  Signatures::Ptr out(new Signatures);
  icpgpu::FPFHEstimation<Cloud, Normals, Signatures> fpfh;          // was: pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33>
  fpfh.setInputCloud(cloud);
  fpfh.setInputNormals(normals);
  fpfh.setRadiusSearch(radius);
  fpfh.compute(*out);
  std::printf("%d", out->is_dense ? 1 : 0);
  for (const auto& p : out->points) print_words(p.histogram, 33);
  std::printf("\n");
  return out;
}

int main(int argc, char** argv) {
  if (argc < 14) return 2;
  auto source = load(argv[1], std::strtoull(argv[2], nullptr, 10));
  auto target = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  const int normals_k = std::atoi(argv[5]);
  const double radius = std::atof(argv[6]);
  const int nr_samples = std::atoi(argv[7]), randomness = std::atoi(argv[8]);
  const float similarity = (float)std::atof(argv[9]);
  const double distance = std::atof(argv[10]);
  const float fraction = (float)std::atof(argv[11]);
  const int iterations = std::atoi(argv[12]);
  const unsigned long long seed = std::strtoull(argv[13], nullptr, 10);
  try {
    Signatures::Ptr source_features = describe(source, normals_k, radius), target_features = describe(target, normals_k, radius);

    Cloud aligned;
    icpgpu::SampleConsensusPrerejective<Cloud, Signatures> align;   // was: pcl::SampleConsensusPrerejective<pcl::PointXYZ, pcl::PointXYZ, pcl::FPFHSignature33>
    if (align.getNumberOfSamples() != 3 || align.getCorrespondenceRandomness() != 2 || align.getSimilarityThreshold() != 0.9f ||
        align.getInlierFraction() != 0.0f || align.hasConverged())
      return 3;                                                     // PCL's defaults
    align.align(aligned);                                           // nothing set: refused, the output is empty
    if (!aligned.points.empty() || align.hasConverged()) return 4;
    align.setInputSource(source);
    align.setSourceFeatures(source_features);
    align.setInputTarget(target);
    align.setTargetFeatures(target_features);
    align.setMaximumIterations(iterations);
    align.setNumberOfSamples(nr_samples);
    align.setCorrespondenceRandomness(randomness);
    align.setSimilarityThreshold(similarity);
    align.setMaxCorrespondenceDistance(distance);
    align.setInlierFraction(fraction);
    align.setSeed(seed);
    align.align(aligned);
    if (aligned.points.size() != source->points.size() || aligned.width != source->points.size()) return 5;
    const icpgpu::Matrix4 T = align.getFinalTransformation();
    const float fitness = (float)align.getFitnessScore();
    std::printf("%d %zu", align.hasConverged() ? 1 : 0, align.getInliers().size());
    print_words(&fitness, 1);
    for (int col = 0; col < 4; ++col)
      for (int row = 0; row < 4; ++row) {
        const float v = T(row, col);
        print_words(&v, 1);
      }
    std::printf("\n");
    for (int i : align.getInliers()) std::printf("%d ", i);
    std::printf("\n");
    for (const auto& p : aligned.points) {
      const float v[4] = {p.x, p.y, p.z, p.pad};
      print_words(v, 4);
    }
    std::printf("\n");

    icpgpu::FeatureKdTree<Signatures> tree;                         // was: pcl::KdTreeFLANN<pcl::FPFHSignature33>
    tree.setInputCloud(target_features);
    std::vector<int> indices, found;
    std::vector<float> sqr;
    if (tree.nearestKSearch(*source_features, randomness, indices, sqr, found) != (int)source->points.size()) return 6;
    for (int i : indices) std::printf("%d ", i);
    std::printf("\n");
    const int m = tree.nearestKSearch(source_features->points[0], randomness, indices, sqr);
    std::printf("%d", m);
    for (int i : indices) std::printf(" %d", i);
    std::printf("\n");
    if (tree.nearestKSearch(0, 0, indices, sqr) != 0 || !indices.empty()) return 7;   // k = 0: refused

    Cloud refined;
    icpgpu::IterativeClosestPoint<Cloud> icp;                       // was: pcl::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ>
    icp.setMaximumIterations(50);
    icp.setMaxCorrespondenceDistance(1.0);
    icp.setInputSource(source);
    icp.setInputTarget(target);
    icp.align(refined, T);                                          // the alignment is the guess no ICP had before
    const icpgpu::Matrix4 Ti = icp.getFinalTransformation();
    std::printf("%d", icp.hasConverged() ? 1 : 0);
    for (int col = 0; col < 4; ++col)
      for (int row = 0; row < 4; ++row) {
        const float v = Ti(row, col);
        print_words(&v, 1);
      }
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "scp_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
