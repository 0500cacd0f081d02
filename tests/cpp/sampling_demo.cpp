// sampling_demo.cpp -- pcl::PassThrough, pcl::CropBox, pcl::UniformSampling and pcl::FarthestPointSampling's calls with the shim's
// classes in their place, in the chain a LIDAR front end runs before descriptor matching:
//   PassThrough(z) -> CropBox(negative, the vehicle's own box) -> VoxelGrid -> NormalEstimation -> UniformSampling -> FPFHEstimation at
//   the sampled points over the filtered surface; and FarthestPointSampling over the same surface.
// usage: sampling_demo <raw.bin> <n> <z_lo> <z_hi> <leaf> <sample_leaf> <normals_k> <fpfh_radius> <n_far> <seed>
// (the cloud: raw float32 records of four; the vehicle's box is fixed below).  Prints
//   line 1: the cropped cloud: its size, then every point's x, y, z, w as hex words
//   line 2: the rows PassThrough removed, then "|" and the rows CropBox removed (indices into its own input)
//   line 3: the voxel-filtered surface: its size, then every point as hex words
//   line 4: UniformSampling's kept indices into the surface
//   line 5: the sampled points' FPFH signatures: their number, then 33 hex words each
//   line 6: FarthestPointSampling's indices into the surface, in selection order
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
struct Vector4f {  // Eigen::Vector4f, as far as CropBox reads it
  float v[4];
  float operator[](int i) const { return v[i]; }
};
}  // namespace mock_pcl
typedef mock_pcl::PointCloud<mock_pcl::PointXYZ> Cloud;
typedef mock_pcl::PointCloud<mock_pcl::Normal> Normals;
typedef mock_pcl::PointCloud<mock_pcl::FPFHSignature33> Signatures;

static void print_cloud(const Cloud& c) {
  std::printf("%zu", c.points.size());
  for (const auto& p : c.points) {
    const float v[4] = {p.x, p.y, p.z, p.pad};
    for (int e = 0; e < 4; ++e) {
      std::uint32_t w;
      std::memcpy(&w, &v[e], 4);
      std::printf(" %08x", w);
    }
  }
  std::printf("\n");
}

static void print_indices(const std::vector<int>& idx, const char* end) {
  for (int i : idx) std::printf(" %d", i);
  std::printf("%s", end);
}

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  const std::size_t n = std::strtoull(argv[2], nullptr, 10);
  auto raw = std::make_shared<Cloud>();
  raw->points.resize(n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  if (n && std::fread(raw->points.data(), sizeof(mock_pcl::PointXYZ), n, f) != n) return 2;
  std::fclose(f);
  const float z_lo = (float)std::atof(argv[3]), z_hi = (float)std::atof(argv[4]), leaf = (float)std::atof(argv[5]);
  const double sample_leaf = std::atof(argv[6]);
  const int normals_k = std::atoi(argv[7]);
  const double fpfh_radius = std::atof(argv[8]);
  const std::size_t n_far = std::strtoull(argv[9], nullptr, 10);
  const unsigned int seed = (unsigned int)std::strtoul(argv[10], nullptr, 10);
  try {
    Cloud::Ptr in_range(new Cloud), cropped(new Cloud), surface(new Cloud);
    icpgpu::PassThrough<Cloud> pass;                                // was: pcl::PassThrough<pcl::PointXYZ>
    pass.setInputCloud(raw);
    pass.setFilterFieldName("z");
    pass.setFilterLimits(z_lo, z_hi);
    pass.filter(*in_range);
    const std::vector<int> pass_removed = pass.getRemovedIndices();
    bool refused = false;
    try { pass.setFilterFieldName("intensity"); } catch (const std::invalid_argument&) { refused = true; }
    if (!refused) return 3;

    icpgpu::CropBox<Cloud> crop;                                    // was: pcl::CropBox<pcl::PointXYZ>
    crop.setInputCloud(in_range);
    crop.setMin(mock_pcl::Vector4f{{-1.5f, -1.0f, -2.0f, 1.0f}});    // the vehicle's own body
    crop.setMax(mock_pcl::Vector4f{{2.5f, 1.0f, 0.5f, 1.0f}});
    crop.setNegative(true);
    crop.filter(*cropped);
    print_cloud(*cropped);
    print_indices(pass_removed, " |");
    print_indices(crop.getRemovedIndices(), "\n");

    icpgpu::VoxelGrid<Cloud> vg;                                    // was: pcl::VoxelGrid<pcl::PointXYZ>
    vg.setInputCloud(cropped);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*surface);
    print_cloud(*surface);

    Normals::Ptr normals(new Normals);
    icpgpu::NormalEstimation<Cloud, Normals> ne;                     // was: pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal>
    ne.setInputCloud(surface);
    ne.setKSearch(normals_k);
    ne.compute(*normals);

    Cloud::Ptr keypoints(new Cloud);
    std::vector<int> key_index;
    icpgpu::UniformSampling<Cloud> us;                              // was: pcl::UniformSampling<pcl::PointXYZ>
    us.setInputCloud(surface);
    us.setRadiusSearch(sample_leaf);
    us.filter(*keypoints);
    us.filter(key_index);                                           // (the same rows as indices)
    if (key_index.size() != keypoints->points.size() || key_index.size() + us.getRemovedIndices().size() != surface->points.size()) return 4;
    for (std::size_t j = 0; j < key_index.size(); ++j)
      if (std::memcmp(&keypoints->points[j], &surface->points[key_index[j]], 16) != 0) return 5;
    print_indices(key_index, "\n");

    Signatures at_keypoints;
    icpgpu::FPFHEstimation<Cloud, Normals, Signatures> fpfh;         // was: pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33>
    fpfh.setInputCloud(keypoints);
    fpfh.setSearchSurface(surface);
    fpfh.setInputNormals(normals);
    fpfh.setRadiusSearch(fpfh_radius);
    fpfh.compute(at_keypoints);
    std::printf("%zu", at_keypoints.points.size());
    for (const auto& s : at_keypoints.points)
      for (int e = 0; e < 33; ++e) {
        std::uint32_t w;
        std::memcpy(&w, &s.histogram[e], 4);
        std::printf(" %08x", w);
      }
    std::printf("\n");

    std::vector<int> far_index;
    icpgpu::FarthestPointSampling<Cloud> fps;                       // was: pcl::FarthestPointSampling<pcl::PointXYZ>
    fps.setInputCloud(surface);
    fps.setSample(n_far);
    fps.setSeed(seed);
    fps.filter(far_index);
    print_indices(far_index, "\n");
    fps.setSample(surface->points.size() + 1);                      // more samples than rows: refused, the output is empty (PCL throws)
    fps.filter(far_index);
    if (!far_index.empty()) return 6;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sampling_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
