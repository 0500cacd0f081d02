// icp_sampling.h -- the arithmetic of the cropping and sampling filters (pcl::PassThrough, pcl::CropBox, pcl::UniformSampling,
// pcl::FarthestPointSampling; rules: include/icpgpu.h "cropping and sampling filters"): ONE definition, for the device
// (icp_sampling.hip), the host (icpgpu_sampling.cpp) and the host check (tests/cpp/sampling_host_check.cpp).  Every unit that
// includes it is compiled with -ffp-contract=off: the only fused multiply-adds are the explicit ones.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICP_SAMPLING_HD __host__ __device__
#else
#define ICP_SAMPLING_HD
#endif

namespace icpgpu {

enum : int { kSubsetNone = 0, kSubsetPassThrough = 1, kSubsetCropBox = 2, kSubsetUniform = 3, kSubsetFarthest = 4 };  // ICPGPU_SUBSET_*
enum : int { kFpsPathNone = 0, kFpsPathOne = 1, kFpsPathMany = 2 };                                                  // ICPGPU_FPS_PATH_*

// x, y and z are finite (a NaN fails the comparison, an infinity exceeds the bound)
ICP_SAMPLING_HD inline bool sampling_finite3(float x, float y, float z) {
  const float big = 3.402823466e+38f;
  return __builtin_fabsf(x) <= big && __builtin_fabsf(y) <= big && __builtin_fabsf(z) <= big;
}

// PassThrough: 1 where the row is kept.  field -1: every finite row, whatever `negative`.
ICP_SAMPLING_HD inline int pass_through_keep(float x, float y, float z, int field, float lo, float hi, int negative) {
  if (!sampling_finite3(x, y, z)) return 0;
  if (field < 0) return 1;
  const float v = field == 0 ? x : (field == 1 ? y : z);
  if (negative) return (v >= lo && v <= hi) ? 0 : 1;
  return (v < lo || v > hi) ? 0 : 1;
}

// q = T * p, T row-major 3 x 4: the three fma chains of xform_point (icp_device.h), the arithmetic of icpgpu_transform
ICP_SAMPLING_HD inline void sampling_xform(const float m[12], float x, float y, float z, float q[3]) {
  q[0] = __builtin_fmaf(m[2], z, __builtin_fmaf(m[1], y, __builtin_fmaf(m[0], x, m[3])));
  q[1] = __builtin_fmaf(m[6], z, __builtin_fmaf(m[5], y, __builtin_fmaf(m[4], x, m[7])));
  q[2] = __builtin_fmaf(m[10], z, __builtin_fmaf(m[9], y, __builtin_fmaf(m[8], x, m[11])));
}

// CropBox: 1 where the row p (finite or not) with its image q is kept.  Outside iff a comparison holds: a NaN q is inside.
ICP_SAMPLING_HD inline int crop_box_keep(float px, float py, float pz, const float q[3], const float mn[3], const float mx[3], int negative) {
  if (!sampling_finite3(px, py, pz)) return 0;
  const bool outside = q[0] < mn[0] || q[1] < mn[1] || q[2] < mn[2] || q[0] > mx[0] || q[1] > mx[1] || q[2] > mx[2];
  return negative ? (outside ? 1 : 0) : (outside ? 0 : 1);
}

// UniformSampling: the cell of a finite row and its squared distance to the cell's centre, every operation rounded on its own.
// (The cell fits int32 on every axis whenever voxel_grid_plan's verdict over the finite rows' box is kVoxelPlanDirect.)
ICP_SAMPLING_HD inline float uniform_cell(float x, float y, float z, float inv, float leaf, int cell[3]) {
  const float p[3] = {x, y, z};
  float d[3];
  for (int a = 0; a < 3; ++a) {
    cell[a] = (int)floorf(p[a] * inv);
    const float c = ((float)cell[a] + 0.5f) * leaf;
    d[a] = p[a] - c;
  }
  return __builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0]));
}
// ... the cell's index in the plan's lattice (0 .. ncells - 1 <= INT32_MAX - 1)
ICP_SAMPLING_HD inline int uniform_cell_index(const int cell[3], const int minb[3], const int divb[3]) {
  const long long i0 = (long long)cell[0] - minb[0], i1 = (long long)cell[1] - minb[1], i2 = (long long)cell[2] - minb[2];
  return (int)(i0 + (long long)divb[0] * (i1 + (long long)divb[1] * i2));
}

ICP_SAMPLING_HD inline unsigned int sampling_float_bits(float f) {
  unsigned int u;
  __builtin_memcpy(&u, &f, sizeof u);
  return u;
}
ICP_SAMPLING_HD inline float sampling_bits_float(unsigned int u) {
  float f;
  __builtin_memcpy(&f, &u, sizeof f);
  return f;
}
// the search's 64-bit key: (d2 bits, index), smallest first -- ties go to the lowest index
ICP_SAMPLING_HD inline unsigned long long uniform_key(float d2, int index) {
  return ((unsigned long long)sampling_float_bits(d2) << 32) | (unsigned int)index;
}

// FarthestPointSampling: d2 of the outlier section, and the arg-max key of a candidate (m >= 0 or +inf): LARGEST first, ties to the
// lowest index.  0 is below every candidate's key: "no candidate".
ICP_SAMPLING_HD inline float fps_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
ICP_SAMPLING_HD inline unsigned long long fps_key(float m, int index) {
  return ((unsigned long long)sampling_float_bits(m) << 32) | (unsigned int)~(unsigned int)index;
}
ICP_SAMPLING_HD inline int fps_key_index(unsigned long long key) { return (int)~(unsigned int)key; }
ICP_SAMPLING_HD inline float fps_key_measure(unsigned long long key) { return sampling_bits_float((unsigned int)(key >> 32)); }

// the plane segmentation's generator (splitmix64 of the rule's counter, hypothesis t = 0, sample c = 0) over n rows: setSeed's first row
ICP_SAMPLING_HD inline unsigned long long sampling_seed_draw(unsigned long long seed, unsigned long long n) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return ((z >> 32) * n) >> 32;
}

}  // namespace icpgpu
