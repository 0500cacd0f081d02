// icp_voxel_plan.h -- the voxel filter's plan: ONE definition, for the host (icpgpu_voxel.cpp, icpgpu_ndt.cpp) and the device
// (voxel_plan_kernel, icp_voxel.hip), defined for every box and every leaf.
//
// From the cloud's bounding box [lo, hi] and inv = 1 / leaf (float, PCL's inverse_leaf_size_) it derives what
// pcl::VoxelGrid::applyFilter derives -- min_b = floor(lo * inv), div_b = floor(hi * inv) - min_b + 1 -- and the verdict:
//   kVoxelPlanDirect       the cell index fits int32: the direct path (or, by size or switch, the sort path) runs on it
//   kVoxelPlanNoFinite     lo > hi on an axis: the cloud has no finite point, the result is empty
//   kVoxelPlanPassThrough  PCL's "leaf size is too small for the input dataset, integer indices would overflow": input returned
//   kVoxelPlanWrap         PCL's test (on the float extents) passes, the integer extents are a cell wider and their product exceeds
//                          int32: PCL indexes with them anyway, the topmost cells wrap negative and sort first -- the sort path's
// PCL's own test is dx * dy * dz > INT32_MAX with d = (int64)((hi - lo) * inv) + 1: its product wraps in int64 for three ordinary
// extents of 2^21+ cells each, and its casts are undefined beyond int64 / int32.  The rule here is PCL's wherever PCL's arithmetic is
// defined and its stated intent elsewhere: pass-through if and only if
//   (a) the EXACT product dx * dy * dz exceeds INT32_MAX (tested in stages: nothing wraps), or
//   (b) (hi - lo) * inv is not finite or >= 2^63 on an axis (tested in float, before the cast), or
//   (c) floor(lo * inv) or floor(hi * inv) lies outside int32 on an axis (likewise; a NaN counts as outside).
// No float outside the target type's range is ever cast.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICP_VOXEL_PLAN_HD __host__ __device__
#else
#define ICP_VOXEL_PLAN_HD
#endif

namespace icpgpu {

enum : int { kVoxelPlanDirect = 0, kVoxelPlanNoFinite = 1, kVoxelPlanPassThrough = 2, kVoxelPlanWrap = 3 };

// minb / divb: valid for kVoxelPlanDirect and kVoxelPlanWrap (zero / one otherwise).  Under kVoxelPlanWrap a div_b beyond int32
// is reduced modulo 2^32, as PCL's int arithmetic does on every platform it runs on; *ncells = the exact product of the integer
// extents under kVoxelPlanDirect (1 .. INT32_MAX), INT32_MAX + 1 under kVoxelPlanWrap, 0 when there is no lattice.
ICP_VOXEL_PLAN_HD inline int voxel_grid_plan(const float lo[3], const float hi[3], float inv, int minb[3], int divb[3], long long* ncells) {
  for (int a = 0; a < 3; ++a) minb[a] = 0, divb[a] = 1;
  *ncells = 0;
  if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return kVoxelPlanNoFinite;
  const long long kMax = 0x7FFFFFFFll;
  long long d[3] = {0, 0, 0}, dv[3] = {1, 1, 1};
  bool over = false;
  for (int a = 0; a < 3 && !over; ++a) {
    const float e = (hi[a] - lo[a]) * inv;
    const float fl = floorf(lo[a] * inv), fh = floorf(hi[a] * inv);
    over = !(e < 9223372036854775808.0f) ||  // (b): inf, NaN (0 * inf), >= 2^63
           !(fl >= -2147483648.0f && fl < 2147483648.0f && fh >= -2147483648.0f && fh < 2147483648.0f);  // (c)
    if (over) break;
    d[a] = (long long)e + 1;  // e in [0, 2^63): defined
    const long long il = (long long)fl, ih = (long long)fh;
    minb[a] = (int)il;
    dv[a] = ih - il + 1;  // in [1, 2^32]
    divb[a] = (int)(unsigned int)(unsigned long long)dv[a];
  }
  // (a), in stages: each factor <= 2^31 - 1 before it is multiplied, so every product is below 2^62
  over = over || d[0] > kMax || d[1] > kMax || d[2] > kMax;
  if (!over) {
    const long long p = d[0] * d[1];
    over = p > kMax || p * d[2] > kMax;
  }
  if (over) {
    for (int a = 0; a < 3; ++a) minb[a] = 0, divb[a] = 1;
    return kVoxelPlanPassThrough;
  }
  // the integer extents' product, saturated at INT32_MAX + 1 (nc <= INT32_MAX and dv <= 2^32 in front of every product: < 2^63)
  long long nc = 1;
  for (int a = 0; a < 3; ++a) nc = nc > kMax ? kMax + 1 : nc * dv[a];
  if (nc > kMax) nc = kMax + 1;
  *ncells = nc;
  return nc > kMax ? kVoxelPlanWrap : kVoxelPlanDirect;
}

}  // namespace icpgpu
