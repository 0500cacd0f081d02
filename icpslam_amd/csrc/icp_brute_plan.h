// icp_brute_plan.h -- the launch shape of a matrix-core brute-force sweep (icp_brute_mfma.hip, icp_brute_bf16.hip).  ONE
// definition, pure arithmetic over integers: no HIP, no environment -- the two units read their switches and hand the numbers in
// (tests/cpp/brute_plan_check.cpp prints it on the host, tests/test_brute_plan_host.py holds it to the Python restatement).
//
// g groups of 32 sources per wave, block threads per workgroup (block / 64 * 32 g sources), tile targets per LDS tile; grid
// (grid_x, splits), every split tgt_per_split targets (whole tiles).  The launchers launch what this says; nn_keys_brute prints
// it under ICPGPU_DEBUG.
#pragma once

namespace icpgpu {

struct MatrixNnShape {
  int g, tile, block;
};
struct MatrixNnPlan {
  int g, tile, block;
  int grid_x, splits, tgt_per_split;
};

constexpr MatrixNnShape kMfmaShape = {2, 1024, 256};       // icp_brute_mfma.hip: 4 waves, 16 KiB of points per tile
constexpr MatrixNnShape kBf16Shape = {2, 1024, 512};       // icp_brute_bf16.hip as shipped
constexpr MatrixNnShape kBf16CheckShape = {2, 512, 256};   // its bound-check mode: one instantiation
constexpr int kMatrixNnWavesPerSimd = 32;

// Target splits for ~waves_per_simd waves' worth of workgroups per SIMD (f32 kernel, measured at 200k x 200k: 2 -> 4.8 ms,
// 8 -> 3.45, 16 -> 3.23, 32 -> 3.14: the tail of the last round of workgroups), never less than one tile per split.
inline MatrixNnPlan matrix_nn_plan(int n_q, int n_t, int num_cus, MatrixNnShape s, int waves_per_simd) {
  MatrixNnPlan p;
  p.g = s.g;
  p.tile = s.tile;
  p.block = s.block;
  const int waves = s.block / 64, per_block = waves * 32 * s.g;
  p.grid_x = (n_q + per_block - 1) / per_block;
  int splits = (num_cus * waves_per_simd * 4 / waves + p.grid_x - 1) / p.grid_x;
  const int max_splits = (n_t + s.tile - 1) / s.tile;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  int per = (n_t + splits - 1) / splits;
  per = ((per + s.tile - 1) / s.tile) * s.tile;
  p.tgt_per_split = per;
  p.splits = (n_t + per - 1) / per;
  return p;
}

}  // namespace icpgpu
