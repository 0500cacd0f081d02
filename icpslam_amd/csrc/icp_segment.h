// icp_segment.h -- the float64 finish of a segment's record (rules: include/icpgpu.h "segment moments"): ONE definition for the
// device (icp_segment.hip: a thread per segment) and the host (tests/cpp/segment_host_check.cpp, which holds it to
// tests/segment_restated.py bit for bit on the CPU).  Every operation is float64 and rounded on its own (-ffp-contract=off).
//   segment_order_key / key64: the order-preserving integer images the extents are taken on (-0 below +0)
//   segment_finish:           count, K, the nine sums, the float32 box -> means, covariance, centroid, eigenvalues, axes
//   segment_project:          a point's three coordinates u_a along the axes
//   segment_finish_box:       the extents of u -> obb_lo / hi / dims / position
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/icpgpu.h"
#include "icp_jacobi3.h"

namespace icpgpu {

// a float's bits with the sign flipped (a negative one: all bits): unsigned order == numeric order, -0 below +0 (the ground filter's key)
__host__ __device__ __forceinline__ unsigned int segment_order_key(unsigned int bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__host__ __device__ __forceinline__ unsigned int segment_order_unkey(unsigned int key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
__host__ __device__ __forceinline__ unsigned long long segment_order_key64(unsigned long long bits) {
  return bits ^ ((bits >> 63) ? ~0ull : 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ unsigned long long segment_order_unkey64(unsigned long long key) {
  return key ^ ((key >> 63) ? 0x8000000000000000ull : ~0ull);
}

// the component of largest magnitude, the lowest index among equals
__host__ __device__ __forceinline__ double segment_largest(double x, double y, double z) {
  double big = x;
  if (fabs(y) > fabs(big)) big = y;
  if (fabs(z) > fabs(big)) big = z;
  return big;
}
// columns i < j of (lambda, v) change places iff lambda_j > lambda_i, strictly
#define ICPGPU_SEGMENT_ORDER(i, j)                \
  if (lam[j] > lam[i]) {                          \
    const double t_ = lam[i];                     \
    lam[i] = lam[j], lam[j] = t_;                 \
    for (int k_ = 0; k_ < 3; ++k_) {              \
      const double c_ = v[k_][i];                 \
      v[k_][i] = v[k_][j], v[k_][j] = c_;         \
    }                                             \
  }

// r: count, first and the float32 box are the caller's; status, K, moments, centroid, cov, eigenvalues and axes are written here.
// The box fields of the oriented box stay as they are (segment_finish_box).
__host__ __device__ inline void segment_finish(icpgpu_segment_record& r, const float K[3], const double S[9]) {
  const double m = (double)r.count;
  r.status = ICPGPU_SEGMENT_OK;
  double mean[3];
  for (int a = 0; a < 3; ++a) {
    r.K[a] = (double)K[a];
    mean[a] = S[6 + a] / m;
    r.centroid[a] = (double)K[a] + mean[a];
  }
  for (int e = 0; e < 9; ++e) r.moments[e] = S[e];
  r.cov[0] = S[0] / m - mean[0] * mean[0];
  r.cov[1] = S[1] / m - mean[0] * mean[1];
  r.cov[2] = S[2] / m - mean[0] * mean[2];
  r.cov[3] = S[3] / m - mean[1] * mean[1];
  r.cov[4] = S[4] / m - mean[1] * mean[2];
  r.cov[5] = S[5] / m - mean[2] * mean[2];
  double a[3][3] = {{r.cov[0], r.cov[1], r.cov[2]}, {r.cov[1], r.cov[3], r.cov[4]}, {r.cov[2], r.cov[4], r.cov[5]}}, v[3][3];
  jacobi3(a, v);
  // major >= middle >= minor, the lower column first among equals: three exchanges of neighbours
  double lam[3] = {a[0][0], a[1][1], a[2][2]};
  ICPGPU_SEGMENT_ORDER(0, 1)
  ICPGPU_SEGMENT_ORDER(1, 2)
  ICPGPU_SEGMENT_ORDER(0, 1)
  double e[2][3];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    for (int k = 0; k < 3; ++k) e[w][k] = v[k][w];
    if (segment_largest(e[w][0], e[w][1], e[w][2]) < 0.0)
      for (int k = 0; k < 3; ++k) e[w][k] = -e[w][k];
  }
  for (int w = 0; w < 3; ++w) r.eigenvalues[w] = lam[w];
  for (int k = 0; k < 3; ++k) r.axes[k] = e[0][k], r.axes[3 + k] = e[1][k];
  r.axes[6] = e[0][1] * e[1][2] - e[0][2] * e[1][1];
  r.axes[7] = e[0][2] * e[1][0] - e[0][0] * e[1][2];
  r.axes[8] = e[0][0] * e[1][1] - e[0][1] * e[1][0];
}

// u_a = (dx e_ax + dy e_ay) + dz e_az with d = q - K in float32, widened
__host__ __device__ __forceinline__ void segment_project(const double axes[9], const float K[3], float qx, float qy, float qz, double u[3]) {
  const double dx = (double)(qx - K[0]), dy = (double)(qy - K[1]), dz = (double)(qz - K[2]);
  for (int a = 0; a < 3; ++a) u[a] = (dx * axes[3 * a] + dy * axes[3 * a + 1]) + dz * axes[3 * a + 2];
}

__host__ __device__ inline void segment_finish_box(icpgpu_segment_record& r, const double lo[3], const double hi[3]) {
  double c[3];
  for (int a = 0; a < 3; ++a) {
    r.obb_lo[a] = lo[a];
    r.obb_hi[a] = hi[a];
    r.obb_dims[a] = hi[a] - lo[a];
    c[a] = (hi[a] + lo[a]) / 2.0;
  }
  for (int k = 0; k < 3; ++k) r.obb_position[k] = r.K[k] + ((c[0] * r.axes[k] + c[1] * r.axes[3 + k]) + c[2] * r.axes[6 + k]);
}

}  // namespace icpgpu
