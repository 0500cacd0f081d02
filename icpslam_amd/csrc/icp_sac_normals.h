// icp_sac_normals.h -- the per-hypothesis, per-pair and per-inlier expressions of the segmentation from normals (include/icpgpu.h
// "segmentation from normals"), shared by the kernels (icp_sac_normals.hip), the host (icpgpu_sac_normals.cpp) and the host check
// (tests/cpp/sac_normals_host_check.cpp).  Every expression is written out operation by operation and the units are built with
// -ffp-contract=off, so each rounds where the header says; tests/sac_normals_restated.py states the same in NumPy.
#pragma once

#include <cmath>

#include "icp_angle.h"

namespace icpgpu {

constexpr int kSacnPlane = 11, kSacnCylinder = 5;  // = ICPGPU_SACMODEL_NORMAL_PLANE, ICPGPU_SACMODEL_CYLINDER
constexpr int kSacnCylTerms = 21;                  // 15 of J^T J's upper triangle (row-major), 5 of J^T rho, rho rho

// correctly rounded sqrtf through float64 (53 >= 2 * 24 + 2 bits: the second rounding cannot change the result; icp_outlier.hip)
__host__ __device__ inline float sacn_sqrtf(float v) { return (float)__builtin_sqrt((double)v); }

// ANGLE OF A PAIR: y = |m x g| (the cross product's components a b - c d, its squared norm (x x + y y) + z z, sqrtf), x = |m . g|
// ((x x' + y y') + z z'), folded_angle(y, x)
__host__ __device__ inline float sacn_angle(float mx, float my, float mz, float gx, float gy, float gz) {
  const float cx = my * gz - mz * gy, cy = mz * gx - mx * gz, cz = mx * gy - my * gx;
  const float y = sacn_sqrtf((cx * cx + cy * cy) + cz * cz);
  const float x = __builtin_fabsf((mx * gx + my * gy) + mz * gz);
  return folded_angle(y, x);
}

// PLANE PAIR.  d_e by the plane section's fma chain; b = (1 - w) d_e; the value is w theta + b.
__host__ __device__ inline float sacn_plane_de(const float pl[4], float qx, float qy, float qz) {
  return __builtin_fabsf(__builtin_fmaf(pl[2], qz, __builtin_fmaf(pl[1], qy, pl[0] * qx)) + pl[3]);
}
__host__ __device__ inline float sacn_plane_value(const float pl[4], float qx, float qy, float qz, float mx, float my, float mz, float w) {
  const float b = (1.f - w) * sacn_plane_de(pl, qx, qy, qz);
  return w * sacn_angle(mx, my, mz, pl[0], pl[1], pl[2]) + b;
}

// CYLINDER PAIR.  cy = (A, dir, r).  v = q - A; c = v x dir; dist = sqrtf((c.x c.x + c.y c.y) + c.z c.z); d_e = |dist - r|;
// t = (v.x dir.x + v.y dir.y) + v.z dir.z; g = v - t dir (a product and a difference per component): the direction from the axis to
// q.  *on_axis: g is (0, 0, 0) -- never an inlier.
__host__ __device__ inline float sacn_cyl_c2(const float cy[7], float qx, float qy, float qz, float& vx, float& vy, float& vz) {
  vx = qx - cy[0], vy = qy - cy[1], vz = qz - cy[2];
  const float cx = vy * cy[5] - vz * cy[4], cyy = vz * cy[3] - vx * cy[5], cz = vx * cy[4] - vy * cy[3];
  return (cx * cx + cyy * cyy) + cz * cz;
}
__host__ __device__ inline float sacn_cyl_value_from(const float cy[7], float c2, float vx, float vy, float vz, float mx, float my, float mz, float w,
                                                      bool* on_axis) {
  const float de = __builtin_fabsf(sacn_sqrtf(c2) - cy[6]);
  const float b = (1.f - w) * de;
  const float t = (vx * cy[3] + vy * cy[4]) + vz * cy[5];
  const float gx = vx - t * cy[3], gy = vy - t * cy[4], gz = vz - t * cy[5];
  *on_axis = gx == 0.f && gy == 0.f && gz == 0.f;
  return w * sacn_angle(mx, my, mz, gx, gy, gz) + b;
}
__host__ __device__ inline float sacn_cyl_value(const float cy[7], float qx, float qy, float qz, float mx, float my, float mz, float w, bool* on_axis) {
  float vx, vy, vz;
  const float c2 = sacn_cyl_c2(cy, qx, qy, qz, vx, vy, vz);
  return sacn_cyl_value_from(cy, c2, vx, vy, vz, mx, my, mz, w, on_axis);
}

// CYLINDER MODEL from two finite points with finite normals, float32, every operation rounded on its own.  false: degenerate.
__host__ __device__ inline bool sacn_cylinder_model(const float p1[3], const float n1[3], const float p2[3], const float n2[3], float out[7]) {
  const float wx = p1[0] - p2[0], wy = p1[1] - p2[1], wz = p1[2] - p2[2];
  const float a = (n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2];
  const float b = (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2];
  const float c = (n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2];
  const float d = (n1[0] * wx + n1[1] * wy) + n1[2] * wz;
  const float e = (n2[0] * wx + n2[1] * wy) + n2[2] * wz;
  const float den = a * c - b * b;
  if (!(den > 0.f) || !std::isfinite(den)) return false;  // (parallel lines)
  const float sc = (b * e - c * d) / den, tc = (a * e - b * d) / den;
  const float Ax = p1[0] + sc * n1[0], Ay = p1[1] + sc * n1[1], Az = p1[2] + sc * n1[2];
  const float Bx = p2[0] + tc * n2[0], By = p2[1] + tc * n2[1], Bz = p2[2] + tc * n2[2];
  const float ux = Bx - Ax, uy = By - Ay, uz = Bz - Az;
  const float l2 = (ux * ux + uy * uy) + uz * uz;
  if (l2 == 0.f || !std::isfinite(l2)) return false;  // (the closest points coincide, or an overflow)
  const float l = sacn_sqrtf(l2);
  const float dx = ux / l, dy = uy / l, dz = uz / l;
  const float vx = p1[0] - Ax, vy = p1[1] - Ay, vz = p1[2] - Az;
  const float cx = vy * dz - vz * dy, cy = vz * dx - vx * dz, cz = vx * dy - vy * dx;
  const float r = sacn_sqrtf((cx * cx + cy * cy) + cz * cz);
  if (!std::isfinite(Ax) || !std::isfinite(Ay) || !std::isfinite(Az) || !std::isfinite(r)) return false;
  out[0] = Ax, out[1] = Ay, out[2] = Az, out[3] = dx, out[4] = dy, out[5] = dz, out[6] = r;
  return true;
}

// CYLINDER REFINEMENT, the 21 terms of one inlier q, float64, every operation rounded on its own.  The axis is P + s D (D not
// normalised), ia < ib the two chart coordinates (the third is the chart's e).
//   v = (double)q - P;  c = v x D;  cn = sqrt((c.x c.x + c.y c.y) + c.z c.z);  L2 = (D.x D.x + D.y D.y) + D.z D.z;  L = sqrt(L2)
//   cn == 0 (q on the axis): rho = -r, J = (0, 0, 0, 0, -1)
//   else dist = cn / L, rho = dist - r, den = cn L, u = D x c, w = c x v,
//        JP_j = -u_j / den, JD_j = w_j / den - (dist D_j) / L2, J = (JP_ia, JP_ib, JD_ia, JD_ib, -1)
//   out = J_i J_j for i <= j row by row, then J_i rho, then rho rho
__host__ __device__ inline void sacn_cyl_terms(const double P[3], const double D[3], int ia, int ib, double r, float qx, float qy, float qz, double out[21]) {
  const double v[3] = {(double)qx - P[0], (double)qy - P[1], (double)qz - P[2]};
  const double c[3] = {v[1] * D[2] - v[2] * D[1], v[2] * D[0] - v[0] * D[2], v[0] * D[1] - v[1] * D[0]};
  const double cn = __builtin_sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  double J[5] = {0.0, 0.0, 0.0, 0.0, -1.0}, rho = -r;
  if (cn != 0.0) {
    const double L2 = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2];
    const double L = __builtin_sqrt(L2);
    const double dist = cn / L, den = cn * L;
    rho = dist - r;
    const double u[3] = {D[1] * c[2] - D[2] * c[1], D[2] * c[0] - D[0] * c[2], D[0] * c[1] - D[1] * c[0]};
    const double w[3] = {c[1] * v[2] - c[2] * v[1], c[2] * v[0] - c[0] * v[2], c[0] * v[1] - c[1] * v[0]};
    J[0] = -u[ia] / den, J[1] = -u[ib] / den;
    J[2] = w[ia] / den - (dist * D[ia]) / L2;
    J[3] = w[ib] / den - (dist * D[ib]) / L2;
  }
  int k = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = i; j < 5; ++j) out[k++] = J[i] * J[j];
  for (int i = 0; i < 5; ++i) out[k++] = J[i] * rho;
  out[k] = rho * rho;
}

}  // namespace icpgpu
