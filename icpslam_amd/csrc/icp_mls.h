// icp_mls.h -- the per-query steps of the moving least squares projection that are not sums over a row, in float64: ONE definition
// for the device (icp_mls.hip: mls_plane_kernel, mls_solve_kernel) and for a host program that checks them.  Their expressions are
// part of the rule (include/icpgpu.h "moving least squares": PLANE, FRAME, SOLVE); tests/mls_restated.py takes the same steps.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "icp_jacobi3.h"

namespace icpgpu {

struct MlsPlane {
  double N[3], U[3], V[3];  // the plane's normal and the frame on it (U = N x V)
  double Q[3];              // the query projected onto the plane
  double c[3];              // the row's centroid
  double lambda;            // the smallest eigenvalue of the row's covariance
  float curvature;
};

// PLANE and FRAME: sums = the nine sums of a row of m >= 3 entries about K (dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz),
// P the query.
__host__ __device__ __forceinline__ void mls_plane(const double (&sums)[9], int m, const double (&K)[3], const double (&P)[3], MlsPlane& pl) {
  const double fm = (double)m;
  const double a0 = sums[0] / fm, a1 = sums[1] / fm, a2 = sums[2] / fm, a3 = sums[3] / fm, a4 = sums[4] / fm, a5 = sums[5] / fm, a6 = sums[6] / fm,
               a7 = sums[7] / fm, a8 = sums[8] / fm;
  const double xx = a0 - a6 * a6, xy = a1 - a6 * a7, xz = a2 - a6 * a8, yy = a3 - a7 * a7, yz = a4 - a7 * a8, zz = a5 - a8 * a8;
  pl.c[0] = a6 + K[0], pl.c[1] = a7 + K[1], pl.c[2] = a8 + K[2];
  double a[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}}, E[3][3];
  jacobi3(a, E);
  // the smallest eigenvalue, the lowest index among equals, and its column of E -- by selects, as icp_normals.hip takes them
  const bool b1 = a[1][1] < a[0][0];
  const double lam01 = b1 ? a[1][1] : a[0][0];
  const bool b2 = a[2][2] < lam01;
  pl.lambda = b2 ? a[2][2] : lam01;
  const double nx = b2 ? E[0][2] : (b1 ? E[0][1] : E[0][0]);
  const double ny = b2 ? E[1][2] : (b1 ? E[1][1] : E[1][0]);
  const double nz = b2 ? E[2][2] : (b1 ? E[2][1] : E[2][0]);
  pl.N[0] = nx, pl.N[1] = ny, pl.N[2] = nz;
  const double tr = (xx + yy) + zz;
  pl.curvature = tr != 0.0 ? fabsf((float)(pl.lambda / tr)) : 0.f;
  const double ex = P[0] - pl.c[0], ey = P[1] - pl.c[1], ez = P[2] - pl.c[2];
  const double dist = (ex * nx + ey * ny) + ez * nz;
  pl.Q[0] = P[0] - dist * nx, pl.Q[1] = P[1] - dist * ny, pl.Q[2] = P[2] - dist * nz;
  double vx, vy, vz;  // Eigen's unitOrthogonal
  if (fabs(nx) > 1e-12 * fabs(nz) || fabs(ny) > 1e-12 * fabs(nz)) {
    const double inv = 1.0 / sqrt(nx * nx + ny * ny);
    vx = -ny * inv, vy = nx * inv, vz = 0.0;
  } else {
    const double inv = 1.0 / sqrt(ny * ny + nz * nz);
    vx = 0.0, vy = -nz * inv, vz = ny * inv;
  }
  pl.V[0] = vx, pl.V[1] = vy, pl.V[2] = vz;
  pl.U[0] = ny * vz - nz * vy, pl.U[1] = nz * vx - nx * vz, pl.U[2] = nx * vy - ny * vx;
}

constexpr int mls_coefficients(int order) { return (order + 1) * (order + 2) / 2; }
constexpr int mls_sums(int order) { return mls_coefficients(order) * (mls_coefficients(order) + 1) / 2 + mls_coefficients(order); }  // A's lower triangle, then b

// SOLVE: A c = b by Cholesky.  A is the lower triangle in rows -- A(i, j), j <= i, at i (i + 1) / 2 + j -- and becomes L; b becomes
// c.  Nothing is special-cased: a pivot that is not positive yields the NaN or infinity the arithmetic yields.
template <int NC>
__host__ __device__ __forceinline__ void mls_solve(double (&A)[NC * (NC + 1) / 2], double (&b)[NC]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    double s = A[j * (j + 1) / 2 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - A[j * (j + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
    const double d = sqrt(s);
    A[j * (j + 1) / 2 + j] = d;
#pragma unroll
    for (int i = j + 1; i < NC; ++i) {
      double t = A[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t = t - A[i * (i + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
      A[i * (i + 1) / 2 + j] = t / d;
    }
  }
#pragma unroll
  for (int i = 0; i < NC; ++i) {  // L y = b
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - A[i * (i + 1) / 2 + k] * b[k];
    b[i] = s / A[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = NC - 1; i >= 0; --i) {  // L^T c = y
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < NC; ++k) s = s - A[k * (k + 1) / 2 + i] * b[k];
    b[i] = s / A[i * (i + 1) / 2 + i];
  }
}

}  // namespace icpgpu
