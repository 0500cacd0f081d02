// icp_normals.hip -- pcl::NormalEstimation<PointXYZ, Normal>: surface normals and curvature from the neighbour rows of the search
// cloud (rules: include/icpgpu.h "normal estimation"; host: icpgpu_search.cpp, icpgpu_normal_estimation).
//
// The neighbour rows are the neighbour search's (icp_search.hip), still in device memory: dense rows of stride k with n_found
// (setKSearch) or CSR rows with row_start (setRadiusSearch), ascending by key either way.  normals_from_rows_kernel turns a row
// into a normal, one lane per query:
//   * the row's indices and points eight at a time -- independent gathers, as ndt_cell_kernel walks a cell -- while the nine
//     float32 sums about the row's first point take them in row order (every product, sum, difference and quotient rounded on its
//     own: the tree builds with -ffp-contract=off);
//   * the six covariance entries widened to float64 through NDT's cyclic Jacobi (icp_jacobi3.h), the column of the smallest
//     eigenvalue (lowest index among equals) rounded to float32, PCL's curvature, flipNormalTowardsViewpoint;
//   * one float4 store, and nine more floats when the caller wants the moments.
// A row of fewer than three entries (a non-finite query's row is empty) or a non-finite covariance entry gives NaN.
#include <hip/hip_runtime.h>
#include <math.h>

#include "icp_device.h"
#include "icp_env.h"
#include "icp_jacobi3.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

constexpr int NE_BLOCK = 64;  // a wave per workgroup: 18 883 queries spread over every CU
constexpr int NE_GATHER = 8;  // row entries in flight per lane

// the sums of a row of m >= 3 entries about K -> the moments and, unless a covariance entry is not finite, the oriented normal
__device__ __forceinline__ void finish_normal(int m, const float4& K, const float4& p, float a0, float a1, float a2, float a3, float a4, float a5,
                                              float a6, float a7, float a8, float vpx, float vpy, float vpz, float4& result, float (&mom)[9]) {
  const float fm = (float)m;
  a0 /= fm, a1 /= fm, a2 /= fm, a3 /= fm, a4 /= fm, a5 /= fm, a6 /= fm, a7 /= fm, a8 /= fm;
  const float xx = a0 - a6 * a6, xy = a1 - a6 * a7, xz = a2 - a6 * a8, yy = a3 - a7 * a7, yz = a4 - a7 * a8, zz = a5 - a8 * a8;
  mom[0] = xx, mom[1] = xy, mom[2] = xz, mom[3] = yy, mom[4] = yz, mom[5] = zz;
  mom[6] = a6 + K.x, mom[7] = a7 + K.y, mom[8] = a8 + K.z;
  if (!(isfinite(xx) && isfinite(xy) && isfinite(xz) && isfinite(yy) && isfinite(yz) && isfinite(zz))) return;
  double a[3][3] = {{(double)xx, (double)xy, (double)xz}, {(double)xy, (double)yy, (double)yz}, {(double)xz, (double)yz, (double)zz}};
  double V[3][3];
  jacobi3(a, V);
  // the smallest eigenvalue, the lowest index among equals, and its eigenvector (a column of V) -- by selects: indexing V by the
  // column's number puts V into scratch
  const bool b1 = a[1][1] < a[0][0];
  const double lam01 = b1 ? a[1][1] : a[0][0];
  const bool b2 = a[2][2] < lam01;
  const double lam = b2 ? a[2][2] : lam01;
  const double ex = b2 ? V[0][2] : (b1 ? V[0][1] : V[0][0]);
  const double ey = b2 ? V[1][2] : (b1 ? V[1][1] : V[1][0]);
  const double ez = b2 ? V[2][2] : (b1 ? V[2][1] : V[2][0]);
  float nx = (float)ex, ny = (float)ey, nz = (float)ez;
  const float tr = (xx + yy) + zz;
  const float curvature = tr != 0.f ? fabsf((float)lam / tr) : 0.f;
  // flipNormalTowardsViewpoint with the QUERY point
  const float vx = vpx - p.x, vy = vpy - p.y, vz = vpz - p.z;
  const float cs = (vx * nx + vy * ny) + vz * nz;
  if (cs < 0.f) nx = -nx, ny = -ny, nz = -nz;
  result = make_float4(nx, ny, nz, curvature);
}

// rows: n_found != null: row i = idx[i * k, i * k + n_found[i]); else row i = idx[row_start[i], row_start[i + 1])
__global__ __launch_bounds__(NE_BLOCK) void normals_from_rows_kernel(const float4* __restrict__ queries, int n_q, const float4* __restrict__ cloud,
                                                                     int n, const int32_t* __restrict__ idx, const int32_t* __restrict__ n_found,
                                                                     int k, const int* __restrict__ row_start, float vpx, float vpy, float vpz,
                                                                     float4* __restrict__ out, float* __restrict__ moments) {
  const int i = blockIdx.x * NE_BLOCK + threadIdx.x;
  if (i >= n_q) return;
  size_t base;
  int m;
  if (n_found) {
    base = (size_t)i * (size_t)k;
    m = min(n_found[i], k);
  } else {
    base = (size_t)row_start[i];
    m = row_start[i + 1] - row_start[i];
  }
  const float nan = __builtin_nanf("");
  float4 result = make_float4(nan, nan, nan, nan);
  float mom[9] = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
  if (m >= 3 && n > 0) {
    const float4 p = queries[i];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f;
    float4 K = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < m; t0 += NE_GATHER) {
      int jj[NE_GATHER];
#pragma unroll
      for (int u = 0; u < NE_GATHER; ++u) jj[u] = min(max(idx[base + (size_t)min(t0 + u, m - 1)], 0), n - 1);  // (a row names cloud points)
      float4 pp[NE_GATHER];
#pragma unroll
      for (int u = 0; u < NE_GATHER; ++u) pp[u] = cloud[jj[u]];
      if (t0 == 0) K = pp[0];
#pragma unroll
      for (int u = 0; u < NE_GATHER; ++u) {
        if (t0 + u < m) {
          const float dx = pp[u].x - K.x, dy = pp[u].y - K.y, dz = pp[u].z - K.z;
          a0 += dx * dx;
          a1 += dx * dy;
          a2 += dx * dz;
          a3 += dy * dy;
          a4 += dy * dz;
          a5 += dz * dz;
          a6 += dx;
          a7 += dy;
          a8 += dz;
        }
      }
    }
    finish_normal(m, K, p, a0, a1, a2, a3, a4, a5, a6, a7, a8, vpx, vpy, vpz, result, mom);
  }
  out[i] = result;
  if (moments) {
#pragma unroll
    for (int e = 0; e < 9; ++e) moments[(size_t)i * 9 + e] = mom[e];
  }
}

#if defined(ICPGPU_DEV_SWITCHES)
// The alternative EXPERIMENTS.md records (ICPGPU_NORMALS_WAVE=1, development flavour only): a wave per query.  The lanes gather 64
// row entries at once -- one coalesced index load, one gather of points -- and every lane takes the sums through lane reads in row
// order (the same sequence of float32 operations); lane 0 stores.
__global__ __launch_bounds__(256) void normals_from_rows_wave_kernel(const float4* __restrict__ queries, int n_q, const float4* __restrict__ cloud,
                                                                     int n, const int32_t* __restrict__ idx, const int32_t* __restrict__ n_found,
                                                                     int k, const int* __restrict__ row_start, float vpx, float vpy, float vpz,
                                                                     float4* __restrict__ out, float* __restrict__ moments) {
  const int lane = (int)(threadIdx.x & 63u);
  const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (i >= n_q) return;  // (wave-uniform)
  size_t base;
  int m;
  if (n_found) {
    base = (size_t)i * (size_t)k;
    m = min(n_found[i], k);
  } else {
    base = (size_t)row_start[i];
    m = row_start[i + 1] - row_start[i];
  }
  m = __builtin_amdgcn_readfirstlane(m);
  const float nan = __builtin_nanf("");
  float4 result = make_float4(nan, nan, nan, nan);
  float mom[9] = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
  if (m >= 3 && n > 0) {
    const float4 p = queries[i];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f;
    float4 K = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < m; t0 += 64) {
      const int j = min(max(idx[base + (size_t)min(t0 + lane, m - 1)], 0), n - 1);
      const float4 q = cloud[j];
      if (t0 == 0) K = make_float4(__shfl(q.x, 0, 64), __shfl(q.y, 0, 64), __shfl(q.z, 0, 64), 0.f);
      const int cnt = min(64, m - t0);
      for (int t = 0; t < cnt; ++t) {
        const float dx = __shfl(q.x, t, 64) - K.x, dy = __shfl(q.y, t, 64) - K.y, dz = __shfl(q.z, t, 64) - K.z;
        a0 += dx * dx;
        a1 += dx * dy;
        a2 += dx * dz;
        a3 += dy * dy;
        a4 += dy * dz;
        a5 += dz * dz;
        a6 += dx;
        a7 += dy;
        a8 += dz;
      }
    }
    if (lane == 0) finish_normal(m, K, p, a0, a1, a2, a3, a4, a5, a6, a7, a8, vpx, vpy, vpz, result, mom);
  }
  if (lane != 0) return;
  out[i] = result;
  if (moments) {
#pragma unroll
    for (int e = 0; e < 9; ++e) moments[(size_t)i * 9 + e] = mom[e];
  }
}
#endif

}  // namespace

hipError_t launch_normals_from_rows(const float4* queries, int n_q, const float4* cloud, int n, const int32_t* idx, const int32_t* n_found, int k,
                                    const int* row_start, const float viewpoint[3], float4* out, float* moments, hipStream_t stream) {
  if (n_q <= 0) return hipSuccess;
  if ((n_found == nullptr) == (row_start == nullptr)) return hipErrorInvalidValue;
#if defined(ICPGPU_DEV_SWITCHES)
  if (const char* e = ICPGPU_DEV_ENV("ICPGPU_NORMALS_WAVE"); e && *e == '1') {
    hipLaunchKernelGGL(normals_from_rows_wave_kernel, dim3((n_q + 3) / 4), dim3(256), 0, stream, queries, n_q, cloud, n, idx, n_found, k, row_start,
                       viewpoint[0], viewpoint[1], viewpoint[2], out, moments);
    return hipGetLastError();
  }
#endif
  hipLaunchKernelGGL(normals_from_rows_kernel, dim3((n_q + NE_BLOCK - 1) / NE_BLOCK), dim3(NE_BLOCK), 0, stream, queries, n_q, cloud, n, idx, n_found,
                     k, row_start, viewpoint[0], viewpoint[1], viewpoint[2], out, moments);
  return hipGetLastError();
}

}  // namespace icpgpu
