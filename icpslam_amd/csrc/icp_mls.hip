// icp_mls.hip -- moving least squares over the search cloud's radius rows (pcl::MovingLeastSquares, UpsamplingMethod NONE; rules:
// include/icpgpu.h "moving least squares"; host: icpgpu_mls.cpp).  Every query is a small weighted least-squares problem in float64,
// defined operation by operation (tests/mls_restated.py computes the same bits).  The sums over a row take a wave per query, as
// iss_scatter_kernel's do; what follows them is one thread's work and takes a thread per query, as iss_eigen_kernel does:
//   * mls_moments_kernel, a wave per query: lane l adds the row's entries l, l + 64, ... into nine accumulators of its own -- the 64
//     partials of the rule's WSUM -- which six xor exchanges fold, every lane ending with the same bits.
//   * mls_plane_kernel, a thread per query: the plane, the frame and the projection (icp_mls.h: mls_plane); the plane's answer is
//     written as the query's result, which stands unless a polynomial replaces it.
//   * mls_fit_kernel<ORDER>, a wave per query: the weights (icp_exp.h: exp_neg), the monomials and the 27 (order 2) or 65 (order 3)
//     sums of the normal equations, lane partials folded the same way.
//   * mls_solve_kernel<ORDER>, a thread per query: the Cholesky solve (icp_mls.h: mls_solve), fully unrolled, and the polynomial's point
//     and normal where c_0 is finite.
//   * the kept queries are compacted by icp_scan.hip's launch_compact over the 0 / 1 flags; mls_gather_kernel moves their points and
//     normals to the positions it found.
#include <hip/hip_runtime.h>
#include <math.h>

#include "icp_device.h"
#include "icp_exp.h"
#include "icp_kernels.h"
#include "icp_mls.h"

namespace icpgpu {
namespace {

constexpr int MLS_BLOCK = 256, MLS_WAVES = MLS_BLOCK / 64;

// WSUM's fold: partial l becomes partial[l] + partial[l ^ mask] for mask = 32 .. 1 (IEEE addition commutes: all lanes agree)
__device__ __forceinline__ double wave_fold(double v) {
#pragma unroll
  for (int mask = 32; mask > 0; mask >>= 1) v = v + __shfl_xor(v, mask, 64);
  return v;
}

__device__ __forceinline__ int row_point(const int32_t* __restrict__ idx, size_t at, int n) {  // (a row names cloud points)
  return min(max(idx[at], 0), n - 1);
}

__global__ __launch_bounds__(MLS_BLOCK) void mls_moments_kernel(int n_q, const float4* __restrict__ cloud, int n, const int32_t* __restrict__ idx,
                                                                const int* __restrict__ row_start, int32_t* __restrict__ n_neighbours,
                                                                double* __restrict__ sums9) {
  const int lane = (int)(threadIdx.x & 63u);
  const int i = blockIdx.x * MLS_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n_q) return;  // (wave-uniform)
  const size_t base = (size_t)row_start[i];
  const int m = __builtin_amdgcn_readfirstlane(row_start[i + 1] - row_start[i]);
  if (lane == 0) n_neighbours[i] = m;
  if (m < 3 || n <= 0) return;  // (wave-uniform)
  const float4 K = cloud[row_point(idx, base, n)];
  const double kx = (double)K.x, ky = (double)K.y, kz = (double)K.z;
  double acc[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) acc[e] = 0.0;
  for (int t = lane; t < m; t += 64) {
    const float4 q = cloud[row_point(idx, base + (size_t)t, n)];
    const double dx = (double)q.x - kx, dy = (double)q.y - ky, dz = (double)q.z - kz;
    acc[0] = acc[0] + dx * dx;
    acc[1] = acc[1] + dx * dy;
    acc[2] = acc[2] + dx * dz;
    acc[3] = acc[3] + dy * dy;
    acc[4] = acc[4] + dy * dz;
    acc[5] = acc[5] + dz * dz;
    acc[6] = acc[6] + dx;
    acc[7] = acc[7] + dy;
    acc[8] = acc[8] + dz;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) acc[e] = wave_fold(acc[e]);
  if (lane != 0) return;
#pragma unroll
  for (int e = 0; e < 9; ++e) sums9[(size_t)i * 9 + e] = acc[e];
}

// frame12: Q, N, U, V.  Every per-query output is written here for every query: status 0 with NaN where the row is too short.
__global__ __launch_bounds__(MLS_BLOCK) void mls_plane_kernel(const float4* __restrict__ queries, int n_q, const float4* __restrict__ cloud, int n,
                                                              const int32_t* __restrict__ idx, const int* __restrict__ row_start,
                                                              const int32_t* __restrict__ n_neighbours, const double* __restrict__ sums9,
                                                              double* __restrict__ frame12, int32_t* __restrict__ status, int* __restrict__ flags,
                                                              double* __restrict__ plane7, double* __restrict__ coeff10, float4* __restrict__ points,
                                                              float4* __restrict__ normals) {
  const int i = blockIdx.x * MLS_BLOCK + (int)threadIdx.x;
  if (i >= n_q) return;
  const double nan = __builtin_nan("");
  const float nanf_ = __builtin_nanf("");
#pragma unroll
  for (int e = 0; e < 10; ++e) coeff10[(size_t)i * 10 + e] = nan;
  const int m = n_neighbours[i];
  if (m < 3 || n <= 0) {
    status[i] = 0;
    flags[i] = 0;
#pragma unroll
    for (int e = 0; e < 7; ++e) plane7[(size_t)i * 7 + e] = nan;
    points[i] = make_float4(nanf_, nanf_, nanf_, nanf_);
    normals[i] = make_float4(nanf_, nanf_, nanf_, nanf_);
    return;
  }
  const float4 p = queries[i], k4 = cloud[row_point(idx, (size_t)row_start[i], n)];
  const double P[3] = {(double)p.x, (double)p.y, (double)p.z}, K[3] = {(double)k4.x, (double)k4.y, (double)k4.z};
  double sums[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) sums[e] = sums9[(size_t)i * 9 + e];
  MlsPlane pl;
  mls_plane(sums, m, K, P, pl);
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    frame12[(size_t)i * 12 + e] = pl.Q[e];
    frame12[(size_t)i * 12 + 3 + e] = pl.N[e];
    frame12[(size_t)i * 12 + 6 + e] = pl.U[e];
    frame12[(size_t)i * 12 + 9 + e] = pl.V[e];
    plane7[(size_t)i * 7 + e] = pl.N[e];
    plane7[(size_t)i * 7 + 3 + e] = pl.c[e];
  }
  plane7[(size_t)i * 7 + 6] = pl.lambda;
  status[i] = 1;
  flags[i] = 1;
  points[i] = make_float4((float)pl.Q[0], (float)pl.Q[1], (float)pl.Q[2], 1.f);
  normals[i] = make_float4((float)pl.N[0], (float)pl.N[1], (float)pl.N[2], pl.curvature);
}

// fit: A's lower triangle in rows, then b (icp_mls.h: mls_sums(ORDER) doubles per query); written for the rows of at least nc entries
template <int ORDER>
__global__ __launch_bounds__(MLS_BLOCK) void mls_fit_kernel(int n_q, const float4* __restrict__ cloud, int n, const int32_t* __restrict__ idx,
                                                            const int* __restrict__ row_start, const double* __restrict__ frame12, double s,
                                                            double* __restrict__ fit) {
  constexpr int NC = mls_coefficients(ORDER), NA = NC * (NC + 1) / 2, NS = mls_sums(ORDER);
  const int lane = (int)(threadIdx.x & 63u);
  const int i = blockIdx.x * MLS_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n_q) return;  // (wave-uniform)
  const size_t base = (size_t)row_start[i];
  const int m = __builtin_amdgcn_readfirstlane(row_start[i + 1] - row_start[i]);
  if (m < 3 || m < NC || n <= 0) return;  // (wave-uniform)
  double F[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) F[e] = frame12[(size_t)i * 12 + e];
  double acc[NS];
#pragma unroll
  for (int e = 0; e < NS; ++e) acc[e] = 0.0;
  for (int t = lane; t < m; t += 64) {
    const float4 q = cloud[row_point(idx, base + (size_t)t, n)];
    const double dx = (double)q.x - F[0], dy = (double)q.y - F[1], dz = (double)q.z - F[2];
    const double dd = (dx * dx + dy * dy) + dz * dz;
    const double w = exp_neg(-dd / s);
    const double u = (dx * F[6] + dy * F[7]) + dz * F[8];
    const double v = (dx * F[9] + dy * F[10]) + dz * F[11];
    const double f = (dx * F[3] + dy * F[4]) + dz * F[5];
    double P[NC];
    {
      int j = 0;
      double u_pow = 1.0;
#pragma unroll
      for (int ui = 0; ui <= ORDER; ++ui) {
        double v_pow = 1.0;
#pragma unroll
        for (int vi = 0; vi <= ORDER - ui; ++vi) {
          P[j++] = u_pow * v_pow;
          v_pow = v_pow * v;
        }
        u_pow = u_pow * u;
      }
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) {
      const double pw = P[a] * w;
#pragma unroll
      for (int b = 0; b <= a; ++b) acc[a * (a + 1) / 2 + b] = acc[a * (a + 1) / 2 + b] + pw * P[b];
      acc[NA + a] = acc[NA + a] + pw * f;
    }
  }
#pragma unroll
  for (int e = 0; e < NS; ++e) acc[e] = wave_fold(acc[e]);
  if (lane != 0) return;
#pragma unroll
  for (int e = 0; e < NS; ++e) fit[(size_t)i * NS + e] = acc[e];
}

template <int ORDER>
__global__ __launch_bounds__(64) void mls_solve_kernel(int n_q, const int32_t* __restrict__ n_neighbours, const double* __restrict__ frame12,
                                                       const double* __restrict__ fit, int32_t* __restrict__ status, double* __restrict__ coeff10,
                                                       float4* __restrict__ points, float4* __restrict__ normals) {
  constexpr int NC = mls_coefficients(ORDER), NA = NC * (NC + 1) / 2, NS = mls_sums(ORDER);
  const int i = blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_q) return;
  const int m = n_neighbours[i];
  if (m < 3 || m < NC) return;
  double A[NA], c[NC];
#pragma unroll
  for (int e = 0; e < NA; ++e) A[e] = fit[(size_t)i * NS + e];
#pragma unroll
  for (int e = 0; e < NC; ++e) c[e] = fit[(size_t)i * NS + NA + e];
  mls_solve<NC>(A, c);
#pragma unroll
  for (int e = 0; e < NC; ++e) coeff10[(size_t)i * 10 + e] = c[e];
  if (!isfinite(c[0])) {
    status[i] = 3;
    return;
  }
  status[i] = 2;
  double F[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) F[e] = frame12[(size_t)i * 12 + e];
  const double cu = c[ORDER + 1], cv = c[1];
  float out[3], nrm[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    out[e] = (float)(F[e] + c[0] * F[3 + e]);
    nrm[e] = (float)((F[3 + e] - cu * F[6 + e]) - cv * F[9 + e]);
  }
  points[i] = make_float4(out[0], out[1], out[2], 1.f);
  normals[i] = make_float4(nrm[0], nrm[1], nrm[2], normals[i].w);
}

__global__ __launch_bounds__(MLS_BLOCK) void mls_gather_kernel(int n_q, const int* __restrict__ flags, const int* __restrict__ pos,
                                                               const float4* __restrict__ points, const float4* __restrict__ normals,
                                                               float4* __restrict__ out_points, float4* __restrict__ out_normals) {
  const int i = blockIdx.x * MLS_BLOCK + (int)threadIdx.x;
  if (i >= n_q || !flags[i]) return;
  const int at = pos[i];
  out_points[at] = points[i];
  out_normals[at] = normals[i];
}

template <int ORDER>
void launch_fit_and_solve(int n_q, const float4* cloud, int n, const int32_t* idx, const int* row_start, const int32_t* n_neighbours,
                          const double* frame12, double s, double* fit, int32_t* status, double* coeff10, float4* points, float4* normals,
                          hipStream_t stream) {
  hipLaunchKernelGGL(mls_fit_kernel<ORDER>, dim3((n_q + MLS_WAVES - 1) / MLS_WAVES), dim3(MLS_BLOCK), 0, stream, n_q, cloud, n, idx, row_start,
                     frame12, s, fit);
  hipLaunchKernelGGL(mls_solve_kernel<ORDER>, dim3((n_q + 63) / 64), dim3(64), 0, stream, n_q, n_neighbours, frame12, fit, status, coeff10, points,
                     normals);
}

}  // namespace

size_t mls_fit_doubles(int order) { return order == 3 ? (size_t)mls_sums(3) : order == 2 ? (size_t)mls_sums(2) : 0; }

hipError_t launch_mls(const float4* queries, int n_q, const float4* cloud, int n, const int32_t* idx, const int* row_start, int order, double s,
                      int32_t* n_neighbours, double* sums9, double* frame12, double* fit, int32_t* status, double* plane7, double* coeff10,
                      float4* points, float4* normals, int* flags, int* pos, int* scan_scratch, int* kept, int* n_kept, float4* out_points,
                      float4* out_normals, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(n_kept, 0, sizeof(int), stream)) != hipSuccess) return e;
  if (n_q <= 0) return hipSuccess;
  const dim3 waves((n_q + MLS_WAVES - 1) / MLS_WAVES), threads((n_q + MLS_BLOCK - 1) / MLS_BLOCK), block(MLS_BLOCK);
  hipLaunchKernelGGL(mls_moments_kernel, waves, block, 0, stream, n_q, cloud, n, idx, row_start, n_neighbours, sums9);
  hipLaunchKernelGGL(mls_plane_kernel, threads, block, 0, stream, queries, n_q, cloud, n, idx, row_start, n_neighbours, sums9, frame12, status,
                     flags, plane7, coeff10, points, normals);
  if (order == 2) launch_fit_and_solve<2>(n_q, cloud, n, idx, row_start, n_neighbours, frame12, s, fit, status, coeff10, points, normals, stream);
  if (order == 3) launch_fit_and_solve<3>(n_q, cloud, n, idx, row_start, n_neighbours, frame12, s, fit, status, coeff10, points, normals, stream);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_compact(flags, n_q, pos, scan_scratch, kept, n_kept, nullptr, nullptr, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(mls_gather_kernel, threads, block, 0, stream, n_q, flags, pos, points, normals, out_points, out_normals);
  return hipGetLastError();
}

}  // namespace icpgpu
