// icp_iss.hip -- intrinsic shape signature keypoints over the search cloud (pcl::ISSKeypoint3D; rules: include/icpgpu.h "ISS
// keypoints").  Two walks of a ball per point, a wave each, and no neighbour rows in this unit: without border estimation memory is
// O(n) whatever the radii.  With it, the edge flags come from icp_boundary.hip over the border radius's rows (icpgpu_iss.cpp), and
// iss_border_kernel here spreads them over the border ball by a third walk.
//   * iss_scatter_kernel walks the salient ball over icp_search_device.h's ball_batches -- the cube of `shells` cells, or the whole
//     cloud, exactly as search_radius_count_kernel chooses.  A lane takes one candidate per batch and adds the six exact products of
//     an in-ball candidate into double-double accumulators of its own (icp_dd.h); the 64 lanes' accumulators are folded by dd_add in
//     a fixed butterfly, the count is a ballot's popcount.
//   * iss_eigen_kernel, a thread per point, runs the cyclic Jacobi (icp_jacobi3.h) on the six sums, sorts the diagonal and applies
//     the threshold tests.
//   * iss_suppress_kernel walks the non-max ball, reads saliency[j] through the candidate's index (the key's low word), counts the
//     ball and leaves -- wave-uniformly -- at the first neighbour with a larger saliency.  It writes a 0 / 1 flag per point.
//   * the flags are compacted by icp_scan.hip's launch_compact, which gathers the keypoints too.
#include <hip/hip_runtime.h>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_jacobi3.h"
#include "icp_kernels.h"
#include "icp_search_device.h"

namespace icpgpu {
namespace {

constexpr int ISS_BLOCK = 256, ISS_WAVES = ISS_BLOCK / 64;

// n_salient and scatter6 are zero before: what a non-finite point and a point with too few neighbours keep (n_salient of the latter
// is written).
__global__ __launch_bounds__(ISS_BLOCK) void iss_scatter_kernel(const float4* __restrict__ cloud, int n, const float4* __restrict__ sorted,
                                                                const int* __restrict__ cell_start, GridDesc g, int R, float r2, int min_neighbors,
                                                                const int32_t* __restrict__ border, int32_t* __restrict__ n_salient,
                                                                double* __restrict__ scatter6) {
  const unsigned int lane = threadIdx.x & 63u;
  const int i = blockIdx.x * ISS_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n) return;  // (wave-uniform)
  const float4 p = cloud[i];
  if (!finite3(p.x, p.y, p.z)) return;
  const bool skip = border && border[i] != 0;  // (wave-uniform) a border point: its ball is counted, nothing else
  DD acc[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) acc[e].hi = acc[e].lo = 0.0;
  int c = 0;
  ball_batches(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) {
    const bool in = key_in_ball(key, r2);
    c += __popcll(__ballot(in));
    if (in && !skip) {
      const float4 q = cloud[min((unsigned int)key, (unsigned int)(n - 1))];  // (the key names a cloud point)
      const double dx = (double)(q.x - p.x), dy = (double)(q.y - p.y), dz = (double)(q.z - p.z);
      dd_add_term(acc[0], dx * dx);  // (24 x 24 bits: exact)
      dd_add_term(acc[1], dx * dy);
      dd_add_term(acc[2], dx * dz);
      dd_add_term(acc[3], dy * dy);
      dd_add_term(acc[4], dy * dz);
      dd_add_term(acc[5], dz * dz);
    }
  });
  if (lane == 0) n_salient[i] = c;
  if (c < min_neighbors || skip) return;  // (wave-uniform)
  double s[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    DD a = acc[e];
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {  // (TwoSum is exact in either order: every lane holds the same pair after each step)
      DD o;
      o.hi = shfl_xor_f64(a.hi, j);
      o.lo = shfl_xor_f64(a.lo, j);
      a = dd_add(a, o);
    }
    s[e] = a.hi + a.lo;
  }
  if (lane != 0) return;
#pragma unroll
  for (int e = 0; e < 6; ++e) scatter6[(size_t)i * 6 + e] = s[e];
}

// A thread per point: the eigenvalues of its scatter matrix and its saliency.  eig3 and saliency are zero before: what a non-finite
// point and a point with too few neighbours keep.  (In the scatter kernel this would be one lane's work under a wave's exec mask: at
// 19k points it was three quarters of that kernel's time.)
__global__ __launch_bounds__(ISS_BLOCK) void iss_eigen_kernel(const float4* __restrict__ cloud, int n, int min_neighbors, double gamma_21,
                                                              double gamma_32, const int32_t* __restrict__ border,
                                                              const int32_t* __restrict__ n_salient, const double* __restrict__ scatter6, double* __restrict__ eig3,
                                                              double* __restrict__ saliency) {
  const int i = blockIdx.x * ISS_BLOCK + (int)threadIdx.x;
  if (i >= n) return;
  const float4 p = cloud[i];
  if (!finite3(p.x, p.y, p.z) || n_salient[i] < min_neighbors || (border && border[i] != 0)) return;
  double s[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) s[e] = scatter6[(size_t)i * 6 + e];
  double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}}, v[3][3];
  jacobi3(a, v);
  double e1 = a[0][0], e2 = a[1][1], e3 = a[2][2], t;
  if (e1 < e2) t = e1, e1 = e2, e2 = t;  // descending, by this network
  if (e2 < e3) t = e2, e2 = e3, e3 = t;
  if (e1 < e2) t = e1, e1 = e2, e2 = t;
  eig3[(size_t)i * 3 + 0] = e1;
  eig3[(size_t)i * 3 + 1] = e2;
  eig3[(size_t)i * 3 + 2] = e3;
  const bool fin = isfinite(e1) && isfinite(e2) && isfinite(e3);
  const bool ok = fin && e3 >= 0.0 && e2 / e1 < gamma_21 && e3 / e2 < gamma_32;  // (a NaN quotient fails)
  if (ok) saliency[i] = e3;
}

// cube_batches / sweep_batches / ball_batches of icp_search_device.h with a way out: f(key) returns false -- wave-uniformly -- when
// the wave needs no further candidate.  The same candidates in the same order up to there.
template <class F>
__device__ __forceinline__ bool segment_batches_while(const float4* __restrict__ sorted, int lo, int len, const float4& p, unsigned int lane, F&& f) {
  for (int k = 0; k < len; k += 64) {
    const int j = k + (int)lane;
    u64 key = kEmptyKey;
    if (j < len) {
      const float4 q = sorted[lo + j];
      key = make_key(dist2(q.x, q.y, q.z, p.x, p.y, p.z), __float_as_uint(q.w));
    }
    if (!f(key)) return false;
  }
  return true;
}

template <class F>
__device__ __forceinline__ void ball_batches_while(const float4* __restrict__ cloud, int n, const float4* __restrict__ sorted,
                                                   const int* __restrict__ cell_start, const GridDesc& g, int R, const float4& p, unsigned int lane,
                                                   F&& f) {
  int ux, uy, uz;
  if (R >= 0 && query_cell(sorted, g, p, ux, uy, uz)) {
    const int side = 2 * R + 1, nrows = side * side;
    const int x0 = max(ux - R, 0), x1 = min(ux + R, g.nx - 1);
    if (x0 > x1) return;  // (wave-uniform)
    for (int rb = 0; rb < nrows; rb += 64) {
      const int r = rb + (int)lane;
      const int zr = r / side, yr = r - zr * side;
      const int yy = uy + yr - R, zz = uz + zr - R;
      int lo = 0, len = 0;
      if (r < nrows && yy >= 0 && yy < g.ny && zz >= 0 && zz < g.nz) {
        const int row = zz * g.sz + yy * g.sy;
        lo = cell_start[row + x0];
        len = cell_start[row + x1 + 1] - lo;
      }
      unsigned long long mask = __ballot(len > 0);
      while (mask) {
        const int ra = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (!segment_batches_while(sorted, __builtin_amdgcn_readlane(lo, ra), __builtin_amdgcn_readlane(len, ra), p, lane, f)) return;
      }
    }
  } else {
    for (int base = 0; base < n; base += 64) {
      const int j = base + (int)lane;
      u64 key = kEmptyKey;
      if (j < n) {
        const float4 q = cloud[j];
        if (finite3(q.x, q.y, q.z)) key = make_key(dist2(q.x, q.y, q.z, p.x, p.y, p.z), (unsigned int)j);
      }
      if (!f(key)) return;
    }
  }
}

// flags[i] = 1 iff saliency[i] > 0, the non-max ball holds at least min_neighbors points and none of them has a larger saliency
__global__ __launch_bounds__(ISS_BLOCK) void iss_suppress_kernel(const float4* __restrict__ cloud, int n, const float4* __restrict__ sorted,
                                                                 const int* __restrict__ cell_start, GridDesc g, int R, float r2, int min_neighbors,
                                                                 const double* __restrict__ saliency, int* __restrict__ flags) {
  const unsigned int lane = threadIdx.x & 63u;
  const int i = blockIdx.x * ISS_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n) return;  // (wave-uniform)
  const double mine = saliency[i];
  int keep = 0;
  if (mine > 0.0) {  // (wave-uniform; a non-finite point has no saliency)
    const float4 p = cloud[i];
    int c = 0;
    bool larger = false;
    ball_batches_while(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) {
      const bool in = key_in_ball(key, r2);
      c += __popcll(__ballot(in));
      const bool above = in && saliency[min((unsigned int)key, (unsigned int)(n - 1))] > mine;
      larger = __ballot(above) != 0ull;
      return !larger;
    });
    keep = !larger && c >= min_neighbors ? 1 : 0;
  }
  if (lane == 0) flags[i] = keep;
}

// border[i] = 1 iff point i is finite and some point of its border ball, itself included, is an edge point.  The walk leaves at the
// first one.
__global__ __launch_bounds__(ISS_BLOCK) void iss_border_kernel(const float4* __restrict__ cloud, int n, const float4* __restrict__ sorted,
                                                               const int* __restrict__ cell_start, GridDesc g, int R, float r2,
                                                               const int32_t* __restrict__ edge, int32_t* __restrict__ border) {
  const unsigned int lane = threadIdx.x & 63u;
  const int i = blockIdx.x * ISS_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n) return;  // (wave-uniform)
  const float4 p = cloud[i];
  bool found = false;
  if (finite3(p.x, p.y, p.z)) {  // (wave-uniform)
    ball_batches_while(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) {
      const bool hit = key_in_ball(key, r2) && edge[min((unsigned int)key, (unsigned int)(n - 1))] != 0;
      found = __ballot(hit) != 0ull;
      return !found;
    });
  }
  if (lane == 0) border[i] = found ? 1 : 0;
}

}  // namespace

hipError_t launch_iss_border(const float4* cloud, int n, const float4* sorted, const int* cell_start, const GridDesc& g, int shells, float r2,
                             const int32_t* edge, int32_t* border, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(iss_border_kernel, dim3((n + ISS_WAVES - 1) / ISS_WAVES), dim3(ISS_BLOCK), 0, stream, cloud, n, sorted, cell_start, g, shells, r2,
                     edge, border);
  return hipGetLastError();
}

hipError_t launch_iss_keypoints(const float4* cloud, int n, bool any_finite, const float4* sorted, const int* cell_start, const GridDesc& g,
                                int shells_salient, float r2_salient, int shells_non_max, float r2_non_max, int min_neighbors, double gamma_21,
                                double gamma_32, const int32_t* border, int32_t* n_salient, double* scatter6, double* eig3, double* saliency,
                                int* flags, int* pos, int* scan_scratch, float4* points, int* kept, int* n_kept, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(n_kept, 0, sizeof(int), stream)) != hipSuccess) return e;
  if (n <= 0) return hipSuccess;
  if ((e = hipMemsetAsync(n_salient, 0, (size_t)n * sizeof(int32_t), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(scatter6, 0, (size_t)n * 6 * sizeof(double), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(eig3, 0, (size_t)n * 3 * sizeof(double), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(saliency, 0, (size_t)n * sizeof(double), stream)) != hipSuccess) return e;
  const dim3 grid((n + ISS_WAVES - 1) / ISS_WAVES), block(ISS_BLOCK);
  if (any_finite) {
    hipLaunchKernelGGL(iss_scatter_kernel, grid, block, 0, stream, cloud, n, sorted, cell_start, g, shells_salient, r2_salient, min_neighbors, border,
                       n_salient, scatter6);
    hipLaunchKernelGGL(iss_eigen_kernel, dim3((n + ISS_BLOCK - 1) / ISS_BLOCK), block, 0, stream, cloud, n, min_neighbors, gamma_21, gamma_32, border,
                       n_salient, scatter6, eig3, saliency);
  }
  hipLaunchKernelGGL(iss_suppress_kernel, grid, block, 0, stream, cloud, n, sorted, cell_start, g, shells_non_max, r2_non_max, min_neighbors, saliency,
                     flags);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return launch_compact(flags, n, pos, scan_scratch, kept, n_kept, cloud, points, stream);
}

}  // namespace icpgpu
