// icp_outlier.hip -- pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval (rules: include/icpgpu.h).
//
// SOR's hot path is an EXACT selection of the mean_k + 1 smallest squared distances of every point, mean_k variable up to 63:
//   * sor_dist_kernel: one wave64 per query.  The wave keeps the 64 smallest d2 seen so far SORTED, one per lane (the answer is
//     the first mean_k + 1 of them).  Candidates come 64 at a time from the cells of the cloud's own uniform grid, in shells of
//     growing Chebyshev radius around the query's cell -- every cell exactly once, the selection is over a multiset.  A batch none
//     of whose d2 is below the kept worst is skipped after one ballot; any other is sorted across the wave (bitonic, descending),
//     min-ed lane by lane against the kept list -- the 64 smallest of the 128, as a bitonic sequence -- and merged (6 steps).
//     After shell rho every cell within rho cells of the query's has been seen, so every unseen point lies at least rho * h away
//     (rho * h * kGridSafety once the float binning's rounding is allowed for: the grid search's own bound, too small if anything);
//     the search ends when the kept worst is not above that, or when the shells have covered the whole grid.
//   * a query that is not certified after kSorShells shells (an isolated return, metres from everything) goes on a list, and
//     sor_far_kernel -- a workgroup per listed point, the same selection fed from a linear sweep of the whole cloud -- finishes it.
//     A cloud the grid refuses goes through that kernel point by point (the host caps its size, as for GICP's covariances).
// ROR counts, per point, the grid neighbours inside the radius: the cells of the cube that contains the ball, one thread per point.
// The rest is shared: one fixed-order double-double reduction for SOR's sums and its threshold, keep flags, and the compaction
// of icp_scan.hip (launch_compact), which writes the kept points where the host will read them.
#include <hip/hip_runtime.h>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

constexpr int OL_BLOCK = 256, OL_WAVES = OL_BLOCK / 64;
constexpr int kSorShells = 6;      // shells 0..6 (13^3 cells at most) before a query is left to the far list
constexpr int OL_REDUCE = 1024;    // the one workgroup of the statistics kernel

// ---- the selection ---------------------------------------------------------------------------------------------------
// keep: ascending over the lanes (+inf = nothing yet); d: one candidate per lane (+inf = none).  No NaN reaches this: both
// points are finite, so d2 is a finite float or +inf.  K - 1 (wave-uniform) is the lane of the worst value that still counts.
__device__ __forceinline__ void knn_offer(float d, float& keep, int K, unsigned int lane) {
  const float worst = readlane_f(keep, K - 1);
  if (__ballot(d < worst) == 0ull) return;  // (a tie with the worst changes nothing: only the multiset of distances is used)
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const float o = __shfl_xor(d, j, 64);
      const bool desc = (lane & (unsigned int)k) == 0u, lower = (lane & (unsigned int)j) == 0u;
      d = (lower == desc) ? fmaxf(d, o) : fminf(d, o);
    }
  }
  keep = fminf(keep, d);  // ascending against descending: the 64 smallest of both, a bitonic sequence
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const float o = __shfl_xor(keep, j, 64);
    keep = (lane & (unsigned int)j) == 0u ? fminf(keep, o) : fmaxf(keep, o);
  }
}

// PCL's mean distance from the kept list: drop the smallest (the query itself), add sqrtf of the next mean_k in ascending order
// into a double, divide by mean_k, round to float (the same value in every lane)
__device__ __forceinline__ float sor_mean_distance(float keep, int K) {
  // correctly rounded sqrtf: through float64 (53 >= 2 * 24 + 2 bits, so the second rounding cannot change the result).  Not
  // __fsqrt_rn, which this toolchain maps to the 1-ulp native square root.
  const float root = (float)__builtin_sqrt((double)keep);
  double s = 0.0;
  for (int j = 1; j < K; ++j) s += (double)readlane_f(root, j);
  return (float)(s / (double)(K - 1));
}

// one row segment of `sorted` ([lo, lo + len)) offered to the wave's list
__device__ __forceinline__ void offer_segment(const float4* __restrict__ sorted, int lo, int len, const float4& p, float& keep, int K,
                                              unsigned int lane) {
  for (int k = 0; k < len; k += 64) {
    const int j = k + (int)lane;
    float d = __builtin_inff();
    if (j < len) {
      const float4 q = sorted[lo + j];
      d = dist2(q.x, q.y, q.z, p.x, p.y, p.z);
    }
    knn_offer(d, keep, K, lane);
  }
}

// far: [0] the number of listed points, [2 ...] their indices in the cloud
__global__ __launch_bounds__(OL_BLOCK) void sor_dist_kernel(const float4* __restrict__ sorted, const int* __restrict__ cell_start, GridDesc g,
                                                            int n_binned, int K, float* __restrict__ dist, int* __restrict__ far) {
  const unsigned int lane = threadIdx.x & 63u;
  const int s = blockIdx.x * OL_WAVES + (int)(threadIdx.x >> 6);
  if (s >= n_binned) return;  // (wave-uniform)
  const float4 p = sorted[s];
  int cx, cy, cz;
  cell_of(g, p.x, p.y, p.z, cx, cy, cz);
  float keep = __builtin_inff();
  bool done = false;
  for (int rho = 0; rho <= kSorShells && !done; ++rho) {
    const int side = 2 * rho + 1, nrows = side * side;
    const int x0 = max(cx - rho, 0), x1 = min(cx + rho, g.nx - 1);
    // pass 0: the rows on the shell's y / z faces in full, and of the rows inside them the cell at x = cx - rho;
    // pass 1: of the rows inside, the cell at x = cx + rho
    for (int pass = 0; pass < (rho > 0 ? 2 : 1); ++pass) {
      for (int rb = 0; rb < nrows; rb += 64) {
        const int r = rb + (int)lane;
        const int zr = r / side, yr = r - zr * side;
        const int dy = yr - rho, dz = zr - rho, yy = cy + dy, zz = cz + dz;
        int lo = 0, len = 0;
        if (r < nrows && yy >= 0 && yy < g.ny && zz >= 0 && zz < g.nz) {
          const bool face = max(abs(dy), abs(dz)) == rho;
          int xa = 1, xb = 0;
          if (pass == 0) {
            xa = face ? x0 : cx - rho;
            xb = face ? x1 : cx - rho;
          } else if (!face) {
            xa = xb = cx + rho;
          }
          if (xa <= xb && xa >= 0 && xb <= g.nx - 1) {
            const int row = zz * g.sz + yy * g.sy;
            lo = cell_start[row + xa];
            len = cell_start[row + xb + 1] - lo;
          }
        }
        unsigned long long mask = __ballot(len > 0);
        while (mask) {
          const int ra = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          offer_segment(sorted, __builtin_amdgcn_readlane(lo, ra), __builtin_amdgcn_readlane(len, ra), p, keep, K, lane);
        }
      }
    }
    const float worst = readlane_f(keep, K - 1);
    const float safe = (float)rho * g.h * kGridSafety;
    const bool whole = cx - rho <= 0 && cx + rho >= g.nx - 1 && cy - rho <= 0 && cy + rho >= g.ny - 1 && cz - rho <= 0 && cz + rho >= g.nz - 1;
    done = whole || worst <= safe * safe;
  }
  const unsigned int i = __float_as_uint(p.w);  // (grid builds put the point's index there)
  if (done) {
    const float m = sor_mean_distance(keep, K);
    if (lane == 0) dist[i] = m;
  } else if (lane == 0) {
    far[2 + atomicAdd(far, 1)] = (int)i;
  }
}

// list == null: every point of the cloud (no grid); else the *count points of the list.  A workgroup per point: its four waves
// take every fourth batch of the cloud, wave 0 merges the four lists.
__global__ __launch_bounds__(OL_BLOCK) void sor_far_kernel(const float4* __restrict__ cloud, int n, const int* __restrict__ count,
                                                           const int* __restrict__ list, int K, float* __restrict__ dist) {
  __shared__ float lists[OL_WAVES][64];
  const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const int m = list ? *count : n;
  for (int e = blockIdx.x; e < m; e += gridDim.x) {
    const int i = list ? list[e] : e;
    const float4 p = cloud[i];
    if (!finite3(p.x, p.y, p.z)) continue;  // (workgroup-uniform; such a point's dist stays 0)
    float keep = __builtin_inff();
    for (int base = 0; base < n; base += OL_BLOCK) {
      const int j = base + (int)threadIdx.x;
      float d = __builtin_inff();
      if (j < n) {
        const float4 q = cloud[j];
        if (finite3(q.x, q.y, q.z)) d = dist2(q.x, q.y, q.z, p.x, p.y, p.z);
      }
      knn_offer(d, keep, K, lane);
    }
    lists[wave][lane] = keep;
    __syncthreads();
    if (wave == 0) {
      for (int w = 1; w < OL_WAVES; ++w) knn_offer(lists[w][lane], keep, K, lane);
      const float mean = sor_mean_distance(keep, K);
      if (lane == 0) dist[i] = mean;
    }
    __syncthreads();
  }
}

// ---- ROR ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ror_flag(int k, int min_pts, int negative) {
  const bool removed = negative ? (k > min_pts) : (k <= min_pts);
  return removed ? 0 : 1;
}

// every point: k = 0 (what a non-finite point keeps, and every point when r2 == 0)
__global__ __launch_bounds__(OL_BLOCK) void ror_init_kernel(int n, int min_pts, int negative, float* __restrict__ measure, int* __restrict__ flags) {
  const int i = blockIdx.x * OL_BLOCK + threadIdx.x;
  if (i >= n) return;
  measure[i] = 0.f;
  flags[i] = ror_flag(0, min_pts, negative);
}

// one thread per binned point: the cells of the cube of g.r_max cells around its own (r_max * h * kGridSafety >= radius: the grid
// was built for the radius as a grid search's is for its gate, so the cube contains the ball)
__global__ __launch_bounds__(OL_BLOCK) void ror_count_kernel(const float4* __restrict__ sorted, const int* __restrict__ cell_start, GridDesc g,
                                                             int n_binned, float r2, int min_pts, int negative, float* __restrict__ measure,
                                                             int* __restrict__ flags) {
  const int s = blockIdx.x * OL_BLOCK + threadIdx.x;
  if (s >= n_binned) return;
  const float4 p = sorted[s];
  int cx, cy, cz;
  cell_of(g, p.x, p.y, p.z, cx, cy, cz);
  const int R = g.r_max;
  const int x0 = max(cx - R, 0), x1 = min(cx + R, g.nx - 1);
  int k = 0;
  if (x0 <= x1)
    for (int zz = max(cz - R, 0); zz <= min(cz + R, g.nz - 1); ++zz)
      for (int yy = max(cy - R, 0); yy <= min(cy + R, g.ny - 1); ++yy) {
        const int row = zz * g.sz + yy * g.sy;
        const int lo = cell_start[row + x0], hi = cell_start[row + x1 + 1];
        for (int j = lo; j < hi; ++j) {
          const float4 q = sorted[j];
          k += dist2(q.x, q.y, q.z, p.x, p.y, p.z) < r2 ? 1 : 0;
        }
      }
  const unsigned int i = __float_as_uint(p.w);
  measure[i] = (float)k;
  flags[i] = ror_flag(k, min_pts, negative);
}

// no grid: every point against the whole cloud, through LDS tiles
__global__ __launch_bounds__(OL_BLOCK) void ror_brute_kernel(const float4* __restrict__ cloud, int n, float r2, int min_pts, int negative,
                                                             float* __restrict__ measure, int* __restrict__ flags) {
  __shared__ float4 tile[OL_BLOCK];
  const int i = blockIdx.x * OL_BLOCK + threadIdx.x;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  bool live = false;
  if (i < n) {
    p = cloud[i];
    live = finite3(p.x, p.y, p.z);
  }
  int k = 0;
  for (int base = 0; base < n; base += OL_BLOCK) {
    const int j = base + (int)threadIdx.x;
    float4 q = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
    if (j < n) q = cloud[j];
    __syncthreads();
    tile[threadIdx.x] = q;
    __syncthreads();
    const int m = min(OL_BLOCK, n - base);
    if (live)
      for (int t = 0; t < m; ++t) {
        const float4 c = tile[t];
        if (finite3(c.x, c.y, c.z)) k += dist2(c.x, c.y, c.z, p.x, p.y, p.z) < r2 ? 1 : 0;
      }
  }
  if (i < n) {
    measure[i] = (float)k;
    flags[i] = ror_flag(k, min_pts, negative);
  }
}

// ---- SOR's statistics ---------------------------------------------------------------------------------------------------
// (double-double accumulation: icp_dd.h, shared with the plane refinement's sums in icp_sac.hip)

// ONE workgroup, a fixed order (thread t takes i = t, t + 1024, ...; then a binary tree): sum and sq_sum of dist[] as exact sums
// rounded once, n_valid = the finite points; then the threshold, every operation an IEEE float64 operation on its own.
// stats: mean, stddev, threshold, n_valid (as a double)
__global__ __launch_bounds__(OL_REDUCE) void sor_stats_kernel(const float4* __restrict__ cloud, const float* __restrict__ dist, int n,
                                                              double stddev_mult, double* __restrict__ stats) {
  __shared__ DD sh_s[OL_REDUCE], sh_q[OL_REDUCE];
  __shared__ int sh_n[OL_REDUCE];
  DD s = {0.0, 0.0}, q = {0.0, 0.0};
  int nv = 0;
  for (int i = threadIdx.x; i < n; i += OL_REDUCE) {
    const float4 p = cloud[i];
    const double d = (double)dist[i];
    dd_add_term(s, d);
    dd_add_term(q, d * d);  // (24 x 24 bits: exact)
    nv += finite3(p.x, p.y, p.z) ? 1 : 0;
  }
  sh_s[threadIdx.x] = s;
  sh_q[threadIdx.x] = q;
  sh_n[threadIdx.x] = nv;
  __syncthreads();
  for (int step = OL_REDUCE / 2; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) {
      sh_s[threadIdx.x] = dd_add(sh_s[threadIdx.x], sh_s[threadIdx.x + step]);
      sh_q[threadIdx.x] = dd_add(sh_q[threadIdx.x], sh_q[threadIdx.x + step]);
      sh_n[threadIdx.x] += sh_n[threadIdx.x + step];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sum = sh_s[0].hi + sh_s[0].lo, sq_sum = sh_q[0].hi + sh_q[0].lo;
    const double n_valid = (double)sh_n[0];
    const double mean = sum / n_valid;
    const double var = (sq_sum - sum * sum / n_valid) / (n_valid - 1.0);
    const double stddev = __builtin_sqrt(var);  // (IEEE: correctly rounded)
    stats[0] = mean;
    stats[1] = stddev;
    stats[2] = mean + stddev_mult * stddev;
    stats[3] = n_valid;
  }
}

__global__ __launch_bounds__(OL_BLOCK) void sor_flags_kernel(const float* __restrict__ dist, int n, const double* __restrict__ stats, int negative,
                                                             int* __restrict__ flags) {
  const int i = blockIdx.x * OL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double d = (double)dist[i], thr = stats[2];
  const bool removed = negative ? (d <= thr) : (d > thr);  // (a NaN threshold removes nothing either way)
  flags[i] = removed ? 0 : 1;
}

}  // namespace

hipError_t launch_sor_distances(const float4* cloud, int n, const float4* sorted, const int* cell_start, const GridDesc& g, int n_binned,
                                int mean_k, float* dist, int* far, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (mean_k < 1 || mean_k > 63) return hipErrorInvalidValue;
  const int K = mean_k + 1;
  hipError_t e = hipMemsetAsync(dist, 0, (size_t)n * sizeof(float), stream);  // (what a non-finite point keeps)
  if (e != hipSuccess) return e;
  if (sorted) {
    if ((e = hipMemsetAsync(far, 0, 2 * sizeof(int), stream)) != hipSuccess) return e;
    if (n_binned > 0) {
      hipLaunchKernelGGL(sor_dist_kernel, dim3((n_binned + OL_WAVES - 1) / OL_WAVES), dim3(OL_BLOCK), 0, stream, sorted, cell_start, g, n_binned, K,
                         dist, far);
      hipLaunchKernelGGL(sor_far_kernel, dim3(min(n_binned, 4096)), dim3(OL_BLOCK), 0, stream, cloud, n, far, far + 2, K, dist);
    }
  } else {
    hipLaunchKernelGGL(sor_far_kernel, dim3(min(n, 4096)), dim3(OL_BLOCK), 0, stream, cloud, n, static_cast<const int*>(nullptr),
                       static_cast<const int*>(nullptr), K, dist);
  }
  return hipGetLastError();
}

hipError_t launch_sor_flags(const float4* cloud, const float* dist, int n, double stddev_mult, int negative, double* stats, int* flags,
                            hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sor_stats_kernel, dim3(1), dim3(OL_REDUCE), 0, stream, cloud, dist, n, stddev_mult, stats);
  hipLaunchKernelGGL(sor_flags_kernel, dim3((n + OL_BLOCK - 1) / OL_BLOCK), dim3(OL_BLOCK), 0, stream, dist, n, stats, negative, flags);
  return hipGetLastError();
}

hipError_t launch_ror_counts(const float4* cloud, int n, const float4* sorted, const int* cell_start, const GridDesc& g, int n_binned, float r2,
                             int min_pts, int negative, bool brute, float* measure, int* flags, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 block(OL_BLOCK);
  if (brute) {
    hipLaunchKernelGGL(ror_brute_kernel, dim3((n + OL_BLOCK - 1) / OL_BLOCK), block, 0, stream, cloud, n, r2, min_pts, negative, measure, flags);
  } else {
    hipLaunchKernelGGL(ror_init_kernel, dim3((n + OL_BLOCK - 1) / OL_BLOCK), block, 0, stream, n, min_pts, negative, measure, flags);
    if (sorted && n_binned > 0)
      hipLaunchKernelGGL(ror_count_kernel, dim3((n_binned + OL_BLOCK - 1) / OL_BLOCK), block, 0, stream, sorted, cell_start, g, n_binned, r2, min_pts,
                         negative, measure, flags);
  }
  return hipGetLastError();
}

}  // namespace icpgpu
