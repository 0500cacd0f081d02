// icp_search.hip -- pcl::search::KdTree / pcl::KdTreeFLANN: nearestKSearch and radiusSearch over a context's search cloud (rules:
// include/icpgpu.h "neighbour search").
//
// A neighbour is a KEY: (bits of d2) << 32 | index of the cloud point.  d2 >= +0 for finite points, so keys order like
// (d2, index), they are unique (one per cloud point), and the all-ones key (kEmptyKey) sorts behind every real one.  Every result
// row is ascending by key: by distance, the lowest index first among equal distances.
//
// k-nearest is the outlier filter's selection (icp_outlier.hip: knn_offer) with keys in place of bare distances:
//   * search_knn_kernel: one wave64 per query keeps the 64 smallest keys seen so far sorted across its lanes, takes candidates 64 at a
//     time from shells of the cloud's k-NN grid, skips a batch after one ballot or merges it bitonically, and stops on the grid
//     search's certificate.  Two things differ from the distance-only selection, because the indices are part of the answer:
//       - a batch is skipped only when no candidate KEY is below the kept worst key (a candidate that ties the worst distance with
//         a lower index replaces it);
//       - the walk stops only when the kept worst d2 is STRICTLY below the bound on every unseen point (an unseen point at exactly
//         the bound may carry a lower index than the kept worst), or when the shells have covered the whole grid.
//     A query need not lie inside the cloud's box: the walk starts from its cell CLAMPED into the grid.  The certificate still
//     holds: a cell not yet seen differs from the clamped cell by more than rho on some axis, and because clamping moves the
//     query's cell towards every cell of the grid it differs from the query's own (unclamped) cell by more than rho on that axis
//     too -- which is all the bound rho * h * kGridSafety rests on.  (Equivalently: the per-axis clamp of the query lies in the
//     clamped cell and no point of the box is nearer to the query than to its clamp on any axis.)  Queries more than
//     kSearchOutside cells outside the grid are not walked at all: their cell coordinates are too large for the float binning's
//     rounding to stay inside kGridSafety.
//   * a query that is not certified after kSearchShells shells, one too far outside, and every query of a cloud the grid refuses
//     goes on a list; search_far_kernel -- a workgroup per listed query, the same selection fed from a sweep of the whole cloud,
//     four waves merged through LDS -- finishes it.
// Radius search walks the cube of R = ceil(radius / (h * kGridSafety)) cells around the query's cell (every cloud point with
// d2 < r2 lies in it, by the same bound), or the whole cloud when the host found R above kSearchRadiusShells, the cloud has no grid,
// or the query lies too far outside:
//   * search_radius_count_kernel counts per query (and cuts the count at max_nn);
//   * an exclusive scan (icp_scan.hip) makes row_start;
//   * search_radius_fill_kernel, the wave that owns a row, fills and orders it.  A row of at most 64 entries IS a keyed selection
//     with the extra cut d2 < r2 (K = the row's length): it is sorted in the lanes when the walk ends.  A longer row is written
//     unordered into scratch and ranked by counting -- keys are unique, so the ranks are a permutation (gicp_cov_select_kernel's
//     trick) -- and entries whose rank is below the row's length land at their rank: that both orders the row and truncates it to
//     max_nn.  Ranking is quadratic in the row's length: right for a voxel-filtered scan, whose rows stay below 64 entries at LIDAR
//     radii, and the first thing to replace (a bitonic pass through LDS) for raw scans, whose near-field rows run to thousands.
#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"
#include "icp_search_device.h"

namespace icpgpu {
namespace {

constexpr int SR_BLOCK = 256, SR_WAVES = SR_BLOCK / 64;
constexpr int kSearchShells = 6;    // shells 0..6 (13^3 cells at most) before a query is left to the far list

// (the keyed selection -- shfl_xor_key, readlane_key, key_offer -- and write_knn_row: icp_search_device.h)

// (where candidates come from -- segment_batches, cube_batches, sweep_batches, query_cell, ball_batches: icp_search_device.h)

// the cells of shell rho (Chebyshev distance exactly rho) around cell (cx, cy, cz), clipped to the grid: icp_outlier.hip's walk
template <class F>
__device__ __forceinline__ void shell_batches(const float4* __restrict__ sorted, const int* __restrict__ cell_start, const GridDesc& g, int cx,
                                              int cy, int cz, int rho, const float4& p, unsigned int lane, F&& f) {
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
        segment_batches(sorted, __builtin_amdgcn_readlane(lo, ra), __builtin_amdgcn_readlane(len, ra), p, lane, f);
      }
    }
  }
}

// ---- k-nearest -------------------------------------------------------------------------------------------------------
// far: [0] the number of listed queries, [2 ...] their indices
__global__ __launch_bounds__(SR_BLOCK) void search_knn_kernel(const float4* __restrict__ queries, int n_q, const float4* __restrict__ sorted,
                                                              const int* __restrict__ cell_start, GridDesc g, int k, int32_t* __restrict__ idx,
                                                              float* __restrict__ d2, int32_t* __restrict__ n_found, int* __restrict__ far) {
  const unsigned int lane = threadIdx.x & 63u;
  const int q = blockIdx.x * SR_WAVES + (int)(threadIdx.x >> 6);
  if (q >= n_q) return;  // (wave-uniform)
  const float4 p = queries[q];
  u64 keep = kEmptyKey;
  if (!finite3(p.x, p.y, p.z)) {  // a non-finite query finds nothing
    write_knn_row(keep, k, (size_t)q, lane, idx, d2, n_found);
    return;
  }
  int ux, uy, uz;
  bool done = false;
  if (query_cell(sorted, g, p, ux, uy, uz)) {
    const int cx = min(max(ux, 0), g.nx - 1), cy = min(max(uy, 0), g.ny - 1), cz = min(max(uz, 0), g.nz - 1);
    for (int rho = 0; rho <= kSearchShells && !done; ++rho) {
      shell_batches(sorted, cell_start, g, cx, cy, cz, rho, p, lane, [&](u64 key) { key_offer(key, keep, k, lane); });
      const float worst = __uint_as_float((unsigned int)(readlane_key(keep, k - 1) >> 32));  // (an empty slot reads as a NaN: never certified)
      const float safe = (float)rho * g.h * kGridSafety;
      const bool whole = cx - rho <= 0 && cx + rho >= g.nx - 1 && cy - rho <= 0 && cy + rho >= g.ny - 1 && cz - rho <= 0 && cz + rho >= g.nz - 1;
      done = whole || worst < safe * safe;  // strictly: an unseen point AT the bound may carry a lower index than the kept worst
    }
  }
  if (done) write_knn_row(keep, k, (size_t)q, lane, idx, d2, n_found);
  else if (lane == 0) far[2 + atomicAdd(far, 1)] = q;
}

// the *count listed queries, a workgroup each: its four waves take every fourth batch of the cloud, wave 0 merges the four lists
__global__ __launch_bounds__(SR_BLOCK) void search_far_kernel(const float4* __restrict__ queries, const float4* __restrict__ cloud, int n,
                                                              const int* __restrict__ count, const int* __restrict__ list, int k,
                                                              int32_t* __restrict__ idx, float* __restrict__ d2, int32_t* __restrict__ n_found) {
  __shared__ u64 lists[SR_WAVES][64];
  const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const int m = *count;
  for (int e = blockIdx.x; e < m; e += gridDim.x) {
    const int q = list[e];
    const float4 p = queries[q];
    u64 keep = kEmptyKey;
    sweep_batches(cloud, n, (int)threadIdx.x, SR_BLOCK, p, [&](u64 key) { key_offer(key, keep, k, lane); });
    lists[wave][lane] = keep;
    __syncthreads();
    if (wave == 0) {
      for (int w = 1; w < SR_WAVES; ++w) key_offer(lists[w][lane], keep, k, lane);
      write_knn_row(keep, k, (size_t)q, lane, idx, d2, n_found);
    }
    __syncthreads();
  }
}

// ---- radius ----------------------------------------------------------------------------------------------------------
// counts[q] = the row's length (cut at max_nn when max_nn > 0); longs[q] = the qualifying neighbours of a row longer than 64
// entries (the scratch its filling needs), else 0.  counts and longs are zero before (what a non-finite query keeps).
__global__ __launch_bounds__(SR_BLOCK) void search_radius_count_kernel(const float4* __restrict__ queries, int n_q, const float4* __restrict__ cloud,
                                                                       int n, const float4* __restrict__ sorted,
                                                                       const int* __restrict__ cell_start, GridDesc g, int R, float r2, int max_nn,
                                                                       int* __restrict__ counts, int* __restrict__ longs) {
  const unsigned int lane = threadIdx.x & 63u;
  const int q = blockIdx.x * SR_WAVES + (int)(threadIdx.x >> 6);
  if (q >= n_q) return;  // (wave-uniform)
  const float4 p = queries[q];
  if (!finite3(p.x, p.y, p.z)) return;
  int c = 0;
  ball_batches(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) { c += __popcll(__ballot(key_in_ball(key, r2))); });
  const int len = max_nn > 0 ? min(c, max_nn) : c;
  if (lane == 0 && c > 0) {
    counts[q] = len;
    if (len > 64) longs[q] = c;
  }
}

// totals[0], [1] (zero before) += the sums of counts and longs, in 64 bits: the scans behind them are int32 and a total they
// cannot carry must be seen.  One atomic per wave (a wave per query adding to one word serialises the whole count pass).
__global__ __launch_bounds__(SR_BLOCK) void search_totals_kernel(const int* __restrict__ counts, const int* __restrict__ longs, int n_q,
                                                                 u64* __restrict__ totals) {
  u64 a = 0, b = 0;
  for (int i = blockIdx.x * SR_BLOCK + threadIdx.x; i < n_q; i += gridDim.x * SR_BLOCK) {
    a += (u64)counts[i];
    b += (u64)longs[i];
  }
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    a += shfl_xor_key(a, j);
    b += shfl_xor_key(b, j);
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (a) atomicAdd(&totals[0], a);
    if (b) atomicAdd(&totals[1], b);
  }
}

// row q = idx / d2 [row_start[q], row_start[q + 1]), ascending by key; scratch_start: the exclusive scan of longs
__global__ __launch_bounds__(SR_BLOCK) void search_radius_fill_kernel(const float4* __restrict__ queries, int n_q, const float4* __restrict__ cloud,
                                                                      int n, const float4* __restrict__ sorted,
                                                                      const int* __restrict__ cell_start, GridDesc g, int R, float r2,
                                                                      const int* __restrict__ row_start, const int* __restrict__ scratch_start,
                                                                      u64* scratch, int32_t* __restrict__ idx, float* __restrict__ d2) {
  const unsigned int lane = threadIdx.x & 63u;
  const int q = blockIdx.x * SR_WAVES + (int)(threadIdx.x >> 6);
  if (q >= n_q) return;  // (wave-uniform)
  const int at = row_start[q], len = row_start[q + 1] - at;
  if (len <= 0) return;
  const float4 p = queries[q];
  if (len <= 64) {
    u64 keep = kEmptyKey;
    ball_batches(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) { key_offer(key_in_ball(key, r2) ? key : kEmptyKey, keep, len, lane); });
    if ((int)lane < len) {
      idx[at + (int)lane] = (int32_t)(unsigned int)keep;
      d2[at + (int)lane] = __uint_as_float((unsigned int)(keep >> 32));
    }
    return;
  }
  u64* mine = scratch + scratch_start[q];
  const int have = scratch_start[q + 1] - scratch_start[q];
  int filled = 0;
  ball_batches(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) {
    const bool in = key_in_ball(key, r2);
    const unsigned long long mask = __ballot(in);
    const int slot = filled + __popcll(mask & ((1ull << lane) - 1ull));
    if (in && slot < have) mine[slot] = key;  // (slot < have always: the count pass walked the same candidates)
    filled += __popcll(mask);
  });
  __threadfence();  // the wave reads what its other lanes wrote
  const int m = min(filled, have);
  for (int e = (int)lane; e < m; e += 64) {
    const u64 key = mine[e];
    int rank = 0;
    for (int j = 0; j < m; ++j) rank += mine[j] < key ? 1 : 0;
    if (rank < len) {
      idx[at + rank] = (int32_t)(unsigned int)key;
      d2[at + rank] = __uint_as_float((unsigned int)(key >> 32));
    }
  }
}

__global__ __launch_bounds__(SR_BLOCK) void search_rows64_kernel(const int* __restrict__ row_start, int n, long long* __restrict__ out) {
  const int i = blockIdx.x * SR_BLOCK + threadIdx.x;
  if (i < n) out[i] = (long long)row_start[i];
}

}  // namespace

hipError_t launch_search_knn(const float4* queries, int n_q, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                             const GridDesc& g, int k, int32_t* idx, float* d2, int32_t* n_found, int* far, hipStream_t stream) {
  if (n_q <= 0) return hipSuccess;
  if (k < 1 || k > 64) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(far, 0, 2 * sizeof(int), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(search_knn_kernel, dim3((n_q + SR_WAVES - 1) / SR_WAVES), dim3(SR_BLOCK), 0, stream, queries, n_q, sorted, cell_start, g, k, idx,
                     d2, n_found, far);
  // (always launched: how many queries are listed is known on the device only; with an empty list every workgroup reads the count and ends)
  hipLaunchKernelGGL(search_far_kernel, dim3(min(n_q, 4096)), dim3(SR_BLOCK), 0, stream, queries, cloud, n, far, far + 2, k, idx, d2, n_found);
  return hipGetLastError();
}

hipError_t launch_search_radius_count(const float4* queries, int n_q, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                                      const GridDesc& g, int shells, float r2, int max_nn, int* counts, int* longs, int* row_start,
                                      int* scratch_start, int* scan_scratch, unsigned long long* totals, long long* row_start64,
                                      hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(counts, 0, ((size_t)n_q + 1) * sizeof(int), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(longs, 0, ((size_t)n_q + 1) * sizeof(int), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(totals, 0, 2 * sizeof(unsigned long long), stream)) != hipSuccess) return e;
  if (n_q > 0 && n > 0 && r2 > 0.f)  // (r2 == 0: no d2 is below it)
    hipLaunchKernelGGL(search_radius_count_kernel, dim3((n_q + SR_WAVES - 1) / SR_WAVES), dim3(SR_BLOCK), 0, stream, queries, n_q, cloud, n, sorted,
                       cell_start, g, shells, r2, max_nn, counts, longs);
  if (n_q > 0) hipLaunchKernelGGL(search_totals_kernel, dim3(min((n_q + SR_BLOCK - 1) / SR_BLOCK, 256)), dim3(SR_BLOCK), 0, stream, counts, longs, n_q, totals);
  if ((e = launch_exclusive_scan(counts, row_start, n_q + 1, scan_scratch, stream)) != hipSuccess) return e;
  if ((e = launch_exclusive_scan(longs, scratch_start, n_q + 1, scan_scratch, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(search_rows64_kernel, dim3((n_q + 1 + SR_BLOCK - 1) / SR_BLOCK), dim3(SR_BLOCK), 0, stream, row_start, n_q + 1, row_start64);
  return hipGetLastError();
}

hipError_t launch_search_radius_fill(const float4* queries, int n_q, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                                     const GridDesc& g, int shells, float r2, const int* row_start, const int* scratch_start,
                                     unsigned long long* scratch, int32_t* idx, float* d2, hipStream_t stream) {
  if (n_q <= 0) return hipSuccess;
  hipLaunchKernelGGL(search_radius_fill_kernel, dim3((n_q + SR_WAVES - 1) / SR_WAVES), dim3(SR_BLOCK), 0, stream, queries, n_q, cloud, n, sorted,
                     cell_start, g, shells, r2, row_start, scratch_start, scratch, idx, d2);
  return hipGetLastError();
}

}  // namespace icpgpu
