// icp_search_device.h -- device helpers of the neighbour search that more than one unit walks a ball with (internal): the keys and
// the walk of icp_search.hip's radius search, shared with icp_cluster.hip and icp_iss.hip, and the keyed selection of its k-nearest search, shared
// with icp_feature.hip.  (The lane moves and finite3 underneath: icp_wave.h; cell_of: icp_grid_device.h.)
#pragma once

#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

typedef unsigned long long u64;

constexpr int kSearchOutside = 64;  // cells a query may lie outside the grid and still be walked from its clamped cell

__device__ __forceinline__ u64 make_key(float d, unsigned int index) { return ((u64)__float_as_uint(d) << 32) | index; }

// a key moves between lanes in two halves (icp_wave.h)
__device__ __forceinline__ u64 shfl_xor_key(u64 v, int j) { return shfl_xor_u64(v, j); }
__device__ __forceinline__ u64 readlane_key(u64 v, int lane) { return readlane_u64(v, lane); }  // lane must be wave-uniform
__device__ __forceinline__ u64 key_min(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 key_max(u64 a, u64 b) { return a < b ? b : a; }

// ---- the keyed selection ---------------------------------------------------------------------------------------------
// keep: ascending over the lanes (kEmptyKey = nothing yet); cand: one candidate per lane (kEmptyKey = none).  K - 1 (wave-uniform)
// is the lane of the worst key that still counts.  Whole keys are compared everywhere.
__device__ __forceinline__ void key_offer(u64 cand, u64& keep, int K, unsigned int lane) {
  const u64 worst = readlane_key(keep, K - 1);
  if (__ballot(cand < worst) == 0ull) return;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const u64 o = shfl_xor_key(cand, j);
      const bool desc = (lane & (unsigned int)k) == 0u, lower = (lane & (unsigned int)j) == 0u;
      cand = (lower == desc) ? key_max(cand, o) : key_min(cand, o);
    }
  }
  keep = key_min(keep, cand);  // ascending against descending: the 64 smallest of both, a bitonic sequence
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const u64 o = shfl_xor_key(keep, j);
    keep = (lane & (unsigned int)j) == 0u ? key_min(keep, o) : key_max(keep, o);
  }
}

// the first k lanes of a kept list as row `q` of idx / d2 (k entries, row-major) and n_found[q]
__device__ __forceinline__ void write_knn_row(u64 keep, int k, size_t q, unsigned int lane, int32_t* __restrict__ idx, float* __restrict__ d2,
                                              int32_t* __restrict__ n_found) {
  const bool mine = (int)lane < k, found = mine && keep != kEmptyKey;
  if (mine) {
    idx[q * (size_t)k + lane] = found ? (int32_t)(unsigned int)keep : -1;
    d2[q * (size_t)k + lane] = found ? __uint_as_float((unsigned int)(keep >> 32)) : __builtin_inff();
  }
  const int m = __popcll(__ballot(found));
  if (n_found && lane == 0) n_found[q] = m;
}

// ---- where candidates come from --------------------------------------------------------------------------------------
// f(key) is called by the whole wave once per batch of 64 candidates: the candidate's key in its lane, kEmptyKey in a lane that
// has none.  Every finite cloud point of the region is offered exactly once.

// one row segment of `sorted` ([lo, lo + len)); sorted[].w carries the point's index in the cloud
template <class F>
__device__ __forceinline__ void segment_batches(const float4* __restrict__ sorted, int lo, int len, const float4& p, unsigned int lane, F&& f) {
  for (int k = 0; k < len; k += 64) {
    const int j = k + (int)lane;
    u64 key = kEmptyKey;
    if (j < len) {
      const float4 q = sorted[lo + j];
      key = make_key(dist2(q.x, q.y, q.z, p.x, p.y, p.z), __float_as_uint(q.w));
    }
    f(key);
  }
}

// the cube of R cells around cell (ux, uy, uz) -- which may lie outside the grid -- clipped to the grid: one lane per cell row
template <class F>
__device__ __forceinline__ void cube_batches(const float4* __restrict__ sorted, const int* __restrict__ cell_start, const GridDesc& g, int ux,
                                             int uy, int uz, int R, const float4& p, unsigned int lane, F&& f) {
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
      segment_batches(sorted, __builtin_amdgcn_readlane(lo, ra), __builtin_amdgcn_readlane(len, ra), p, lane, f);
    }
  }
}

// cloud[first], cloud[first + step], ...: 64 points per batch starting at first + lane (finite points only)
template <class F>
__device__ __forceinline__ void sweep_batches(const float4* __restrict__ cloud, int n, int first, int step, const float4& p, F&& f) {
  for (int base = 0; base < n; base += step) {
    const int j = base + first;
    u64 key = kEmptyKey;
    if (j < n) {
      const float4 q = cloud[j];
      if (finite3(q.x, q.y, q.z)) key = make_key(dist2(q.x, q.y, q.z, p.x, p.y, p.z), (unsigned int)j);
    }
    f(key);
  }
}

// the query's own cell (ux, uy, uz: may lie outside the grid) and whether the grid is walked for it at all
__device__ __forceinline__ bool query_cell(const float4* sorted, const GridDesc& g, const float4& p, int& ux, int& uy, int& uz) {
  if (!sorted) {
    ux = uy = uz = 0;
    return false;
  }
  cell_of(g, p.x, p.y, p.z, ux, uy, uz);
  return ux >= -kSearchOutside && ux <= g.nx - 1 + kSearchOutside && uy >= -kSearchOutside && uy <= g.ny - 1 + kSearchOutside &&
         uz >= -kSearchOutside && uz <= g.nz - 1 + kSearchOutside;
}

// ---- radius ----------------------------------------------------------------------------------------------------------
// every finite cloud point that can have d2 < r2 for query p, once: the cube of R cells, or the whole cloud (R < 0, no grid, or a
// query too far outside)
template <class F>
__device__ __forceinline__ void ball_batches(const float4* __restrict__ cloud, int n, const float4* __restrict__ sorted,
                                             const int* __restrict__ cell_start, const GridDesc& g, int R, const float4& p, unsigned int lane, F&& f) {
  int ux, uy, uz;
  if (R >= 0 && query_cell(sorted, g, p, ux, uy, uz)) cube_batches(sorted, cell_start, g, ux, uy, uz, R, p, lane, f);
  else sweep_batches(cloud, n, (int)lane, 64, p, f);
}

__device__ __forceinline__ bool key_in_ball(u64 key, float r2) { return key != kEmptyKey && __uint_as_float((unsigned int)(key >> 32)) < r2; }

}  // namespace
}  // namespace icpgpu
