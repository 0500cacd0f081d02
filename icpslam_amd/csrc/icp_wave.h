// icp_wave.h -- wave and workgroup primitives that more than one kernel unit uses (internal): the inclusive scan over a wave's
// lanes and the workgroup scan built on it, 64-bit lane moves, the workgroup's count into one atomic, finite3.  Reductions with
// another shuffle pattern (wave_sum in icp_device.h, the all-lane folds of icp_mls.hip and icp_morph.hip) are other operations and
// live with their users.  Anonymous namespace: a helper's LDS words keep the names they had inside the units, and with them
// every kernel its LDS layout.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace icpgpu {
namespace {

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ---- scans ------------------------------------------------------------------------------------------------------------
// `incl` (an int variable) becomes its inclusive prefix sum over the wave's 64 lanes (lane = threadIdx.x & 63); lane 63 ends with
// the wave's sum.  A macro, so that the ladder is compiled as part of the kernel that uses it: an inline function is simplified on
// its own before it is inlined, and eight kernels (the covariance kernels' row batches, the radix scatter, the voxel filter's
// scans, the two one-workgroup scans) then came out with other register assignments and schedules than the loops they had
// written out (scripts/kernel_isa.py).
#define ICPGPU_WAVE_INCLUSIVE_SCAN(incl, lane)                           \
  _Pragma("unroll") for (int off_ = 1; off_ < 64; off_ <<= 1) {          \
    const int t_ = __shfl_up(incl, off_, 64);                            \
    if ((lane) >= off_) incl += t_;                                      \
  }
// (the function form, for the caller that had the ladder as a function of its own: icp_tile.hip)
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
  ICPGPU_WAVE_INCLUSIVE_SCAN(v, lane);
  return v;
}

// exclusive prefix of v over the 64 x WAVES threads of the workgroup (one value each); *total = the workgroup's sum, in every
// thread.  wsum: WAVES ints of LDS.  (The 16-wave form tests total for null, as the voxel filter's kernels were compiled with that
// test; no caller passes null.)
template <int WAVES>
__device__ __forceinline__ int wg_exclusive_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
  ICPGPU_WAVE_INCLUSIVE_SCAN(incl, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int s = wsum[w];
    base += w < wave ? s : 0;
    all += s;
  }
  __syncthreads();  // wsum may be reused
  if (WAVES == 4 || total) *total = all;
  return base + incl - v;
}

// the sum of the workgroup's lane counts into *counter (one device atomic per workgroup); every thread of the workgroup calls it
__device__ __forceinline__ void block_count_add(unsigned int lane_count, unsigned int* counter) {
  __shared__ unsigned int total;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  unsigned int v = lane_count;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(&total, v);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(counter, total);
}

// ---- 64-bit lane moves: a value moves in two 32-bit halves --------------------------------------------------------------
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int lane) {  // lane: wave-uniform
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, lane);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  return __longlong_as_double((long long)readlane_u64((unsigned long long)__double_as_longlong(v), lane));
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int j) {
  const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)v, j, 64), hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), j, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_xor_f64(double v, int j) {
  return __longlong_as_double((long long)shfl_xor_u64((unsigned long long)__double_as_longlong(v), j));
}

}  // namespace
}  // namespace icpgpu
