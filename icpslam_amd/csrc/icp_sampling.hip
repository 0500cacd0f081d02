// icp_sampling.hip -- the cropping and sampling filters' kernels (pcl::PassThrough, pcl::CropBox, pcl::UniformSampling,
// pcl::FarthestPointSampling; rules: include/icpgpu.h "cropping and sampling filters"; arithmetic: icp_sampling.h; host side:
// icpgpu_sampling.cpp).  All four end in flags or a list of kept rows; the crops and the uniform sampling go through launch_compact
// (icp_scan.hip) into the pinned staging buffer, the farthest point sampling gathers its rows in selection order.
//   * crop_flags_kernel: one lane per row, flags[i] = the rule's verdict.  No grid cap: ceil(n / 256) workgroups.
//   * uniform sampling: an open-addressing table of 2 n .. 4 n slots (a power of two) over the plan's cell indices.  us_insert_kernel
//     claims a row's cell with one 32-bit compare-and-swap per probe and offers the row's (d2 bits, index) key with ONE 64-bit
//     atomicMin; us_flags_kernel keeps the row whose index its cell's slot ended with.  Which slot a cell lands in depends on the
//     arrival order, the slot's final key does not: the minimum of a set.  A probe sequence ends at the first slot that is empty or
//     the cell's own -- it never waits for another lane.  No grid cap.
//   * farthest point sampling, ONE workgroup (n <= kFpsOneMax): fps_one_kernel, all samples in one launch.  Lane t owns rows t,
//     t + 1024, ...: 16 rows' coordinates and m stay in 64 VGPRs.  Per sample a lane updates its rows against the last winner and keeps
//     its best; the wave folds the (m bits, ~index) keys with shfl_xor_u64 (icp_wave.h); the lane that holds the wave's key puts it
//     and its row's coordinates into the wave's LDS slot; after ONE barrier every lane reads the 16 slots (broadcast reads) and knows the
//     winner and its coordinates.  The slots are double-buffered, so a sample costs one barrier.
//   * farthest point sampling, MANY workgroups: fps_many_kernel, one launch per sample over a fixed grid (at most kFpsManyBlocksMax
//     workgroups, 1024 rows per workgroup and trip).  m lives in HBM.  Every workgroup first folds the previous launch's per-workgroup
//     keys -- a maximum of 64-bit integers, the same whatever the order -- learns the last winner from it, updates its rows and writes
//     its own key into the OTHER slot array.  Launch boundaries are the only synchronisation across workgroups: no float atomics,
//     no device-wide barrier, no spin-wait in either shape.
#include <hip/hip_runtime.h>

#include "icp_kernels.h"
#include "icp_sampling.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int FPS_ONE_BLOCK = 1024, FPS_ONE_WAVES = FPS_ONE_BLOCK / 64, FPS_ONE_ROWS = 16;
static_assert(FPS_ONE_BLOCK * FPS_ONE_ROWS == kFpsOneMax, "icp_kernels.h states the rows of the one-workgroup shape");
constexpr int FPS_MANY_BLOCK = 256, FPS_MANY_WAVES = FPS_MANY_BLOCK / 64, FPS_MANY_PER = 4, FPS_MANY_TILE = FPS_MANY_BLOCK * FPS_MANY_PER;

__global__ __launch_bounds__(256) void crop_flags_kernel(const float4* __restrict__ cloud, int n, CropRule rule, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = cloud[i];
  int keep;
  if (rule.box) {
    float q[3] = {p.x, p.y, p.z};
    if (rule.has_T) sampling_xform(rule.T.m, p.x, p.y, p.z, q);
    keep = crop_box_keep(p.x, p.y, p.z, q, rule.lo, rule.hi, rule.negative);
  } else {
    keep = pass_through_keep(p.x, p.y, p.z, rule.field, rule.lo[0], rule.hi[0], rule.negative);
  }
  flags[i] = keep;
}

// ---- uniform sampling ------------------------------------------------------------------------------------------------------------
constexpr unsigned int US_NO_SLOT = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void us_clear_kernel(int* __restrict__ cells, unsigned long long* __restrict__ best, unsigned int cap) {
  const unsigned int s = blockIdx.x * 256u + threadIdx.x;
  if (s >= cap) return;
  cells[s] = -1;
  best[s] = kEmptyKey;
}

__global__ __launch_bounds__(256) void us_insert_kernel(const float4* __restrict__ cloud, int n, UniformLattice L, unsigned int mask,
                                                        int* __restrict__ cells, unsigned long long* __restrict__ best,
                                                        unsigned int* __restrict__ slot_of, float* __restrict__ d2_of) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = cloud[i];
  if (!sampling_finite3(p.x, p.y, p.z)) {
    slot_of[i] = US_NO_SLOT;
    d2_of[i] = 0.f;
    return;
  }
  int cell[3];
  const float d2 = uniform_cell(p.x, p.y, p.z, L.inv, L.leaf, cell);
  const int id = uniform_cell_index(cell, L.minb, L.divb);
  unsigned int h = (unsigned int)id * 0x9E3779B1u;
  h = (h ^ (h >> 15)) & mask;
  // at most 2 n of the >= 2 n slots are ever claimed by n rows' cells: an empty slot ends every probe sequence
  for (;;) {
    const int seen = atomicCAS(&cells[h], -1, id);
    if (seen == -1 || seen == id) break;
    h = (h + 1u) & mask;
  }
  atomicMin(&best[h], uniform_key(d2, i));
  slot_of[i] = h;
  d2_of[i] = d2;
}

__global__ __launch_bounds__(256) void us_flags_kernel(int n, const unsigned long long* __restrict__ best, const unsigned int* __restrict__ slot_of,
                                                       int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned int s = slot_of[i];
  flags[i] = (s != US_NO_SLOT && (unsigned int)best[s] == (unsigned int)i) ? 1 : 0;
}

// ---- what the four share behind the kept list ---------------------------------------------------------------------------------------
// j < count (d_count: read from device memory, else `count`): points[j] = cloud[kept[j]], measure_out[j] = measure_in[kept[j]] where
// given; *n_out = count where given
__global__ __launch_bounds__(256) void subset_gather_kernel(const int* __restrict__ kept, const int* __restrict__ d_count, int count,
                                                            const float4* __restrict__ cloud, float4* __restrict__ points,
                                                            const float* __restrict__ measure_in, float* __restrict__ measure_out,
                                                            int* __restrict__ n_out) {
  const int m = d_count ? *d_count : count;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0 && n_out) *n_out = m;
  if (j >= m) return;
  const int i = kept[j];
  if (points) points[j] = cloud[i];
  if (measure_out) measure_out[j] = measure_in[i];
}

__global__ __launch_bounds__(256) void subset_fill_kernel(int* __restrict__ flags, int n, int value) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = value;
}

__global__ __launch_bounds__(256) void subset_unflag_kernel(const int* __restrict__ kept, int count, int* __restrict__ flags) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < count) flags[kept[j]] = 0;
}

// ---- farthest point sampling ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long u64_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = u64_max(v, shfl_xor_u64(v, off));
  return v;  // (in every lane)
}

// m of a row: +inf / the squared distance to the selected set for a finite unselected row, -1 for a selected or non-finite one
__global__ __launch_bounds__(FPS_ONE_BLOCK) void fps_one_kernel(const float4* __restrict__ cloud, int n, int n_samples, int first,
                                                                 int* __restrict__ kept, float* __restrict__ measure) {
  __shared__ unsigned long long s_key[2][FPS_ONE_WAVES];
  __shared__ float4 s_xyz[2][FPS_ONE_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float x[FPS_ONE_ROWS], y[FPS_ONE_ROWS], z[FPS_ONE_ROWS], m[FPS_ONE_ROWS];
#pragma unroll
  for (int k = 0; k < FPS_ONE_ROWS; ++k) {
    const int i = tid + FPS_ONE_BLOCK * k;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool live = false;
    if (i < n) {
      p = cloud[i];
      live = sampling_finite3(p.x, p.y, p.z);
    }
    x[k] = p.x, y[k] = p.y, z[k] = p.z;
    m[k] = live ? __builtin_inff() : -1.f;
  }
  int w = first;  // (0 <= first < n, a finite row: the host has checked)
  const float4 pw = cloud[w];
  float wx = pw.x, wy = pw.y, wz = pw.z;
  if (tid == 0) {
    kept[0] = w;
    measure[0] = __builtin_inff();
  }
  for (int j = 1; j < n_samples; ++j) {
    const int wk = w >> 10;
    const bool mine = (w & (FPS_ONE_BLOCK - 1)) == tid;
    float bm = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    int bk = 0;
#pragma unroll
    for (int k = 0; k < FPS_ONE_ROWS; ++k) {
      float mk = m[k];
      if (mine && k == wk) {
        mk = -1.f;
      } else if (mk >= 0.f) {
        const float d = fps_d2(x[k], y[k], z[k], wx, wy, wz);
        mk = d < mk ? d : mk;
      }
      m[k] = mk;
      if (mk > bm) bm = mk, bk = k, bx = x[k], by = y[k], bz = z[k];  // (strict: the lane's lowest row of a tie)
    }
    const unsigned long long key = bm >= 0.f ? fps_key(bm, tid + FPS_ONE_BLOCK * bk) : 0ull;
    const unsigned long long wkey = wave_max_u64(key);
    const int b = j & 1;
    if (wkey == 0ull) {
      if (lane == 0) s_key[b][wave] = 0ull;
    } else if (key == wkey) {  // (one lane: the key holds the row's index)
      s_key[b][wave] = wkey;
      s_xyz[b][wave] = make_float4(bx, by, bz, 0.f);
    }
    __syncthreads();
    unsigned long long best = 0ull;
    int bw = 0;
#pragma unroll
    for (int v = 0; v < FPS_ONE_WAVES; ++v) {
      const unsigned long long kv = s_key[b][v];
      if (kv > best) best = kv, bw = v;
    }
    if (best == 0ull) break;  // (uniform; not reached: the host refuses n_samples above the finite rows)
    const float4 c = s_xyz[b][bw];
    w = fps_key_index(best);
    wx = c.x, wy = c.y, wz = c.z;
    if (tid == 0) {
      kept[j] = w;
      measure[j] = fps_key_measure(best);
    }
  }
}

__global__ __launch_bounds__(256) void fps_init_kernel(const float4* __restrict__ cloud, int n, float* __restrict__ m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = cloud[i];
  m[i] = sampling_finite3(p.x, p.y, p.z) ? __builtin_inff() : -1.f;
}

// launch j = 1 .. n_samples: learns s_(j-1) (j == 1: `first`; else the maximum of prev_slots[0 .. n_slots)), workgroup 0 records it;
// j < n_samples: m is updated against it and the workgroup's best key for s_j goes to next_slots[blockIdx.x]
__global__ __launch_bounds__(FPS_MANY_BLOCK) void fps_many_kernel(const float4* __restrict__ cloud, int n, float* __restrict__ m, int j, int n_samples,
                                                                   int first, const unsigned long long* __restrict__ prev_slots,
                                                                   unsigned long long* __restrict__ next_slots, int n_slots, int* __restrict__ kept,
                                                                   float* __restrict__ measure) {
  __shared__ unsigned long long s_in[FPS_MANY_WAVES], s_out[FPS_MANY_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int w = first;
  float meas = __builtin_inff();
  if (j > 1) {
    unsigned long long k = 0ull;
    for (int s = tid; s < n_slots; s += FPS_MANY_BLOCK) k = u64_max(k, prev_slots[s]);
    k = wave_max_u64(k);
    if (lane == 0) s_in[wave] = k;
    __syncthreads();
    unsigned long long best = 0ull;
#pragma unroll
    for (int v = 0; v < FPS_MANY_WAVES; ++v) best = u64_max(best, s_in[v]);
    if (best == 0ull) return;  // (uniform over the grid; not reached: the host refuses n_samples above the finite rows)
    w = fps_key_index(best);
    meas = fps_key_measure(best);
  }
  if (blockIdx.x == 0 && tid == 0) {
    kept[j - 1] = w;
    measure[j - 1] = meas;
  }
  if (j >= n_samples) return;
  const float4 pw = cloud[w];
  unsigned long long mine = 0ull;
  for (long long base = (long long)blockIdx.x * FPS_MANY_TILE; base < n; base += (long long)gridDim.x * FPS_MANY_TILE) {
#pragma unroll
    for (int r = 0; r < FPS_MANY_PER; ++r) {
      const long long i = base + r * FPS_MANY_BLOCK + tid;
      if (i >= n) continue;
      float mk = m[i];
      if (i == w) {
        m[i] = mk = -1.f;
      } else if (mk >= 0.f) {
        const float4 p = cloud[i];
        const float d = fps_d2(p.x, p.y, p.z, pw.x, pw.y, pw.z);
        if (d < mk) m[i] = mk = d;
      }
      if (mk >= 0.f) mine = u64_max(mine, fps_key(mk, (int)i));
    }
  }
  mine = wave_max_u64(mine);
  if (lane == 0) s_out[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    unsigned long long best = 0ull;
#pragma unroll
    for (int v = 0; v < FPS_MANY_WAVES; ++v) best = u64_max(best, s_out[v]);
    next_slots[blockIdx.x] = best;
  }
}

}  // namespace

hipError_t launch_crop_flags(const float4* cloud, int n, const CropRule& rule, int* flags, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crop_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud, n, rule, flags);
  return hipGetLastError();
}

unsigned int uniform_table_slots(int n) {
  unsigned int cap = 64u;
  while (cap < 2u * (unsigned int)(n > 0 ? n : 1)) cap <<= 1;  // (n <= kUniformMaxRows = 2^30: cap <= 2^31)
  return cap;
}

hipError_t launch_uniform_flags(const float4* cloud, int n, const UniformLattice& L, int* cells, unsigned long long* best, unsigned int* slot_of,
                                float* d2_of, int* flags, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const unsigned int cap = uniform_table_slots(n);
  hipLaunchKernelGGL(us_clear_kernel, dim3((cap + 255u) / 256u), dim3(256), 0, stream, cells, best, cap);
  hipLaunchKernelGGL(us_insert_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud, n, L, cap - 1u, cells, best, slot_of, d2_of);
  hipLaunchKernelGGL(us_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, (const unsigned long long*)best, (const unsigned int*)slot_of, flags);
  return hipGetLastError();
}

hipError_t launch_subset_gather(const int* kept, const int* d_count, int count_most, const float4* cloud, float4* points, const float* measure_in,
                                float* measure_out, int* n_out, hipStream_t stream) {
  const int blocks = count_most > 0 ? (count_most + 255) / 256 : 1;
  hipLaunchKernelGGL(subset_gather_kernel, dim3(blocks), dim3(256), 0, stream, kept, d_count, count_most, cloud, points, measure_in, measure_out, n_out);
  return hipGetLastError();
}

hipError_t launch_subset_removed_flags(const int* kept, int n_kept, int n, int* flags, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(subset_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, flags, n, 1);
  if (n_kept > 0) hipLaunchKernelGGL(subset_unflag_kernel, dim3((n_kept + 255) / 256), dim3(256), 0, stream, kept, n_kept, flags);
  return hipGetLastError();
}

int fps_many_blocks(int n) {
  const long long tiles = ((long long)(n > 0 ? n : 1) + FPS_MANY_TILE - 1) / FPS_MANY_TILE;
  return (int)(tiles < kFpsManyBlocksMax ? tiles : kFpsManyBlocksMax);
}

hipError_t launch_fps_one(const float4* cloud, int n, int n_samples, int first, int* kept, float* measure, hipStream_t stream) {
  if (n <= 0 || n > kFpsOneMax || n_samples <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fps_one_kernel, dim3(1), dim3(FPS_ONE_BLOCK), 0, stream, cloud, n, n_samples, first, kept, measure);
  return hipGetLastError();
}

hipError_t launch_fps_many(const float4* cloud, int n, int n_samples, int first, float* m, unsigned long long* slots, int* kept, float* measure,
                           int* launches, hipStream_t stream) {
  if (n <= 0 || n_samples <= 0) return hipErrorInvalidValue;
  const int blocks = fps_many_blocks(n);
  hipLaunchKernelGGL(fps_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud, n, m);
  for (int j = 1; j <= n_samples; ++j) {
    const unsigned long long* prev = slots + (size_t)((j - 1) & 1) * kFpsManyBlocksMax;
    unsigned long long* next = slots + (size_t)(j & 1) * kFpsManyBlocksMax;
    // (the last launch only records s_(n_samples - 1): one workgroup)
    hipLaunchKernelGGL(fps_many_kernel, dim3(j < n_samples ? blocks : 1), dim3(FPS_MANY_BLOCK), 0, stream, cloud, n, m, j, n_samples, first, prev, next,
                       blocks, kept, measure);
  }
  if (launches) *launches = 1 + n_samples;
  return hipGetLastError();
}

}  // namespace icpgpu
