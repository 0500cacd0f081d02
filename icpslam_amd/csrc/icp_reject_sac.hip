// icp_reject_sac.hip -- device side of pcl::registration::CorrespondenceRejectorSampleConsensus (PCL 1.8: RANSAC with
// SampleConsensusModelRegistration over a list of pairs; rules: include/icpgpu.h "sample-consensus rejector"; host loop:
// icpgpu_reject_sac.cpp).  The stage works on m pairs (P_r, Q_r) gathered into arrays of its own.
//
// A hypothesis is a pure function of (seed, t, the pairs), so 64 of them are taken at once and the host replays the sequential
// loop over their counts, as the plane segmentation does (icp_sac.hip).
//   * gather: the chain's keys become flags of the alive pairs, launch_compact turns them into the ascending source ranks, and
//     rsac_gather_keys_kernel writes P_r = T * source[i] (xform_point, as the search rounds it) and Q_r = target[j]; the call of
//     its own gathers through its two index lists (rsac_gather_index_kernel).
//   * rsac_moments_kernel: the nine sums of the sample-distance rule over the finite P_r about K = the first finite P, ONE
//     workgroup in a fixed order, every term exact in float64 and accumulated in double-double (sac_sums_kernel's scheme).
//   * rsac_model_kernel: one thread per hypothesis of the batch -- up to 16 redraws of three ranks, the spacing test, and for the
//     first good draw the 17 sums of its three pairs in sample order, which the HOST solves (solve_umeyama).
//   * rsac_count_kernel, the hot path: sac_count_kernel's shape.  Hypothesis h of the batch belongs to lane h of every wave.  A
//     wave takes RS_WAVE_PAIRS pairs per step, RS_PPL in every lane's registers (P and Q: twelve floats), and walks the 64 float
//     transforms, twelve floats each, which it reads wave-uniformly (scalar loads): per transform and pair register one ballot
//     of the inlier test, and lane h adds the popcount to its own register.  The grid is capped (kSacGridCap) and every workgroup
//     strides over the pairs.  At the end the four waves add their registers in LDS (integers) and 64 lanes do one integer
//     atomicAdd each into count[h]: integer sums do not depend on their order, so the counts are exact.
//     Register pressure: 12 floats of pairs + 12 uniform floats of the transform + a handful of temporaries per lane -- two pairs
//     per lane keep the transform's scalar loads amortised over two tests without approaching any occupancy step.
//   * rsac_flag_kernel: the inlier test of the best transform per pair -> flags, the kept count, and (in the chain) kEmptyKey
//     into the key of every rejected pair; with keep_all every pair stays.
// No sum depends on the arrival order of atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int RS_BLOCK = 256, RS_WAVES = RS_BLOCK / 64;
constexpr int RS_PPL = 2;  // pairs per lane and step
constexpr int RS_WAVE_PAIRS = 64 * RS_PPL;
constexpr int RS_REDUCE = 1024;  // the one workgroup of the moments kernel
constexpr int RS_MAX_BLOCKS = 1024;
static_assert(RS_WAVES * RS_WAVE_PAIRS == kSacBlockPoints, "the counting grid is sized in icp_kernels.h's workgroup steps");

// splitmix64 of the rule's counter: hypothesis t, redraw d, rank c
__device__ __forceinline__ unsigned long long rsac_mix(unsigned long long seed, unsigned long long t, unsigned int d, unsigned int c) {
  unsigned long long z = seed + (48ull * t + 3ull * (unsigned long long)d + (unsigned long long)c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ bool key_alive(unsigned long long key, float thr) {
  return (unsigned int)key != 0xFFFFFFFFu && __uint_as_float((unsigned int)(key >> 32)) <= thr;
}

// the rule's inlier test: p' = T p by the fma chain, d2(p', q) < thr with thr the smallest float32 not below the double
// threshold squared.  A NaN anywhere fails.
__device__ __forceinline__ bool rsac_inlier(const Xform& T, float px, float py, float pz, float qx, float qy, float qz, float thr) {
  float x, y, z;
  xform_point(T, px, py, pz, x, y, z);
  return dist2(x, y, z, qx, qy, qz) < thr;
}

__device__ __forceinline__ int pairs_of(int m_host, const int* __restrict__ m_dev) { return m_dev ? *m_dev : m_host; }

__global__ __launch_bounds__(RS_BLOCK) void rsac_alive_kernel(const unsigned long long* __restrict__ keys, int n, float thr, int n_t,
                                                              int* __restrict__ flags) {
  const int i = blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  flags[i] = key_alive(key, thr) && (unsigned int)key < (unsigned int)n_t ? 1 : 0;
}

__global__ __launch_bounds__(RS_BLOCK) void rsac_gather_keys_kernel(const float4* __restrict__ src, const float4* __restrict__ tgt,
                                                                    const unsigned long long* __restrict__ keys, Xform T,
                                                                    const int* __restrict__ rank, const int* __restrict__ m_dev, int n_s,
                                                                    int n_t, float4* __restrict__ P, float4* __restrict__ Q) {
  const int m = min(*m_dev, n_s);
  for (int r = blockIdx.x * RS_BLOCK + threadIdx.x; r < m; r += gridDim.x * RS_BLOCK) {
    const int i = min(max(rank[r], 0), n_s - 1);  // (the ranks name source points)
    const unsigned int j = min((unsigned int)keys[i], (unsigned int)(n_t - 1));
    const float4 s = src[i];
    float x, y, z;
    xform_point(T, s.x, s.y, s.z, x, y, z);
    P[r] = make_float4(x, y, z, 1.f);
    Q[r] = tgt[j];
  }
}

// (the host has checked every index against its cloud)
__global__ __launch_bounds__(RS_BLOCK) void rsac_gather_index_kernel(const float4* __restrict__ source, int n_s, const float4* __restrict__ target,
                                                                     int n_t, const int32_t* __restrict__ iq, const int32_t* __restrict__ im,
                                                                     int m, float4* __restrict__ P, float4* __restrict__ Q,
                                                                     int* __restrict__ rank) {
  for (int r = blockIdx.x * RS_BLOCK + threadIdx.x; r < m; r += gridDim.x * RS_BLOCK) {
    P[r] = source[min(max(iq[r], 0), n_s - 1)];
    Q[r] = target[min(max(im[r], 0), n_t - 1)];
    rank[r] = r;
  }
}

// out[0 .. 9): the sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz over the finite P_r, d = P_r - K in float32 with
// K = the first finite P; out[9 .. 12): K; out[12] = the number of finite P_r; out[13] = m.  Thread t takes pairs t, t + 1024, ...;
// then a binary tree per sum.  Without a finite P everything but out[13] is zero.
__global__ __launch_bounds__(RS_REDUCE) void rsac_moments_kernel(const float4* __restrict__ P, int m_host, const int* __restrict__ m_dev,
                                                                 int m_cap, double* __restrict__ out) {
  __shared__ DD sh[RS_REDUCE];
  __shared__ int first, n_finite;
  const int m = min(pairs_of(m_host, m_dev), m_cap);
  if (threadIdx.x == 0) first = m, n_finite = 0;
  __syncthreads();
  int mine = m, cnt = 0;
  for (int k = threadIdx.x; k < m; k += RS_REDUCE) {
    const float4 p = P[k];
    if (finite3(p.x, p.y, p.z)) {
      mine = min(mine, k);
      cnt += 1;
    }
  }
  if (cnt) {
    atomicMin(&first, mine);  // (integers: the result does not depend on the order)
    atomicAdd(&n_finite, cnt);
  }
  __syncthreads();
  const int f = first;
  float4 K = make_float4(0.f, 0.f, 0.f, 0.f);
  if (f < m) K = P[f];
  DD acc[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) acc[e].hi = acc[e].lo = 0.0;
  for (int k = threadIdx.x; k < m; k += RS_REDUCE) {
    const float4 p = P[k];
    if (!finite3(p.x, p.y, p.z)) continue;
    const double dx = (double)(p.x - K.x), dy = (double)(p.y - K.y), dz = (double)(p.z - K.z);
    dd_add_term(acc[0], dx * dx);  // (24 x 24 bits: exact)
    dd_add_term(acc[1], dx * dy);
    dd_add_term(acc[2], dx * dz);
    dd_add_term(acc[3], dy * dy);
    dd_add_term(acc[4], dy * dz);
    dd_add_term(acc[5], dz * dz);
    dd_add_term(acc[6], dx);
    dd_add_term(acc[7], dy);
    dd_add_term(acc[8], dz);
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    sh[threadIdx.x] = acc[e];
    __syncthreads();
    for (int step = RS_REDUCE / 2; step > 0; step >>= 1) {
      if ((int)threadIdx.x < step) sh[threadIdx.x] = dd_add(sh[threadIdx.x], sh[threadIdx.x + step]);
      __syncthreads();
    }
    if (threadIdx.x == 0) out[e] = sh[0].hi + sh[0].lo;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[9] = (double)K.x, out[10] = (double)K.y, out[11] = (double)K.z;
    out[12] = (double)n_finite;
    out[13] = (double)m;
  }
}

__global__ __launch_bounds__(kSacBatch) void rsac_model_kernel(const float4* __restrict__ P, const float4* __restrict__ Q, int m,
                                                               unsigned long long seed, int t0, int max_iterations, double sample_d2,
                                                               RsacModels* __restrict__ out) {
  const int h = (int)threadIdx.x;
  const int t = t0 + h;
  int s[3] = {-1, -1, -1};
  double acc[kReduceTerms];
#pragma unroll
  for (int a = 0; a < kReduceTerms; ++a) acc[a] = 0.0;
  bool good = false;
  if (t < max_iterations && m >= 3) {
#pragma unroll 1
    for (unsigned int d = 0; d < (unsigned int)kRsacDraws && !good; ++d) {
      int r[3];
#pragma unroll
      for (unsigned int c = 0; c < 3u; ++c)
        r[c] = (int)(((rsac_mix(seed, (unsigned long long)t, d, c) >> 32) * (unsigned long long)(unsigned int)m) >> 32);
      if (r[0] == r[1] || r[0] == r[2] || r[1] == r[2]) continue;
      const float4 p0 = P[r[0]], p1 = P[r[1]], p2 = P[r[2]];
      const float4 q0 = Q[r[0]], q1 = Q[r[1]], q2 = Q[r[2]];
      if (!(finite3(p0.x, p0.y, p0.z) && finite3(p1.x, p1.y, p1.z) && finite3(p2.x, p2.y, p2.z) && finite3(q0.x, q0.y, q0.z) &&
            finite3(q1.x, q1.y, q1.z) && finite3(q2.x, q2.y, q2.z)))
        continue;
      const float d01 = dist2(p1.x, p1.y, p1.z, p0.x, p0.y, p0.z), d02 = dist2(p2.x, p2.y, p2.z, p0.x, p0.y, p0.z),
                  d12 = dist2(p2.x, p2.y, p2.z, p1.x, p1.y, p1.z);
      if (!((double)d01 > sample_d2 && (double)d02 > sample_d2 && (double)d12 > sample_d2)) continue;  // (a NaN fails)
      good = true;
      s[0] = r[0], s[1] = r[1], s[2] = r[2];
      accumulate_pair(acc, p0.x, p0.y, p0.z, q0.x, q0.y, q0.z, 0.f);
      accumulate_pair(acc, p1.x, p1.y, p1.z, q1.x, q1.y, q1.z, 0.f);
      accumulate_pair(acc, p2.x, p2.y, p2.z, q2.x, q2.y, q2.z, 0.f);
    }
  }
#pragma unroll
  for (int a = 0; a < kReduceTerms; ++a) out->sums[h][a] = acc[a];
  out->ranks[h][0] = s[0], out->ranks[h][1] = s[1], out->ranks[h][2] = s[2];
  out->good[h] = good ? 1 : 0;
}

__global__ __launch_bounds__(RS_BLOCK) void rsac_count_kernel(const float4* __restrict__ P, const float4* __restrict__ Q, int m, float thr,
                                                              RsacBatch* __restrict__ batch) {
  __shared__ int sums[kSacBatch];
  const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < (unsigned int)kSacBatch) sums[threadIdx.x] = 0;
  __syncthreads();
  const Xform* __restrict__ xf = batch->T;
  const float nan = __builtin_nanf("");
  int acc = 0;
  const long long stride = (long long)gridDim.x * kSacBlockPoints;
  for (long long base = (long long)blockIdx.x * kSacBlockPoints + (long long)wave * RS_WAVE_PAIRS; base < (long long)m; base += stride) {  // (wave-uniform)
    float px[RS_PPL], py[RS_PPL], pz[RS_PPL], qx[RS_PPL], qy[RS_PPL], qz[RS_PPL];
#pragma unroll
    for (int u = 0; u < RS_PPL; ++u) {
      const long long r = base + u * 64 + (long long)lane;
      px[u] = nan, py[u] = pz[u] = qx[u] = qy[u] = qz[u] = 0.f;
      if (r < (long long)m) {
        const float4 p = P[r], q = Q[r];
        if (finite3(p.x, p.y, p.z) && finite3(q.x, q.y, q.z))  // (a pair with a non-finite point stays NaN: never an inlier)
          px[u] = p.x, py[u] = p.y, pz[u] = p.z, qx[u] = q.x, qy[u] = q.y, qz[u] = q.z;
      }
    }
#pragma unroll 2
    for (int h = 0; h < kSacBatch; ++h) {
      const Xform T = xf[h];  // (the same address in every lane)
      int c = 0;
#pragma unroll
      for (int u = 0; u < RS_PPL; ++u) c += __popcll(__ballot(rsac_inlier(T, px[u], py[u], pz[u], qx[u], qy[u], qz[u], thr)));
      acc += lane == (unsigned int)h ? c : 0;
    }
  }
  if (acc) atomicAdd(&sums[lane], acc);
  __syncthreads();
  if (threadIdx.x < (unsigned int)kSacBatch) {
    const int s = sums[threadIdx.x];
    if (s) atomicAdd(&batch->count[threadIdx.x], s);  // (an INVALID hypothesis has NaN entries, s = 0, and keeps its -1)
  }
}

// flags[r] = 1 where pair r stays: an inlier of T, or every pair with keep_all.  keys (or null): the key of a rejected pair's
// source point becomes kEmptyKey.  *n_kept += the pairs that stay; stats (or null): {pairs in, pairs out, 0} of a chain stage.
__global__ __launch_bounds__(RS_BLOCK) void rsac_flag_kernel(const float4* __restrict__ P, const float4* __restrict__ Q,
                                                             const int* __restrict__ rank, int m, Xform T, float thr, int keep_all,
                                                             int* __restrict__ flags, unsigned long long* __restrict__ keys, int n_s,
                                                             unsigned int* __restrict__ n_kept, unsigned int* __restrict__ stats) {
  unsigned int kept = 0;
  for (int r = blockIdx.x * RS_BLOCK + threadIdx.x; r < m; r += gridDim.x * RS_BLOCK) {
    bool in = keep_all != 0;
    if (!in) {
      const float4 p = P[r], q = Q[r];
      in = finite3(p.x, p.y, p.z) && finite3(q.x, q.y, q.z) && rsac_inlier(T, p.x, p.y, p.z, q.x, q.y, q.z, thr);
    }
    if (flags) flags[r] = in ? 1 : 0;
    if (in) kept += 1;
    else if (keys) {
      const int i = rank[r];
      if (i >= 0 && i < n_s) keys[i] = kEmptyKey;
    }
  }
  block_count_add(kept, stats ? stats + 1 : n_kept);
  if (stats && blockIdx.x == 0 && threadIdx.x == 0) stats[0] = (unsigned int)m, stats[2] = 0u;
}

int rsac_blocks(int n) {
  int blocks = (n + 4 * RS_BLOCK - 1) / (4 * RS_BLOCK);
  if (blocks > RS_MAX_BLOCKS) blocks = RS_MAX_BLOCKS;
  return blocks < 1 ? 1 : blocks;
}

}  // namespace

hipError_t launch_rsac_gather_keys(const float4* src, int n_s, const float4* tgt, int n_t, const unsigned long long* keys, float thr, const Xform& T,
                                   int* flags, int* pos, int* scan_scratch, int* rank, int* m_dev, float4* P, float4* Q, hipStream_t stream) {
  if (n_s <= 0 || n_t <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rsac_alive_kernel, dim3((n_s + RS_BLOCK - 1) / RS_BLOCK), dim3(RS_BLOCK), 0, stream, keys, n_s, thr, n_t, flags);
  hipError_t e = launch_compact(flags, n_s, pos, scan_scratch, rank, m_dev, nullptr, nullptr, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rsac_gather_keys_kernel, dim3(rsac_blocks(n_s)), dim3(RS_BLOCK), 0, stream, src, tgt, keys, T, rank, m_dev, n_s, n_t, P, Q);
  return hipGetLastError();
}

hipError_t launch_rsac_gather_index(const float4* source, int n_s, const float4* target, int n_t, const int32_t* iq, const int32_t* im, int m,
                                    float4* P, float4* Q, int* rank, hipStream_t stream) {
  if (m <= 0 || n_s <= 0 || n_t <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rsac_gather_index_kernel, dim3(rsac_blocks(m)), dim3(RS_BLOCK), 0, stream, source, n_s, target, n_t, iq, im, m, P, Q, rank);
  return hipGetLastError();
}

hipError_t launch_rsac_moments(const float4* P, int m_host, const int* m_dev, int m_cap, double* out14, hipStream_t stream) {
  hipLaunchKernelGGL(rsac_moments_kernel, dim3(1), dim3(RS_REDUCE), 0, stream, P, m_host, m_dev, m_cap, out14);
  return hipGetLastError();
}

hipError_t launch_rsac_models(const float4* P, const float4* Q, int m, unsigned long long seed, int t0, int max_iterations, double sample_d2,
                              RsacModels* models, hipStream_t stream) {
  if (m < 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rsac_model_kernel, dim3(1), dim3(kSacBatch), 0, stream, P, Q, m, seed, t0, max_iterations, sample_d2, models);
  return hipGetLastError();
}

hipError_t launch_rsac_count(const float4* P, const float4* Q, int m, float thr, RsacBatch* batch, hipStream_t stream) {
  if (m <= 0) return hipErrorInvalidValue;
  const long long blocks = ((long long)m + kSacBlockPoints - 1) / kSacBlockPoints;
  hipLaunchKernelGGL(rsac_count_kernel, dim3((unsigned int)std::min<long long>(blocks, kSacGridCap)), dim3(RS_BLOCK), 0, stream, P, Q, m, thr, batch);
  return hipGetLastError();
}

hipError_t launch_rsac_flags(const float4* P, const float4* Q, const int* rank, int m, const Xform& T, float thr, bool keep_all, int* flags,
                             unsigned long long* keys, int n_s, unsigned int* n_kept, unsigned int* stats, hipStream_t stream) {
  if (m < 0 || (!n_kept && !stats)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rsac_flag_kernel, dim3(rsac_blocks(m)), dim3(RS_BLOCK), 0, stream, P, Q, rank, m, T, thr, keep_all ? 1 : 0, flags, keys, n_s,
                     n_kept, stats);
  return hipGetLastError();
}

}  // namespace icpgpu
