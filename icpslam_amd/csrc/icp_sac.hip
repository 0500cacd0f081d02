// icp_sac.hip -- pcl::SACSegmentation (SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, SAC_RANSAC) over a context's search cloud
// (rules: include/icpgpu.h "plane segmentation").
//
// RANSAC's hypotheses are a pure function of (seed, t, n), so 64 of them are taken at once and the host replays the sequential loop
// over their counts (icpgpu_sac.cpp); what was evaluated beyond the loop's stop is thrown away.
//   * sac_model_kernel: one thread per hypothesis of the batch -- the three samples, validity, the four coefficients.  An INVALID
//     hypothesis gets NaN coefficients (no point passes a test against them) and the count -1.
//   * sac_count_kernel, the hot path: hypothesis h of the batch belongs to lane h of every wave.  A wave takes SAC_WAVE_POINTS points
//     per step, SAC_PPL in every lane's registers, and walks the 64 planes, which it reads wave-uniformly (scalar loads): per plane
//     and point register one ballot of the inlier test, and lane h adds the popcount to its own register.  The grid is capped and
//     every workgroup strides over the cloud.  At the end the four waves of a workgroup add their registers in LDS and 64 lanes do
//     one integer atomicAdd each into count[h]: integer sums do not depend on their order, so the counts are exact.
//   * selection: flags by the same test, the compaction of icp_scan.hip (launch_compact) -- ascending indices.
//   * sac_sums_kernel: the refinement's nine sums over the inliers about K = cloud[sample[0]], ONE workgroup in a fixed order, every
//     term exact in float64 and accumulated in double-double (icp_dd.h): the exact sums rounded once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

constexpr int SAC_BLOCK = 256, SAC_WAVES = SAC_BLOCK / 64;
constexpr int SAC_PPL = 2;                                  // points per lane and step
constexpr int SAC_WAVE_POINTS = 64 * SAC_PPL;
constexpr int SAC_REDUCE = 1024;                            // the one workgroup of the sums kernel
static_assert(SAC_WAVES * SAC_WAVE_POINTS == kSacBlockPoints, "icp_kernels.h states the points of a workgroup's step");

// splitmix64 of the rule's counter: hypothesis t, sample c
__device__ __forceinline__ unsigned long long sac_mix(unsigned long long seed, unsigned long long t, unsigned int c) {
  unsigned long long z = seed + (3ull * t + (unsigned long long)c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the rule's inlier test: s = fma(n.z, q.z, fma(n.y, q.y, n.x * q.x)) + d, |s| < thr.  thr is the smallest float32 that is not below
// the double threshold, so that for every float32 f: f < thr <=> (double)f < distance_threshold.  A NaN on either side fails.
__device__ __forceinline__ bool sac_inlier(const float4& pl, float qx, float qy, float qz, float thr) {
  const float s = __builtin_fmaf(pl.z, qz, __builtin_fmaf(pl.y, qy, pl.x * qx)) + pl.w;
  return __builtin_fabsf(s) < thr;
}

__global__ __launch_bounds__(kSacBatch) void sac_model_kernel(const float4* __restrict__ cloud, int n, unsigned long long seed, int t0,
                                                              int max_iterations, int use_axis, double ax, double ay, double az, double cos_eps,
                                                              SacBatch* __restrict__ out) {
  const int h = (int)threadIdx.x;
  const int t = t0 + h;
  const float nan = __builtin_nanf("");
  float4 plane = make_float4(nan, nan, nan, nan);
  int s[3] = {-1, -1, -1};
  bool valid = false;
  if (t < max_iterations && n > 0) {
#pragma unroll
    for (unsigned int c = 0; c < 3u; ++c) s[c] = (int)(((sac_mix(seed, (unsigned long long)t, c) >> 32) * (unsigned long long)(unsigned int)n) >> 32);
    if (s[0] != s[1] && s[0] != s[2] && s[1] != s[2]) {
      const float4 p0 = cloud[s[0]], p1 = cloud[s[1]], p2 = cloud[s[2]];
      if (finite3(p0.x, p0.y, p0.z) && finite3(p1.x, p1.y, p1.z) && finite3(p2.x, p2.y, p2.z)) {
        const float ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
        const float vx = p2.x - p0.x, vy = p2.y - p0.y, vz = p2.z - p0.z;
        const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const float l2 = (cx * cx + cy * cy) + cz * cz;
        if (l2 != 0.f && isfinite(l2)) {
          const float l = (float)__builtin_sqrt((double)l2);  // (correctly rounded sqrtf: see icp_outlier.hip)
          const float nx = cx / l, ny = cy / l, nz = cz / l;
          const float d = -((nx * p0.x + ny * p0.y) + nz * p0.z);
          valid = true;
          if (use_axis) valid = fabs((ax * (double)nx + ay * (double)ny) + az * (double)nz) >= cos_eps;
          if (valid) plane = make_float4(nx, ny, nz, d);
        }
      }
    }
  }
  out->plane[h] = plane;
  out->count[h] = valid ? 0 : -1;
  out->sample[h][0] = s[0], out->sample[h][1] = s[1], out->sample[h][2] = s[2];
}

__global__ __launch_bounds__(SAC_BLOCK) void sac_count_kernel(const float4* __restrict__ cloud, int n, float thr, SacBatch* __restrict__ batch) {
  __shared__ int sums[kSacBatch];
  const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < (unsigned int)kSacBatch) sums[threadIdx.x] = 0;
  __syncthreads();
  const float4* __restrict__ planes = batch->plane;
  const float nan = __builtin_nanf("");
  int acc = 0;
  const long long stride = (long long)gridDim.x * kSacBlockPoints;
  for (long long base = (long long)blockIdx.x * kSacBlockPoints + (long long)wave * SAC_WAVE_POINTS; base < (long long)n; base += stride) {  // (wave-uniform)
    float qx[SAC_PPL], qy[SAC_PPL], qz[SAC_PPL];
#pragma unroll
    for (int u = 0; u < SAC_PPL; ++u) {
      const long long j = base + u * 64 + (long long)lane;
      qx[u] = nan, qy[u] = qz[u] = 0.f;
      if (j < (long long)n) {
        const float4 q = cloud[j];
        if (finite3(q.x, q.y, q.z)) qx[u] = q.x, qy[u] = q.y, qz[u] = q.z;  // (a non-finite point stays NaN: never an inlier)
      }
    }
#pragma unroll 4
    for (int h = 0; h < kSacBatch; ++h) {
      const float4 pl = planes[h];  // (the same address in every lane)
      int c = 0;
#pragma unroll
      for (int u = 0; u < SAC_PPL; ++u) c += __popcll(__ballot(sac_inlier(pl, qx[u], qy[u], qz[u], thr)));
      acc += lane == (unsigned int)h ? c : 0;
    }
  }
  if (acc) atomicAdd(&sums[lane], acc);
  __syncthreads();
  if (threadIdx.x < (unsigned int)kSacBatch) {
    const int s = sums[threadIdx.x];
    if (s) atomicAdd(&batch->count[threadIdx.x], s);  // (an INVALID hypothesis has s = 0 and keeps its -1)
  }
}

// flags[i] = 1 where point i is an inlier of `plane` (found = 0: nowhere), the other way round with invert = 1
__global__ __launch_bounds__(SAC_BLOCK) void sac_flag_kernel(const float4* __restrict__ cloud, int n, float4 plane, float thr, int found, int invert,
                                                             int* __restrict__ flags) {
  const int i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 q = cloud[i];
  const bool in = found && finite3(q.x, q.y, q.z) && sac_inlier(plane, q.x, q.y, q.z, thr);
  flags[i] = (in ? 1 : 0) ^ invert;
}

// out[0 .. 9): the sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz over the m listed points, d = q - K in float32 with
// K = cloud[k_index]; out[9 .. 12): K.  Thread t takes entries t, t + 1024, ...; then a binary tree per sum.
__global__ __launch_bounds__(SAC_REDUCE) void sac_sums_kernel(const float4* __restrict__ cloud, const int* __restrict__ list, int n, int m, int k_index,
                                                              double* __restrict__ out) {
  __shared__ DD sh[SAC_REDUCE];
  const float4 K = cloud[k_index];
  DD acc[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) acc[e].hi = acc[e].lo = 0.0;
  for (int k = threadIdx.x; k < m; k += SAC_REDUCE) {
    const float4 q = cloud[min(max(list[k], 0), n - 1)];  // (the list names cloud points)
    const double dx = (double)(q.x - K.x), dy = (double)(q.y - K.y), dz = (double)(q.z - K.z);
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
    for (int step = SAC_REDUCE / 2; step > 0; step >>= 1) {
      if ((int)threadIdx.x < step) sh[threadIdx.x] = dd_add(sh[threadIdx.x], sh[threadIdx.x + step]);
      __syncthreads();
    }
    if (threadIdx.x == 0) out[e] = sh[0].hi + sh[0].lo;
    __syncthreads();
  }
  if (threadIdx.x == 0) out[9] = (double)K.x, out[10] = (double)K.y, out[11] = (double)K.z;
}

}  // namespace

hipError_t launch_sac_batch(const float4* cloud, int n, unsigned long long seed, int t0, int max_iterations, bool use_axis, const double axis[3],
                            double cos_eps, float thr, SacBatch* batch, hipStream_t stream) {
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sac_model_kernel, dim3(1), dim3(kSacBatch), 0, stream, cloud, n, seed, t0, max_iterations, use_axis ? 1 : 0, axis[0], axis[1],
                     axis[2], cos_eps, batch);
  const long long blocks = ((long long)n + kSacBlockPoints - 1) / kSacBlockPoints;
  hipLaunchKernelGGL(sac_count_kernel, dim3((unsigned int)std::min<long long>(blocks, kSacGridCap)), dim3(SAC_BLOCK), 0, stream, cloud, n, thr, batch);
  return hipGetLastError();
}

hipError_t launch_sac_flags(const float4* cloud, int n, const float plane[4], float thr, bool found, bool invert, int* flags, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sac_flag_kernel, dim3((n + SAC_BLOCK - 1) / SAC_BLOCK), dim3(SAC_BLOCK), 0, stream, cloud, n,
                     make_float4(plane[0], plane[1], plane[2], plane[3]), thr, found ? 1 : 0, invert ? 1 : 0, flags);
  return hipGetLastError();
}

hipError_t launch_sac_select(const float4* cloud, int n, const float plane[4], float thr, int* flags, int* pos, int* scan_scratch, int* inliers,
                             int* n_inliers, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipError_t e = launch_sac_flags(cloud, n, plane, thr, true, false, flags, stream);
  if (e != hipSuccess) return e;
  return launch_compact(flags, n, pos, scan_scratch, inliers, n_inliers, nullptr, nullptr, stream);
}

hipError_t launch_sac_sums(const float4* cloud, int n, const int* inliers, int m, int k_index, double* sums12, hipStream_t stream) {
  if (m <= 0 || k_index < 0 || k_index >= n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sac_sums_kernel, dim3(1), dim3(SAC_REDUCE), 0, stream, cloud, inliers, n, m, k_index, sums12);
  return hipGetLastError();
}

}  // namespace icpgpu
