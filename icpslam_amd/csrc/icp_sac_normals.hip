// icp_sac_normals.hip -- pcl::SACSegmentationFromNormals (SACMODEL_NORMAL_PLANE, SACMODEL_CYLINDER, SAC_RANSAC) over a context's
// search cloud and its normals (rules: include/icpgpu.h "segmentation from normals"; the expressions: icp_sac_normals.h).
//
// The scheme is the plane segmentation's (icp_sac.hip): 64 hypotheses at a time, the host replays the sequential loop over their
// counts (icpgpu_sac_normals.cpp).
//   * sacn_model_kernel: one thread per hypothesis -- the samples, validity, the coefficients into a record of kSacnRecord floats;
//     for a cylinder also the band of squared distances from the axis outside which no point can be an inlier (below).
//   * sacn_count_kernel<MODEL>, the hot path: hypothesis h belongs to lane h of every wave.  A wave takes SACN_WAVE_POINTS points
//     per step, SACN_PPL in every lane's registers with their normals and weights, and walks the 64 records, which it reads
//     wave-uniformly.  A pair is an inlier iff w theta + (1 - w) d_e < thr; with w >= 0 that needs b = (1 - w) d_e < thr (theta >= 0
//     and rounding is monotonic), so the angle -- a square root, a division and the polynomial -- is evaluated only where some lane
//     of the wave has b < thr: a wave-uniform branch, and the decision is the rule's bit for bit.  A point whose weight is negative
//     (a curvature above 1) takes no short-cut.  For a cylinder d_e itself costs a square root, so the first test is on the squared
//     distance c2 against the record's band [lo2, hi2], which is wider than the rule's by a factor of 1.001 per operation -- a
//     thousand times the rounding of the operations it stands for -- and the exact test follows inside.
//     12 + 3 registers per point (plane), 2 points per lane: the walk holds 64 VGPRs at most.
//   * selection: flags by the same expressions, the compaction of icp_scan.hip (launch_compact) -- ascending indices.
//   * sacn_cyl_sums_kernel: the 21 sums of one Gauss-Newton pass over the inliers, ONE workgroup in a fixed order, the terms of
//     icp_sac_normals.h accumulated in double-double (icp_dd.h).
//   * sacn_list_flags: flags of a kept inlier list, for icpgpu_sac_extract over a from-normals result.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"
#include "icp_sac_normals.h"

namespace icpgpu {
namespace {

constexpr int SACN_BLOCK = 256, SACN_WAVES = SACN_BLOCK / 64;
constexpr int SACN_PPL = 2;
constexpr int SACN_WAVE_POINTS = 64 * SACN_PPL;
constexpr int SACN_REDUCE = 512;  // the one workgroup of the sums kernel: 21 double-double accumulators a thread want 256 VGPRs
static_assert(SACN_WAVES * SACN_WAVE_POINTS == kSacnBlockPoints, "icp_kernels.h states the points of a workgroup's step");

// splitmix64 of the rule's counter: hypothesis t, sample c of `size`
__device__ __forceinline__ unsigned long long sacn_mix(unsigned long long seed, unsigned long long t, unsigned int c, unsigned int size) {
  unsigned long long z = seed + ((unsigned long long)size * t + (unsigned long long)c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ int sacn_draw(unsigned long long seed, int t, unsigned int c, unsigned int size, int n) {
  return (int)(((sacn_mix(seed, (unsigned long long)t, c, size) >> 32) * (unsigned long long)(unsigned int)n) >> 32);
}

__global__ __launch_bounds__(kSacBatch) void sacn_model_kernel(const float4* __restrict__ cloud, const float4* __restrict__ normals, int n, int model,
                                                               unsigned long long seed, int t0, int max_iterations, int use_axis, double ax, double ay,
                                                               double az, double cos_eps, double radius_min, double radius_max, float thr, float weight,
                                                               SacnBatch* __restrict__ out) {
  const int h = (int)threadIdx.x;
  const int t = t0 + h;
  const float nan = __builtin_nanf("");
  float rec[kSacnRecord];
#pragma unroll
  for (int e = 0; e < kSacnRecord; ++e) rec[e] = nan;
  int s[3] = {-1, -1, -1};
  bool valid = false;
  if (t < max_iterations && n > 0) {
    if (model == kSacnPlane) {
#pragma unroll
      for (unsigned int c = 0; c < 3u; ++c) s[c] = sacn_draw(seed, t, c, 3u, n);
      if (s[0] != s[1] && s[0] != s[2] && s[1] != s[2]) {
        const float4 p0 = cloud[s[0]], p1 = cloud[s[1]], p2 = cloud[s[2]];
        if (finite3(p0.x, p0.y, p0.z) && finite3(p1.x, p1.y, p1.z) && finite3(p2.x, p2.y, p2.z)) {
          const float ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
          const float vx = p2.x - p0.x, vy = p2.y - p0.y, vz = p2.z - p0.z;
          const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
          const float l2 = (cx * cx + cy * cy) + cz * cz;
          if (l2 != 0.f && isfinite(l2)) {
            const float l = sacn_sqrtf(l2);
            const float nx = cx / l, ny = cy / l, nz = cz / l;
            rec[0] = nx, rec[1] = ny, rec[2] = nz, rec[3] = -((nx * p0.x + ny * p0.y) + nz * p0.z);
            valid = true;
          }
        }
      }
    } else {
#pragma unroll
      for (unsigned int c = 0; c < 2u; ++c) s[c] = sacn_draw(seed, t, c, 2u, n);
      if (s[0] != s[1]) {
        const float4 p1 = cloud[s[0]], p2 = cloud[s[1]], n1 = normals[s[0]], n2 = normals[s[1]];
        if (finite3(p1.x, p1.y, p1.z) && finite3(p2.x, p2.y, p2.z) && finite3(n1.x, n1.y, n1.z) && finite3(n2.x, n2.y, n2.z)) {
          const float P1[3] = {p1.x, p1.y, p1.z}, N1[3] = {n1.x, n1.y, n1.z}, P2[3] = {p2.x, p2.y, p2.z}, N2[3] = {n2.x, n2.y, n2.z};
          float cy[7];
          if (sacn_cylinder_model(P1, N1, P2, N2, cy)) {
            valid = true;
            const double r = (double)cy[6];
            if (radius_min != 0.0 || radius_max != 0.0) valid = r >= radius_min && r <= radius_max;
            if (valid && use_axis) valid = fabs((ax * (double)cy[3] + ay * (double)cy[4]) + az * (double)cy[5]) >= cos_eps;
            if (valid) {
#pragma unroll
              for (int e = 0; e < 7; ++e) rec[e] = cy[e];
              // the band of c2 = dist^2 outside which (1 - w) |dist - r| < thr cannot hold, every step widened by 1.001
              const float om = 1.f - weight;
              float lo2 = -1.f, hi2 = __builtin_inff();
              const float band = om > 0.f ? (thr / om) * 1.001f : __builtin_inff();
              if (band >= 1e-30f && isfinite(band)) {
                const float hi = (cy[6] + band) * 1.001f, lo = (cy[6] - band) * 0.999f;
                hi2 = (hi * hi) * 1.001f;
                if (lo > 1e-15f) lo2 = (lo * lo) * 0.999f;
              }
              rec[8] = lo2, rec[9] = hi2;
              rec[12] = p1.x, rec[13] = p1.y, rec[14] = p1.z;  // (K of the refinement's chart)
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < kSacnRecord; ++e) out->rec[h][e] = rec[e];
  out->count[h] = valid ? 0 : -1;
  out->sample[h][0] = s[0], out->sample[h][1] = s[1], out->sample[h][2] = s[2];
}

// what a lane keeps of point j: the point, its normal, its weight w_q and the short-cut's limit (thr, or +inf for w_q < 0).  A point
// that can never be an inlier -- past the cloud's end, or a non-finite point, normal or curvature -- has a NaN x.
template <int MODEL>
__device__ __forceinline__ void sacn_load(const float4* __restrict__ cloud, const float4* __restrict__ normals, long long j, int n, float weight, float thr,
                                          float& qx, float& qy, float& qz, float& mx, float& my, float& mz, float& w, float& lim) {
  qx = __builtin_nanf(""), qy = qz = mx = my = mz = 0.f, w = weight, lim = thr;
  if (j < (long long)n) {
    const float4 q = cloud[j], m = normals[j];
    if (finite3(q.x, q.y, q.z) && finite3(m.x, m.y, m.z) && isfinite(m.w)) {
      qx = q.x, qy = q.y, qz = q.z, mx = m.x, my = m.y, mz = m.z;
      if (MODEL == kSacnPlane) {
        w = weight * (1.f - m.w);
        if (w < 0.f) lim = __builtin_inff();
      }
    }
  }
}

template <int MODEL>
__global__ __launch_bounds__(SACN_BLOCK) void sacn_count_kernel(const float4* __restrict__ cloud, const float4* __restrict__ normals, int n, float thr,
                                                                float weight, SacnBatch* __restrict__ batch) {
  __shared__ int sums[kSacBatch];
  const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < (unsigned int)kSacBatch) sums[threadIdx.x] = 0;
  __syncthreads();
  int acc = 0;
  const long long stride = (long long)gridDim.x * kSacnBlockPoints;
  for (long long base = (long long)blockIdx.x * kSacnBlockPoints + (long long)wave * SACN_WAVE_POINTS; base < (long long)n; base += stride) {  // (wave-uniform)
    float qx[SACN_PPL], qy[SACN_PPL], qz[SACN_PPL], mx[SACN_PPL], my[SACN_PPL], mz[SACN_PPL], w[SACN_PPL], lim[SACN_PPL];
#pragma unroll
    for (int u = 0; u < SACN_PPL; ++u)
      sacn_load<MODEL>(cloud, normals, base + u * 64 + (long long)lane, n, weight, thr, qx[u], qy[u], qz[u], mx[u], my[u], mz[u], w[u], lim[u]);
#pragma unroll 2
    for (int h = 0; h < kSacBatch; ++h) {
      float rec[10];
#pragma unroll
      for (int e = 0; e < (MODEL == kSacnPlane ? 4 : 10); ++e) rec[e] = batch->rec[h][e];  // (the same address in every lane)
      int c = 0;
#pragma unroll
      for (int u = 0; u < SACN_PPL; ++u) {
        if (MODEL == kSacnPlane) {
          const float b = (1.f - w[u]) * sacn_plane_de(rec, qx[u], qy[u], qz[u]);
          if (__ballot(b < lim[u])) {
            const float v = w[u] * sacn_angle(mx[u], my[u], mz[u], rec[0], rec[1], rec[2]) + b;
            c += __popcll(__ballot(v < thr));
          }
        } else {
          float vx, vy, vz;
          const float c2 = sacn_cyl_c2(rec, qx[u], qy[u], qz[u], vx, vy, vz);
          if (__ballot(c2 > rec[8] && c2 < rec[9])) {
            bool on_axis;
            const float v = sacn_cyl_value_from(rec, c2, vx, vy, vz, mx[u], my[u], mz[u], w[u], &on_axis);
            c += __popcll(__ballot(!on_axis && v < thr));
          }
        }
      }
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

struct SacnCoeff {
  float v[8];
};

// flags[i] = 1 where point i is an inlier of the model
__global__ __launch_bounds__(SACN_BLOCK) void sacn_flag_kernel(const float4* __restrict__ cloud, const float4* __restrict__ normals, int n, int model,
                                                               SacnCoeff co, float thr, float weight, int* __restrict__ flags) {
  const int i = blockIdx.x * SACN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 q = cloud[i], m = normals[i];
  bool in = false;
  if (finite3(q.x, q.y, q.z) && finite3(m.x, m.y, m.z) && isfinite(m.w)) {
    if (model == kSacnPlane) {
      in = sacn_plane_value(co.v, q.x, q.y, q.z, m.x, m.y, m.z, weight * (1.f - m.w)) < thr;
    } else {
      bool on_axis;
      const float v = sacn_cyl_value(co.v, q.x, q.y, q.z, m.x, m.y, m.z, weight, &on_axis);
      in = !on_axis && v < thr;
    }
  }
  flags[i] = in ? 1 : 0;
}

// out[0 .. 21): the sums of sacn_cyl_terms over the m listed points.  Thread t takes entries t, t + 512, ...; then a binary tree per sum.
struct SacnChart {
  double P[3], D[3], r;
  int ia, ib;
};
__global__ __launch_bounds__(SACN_REDUCE) void sacn_cyl_sums_kernel(const float4* __restrict__ cloud, const int* __restrict__ list, int n, int m,
                                                                    SacnChart ch, double* __restrict__ out) {
  __shared__ DD sh[SACN_REDUCE];
  DD acc[kSacnCylTerms];
#pragma unroll
  for (int e = 0; e < kSacnCylTerms; ++e) acc[e].hi = acc[e].lo = 0.0;
  for (int k = threadIdx.x; k < m; k += SACN_REDUCE) {
    const float4 q = cloud[min(max(list[k], 0), n - 1)];  // (the list names cloud points)
    double term[kSacnCylTerms];
    sacn_cyl_terms(ch.P, ch.D, ch.ia, ch.ib, ch.r, q.x, q.y, q.z, term);
#pragma unroll
    for (int e = 0; e < kSacnCylTerms; ++e) dd_add_term(acc[e], term[e]);
  }
#pragma unroll
  for (int e = 0; e < kSacnCylTerms; ++e) {
    sh[threadIdx.x] = acc[e];
    __syncthreads();
    for (int step = SACN_REDUCE / 2; step > 0; step >>= 1) {
      if ((int)threadIdx.x < step) sh[threadIdx.x] = dd_add(sh[threadIdx.x], sh[threadIdx.x + step]);
      __syncthreads();
    }
    if (threadIdx.x == 0) out[e] = sh[0].hi + sh[0].lo;
    __syncthreads();
  }
}

__global__ __launch_bounds__(SACN_BLOCK) void sacn_fill_kernel(int* __restrict__ flags, int n, int value) {
  const int i = blockIdx.x * SACN_BLOCK + threadIdx.x;
  if (i < n) flags[i] = value;
}
__global__ __launch_bounds__(SACN_BLOCK) void sacn_mark_kernel(const int* __restrict__ list, int m, int n, int value, int* __restrict__ flags) {
  const int k = blockIdx.x * SACN_BLOCK + threadIdx.x;
  if (k >= m) return;
  const int i = list[k];
  if (i >= 0 && i < n) flags[i] = value;
}

}  // namespace

hipError_t launch_sacn_batch(const float4* cloud, const float4* normals, int n, int model, unsigned long long seed, int t0, int max_iterations,
                             bool use_axis, const double axis[3], double cos_eps, double radius_min, double radius_max, float thr, float weight,
                             SacnBatch* batch, hipStream_t stream) {
  if (n <= 0 || (model != kSacnPlane && model != kSacnCylinder)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sacn_model_kernel, dim3(1), dim3(kSacBatch), 0, stream, cloud, normals, n, model, seed, t0, max_iterations, use_axis ? 1 : 0,
                     axis[0], axis[1], axis[2], cos_eps, radius_min, radius_max, thr, weight, batch);
  const long long blocks = ((long long)n + kSacnBlockPoints - 1) / kSacnBlockPoints;
  const dim3 grid((unsigned int)std::min<long long>(blocks, kSacnGridCap));
  if (model == kSacnPlane) hipLaunchKernelGGL(sacn_count_kernel<kSacnPlane>, grid, dim3(SACN_BLOCK), 0, stream, cloud, normals, n, thr, weight, batch);
  else hipLaunchKernelGGL(sacn_count_kernel<kSacnCylinder>, grid, dim3(SACN_BLOCK), 0, stream, cloud, normals, n, thr, weight, batch);
  return hipGetLastError();
}

hipError_t launch_sacn_select(const float4* cloud, const float4* normals, int n, int model, const float coeff7[7], float thr, float weight, int* flags,
                              int* pos, int* scan_scratch, int* inliers, int* n_inliers, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  SacnCoeff co;
  for (int e = 0; e < 7; ++e) co.v[e] = coeff7[e];
  co.v[7] = 0.f;
  hipLaunchKernelGGL(sacn_flag_kernel, dim3((n + SACN_BLOCK - 1) / SACN_BLOCK), dim3(SACN_BLOCK), 0, stream, cloud, normals, n, model, co, thr, weight,
                     flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_compact(flags, n, pos, scan_scratch, inliers, n_inliers, nullptr, nullptr, stream);
}

hipError_t launch_sacn_cyl_sums(const float4* cloud, int n, const int* inliers, int m, const double P[3], const double D[3], int ia, int ib, double r,
                                double* sums21, hipStream_t stream) {
  if (m <= 0 || n <= 0 || ia < 0 || ia > 2 || ib < 0 || ib > 2) return hipErrorInvalidValue;
  SacnChart ch;
  for (int a = 0; a < 3; ++a) ch.P[a] = P[a], ch.D[a] = D[a];
  ch.r = r, ch.ia = ia, ch.ib = ib;
  hipLaunchKernelGGL(sacn_cyl_sums_kernel, dim3(1), dim3(SACN_REDUCE), 0, stream, cloud, inliers, n, m, ch, sums21);
  return hipGetLastError();
}

hipError_t launch_sacn_list_flags(const int* list, int m, int n, bool invert, int* flags, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sacn_fill_kernel, dim3((n + SACN_BLOCK - 1) / SACN_BLOCK), dim3(SACN_BLOCK), 0, stream, flags, n, invert ? 1 : 0);
  if (m > 0)
    hipLaunchKernelGGL(sacn_mark_kernel, dim3((m + SACN_BLOCK - 1) / SACN_BLOCK), dim3(SACN_BLOCK), 0, stream, list, m, n, invert ? 0 : 1, flags);
  return hipGetLastError();
}

}  // namespace icpgpu
