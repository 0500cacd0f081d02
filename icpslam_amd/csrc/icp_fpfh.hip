// icp_fpfh.hip -- pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33>: fast point feature histograms from the neighbour rows of
// the search cloud and its normals (rules: include/icpgpu.h "fast point feature histograms"; host:
// icpgpu_search.cpp, icpgpu_fpfh_estimation).
//
// The neighbour rows are the neighbour search's (icp_search.hip), still in device memory, in the two forms launch_normals_from_rows
// takes: dense rows of stride k with n_found (setKSearch) or CSR rows with row_start (setRadiusSearch), ascending by key.
//   spfh_from_rows_kernel  a wave per cloud point p, lane t on row entry t (rows longer than 64 in passes): the pair's Darboux frame
//                          in float32, every operation rounded on its own (the tree builds with -ffp-contract=off), its three bins,
//                          three integer LDS atomics into the wave's 33 counters -- counts do not depend on arrival order -- and
//                          lanes 0..32 store count * incr as one 132-byte line.
//   fpfh_from_rows_kernel  a wave per query, lane b < 33 owns bin b: the row's indices and d2 are read 64 at a time, each neighbour's
//                          SPFH line is one 132-byte read with FP_GATHER lines in flight, index and weight come from a lane read,
//                          the float32 sums run strictly in row order, and the three 11-term float64 sums are taken across lanes in
//                          bin order.
// No comparison with another layout (a lane per point, ballot and popcount counters) has been run: EXPERIMENTS.md says so.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/icpgpu.h"
#include "icp_kernels.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int FP_BINS = ICPGPU_FPFH_BINS;
constexpr int FP_SPFH_BLOCK = 64;   // a wave per workgroup: its barrier is the wave's own, whatever the row's length
constexpr int FP_FPFH_BLOCK = 256;  // four queries per workgroup: no LDS, no barrier
constexpr int FP_GATHER = 4;        // SPFH lines in flight per wave

__constant__ const float kEdgeCos[10] = ICPGPU_FPFH_EDGE_COS;
__constant__ const float kEdgeSin[10] = ICPGPU_FPFH_EDGE_SIN;

// rows: n_found != null: row i = [i * k, i * k + n_found[i]); else row i = [row_start[i], row_start[i + 1])
__device__ __forceinline__ void row_of(int i, const int32_t* __restrict__ n_found, int k, const int* __restrict__ row_start, size_t& base, int& m) {
  if (n_found) {
    base = (size_t)i * (size_t)k;
    m = min(n_found[i], k);
  } else {
    base = (size_t)row_start[i];
    m = row_start[i + 1] - row_start[i];
  }
  m = __builtin_amdgcn_readfirstlane(max(m, 0));
}

// bins of f2 and f3: float64 as PCL's expression promotes; a NaN lands in bin 0
__device__ __forceinline__ int bin_of_unit(float f) {
  const double t = floor(11.0 * (((double)f + 1.0) * 0.5));
  return !(t >= 0.0) ? 0 : (t > 10.0 ? 10 : (int)t);
}

// bin of atan2f(y, x) without atan2f: the number of interior bin edges the direction (-x, -y) has passed
__device__ __forceinline__ int bin_of_angle(float y, float x) {
  const float a = -x, b = -y;
  int passed, first;
  if (b >= 0.f) {
    passed = 0, first = 0;
  } else {
    passed = 5, first = 5;
  }
#pragma unroll
  for (int e = 0; e < 5; ++e) {
    const float c = first ? kEdgeCos[5 + e] : kEdgeCos[e], s = first ? kEdgeSin[5 + e] : kEdgeSin[e];
    passed += (c * b - s * a >= 0.f) ? 1 : 0;
  }
  return passed;
}


// the three bins of the pair (p, j); false: the pair is skipped
__device__ __forceinline__ bool pair_bins(const float4 Pp, const float4 Np, const float4 Pj, const float4 Nj, int& b1, int& b2, int& b3) {
  float dx = Pj.x - Pp.x, dy = Pj.y - Pp.y, dz = Pj.z - Pp.z;
  const float f4 = sqrtf((dx * dx + dy * dy) + dz * dz);
  if (f4 == 0.f || !finite3(Np.x, Np.y, Np.z) || !finite3(Nj.x, Nj.y, Nj.z)) return false;
  const float a1 = ((Np.x * dx + Np.y * dy) + Np.z * dz) / f4;
  const float a2 = ((Nj.x * dx + Nj.y * dy) + Nj.z * dz) / f4;
  // the swap by selects on the values (a select between the two normals' addresses puts them into scratch)
  const bool swap = fabsf(a1) < fabsf(a2);
  const float n1x = swap ? Nj.x : Np.x, n1y = swap ? Nj.y : Np.y, n1z = swap ? Nj.z : Np.z;
  const float n2x = swap ? Np.x : Nj.x, n2y = swap ? Np.y : Nj.y, n2z = swap ? Np.z : Nj.z;
  dx = swap ? -dx : dx, dy = swap ? -dy : dy, dz = swap ? -dz : dz;
  const float f3 = swap ? -a2 : a1;
  float vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
  const float vn = sqrtf((vx * vx + vy * vy) + vz * vz);
  if (vn == 0.f) return false;
  vx /= vn, vy /= vn, vz /= vn;
  const float wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
  const float f2 = (vx * n2x + vy * n2y) + vz * n2z;
  const float y = (wx * n2x + wy * n2y) + wz * n2z;
  const float x = (n1x * n2x + n1y * n2y) + n1z * n2z;
  b1 = bin_of_angle(y, x);
  b2 = bin_of_unit(f2);
  b3 = bin_of_unit(f3);
  return true;
}

__global__ __launch_bounds__(FP_SPFH_BLOCK) void spfh_from_rows_kernel(const float4* __restrict__ cloud, int n, const float4* __restrict__ normals,
                                                                       const int32_t* __restrict__ idx, const int32_t* __restrict__ n_found, int k,
                                                                       const int* __restrict__ row_start, float* __restrict__ spfh) {
  __shared__ int counts[FP_BINS];
  const int lane = (int)threadIdx.x;
  const int p = (int)blockIdx.x;  // (< n: the grid has n workgroups)
  if (lane < FP_BINS) counts[lane] = 0;
  __syncthreads();
  size_t base;
  int m;
  row_of(p, n_found, k, row_start, base, m);
  if (m >= 2) {
    const float4 Pp = cloud[p], Np = normals[p];
    for (int t = lane; t < m; t += FP_SPFH_BLOCK) {
      const int j = min(max(idx[base + (size_t)t], 0), n - 1);  // (a row names cloud points)
      if (j == p) continue;
      int b1, b2, b3;
      if (!pair_bins(Pp, Np, cloud[j], normals[j], b1, b2, b3)) continue;
      atomicAdd(&counts[b1], 1);
      atomicAdd(&counts[11 + b2], 1);
      atomicAdd(&counts[22 + b3], 1);
    }
  }
  __syncthreads();
  if (lane < FP_BINS) {
    const int c = counts[lane];
    float v = 0.f;
    if (m >= 2 && c != 0) {
      const float incr = 100.0f / (float)(m - 1);
      v = (float)c * incr;
    }
    spfh[(size_t)p * FP_BINS + lane] = v;
  }
}

__global__ __launch_bounds__(FP_FPFH_BLOCK) void fpfh_from_rows_kernel(const float4* __restrict__ queries, int n_q, int n, const float* __restrict__ spfh,
                                                                       const int32_t* __restrict__ idx, const float* __restrict__ d2,
                                                                       const int32_t* __restrict__ n_found, int k, const int* __restrict__ row_start,
                                                                       float* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63u);
  const int q = (int)blockIdx.x * (FP_FPFH_BLOCK / 64) + (int)(threadIdx.x >> 6);
  if (q >= n_q) return;  // (wave-uniform)
  const int bin = min(lane, FP_BINS - 1);
  const float4 Q = queries[q];
  if (!finite3(Q.x, Q.y, Q.z)) {
    if (lane < FP_BINS) out[(size_t)q * FP_BINS + lane] = __builtin_nanf("");
    return;
  }
  size_t base;
  int m;
  row_of(q, n_found, k, row_start, base, m);
  if (n <= 0) m = 0;
  float h = 0.f;
  for (int t0 = 0; t0 < m; t0 += 64) {
    const int cnt = min(64, m - t0);
    int jl = 0;
    float dl = 0.f;
    if (lane < cnt) {
      jl = min(max(idx[base + (size_t)(t0 + lane)], 0), n - 1);
      dl = d2[base + (size_t)(t0 + lane)];
    }
    for (int u0 = 0; u0 < cnt; u0 += FP_GATHER) {
      float line[FP_GATHER];
#pragma unroll
      for (int g = 0; g < FP_GATHER; ++g) {
        const int j = __builtin_amdgcn_readlane(jl, min(u0 + g, cnt - 1));
        line[g] = spfh[(size_t)j * FP_BINS + bin];
      }
#pragma unroll
      for (int g = 0; g < FP_GATHER; ++g) {
        if (u0 + g < cnt) {
          const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dl), min(u0 + g, cnt - 1)));
          if (d != 0.f) {  // (the point itself, every coincident point)
            const float w = 1.0f / d;
            h += line[g] * w;
          }
        }
      }
    }
  }
  // the sub-histogram's sum, float64, in bin order: every lane of a sub-histogram takes the same eleven terms
  const int first = (bin / 11) * 11;
  double s = (double)__shfl(h, first, 64);
#pragma unroll
  for (int e = 1; e < 11; ++e) s += (double)__shfl(h, first + e, 64);
  if (s != 0.0) h = h * (float)(100.0 / s);
  if (lane < FP_BINS) out[(size_t)q * FP_BINS + lane] = h;
}

}  // namespace

hipError_t launch_spfh_from_rows(const float4* cloud, int n, const float4* normals, const int32_t* idx, const int32_t* n_found, int k,
                                 const int* row_start, float* spfh, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if ((n_found == nullptr) == (row_start == nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(spfh_from_rows_kernel, dim3(n), dim3(FP_SPFH_BLOCK), 0, stream, cloud, n, normals, idx, n_found, k, row_start, spfh);
  return hipGetLastError();
}

hipError_t launch_fpfh_from_rows(const float4* queries, int n_q, int n, const float* spfh, const int32_t* idx, const float* d2, const int32_t* n_found,
                                 int k, const int* row_start, float* out, hipStream_t stream) {
  if (n_q <= 0) return hipSuccess;
  if ((n_found == nullptr) == (row_start == nullptr)) return hipErrorInvalidValue;
  const int per = FP_FPFH_BLOCK / 64;
  hipLaunchKernelGGL(fpfh_from_rows_kernel, dim3((n_q + per - 1) / per), dim3(FP_FPFH_BLOCK), 0, stream, queries, n_q, n, spfh, idx, d2, n_found, k,
                     row_start, out);
  return hipGetLastError();
}

}  // namespace icpgpu
