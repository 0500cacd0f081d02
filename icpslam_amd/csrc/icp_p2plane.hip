// icp_p2plane.hip -- device side of the point-to-plane mode: the per-iteration reduction of
// pcl::IterativeClosestPointWithNormals with pcl::registration::TransformationEstimationPointToPlaneLLS (PCL 1.8), the third
// Registration variant next to the reference's GICP (the reference asks for it at icp_odometer.cpp:187 of the reference).
//
//   p2plane_reduce_kernel  over the keys of a correspondence sweep (icp_grid.hip's key-writing search or the brute-force keys):
//                          pairs with d2 <= thr (the point-to-point accept rule); per pair s = T * source
//                          (float32, xform_point), d = target, n = target normal (float4, icp_gicp_cov.hip: gicp_normal_finish_kernel
//                          or the caller's) and the terms of estimateRigidTransformation in float, widened to double:
//                            a = nz sy - ny sz,  b = nx sz - nz sx,  c = ny sx - nx sy
//                            r = ((((nx dx + ny dy) + nz dz) - nx sx) - ny sy) - nz sz
//                          every product and difference rounded on its own (__fmul_rn / __fsub_rn / __fadd_rn: never contracted).
//                          29 float64 terms per lane, one partial per workgroup (fixed shuffle + LDS tree).
//   p2plane_final_kernel   one workgroup per term adds the workgroups' partials in a fixed order (reduce_final_kernel's scheme) and
//                          stores the sum as a result pair into the host mailbox (or into device memory).
//   p2plane_sym_reduce_kernel  the same sweep for the symmetric objective (TransformationEstimationSymmetricPointToPlaneLLS, PCL 1.10;
//                          icpgpu_set_p2plane_symmetric): it also reads the source's normal, rotates it by T (xform_normal) and
//                          forms, all in float32 and never contracted,
//                            n1 = R(T) source normal,  dot = (n1x n2x + n1y n2y) + n1z n2z
//                            n = (enforce && !(dot >= 0)) ? n1 - n2 : n1 + n2,   m = p + q,   c = m x n
//                            r = ((qx - px) nx + (qy - py) ny) + (qz - pz) nz
//                          over v = (c, n) -- the same 29 terms, the same block reduction, the same final kernel.
// HBM traffic per accepted pair: 8 B key + 16 B source + 16 B gathered target + 16 B gathered normal (+ 16 B source normal for
// the symmetric objective: 72 B against 56 B).
#include <math.h>

#include "icp_device.h"
#include "icp_kernels.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int PP_BLOCK = 256;
constexpr int PP_FINAL_BLOCK = 1024;
constexpr int kP2planeMaxBlocks = 1024;

// one row (v, r) of the linear system into the 27 sums behind count and sum d2: the upper triangle of v v^T row by row, then v r
__device__ __forceinline__ void accumulate_row(double (&acc)[kP2planeTerms], const double (&v)[6], double r) {
  int k = 2;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) acc[k++] += v[i] * v[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[23 + i] += v[i] * r;
}

__device__ __forceinline__ void p2plane_accumulate(double (&acc)[kP2planeTerms], const float4& s_raw, const float4& d, const float4& nrm,
                                                   const Xform& T, float d2) {
  acc[0] += 1.0;
  acc[1] += (double)d2;
  const float nx = nrm.x, ny = nrm.y, nz = nrm.z;
  if (!finite3(nx, ny, nz)) return;  // PCL's estimator skips the pair; it stays a correspondence
  float sx, sy, sz;
  xform_point(T, s_raw.x, s_raw.y, s_raw.z, sx, sy, sz);
  const float fa = __fsub_rn(__fmul_rn(nz, sy), __fmul_rn(ny, sz));
  const float fb = __fsub_rn(__fmul_rn(nx, sz), __fmul_rn(nz, sx));
  const float fc = __fsub_rn(__fmul_rn(ny, sx), __fmul_rn(nx, sy));
  float fr = __fadd_rn(__fadd_rn(__fmul_rn(nx, d.x), __fmul_rn(ny, d.y)), __fmul_rn(nz, d.z));
  fr = __fsub_rn(fr, __fmul_rn(nx, sx));
  fr = __fsub_rn(fr, __fmul_rn(ny, sy));
  fr = __fsub_rn(fr, __fmul_rn(nz, sz));
  const double v[6] = {(double)fa, (double)fb, (double)fc, (double)nx, (double)ny, (double)nz};
  accumulate_row(acc, v, (double)fr);
}

// the symmetric objective's pair: sn_raw = the source's normal as stored (rotated here), nrm = the target's
__device__ __forceinline__ void p2plane_sym_accumulate(double (&acc)[kP2planeTerms], const float4& s_raw, const float4& sn_raw, const float4& d,
                                                       const float4& nrm, const Xform& T, bool enforce, float d2) {
  acc[0] += 1.0;
  acc[1] += (double)d2;
  float n1x, n1y, n1z;
  xform_normal(T, sn_raw.x, sn_raw.y, sn_raw.z, n1x, n1y, n1z);
  const float dot = normal_dot(n1x, n1y, n1z, nrm.x, nrm.y, nrm.z);
  const bool flip = enforce && !(dot >= 0.f);
  const float nx = flip ? __fsub_rn(n1x, nrm.x) : __fadd_rn(n1x, nrm.x);
  const float ny = flip ? __fsub_rn(n1y, nrm.y) : __fadd_rn(n1y, nrm.y);
  const float nz = flip ? __fsub_rn(n1z, nrm.z) : __fadd_rn(n1z, nrm.z);
  if (!finite3(nx, ny, nz)) return;  // PCL's estimator skips the pair; it stays a correspondence
  float px, py, pz;
  xform_point(T, s_raw.x, s_raw.y, s_raw.z, px, py, pz);
  const float mx = __fadd_rn(px, d.x), my = __fadd_rn(py, d.y), mz = __fadd_rn(pz, d.z);
  const float cx = __fsub_rn(__fmul_rn(my, nz), __fmul_rn(mz, ny));
  const float cy = __fsub_rn(__fmul_rn(mz, nx), __fmul_rn(mx, nz));
  const float cz = __fsub_rn(__fmul_rn(mx, ny), __fmul_rn(my, nx));
  const float fr = __fadd_rn(__fadd_rn(__fmul_rn(__fsub_rn(d.x, px), nx), __fmul_rn(__fsub_rn(d.y, py), ny)), __fmul_rn(__fsub_rn(d.z, pz), nz));
  const double v[6] = {(double)cx, (double)cy, (double)cz, (double)nx, (double)ny, (double)nz};
  accumulate_row(acc, v, (double)fr);
}

// fixed-order block reduction: shuffle tree per wave, then the four waves in order -> one partial per workgroup
__device__ __forceinline__ void p2plane_block_store(const double (&acc)[kP2planeTerms], double* __restrict__ partials) {
  __shared__ double wsum[PP_BLOCK / 64][kP2planeTerms];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kP2planeTerms; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) wsum[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kP2planeTerms) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < PP_BLOCK / 64; ++w) v += wsum[w][threadIdx.x];
    partials[(size_t)blockIdx.x * kP2planeTerms + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(PP_BLOCK) void p2plane_reduce_kernel(const float4* __restrict__ src, int n_s, const float4* __restrict__ tgt,
                                                                  const float4* __restrict__ normals,
                                                                  const unsigned long long* __restrict__ keys, Xform T, float thr,
                                                                  double* __restrict__ partials) {
  double acc[kP2planeTerms];
#pragma unroll
  for (int k = 0; k < kP2planeTerms; ++k) acc[k] = 0.0;
  // four points per trip, their loads issued together (as reduce_kernel: key -> target / normal is a dependent pair of reads)
  const int stride = gridDim.x * PP_BLOCK;
  for (int i0 = blockIdx.x * PP_BLOCK + threadIdx.x; i0 < n_s; i0 += 4 * stride) {
    unsigned long long key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) key[u] = i0 + u * stride < n_s ? keys[i0 + u * stride] : kEmptyKey;
    float4 s[4], d[4], nm[4];
    bool use[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned int j = (unsigned int)key[u];
      use[u] = j != 0xFFFFFFFFu && __uint_as_float((unsigned int)(key[u] >> 32)) <= thr;
      s[u] = src[min(i0 + u * stride, n_s - 1)];
      if (use[u]) {
        d[u] = tgt[j];
        nm[u] = normals[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (use[u]) p2plane_accumulate(acc, s[u], d[u], nm[u], T, __uint_as_float((unsigned int)(key[u] >> 32)));
  }
  p2plane_block_store(acc, partials);
}

// the parent's loop with one more coalesced read per pair (the source's normal)
__global__ __launch_bounds__(PP_BLOCK) void p2plane_sym_reduce_kernel(const float4* __restrict__ src, const float4* __restrict__ src_normals,
                                                                      int n_s, const float4* __restrict__ tgt,
                                                                      const float4* __restrict__ normals,
                                                                      const unsigned long long* __restrict__ keys, Xform T, float thr,
                                                                      int enforce, double* __restrict__ partials) {
  double acc[kP2planeTerms];
#pragma unroll
  for (int k = 0; k < kP2planeTerms; ++k) acc[k] = 0.0;
  const int stride = gridDim.x * PP_BLOCK;
  for (int i0 = blockIdx.x * PP_BLOCK + threadIdx.x; i0 < n_s; i0 += 4 * stride) {
    unsigned long long key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) key[u] = i0 + u * stride < n_s ? keys[i0 + u * stride] : kEmptyKey;
    float4 s[4], sn[4], d[4], nm[4];
    bool use[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned int j = (unsigned int)key[u];
      use[u] = j != 0xFFFFFFFFu && __uint_as_float((unsigned int)(key[u] >> 32)) <= thr;
      s[u] = src[min(i0 + u * stride, n_s - 1)];
      if (use[u]) {
        sn[u] = src_normals[i0 + u * stride];  // (use[u]: the index is below n_s)
        d[u] = tgt[j];
        nm[u] = normals[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (use[u]) p2plane_sym_accumulate(acc, s[u], sn[u], d[u], nm[u], T, enforce != 0, __uint_as_float((unsigned int)(key[u] >> 32)));
  }
  p2plane_block_store(acc, partials);
}

// one workgroup per term: thread t adds partials t, t + 1024, ... in that order, then a fixed shuffle + LDS tree
__global__ __launch_bounds__(PP_FINAL_BLOCK) void p2plane_final_kernel(const double* __restrict__ partials, int n_blocks,
                                                                       double* __restrict__ sums, unsigned long long* flags,
                                                                       unsigned long long seq) {
  const int k = blockIdx.x;
  double v = 0.0;
  for (int b = threadIdx.x; b < n_blocks; b += PP_FINAL_BLOCK) v += partials[(size_t)b * kP2planeTerms + k];
  v = wave_sum(v);
  __shared__ double w[PP_FINAL_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[PP_FINAL_BLOCK / 64];
#pragma unroll
    for (int i = 0; i < PP_FINAL_BLOCK / 64; ++i) t[i] = w[i];
#pragma unroll
    for (int span = 1; span < PP_FINAL_BLOCK / 64; span <<= 1)
#pragma unroll
      for (int i = 0; i + span < PP_FINAL_BLOCK / 64; i += 2 * span) t[i] += t[i + span];
    if (flags) store_result_pair(flags + 2 * k, (unsigned long long)__double_as_longlong(t[0]), seq);
    else sums[k] = t[0];
  }
}

}  // namespace

int p2plane_blocks(int n_s) {
  int blocks = (n_s + 4 * PP_BLOCK - 1) / (4 * PP_BLOCK);  // ~4 points per lane
  if (blocks > kP2planeMaxBlocks) blocks = kP2planeMaxBlocks;
  return blocks < 1 ? 1 : blocks;
}

hipError_t launch_p2plane_reduce(const float4* src, int n_s, const float4* tgt, const float4* normals, const unsigned long long* keys,
                                 const Xform& T, float thr, double* partials, double* sums_out, unsigned long long* flags,
                                 unsigned long long seq, hipStream_t stream) {
  const int blocks = p2plane_blocks(n_s);
  if (n_s > 0) {
    hipLaunchKernelGGL(p2plane_reduce_kernel, dim3(blocks), dim3(PP_BLOCK), 0, stream, src, n_s, tgt, normals, keys, T, thr, partials);
  } else {
    const hipError_t e = hipMemsetAsync(partials, 0, (size_t)blocks * kP2planeTerms * sizeof(double), stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(p2plane_final_kernel, dim3(kP2planeTerms), dim3(PP_FINAL_BLOCK), 0, stream, partials, blocks, sums_out, flags, seq);
  return hipGetLastError();
}

hipError_t launch_p2plane_sym_reduce(const float4* src, const float4* src_normals, int n_s, const float4* tgt, const float4* normals,
                                     const unsigned long long* keys, const Xform& T, float thr, bool enforce, double* partials,
                                     double* sums_out, unsigned long long* flags, unsigned long long seq, hipStream_t stream) {
  const int blocks = p2plane_blocks(n_s);
  if (n_s > 0) {
    hipLaunchKernelGGL(p2plane_sym_reduce_kernel, dim3(blocks), dim3(PP_BLOCK), 0, stream, src, src_normals, n_s, tgt, normals, keys, T, thr,
                       enforce ? 1 : 0, partials);
  } else {
    const hipError_t e = hipMemsetAsync(partials, 0, (size_t)blocks * kP2planeTerms * sizeof(double), stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(p2plane_final_kernel, dim3(kP2planeTerms), dim3(PP_FINAL_BLOCK), 0, stream, partials, blocks, sums_out, flags, seq);
  return hipGetLastError();
}

hipError_t launch_terms29_final(const double* partials, int n_blocks, double* sums_out, unsigned long long* flags, unsigned long long seq,
                                hipStream_t stream, int n_terms) {
  hipLaunchKernelGGL(p2plane_final_kernel, dim3(n_terms), dim3(PP_FINAL_BLOCK), 0, stream, partials, n_blocks, sums_out, flags, seq);
  return hipGetLastError();
}

}  // namespace icpgpu
