// icp_feature.hip -- pcl::KdTreeFLANN<pcl::FPFHSignature33>::nearestKSearch: the k nearest descriptors of a target set for every
// query descriptor (rules: include/icpgpu.h "feature-space k-nearest").
//
// The distance is a DIFFERENCE chain -- d_b = q[b] - t[b], d2 = d_0 * d_0, then d2 = fmaf(d_b, d_b, d2) for b = 1 .. 32 -- and not
// a product q . t, so this is vector-ALU work; the chain is one definition per pair whatever the tiling, and the answer is exact.
// A neighbour is the search's key (bits(d2) << 32 | target row), and the selection is the search's (icp_search_device.h: key_offer).
//   * feature_finite_kernel: one flag per target row (every one of its 33 components finite), once per call;
//   * feature_knn_kernel: a workgroup owns FK_QUERIES consecutive queries and streams the whole target set through LDS in tiles of
//     FK_TILE rows, staged BIN-MAJOR with a row stride of FK_TILE + 1 floats (a lane reads t[b][lane] and the staging threads write
//     consecutive bins of one row, both without bank conflicts).  Each of its four waves owns FK_QPW of the queries: a query's 33
//     values sit one per lane in a register and are read wave-uniformly (v_readlane) as the chain goes; each lane owns one target
//     row of the tile at a time, reads a bin ONCE from LDS and advances the chains of all FK_QPW queries with it; the 64 keys of a
//     query then go into its kept list -- one ballot to skip, else a bitonic merge.
//
// pcl::SampleConsensusPrerejective over such rows (rules: include/icpgpu.h "sample-consensus alignment"; host loop: icpgpu_feature.cpp).
// A hypothesis is a pure function of (seed, t, sizes), so a whole chunk of them is sampled at once:
//   * scp_sample_kernel: one thread per hypothesis -- the 2 nr draws, validity, the polygon pre-rejection, and for a survivor the 17
//     sums of its nr pairs in double, which the HOST solves (solve_umeyama);
//   * scp_eval_kernel, the hot path: blockIdx.y is a surviving hypothesis of a batch of up to 64, blockIdx.x a run of
//     SCP_BLOCK_POINTS source points.  A wave takes one transformed point at a time over ball_batches (icp_search_device.h) and
//     keeps the minimum key; a point whose image is not finite or lies outside the target's box grown by the correspondence distance
//     is settled without a walk -- for a wrong hypothesis that is most points.  Counts are integers; the inliers' d2 are summed
//     in double-double (icp_dd.h) in a fixed order: a wave's points ascending, the four waves in order, then
//   * scp_fold_kernel: a thread per hypothesis folds the workgroups' partials in workgroup order -- the exact sum rounded once
//     over the range the header states;
//   * the best hypothesis' inliers: flags by the same test, the compaction of icp_scan.hip (launch_compact).
//
// A feature d2 that overflows is +inf and still a neighbour (its key sorts behind every finite distance and before the empty key); NaN
// cannot arise from finite rows (the terms are squares, the sum only grows).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"
#include "icp_search_device.h"

namespace icpgpu {
namespace {

constexpr int FK_BLOCK = 256, FK_WAVES = FK_BLOCK / 64;
constexpr int FK_BINS = kFeatureBins;
constexpr int FK_TILE = kFeatureTile;         // target rows per LDS tile
constexpr int FK_STRIDE = FK_TILE + 1;        // floats between two bins of the tile
constexpr int FK_QPW = 8;                     // queries a wave carries through the target set
constexpr int FK_QUERIES = FK_WAVES * FK_QPW; // queries per workgroup

__global__ __launch_bounds__(FK_BLOCK) void feature_finite_kernel(const float* __restrict__ feat, int n, int* __restrict__ finite) {
  const int r = blockIdx.x * FK_BLOCK + threadIdx.x;
  if (r >= n) return;
  const float* row = feat + (size_t)r * FK_BINS;
  bool ok = true;
  for (int b = 0; b < FK_BINS; ++b) ok = ok && isfinite(row[b]);
  finite[r] = ok ? 1 : 0;
}

__global__ __launch_bounds__(FK_BLOCK) void feature_knn_kernel(const float* __restrict__ target, const int* __restrict__ target_finite, int n_t,
                                                               const float* __restrict__ query, int n_q, int k, int32_t* __restrict__ idx,
                                                               float* __restrict__ d2, int32_t* __restrict__ n_found) {
  __shared__ float tile[FK_BINS * FK_STRIDE];
  const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const int q0 = blockIdx.x * FK_QUERIES + (int)wave * FK_QPW;

  // the wave's queries: value b of query j in lane b of qv[j]; a query past the end or with a non-finite component offers nothing
  float qv[FK_QPW];
  bool qok[FK_QPW];
  u64 keep[FK_QPW];
#pragma unroll
  for (int j = 0; j < FK_QPW; ++j) {
    const int q = q0 + j;
    float v = 0.f;
    if (q < n_q && lane < (unsigned int)FK_BINS) v = query[(size_t)q * FK_BINS + lane];
    qv[j] = v;
    const bool all_finite = __ballot(!isfinite(v)) == 0ull;
    qok[j] = q < n_q && all_finite;
    keep[j] = kEmptyKey;
  }

  for (int base = 0; base < n_t; base += FK_TILE) {
    __syncthreads();  // (the previous tile has been read)
    const size_t first = (size_t)base * FK_BINS, end = (size_t)n_t * FK_BINS;
    for (int e = (int)threadIdx.x; e < FK_TILE * FK_BINS; e += FK_BLOCK) {
      const int r = e / FK_BINS, b = e - r * FK_BINS;
      tile[b * FK_STRIDE + r] = first + (size_t)e < end ? target[first + (size_t)e] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int sub = 0; sub < FK_TILE; sub += 64) {
      if (base + sub >= n_t) break;  // (workgroup-uniform)
      const int r = sub + (int)lane, row = base + r;
      const bool have = row < n_t && target_finite[min(row, n_t - 1)] != 0;
      float acc[FK_QPW];
      {
        const float t = tile[r];
#pragma unroll
        for (int j = 0; j < FK_QPW; ++j) {
          const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv[j]), 0)) - t;
          acc[j] = d * d;
        }
      }
#pragma unroll
      for (int b = 1; b < FK_BINS; ++b) {
        const float t = tile[b * FK_STRIDE + r];
#pragma unroll
        for (int j = 0; j < FK_QPW; ++j) {
          const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv[j]), b)) - t;
          acc[j] = __builtin_fmaf(d, d, acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < FK_QPW; ++j) key_offer(have && qok[j] ? make_key(acc[j], (unsigned int)row) : kEmptyKey, keep[j], k, lane);
    }
  }

#pragma unroll
  for (int j = 0; j < FK_QPW; ++j)
    if (q0 + j < n_q) write_knn_row(keep[j], k, (size_t)(q0 + j), lane, idx, d2, n_found);  // (wave-uniform)
}

// ---- sample-consensus alignment --------------------------------------------------------------------------------------------------
constexpr int SCP_BLOCK = 256, SCP_WAVES = SCP_BLOCK / 64;
constexpr int SCP_WAVE_POINTS = 16;                              // consecutive source points a wave takes, in order
constexpr int SCP_BLOCK_POINTS = SCP_WAVES * SCP_WAVE_POINTS;
static_assert(SCP_BLOCK_POINTS == kScpBlockPoints, "icp_kernels.h states the points of a workgroup");

// splitmix64 of the rule's counter: draw c of hypothesis t, 2 nr draws per hypothesis
__device__ __forceinline__ unsigned int scp_draw(unsigned long long seed, unsigned long long t, unsigned int c, unsigned int nr, unsigned int range) {
  unsigned long long z = seed + ((unsigned long long)(2u * nr) * t + (unsigned long long)c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned int)(((z >> 32) * (unsigned long long)range) >> 32);
}

__global__ __launch_bounds__(SCP_BLOCK) void scp_sample_kernel(const float4* __restrict__ source, int n_s, const float4* __restrict__ cloud, int n,
                                                               const int32_t* __restrict__ rows, const int32_t* __restrict__ found, int kc,
                                                               unsigned long long seed, int t0, int m, int nr, float sim2,
                                                               int32_t* __restrict__ status, int32_t* __restrict__ sidx, int32_t* __restrict__ tidx,
                                                               double* __restrict__ sums) {
  const int e = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (e >= m) return;
  const unsigned long long t = (unsigned long long)(t0 + e);
  int s[kScpMaxSamples], g[kScpMaxSamples];
  float4 p[kScpMaxSamples], q[kScpMaxSamples];
  bool valid = n_s > 0;
#pragma unroll
  for (int c = 0; c < kScpMaxSamples; ++c) {
    s[c] = g[c] = -1;
    p[c] = q[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < nr && n_s > 0) {
      s[c] = (int)scp_draw(seed, t, (unsigned int)c, (unsigned int)nr, (unsigned int)n_s);
      const int mm = found[s[c]];
      if (mm > 0) {
        const int j = (int)scp_draw(seed, t, (unsigned int)(nr + c), (unsigned int)nr, (unsigned int)mm);
        g[c] = min(max(rows[(size_t)s[c] * kc + j], 0), n - 1);  // (the rows name target points)
        p[c] = source[s[c]];
        q[c] = cloud[g[c]];
        valid = valid && finite3(p[c].x, p[c].y, p[c].z) && finite3(q[c].x, q[c].y, q[c].z);
      } else {
        valid = false;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < kScpMaxSamples; ++a)
#pragma unroll
    for (int b = a + 1; b < kScpMaxSamples; ++b)
      if (b < nr && s[a] == s[b]) valid = false;
  int st = kScpInvalid;
  if (valid) {
    bool pass = true;
#pragma unroll
    for (int c = 0; c < kScpMaxSamples; ++c) {
      if (c < nr) {
        const int c1 = c + 1 < nr ? c + 1 : 0;
        float4 pa = p[0], qa = q[0];  // (c1 as a select chain: the arrays stay in registers)
#pragma unroll
        for (int u = 1; u < kScpMaxSamples; ++u)
          if (u == c1) pa = p[u], qa = q[u];
        const float ds = dist2(pa.x, pa.y, pa.z, p[c].x, p[c].y, p[c].z), dt = dist2(qa.x, qa.y, qa.z, q[c].x, q[c].y, q[c].z);
        const float lo = ds < dt ? ds : dt, hi = ds < dt ? dt : ds;
        const float ratio = lo / hi;
        pass = pass && ratio >= sim2;  // (a NaN -- 0 / 0, inf / inf -- fails)
      }
    }
    st = pass ? kScpEvaluated : kScpPrerejected;
    if (pass) {
      double acc[kReduceTerms];
#pragma unroll
      for (int a = 0; a < kReduceTerms; ++a) acc[a] = 0.0;
#pragma unroll
      for (int c = 0; c < kScpMaxSamples; ++c)
        if (c < nr) accumulate_pair(acc, p[c].x, p[c].y, p[c].z, q[c].x, q[c].y, q[c].z, 0.f);
#pragma unroll
      for (int a = 0; a < kReduceTerms; ++a) sums[(size_t)e * kReduceTerms + a] = acc[a];
    }
  }
  status[e] = st;
  for (int c = 0; c < nr; ++c) {
    int sc = -1, gc = -1;
#pragma unroll
    for (int u = 0; u < kScpMaxSamples; ++u)
      if (u == c) sc = s[u], gc = g[u];
    sidx[(size_t)e * nr + c] = sc;
    tidx[(size_t)e * nr + c] = gc;
  }
}

// the rule's fitness test for one source point (everything wave-uniform but the walk): true and d2 when the image of (x, y, z) under
// T has its nearest finite target point at d2 < r2
__device__ __forceinline__ bool scp_inlier(const Xform& T, float x, float y, float z, const float4* __restrict__ cloud, int n,
                                           const float4* __restrict__ sorted, const int* __restrict__ cell_start, const GridDesc& g, int R,
                                           const ScpBox& box, float r2, unsigned int lane, float& d2) {
  float4 p;
  xform_point(T, x, y, z, p.x, p.y, p.z);
  p.w = 1.f;
  if (!finite3(x, y, z) || !finite3(p.x, p.y, p.z)) return false;
  if (box.use && !(p.x >= box.lo[0] && p.x <= box.hi[0] && p.y >= box.lo[1] && p.y <= box.hi[1] && p.z >= box.lo[2] && p.z <= box.hi[2])) return false;
  u64 best = kEmptyKey;
  ball_batches(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) { best = key_min(best, key); });
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) best = key_min(best, shfl_xor_key(best, j));
  if (!key_in_ball(best, r2)) return false;
  d2 = __uint_as_float((unsigned int)(best >> 32));
  return true;
}

// partials[blockIdx.x * kScpBatch + blockIdx.y]: the workgroup's count and double-double sum for hypothesis xforms[blockIdx.y]
__global__ __launch_bounds__(SCP_BLOCK) void scp_eval_kernel(const float4* __restrict__ source, int n_s, const Xform* __restrict__ xforms,
                                                             const float4* __restrict__ cloud, int n, const float4* __restrict__ sorted,
                                                             const int* __restrict__ cell_start, GridDesc g, int R, ScpBox box, float r2,
                                                             ScpPartial* __restrict__ partials) {
  __shared__ ScpPartial wsum[SCP_WAVES];
  const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const Xform T = xforms[blockIdx.y];
  const int first = (int)blockIdx.x * SCP_BLOCK_POINTS + (int)wave * SCP_WAVE_POINTS, last = min(first + SCP_WAVE_POINTS, n_s);
  long long count = 0;
  DD acc;
  acc.hi = acc.lo = 0.0;
  for (int i = first; i < last; ++i) {  // (wave-uniform)
    const float4 s = source[i];
    float d2;
    if (scp_inlier(T, s.x, s.y, s.z, cloud, n, sorted, cell_start, g, R, box, r2, lane, d2)) {
      ++count;
      dd_add_term(acc, (double)d2);
    }
  }
  if (lane == 0) wsum[wave].count = count, wsum[wave].hi = acc.hi, wsum[wave].lo = acc.lo;
  __syncthreads();
  if (threadIdx.x == 0) {
    ScpPartial out = wsum[0];
    for (int w = 1; w < SCP_WAVES; ++w) {
      DD a, b;
      a.hi = out.hi, a.lo = out.lo, b.hi = wsum[w].hi, b.lo = wsum[w].lo;
      const DD r = dd_add(a, b);
      out.hi = r.hi, out.lo = r.lo, out.count += wsum[w].count;
    }
    partials[(size_t)blockIdx.x * kScpBatch + blockIdx.y] = out;
  }
}

// results[h] = {count, S} of hypothesis h of the batch: the workgroups' partials folded in workgroup order
__global__ __launch_bounds__(kScpBatch) void scp_fold_kernel(const ScpPartial* __restrict__ partials, int blocks, int n_h, ScpResult* __restrict__ results) {
  const int h = (int)threadIdx.x;
  if (h >= n_h) return;
  DD acc;
  acc.hi = acc.lo = 0.0;
  long long count = 0;
  for (int b = 0; b < blocks; ++b) {
    const ScpPartial p = partials[(size_t)b * kScpBatch + h];
    DD t;
    t.hi = p.hi, t.lo = p.lo;
    acc = dd_add(acc, t);
    count += p.count;
  }
  results[h].count = count;
  results[h].sum = acc.hi + acc.lo;
}

// flags[i] = 1 where source point i is an inlier of T: a wave per point, the evaluation's test
__global__ __launch_bounds__(SCP_BLOCK) void scp_flag_kernel(const float4* __restrict__ source, int n_s, Xform T, const float4* __restrict__ cloud, int n,
                                                             const float4* __restrict__ sorted, const int* __restrict__ cell_start, GridDesc g, int R,
                                                             ScpBox box, float r2, int* __restrict__ flags) {
  const unsigned int lane = threadIdx.x & 63u;
  const int i = (int)blockIdx.x * SCP_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n_s) return;  // (wave-uniform)
  const float4 s = source[i];
  float d2;
  const bool in = scp_inlier(T, s.x, s.y, s.z, cloud, n, sorted, cell_start, g, R, box, r2, lane, d2);
  if (lane == 0) flags[i] = in ? 1 : 0;
}

}  // namespace

hipError_t launch_feature_knn(const float* target, int n_t, const float* query, int n_q, int k, int* target_finite, int32_t* idx, float* d2,
                              int32_t* n_found, hipStream_t stream) {
  if (n_q <= 0) return hipSuccess;
  if (k < 1 || k > 64 || n_t < 0) return hipErrorInvalidValue;
  if (n_t > 0) hipLaunchKernelGGL(feature_finite_kernel, dim3((n_t + FK_BLOCK - 1) / FK_BLOCK), dim3(FK_BLOCK), 0, stream, target, n_t, target_finite);
  hipLaunchKernelGGL(feature_knn_kernel, dim3((n_q + FK_QUERIES - 1) / FK_QUERIES), dim3(FK_BLOCK), 0, stream, target, target_finite, n_t, query, n_q,
                     k, idx, d2, n_found);
  return hipGetLastError();
}

hipError_t launch_scp_sample(const float4* source, int n_s, const float4* cloud, int n, const int32_t* rows, const int32_t* found, int kc,
                             unsigned long long seed, int t0, int m, int nr, float sim2, int32_t* status, int32_t* sidx, int32_t* tidx, double* sums,
                             hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  if (nr < 3 || nr > kScpMaxSamples || kc < 1 || m > kScpChunk) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scp_sample_kernel, dim3((m + SCP_BLOCK - 1) / SCP_BLOCK), dim3(SCP_BLOCK), 0, stream, source, n_s, cloud, n, rows, found, kc, seed, t0,
                     m, nr, sim2, status, sidx, tidx, sums);
  return hipGetLastError();
}

int scp_eval_blocks(int n_s) { return (n_s + kScpBlockPoints - 1) / kScpBlockPoints; }

hipError_t launch_scp_eval(const float4* source, int n_s, const Xform* xforms, int n_h, const float4* cloud, int n, const float4* sorted,
                           const int* cell_start, const GridDesc& g, int shells, const ScpBox& box, float r2, ScpPartial* partials, ScpResult* results,
                           hipStream_t stream) {
  if (n_h <= 0) return hipSuccess;
  if (n_h > kScpBatch || n_s <= 0) return hipErrorInvalidValue;
  const int blocks = scp_eval_blocks(n_s);
  hipLaunchKernelGGL(scp_eval_kernel, dim3(blocks, n_h), dim3(SCP_BLOCK), 0, stream, source, n_s, xforms, cloud, n, sorted, cell_start, g, shells, box, r2,
                     partials);
  hipLaunchKernelGGL(scp_fold_kernel, dim3(1), dim3(kScpBatch), 0, stream, partials, blocks, n_h, results);
  return hipGetLastError();
}

hipError_t launch_scp_select(const float4* source, int n_s, const Xform& T, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                             const GridDesc& g, int shells, const ScpBox& box, float r2, int* flags, int* pos, int* scan_scratch, int* inliers,
                             int* n_inliers, hipStream_t stream) {
  if (n_s <= 0) return hipSuccess;
  hipLaunchKernelGGL(scp_flag_kernel, dim3((n_s + SCP_WAVES - 1) / SCP_WAVES), dim3(SCP_BLOCK), 0, stream, source, n_s, T, cloud, n, sorted, cell_start, g,
                     shells, box, r2, flags);
  return launch_compact(flags, n_s, pos, scan_scratch, inliers, n_inliers, nullptr, nullptr, stream);
}

}  // namespace icpgpu
