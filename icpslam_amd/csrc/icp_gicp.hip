// icp_gicp.hip -- ONE evaluation of the GICP mode's cost and the server that answers them:
// what pcl::GeneralizedIterativeClosestPoint does per correspondence.  (computeCovariances: icp_gicp_cov.hip; the BFGS run on
// the device: icp_gicp_solve_device.h and the icp_gicp_solve*.hip units; what they share: icp_gicp_device.h.)
//
//   gicp_maha_kernel       per accepted correspondence (d2 < r^2, strict): M_i = (C_t[j] + R C_s[i] R^T)^-1, symmetric 6.
//   gicp_cost_kernel       one BFGS function/gradient evaluation: sum over correspondences of r^T M r, M r and
//                          (base p)(M r)^T with r = T(x) p - q -- 14 float64 terms, fixed-order two-stage reduction.
//                          HBM-bound: 16 B source + 8 B key + 16 B gathered target + 48 B M per correspondence.
//   gicp_quadratic_kernel  the cost of an outer iteration as a quadratic form in the entries of T: one pass, 75 sums.
//   gicp_server_kernel     resident for a whole BFGS run: evaluations on command.
#include <math.h>

#include <cstdlib>
#include <cstring>

#include "icp_env.h"
#include "icp_device.h"
#include "icp_gicp_device.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

// ---- Mahalanobis matrices --------------------------------------------------------------------------------------
// M = (C_t + R C_s R^T)^-1 of one correspondence, upper triangle (a, b: the two covariances' upper triangles)
__device__ __forceinline__ void gicp_maha_of(const double* __restrict__ a, const double* __restrict__ b, const Rot3d& R, double* __restrict__ M) {
  const double C1[9] = {a[0], a[1], a[2], a[1], a[3], a[4], a[2], a[4], a[5]};
  double RC[9], S[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) RC[3 * r + c] = R.m[3 * r] * C1[c] + R.m[3 * r + 1] * C1[3 + c] + R.m[3 * r + 2] * C1[6 + c];
  const double C2[9] = {b[0], b[1], b[2], b[1], b[3], b[4], b[2], b[4], b[5]};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      S[3 * r + c] = RC[3 * r] * R.m[3 * c] + RC[3 * r + 1] * R.m[3 * c + 1] + RC[3 * r + 2] * R.m[3 * c + 2] + C2[3 * r + c];
  // inverse by adjugate; the result of inverting a (numerically) symmetric matrix is stored as its upper triangle
  const double c00 = S[4] * S[8] - S[5] * S[7], c01 = S[5] * S[6] - S[3] * S[8], c02 = S[3] * S[7] - S[4] * S[6];
  const double id = 1.0 / (S[0] * c00 + S[1] * c01 + S[2] * c02);
  M[0] = c00 * id;
  M[1] = (S[2] * S[7] - S[1] * S[8]) * id;
  M[2] = (S[1] * S[5] - S[2] * S[4]) * id;
  M[3] = (S[0] * S[8] - S[2] * S[6]) * id;
  M[4] = (S[2] * S[3] - S[0] * S[5]) * id;
  M[5] = (S[0] * S[4] - S[1] * S[3]) * id;
}

__global__ __launch_bounds__(256) void gicp_maha_kernel(int n_s, const unsigned long long* __restrict__ keys, float thr,
                                                        Rot3d R, const double* __restrict__ cov_s,
                                                        const double* __restrict__ cov_t, double* __restrict__ maha6) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_s) return;
  const unsigned long long key = keys[i];
  const unsigned int j = (unsigned int)key;
  const float d2 = __uint_as_float((unsigned int)(key >> 32));
  if (j == 0xFFFFFFFFu || !(d2 < thr)) return;
  gicp_maha_of(cov_s + (size_t)i * 6, cov_t + (size_t)j * 6, R, maha6 + (size_t)i * 6);
}

// One evaluation as ONE kernel of <= kGicpDirectBlocks workgroups: every workgroup stores its partials straight into
// host-mapped memory (host_partials) followed by host_flags[block] = seq; the host adds the workgroups' partials.  All
// the stores above come from wave 0, like the flag, so the release orders them.
__global__ __launch_bounds__(256) void gicp_cost_kernel(const float4* __restrict__ src, int n_s,
                                                        const float4* __restrict__ tgt,
                                                        const unsigned long long* __restrict__ keys, float thr, Xform T,
                                                        Xform base, const double* __restrict__ maha6,
                                                        double* __restrict__ partials, unsigned long long* flags,
                                                        unsigned long long seq) {
  GicpAcc acc;
  gicp_accumulate(acc, src, n_s, tgt, keys, thr, T, base, maha6);
  (void)flags;
  gicp_block_reduce_store(acc, partials, seq);
}

// ---- the quadratic form of an outer iteration (icp_gicp_quadratic.h) ------------------------------------------------------------
// ONE pass over the correspondences per outer iteration instead of one per BFGS evaluation: the 73 coefficient sums of the cost as
// a quadratic form in the entries of T, plus m and sum d2 -- sum number n of kGicpQuadSums:
//   n = pair(e, e') * 6 + tri(c, d)   sum p~_e p~_e' M_cd     (pairs e <= e' of p~ = (p.x, p.y, p.z, 1); M's upper triangle)   0..59
//   n = 60 + e * 3 + c                 sum p~_e (M q)_c                                                                       60..71
//   n = 72                             sum q^T M q                                 n = 73: m (count)        n = 74: sum d2
// The Mahalanobis matrix of a correspondence is computed here (gicp_maha_of: the operations of gicp_maha_kernel) and never stored.
// Every sum is an exact double-double sum of its float64 terms, like the sums of an evaluation.  A thread keeps its first
// correspondence in registers and walks the sums thirteen at a time (the workgroup reduction's LDS tile holds thirteen), so clouds
// up to 256 x gridDim.x points -- the reference's voxel-filtered scans -- read their inputs once.
struct QuadPoint {
  bool use;
  double p[4], q[3], M[6], Mq[3], cq, d2;
};
__device__ __forceinline__ void quad_point_load(QuadPoint& P, int i, const float4* __restrict__ src, const float4* __restrict__ tgt,
                                                const unsigned long long* __restrict__ keys, float thr, const Rot3d& R,
                                                const double* __restrict__ cov_s, const double* __restrict__ cov_t) {
  const unsigned long long key = keys[i];
  const unsigned int j = (unsigned int)key;
  const float d2 = __uint_as_float((unsigned int)(key >> 32));
  P.use = j != 0xFFFFFFFFu && d2 < thr;
  if (!P.use) return;
  const float4 s = src[i], q = tgt[j];
  gicp_maha_of(cov_s + (size_t)i * 6, cov_t + (size_t)j * 6, R, P.M);
  P.p[0] = (double)s.x; P.p[1] = (double)s.y; P.p[2] = (double)s.z; P.p[3] = 1.0;
  P.q[0] = (double)q.x; P.q[1] = (double)q.y; P.q[2] = (double)q.z;
  P.Mq[0] = P.M[0] * P.q[0] + P.M[1] * P.q[1] + P.M[2] * P.q[2];
  P.Mq[1] = P.M[1] * P.q[0] + P.M[3] * P.q[1] + P.M[4] * P.q[2];
  P.Mq[2] = P.M[2] * P.q[0] + P.M[4] * P.q[1] + P.M[5] * P.q[2];
  P.cq = P.q[0] * P.Mq[0] + P.q[1] * P.Mq[1] + P.q[2] * P.Mq[2];
  P.d2 = (double)d2;
}
template <int N>
__device__ __forceinline__ double quad_term(const QuadPoint& P) {  // term N of one correspondence
  if constexpr (N < 60) {
    constexpr int pair = N / 6, k = N % 6;
    constexpr int e = pair < 4 ? 0 : pair < 7 ? 1 : pair < 9 ? 2 : 3;
    constexpr int f = pair < 4 ? pair : pair < 7 ? pair - 3 : pair < 9 ? pair - 5 : 3;
    return (P.p[e] * P.p[f]) * P.M[k];  // the product of two floats is exact
  } else if constexpr (N < 72) {
    return P.p[(N - 60) / 3] * P.Mq[(N - 60) % 3];
  } else if constexpr (N == 72) {
    return P.cq;
  } else if constexpr (N == 73) {
    return 1.0;
  } else {
    return P.d2;
  }
}
template <int G, int K>
__device__ __forceinline__ void quad_set_group(DD (&acc)[13], const QuadPoint& P) {  // acc = the terms of a lane's FIRST correspondence
  if constexpr (K < 13 && 13 * G + K < kGicpQuadSums) {
    acc[K].hi = quad_term<13 * G + K>(P);
    quad_set_group<G, K + 1>(acc, P);
  }
}
template <int G, int K>
__device__ __forceinline__ void quad_add_group(DD (&acc)[13], const QuadPoint& P) {
  if constexpr (K < 13 && 13 * G + K < kGicpQuadSums) {
    dd_add_term(acc[K], quad_term<13 * G + K>(P));
    quad_add_group<G, K + 1>(acc, P);
  }
}
// partials[block][kGicpQuadSums] (DD); the last workgroup to finish adds the workgroups' partials and publishes the kGicpQuadSums
// (hi, lo) pairs as 2 x kGicpQuadSums result pairs numbered seq in host_out (gicp_granule_read on the host)
template <int G>
__device__ __forceinline__ void quad_group(const QuadPoint& mine, const QuadPoint& mine2, int i_next, int stride, const float4* __restrict__ src, int n_s,
                                           const float4* __restrict__ tgt, const unsigned long long* __restrict__ keys, float thr,
                                           const Rot3d& R, const double* __restrict__ cov_s, const double* __restrict__ cov_t,
                                           DD* __restrict__ out, DD (*s_lane)[16][17], DD (*s_chunk)[16]) {
  DD acc[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) acc[k].hi = acc[k].lo = 0.0;
  if (mine.use) quad_set_group<G, 0>(acc, mine);  // (0 + t by TwoSum is t, seven operations later)
  if (mine2.use) quad_add_group<G, 0>(acc, mine2);
  for (int i = i_next; i < n_s; i += stride) {  // larger clouds: the further correspondences of this lane, read again per group
    QuadPoint P;
    quad_point_load(P, i, src, tgt, keys, thr, R, cov_s, cov_t);
    if (P.use) quad_add_group<G, 0>(acc, P);
  }
#pragma unroll
  for (int k = 0; k < 13; ++k) s_lane[k][threadIdx.x & 15][threadIdx.x >> 4] = acc[k];
  __syncthreads();
  if (threadIdx.x < 13 * 16) {
    const int k = threadIdx.x >> 4, c = threadIdx.x & 15;
    DD x[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) x[l] = s_lane[k][l][c];
    s_chunk[k][c] = dd_sum16(x);
  }
  __syncthreads();
  if (threadIdx.x < 13 && 13 * G + (int)threadIdx.x < kGicpQuadSums) {
    DD x[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = s_chunk[threadIdx.x][c];
    out[13 * G + threadIdx.x] = dd_sum16(x);
  }
  // (the next group's writes to s_lane come behind this group's second barrier, its writes to s_chunk behind its own first one)
}
__global__ __launch_bounds__(256) void gicp_quadratic_kernel(const float4* __restrict__ src, int n_s, const float4* __restrict__ tgt,
                                                             const unsigned long long* __restrict__ keys, float thr, Rot3d R,
                                                             const double* __restrict__ cov_s, const double* __restrict__ cov_t,
                                                             DD* __restrict__ partials, unsigned int* __restrict__ done,
                                                             unsigned long long* __restrict__ host_out, unsigned long long seq, int stamps) {
  // stamps (development flavour, ICPGPU_GICP_TIMING): the LAST workgroup's 100 MHz clock at six points, as result pairs behind the sums
  const long long st0 = stamps ? (long long)wall_clock64() : 0;
  __shared__ DD s_lane[13][16][17];
  __shared__ DD s_chunk[13][16];
  __shared__ bool s_last;
  const int stride = (int)gridDim.x * 256, i0 = (int)blockIdx.x * 256 + (int)threadIdx.x;
  QuadPoint mine, mine2;  // the lane's first two correspondences stay in registers (half as many workgroups to add up at the end)
  mine.use = mine2.use = false;
  if (i0 < n_s) quad_point_load(mine, i0, src, tgt, keys, thr, R, cov_s, cov_t);
  if (i0 + stride < n_s) quad_point_load(mine2, i0 + stride, src, tgt, keys, thr, R, cov_s, cov_t);
  DD* out = partials + (size_t)blockIdx.x * kGicpQuadSums;
  const long long st1 = stamps ? (long long)wall_clock64() : 0;
  quad_group<0>(mine, mine2, i0 + 2 * stride, stride, src, n_s, tgt, keys, thr, R, cov_s, cov_t, out, s_lane, s_chunk);
  quad_group<1>(mine, mine2, i0 + 2 * stride, stride, src, n_s, tgt, keys, thr, R, cov_s, cov_t, out, s_lane, s_chunk);
  quad_group<2>(mine, mine2, i0 + 2 * stride, stride, src, n_s, tgt, keys, thr, R, cov_s, cov_t, out, s_lane, s_chunk);
  quad_group<3>(mine, mine2, i0 + 2 * stride, stride, src, n_s, tgt, keys, thr, R, cov_s, cov_t, out, s_lane, s_chunk);
  quad_group<4>(mine, mine2, i0 + 2 * stride, stride, src, n_s, tgt, keys, thr, R, cov_s, cov_t, out, s_lane, s_chunk);
  quad_group<5>(mine, mine2, i0 + 2 * stride, stride, src, n_s, tgt, keys, thr, R, cov_s, cov_t, out, s_lane, s_chunk);
  // the last workgroup to get here adds everybody's partials (device-scope release / acquire around the counter)
  const long long st2 = stamps ? (long long)wall_clock64() : 0;
  // (every global store of this workgroup came from threads 0..12 -- wave 0, the wave of thread 0 -- so the counter's RELEASE orders
  //  them by itself: one wave's write-back instead of a fence in all four and a barrier, 3.3 -> ~1.5 us on the last workgroup's path)
  //  Since round 6 the storing lanes say so themselves: an agent-scope release fence in wave 0 (all of its lanes: the fence is
  //  wave-wide on this hardware anyway, and the memory model orders a lane's stores only behind that lane's own release), then
  //  the counter -- ADVICE r5; one more write-back of an already clean wave.)
  if (threadIdx.x < 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();  // (no instruction: the lanes of a wave are in step; it marks the wavefront-scope hand-over to lane 0)
  }
  if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every wave of the last workgroup: its loads below must not be served from stale lines
  const long long st3 = stamps ? (long long)wall_clock64() : 0;
  if (threadIdx.x == 0) *done = 0u;  // ready for the next launch (launches of one context are ordered by its stream)
  // three threads per sum, each over a third of the workgroups, sixteen loads in flight (one load after the other -- 89 workgroups
  // for a voxel-filtered scan at first -- made this tail ~60 us long: every load a trip to L2 and back before the next one left)
  __shared__ DD s_fin[3][kGicpQuadSums];
  const int slice = (int)threadIdx.x / kGicpQuadSums, k = (int)threadIdx.x % kGicpQuadSums, nb = (int)gridDim.x;
  if (slice < 3) {
    DD a{0.0, 0.0};
    for (int b0 = slice; b0 < nb; b0 += 3 * 16) {  // sixteen loads in flight: a voxel-filtered scan's 45 workgroups in ONE trip
      DD v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int bb = b0 + 3 * u;
        v[u] = bb < nb ? partials[(size_t)bb * kGicpQuadSums + k] : DD{0.0, 0.0};
      }
      a = dd_add(a, dd_sum16(v));
    }
    s_fin[slice][k] = a;
  }
  __syncthreads();
  const long long st4 = stamps ? (long long)wall_clock64() : 0;
  if (stamps && threadIdx.x == 255) {
    const long long t[5] = {st0, st1, st2, st3, st4};
    for (int u = 0; u < 5; ++u) store_result_pair(host_out + 2 * (2 * kGicpQuadSums + u), (unsigned long long)t[u], seq);
  }
  if (threadIdx.x < kGicpQuadSums) {
    const DD a = dd_add(dd_add(s_fin[0][k], s_fin[1][k]), s_fin[2][k]);
    store_result_pair(host_out + 2 * (2 * threadIdx.x), (unsigned long long)__double_as_longlong(a.hi), seq);
    store_result_pair(host_out + 2 * (2 * threadIdx.x + 1), (unsigned long long)__double_as_longlong(a.lo), seq);
  }
}

// ---- resident evaluation server ------------------------------------------------------------------------------------
// A BFGS run is ~35 DEPENDENT evaluations of a few microseconds of work each; launched one by one they cost 11 us apiece,
// most of it launch and dispatch latency.  This kernel stays resident for the whole run instead (<= kGicpDirectBlocks
// workgroups, all co-resident by construction).  The command line -- 12 floats of T, then a sequence number -- lives in
// FINE-GRAINED DEVICE memory that the host writes through the PCIe BAR (posted writes, delivered in order: the number is
// written last, behind a store fence), so every workgroup polls it locally: a poll is an uncached read of HBM, not a PCIe
// round trip (polling a line in HOST memory from one workgroup and relaying it through device memory with release /
// acquire fences was measured first: 13 us per evaluation, slower than a launch).  Every workgroup then evaluates its
// share and stores its 17 partials + flag into the host mailbox exactly like gicp_cost_kernel's direct mode.  Sequence
// number kGicpServerExit ends the run; so does 50 ms without a command (the host fell asleep or died: never leave a
// spinning kernel behind -- the host notices the idle stream and goes back to single launches).
template <bool RESIDENT>
__global__ __launch_bounds__(256) void gicp_server_kernel(const float4* __restrict__ src, int n_s,
                                                          const float4* __restrict__ tgt,
                                                          const unsigned long long* __restrict__ keys, float thr, Xform base,
                                                          const double* __restrict__ maha6, double* __restrict__ host_partials,
                                                          unsigned long long* host_flags, unsigned int* cmd,
                                                          unsigned int first_seq, unsigned int seq_hi, int stamps) {
  __shared__ Xform s_T;
  __shared__ unsigned int s_seq;
  __shared__ long long s_seen;
  __shared__ unsigned int s_polls;
  const long long patience = 5000000;  // 50 ms of the 100 MHz wall clock
  unsigned int expect = first_seq;
  // RESIDENT (small problems: every lane's share is one quad): the correspondences do not change during a run, so they are
  // read ONCE and stay in registers -- an evaluation then starts without the key -> (target point, matrix) chain of reads.
  // (298 registers, one wave per SIMD.  Measured twice: slower at 200k points while every evaluation also paid a system-scope
  // release, 9-11 % faster at every size from 5k to 200k once the results travelled as self-tagged pairs.)
  GicpQuad mine;
  if constexpr (RESIDENT) gicp_load_quad(mine, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, src, n_s, tgt, keys, thr, maha6);
  double md[3] = {0.0, 0.0, 0.0};  // this workgroup's m and sum d2: the same at every evaluation of the run
  for (;;) {
    const long long t_loop = (long long)wall_clock64();
    if (threadIdx.x < 64) {
      // lane k < 13 reads word k of the line, all in ONE coalesced read per poll (the line is uncached: every load reads
      // memory).  The words of T were posted before the number, so a read that returns the number returns them too.
      unsigned int got = kGicpServerExit, word = 0u;
      const long long t0 = (long long)wall_clock64();
      // (One read in flight, 0.18 us each.  Four -- a hand-written loop behind s_waitcnt vmcnt(3) -- were measured in round 4 and
      // made an evaluation SLOWER, 8.3 instead of 7.1 us.  Round 5, the other direction: an s_sleep of 128 / 384 clocks between
      // polls changes nothing either, alone or with eight servers resident: profiles/r05_gicp_batch.txt.)
      const unsigned int* line = &cmd[threadIdx.x & 15];
      unsigned int polls_done = 0;
      for (unsigned int polls = 1;; ++polls) {
        polls_done = polls;
        word = __hip_atomic_load(line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned int v = (unsigned int)__builtin_amdgcn_readlane((int)word, 12);
        if (v == expect || v == kGicpServerExit) {
          got = v;
          break;
        }
        if ((polls & 15u) == 0 && (long long)wall_clock64() - t0 > patience) break;  // got stays kGicpServerExit
      }
      if (threadIdx.x < 12) s_T.m[threadIdx.x] = __uint_as_float(word);
      if (threadIdx.x == 12) {
        s_seq = got;
        s_seen = (long long)wall_clock64();
        s_polls = polls_done;
      }
    }
    __syncthreads();
    const unsigned int seq = s_seq;
    if (seq == kGicpServerExit) {
      // acknowledge: the host does not reuse the command line before this kernel has left
      if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(&host_flags[0], ~0ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    const Xform T = s_T;
    GicpAcc acc;
    if constexpr (RESIDENT) {
      gicp_clear(acc);
      gicp_add_quad(acc, mine, T, base);
    } else {
      gicp_accumulate(acc, src, n_s, tgt, keys, thr, T, base, maha6);
    }
    const long long t_acc = stamps ? (long long)wall_clock64() : 0;
    gicp_block_reduce_store(acc, host_partials, ((unsigned long long)seq_hi << 32) | seq, md);
    if (stamps && threadIdx.x == 0) {  // (development flavour, ICPGPU_GICP_TIMING: three spare entries of this workgroup's line; 100 MHz ticks)
      double* o = host_partials + (size_t)blockIdx.x * kGicpPartialStride;
      o[2 * 29] = (double)s_seen;                    // command seen
      o[2 * 30] = (double)t_acc;                     // its share accumulated
      o[2 * 31] = (double)(long long)wall_clock64(); // reduced, results on their way
      o[2 * 29 + 1] = (double)t_loop;                // started polling
      o[2 * 30 + 1] = (double)s_polls;               // reads of the command line it took
      {
        unsigned int xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        o[2 * 31 + 1] = (double)(xcc & 15u);         // the XCD it runs on
      }
    }
    expect = seq + 1u;
    if (expect == kGicpServerExit) expect = 0u;
    __syncthreads();  // s_T / s_seq are rewritten in the next round
  }
}

}  // namespace

hipError_t launch_gicp_mahalanobis(int n_s, const unsigned long long* keys, float thr, const Rot3d& R, const double* cov_s,
                                   const double* cov_t, double* maha6, hipStream_t stream) {
  if (n_s <= 0) return hipSuccess;
  hipLaunchKernelGGL(gicp_maha_kernel, dim3((n_s + 255) / 256), dim3(256), 0, stream, n_s, keys, thr, R, cov_s, cov_t, maha6);
  return hipGetLastError();
}

int gicp_quadratic_blocks(int n_s) {
  const int b = (n_s + 511) / 512;  // two correspondences per lane
  return b < 1 ? 1 : b > kGicpQuadBlocks ? kGicpQuadBlocks : b;
}
hipError_t launch_gicp_quadratic(const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                                 const Rot3d& R, const double* cov_s, const double* cov_t, double* partials, unsigned int* done,
                                 unsigned long long* host_out, unsigned long long seq, hipStream_t stream) {
  static const int stamps = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_GICP_TIMING"); return e && atoi(e) != 0 ? 1 : 0; }();
  hipLaunchKernelGGL(gicp_quadratic_kernel, dim3(gicp_quadratic_blocks(n_s)), dim3(256), 0, stream, src, n_s, tgt, keys, thr, R, cov_s,
                     cov_t, reinterpret_cast<DD*>(partials), done, host_out, seq, stamps);
  return hipGetLastError();
}

int gicp_direct_blocks(int n_s, int most) {
  // ICPGPU_GICP_BLOCKS (tuning): the most workgroups an evaluation may use.  64 until round 2; with one workgroup per 1024
  // points up to 256 a 200k x 200k registration takes 3.9 instead of 4.45 ms (12 instead of 15 us per evaluation: the
  // workgroups' share shrinks faster than the host's merge of their partial sums grows).  Keeping each lane's
  // correspondences in registers for the whole run of the server (gicp_server_kernel<true>) takes another 9-11 % off at
  // every size (launch_gicp_server picks it whenever a lane's share is one quad).
  static const int cap = [] {
    const char* e = ICPGPU_DEV_ENV("ICPGPU_GICP_BLOCKS");
    const int v = e ? std::atoi(e) : kGicpDirectBlocks;
    return v < 1 ? 1 : (v > kGicpDirectBlocks ? kGicpDirectBlocks : v);
  }();
  static const int per_block = [] {  // ICPGPU_GICP_PER_BLOCK (tuning): correspondences per workgroup of 256 lanes
    const char* e = ICPGPU_DEV_ENV("ICPGPU_GICP_PER_BLOCK");
    // 512 since round 6 (1024 before): two correspondences per lane halve a workgroup's accumulation (1.3 us of an evaluation's ~6),
    // and twice the answer lines cost the host little now that it validates and merges them as vectors -- the alignment stage of a
    // pipeline scan 1.24 -> 1.15 ms (256: 1.25, 384: 1.17, 640: 1.19, 768: 1.25; scripts/r6/perblock.sh).  The sums do not depend on
    // the split: they are exact sums rounded once.
    const int v = e ? std::atoi(e) : 512;
    return v < 256 ? 256 : (v > 4096 ? 4096 : v);
  }();
  int blocks = (n_s + per_block - 1) / per_block;
  if (blocks > cap) blocks = cap;
  if (blocks > most) blocks = most;  // (the caller's share of the chip: several contexts' servers must all be resident)
  if (blocks < 1) blocks = 1;
  return blocks;
}

hipError_t launch_gicp_cost_direct(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                                   const Xform& T, const Xform& base, const double* maha6, double* host_partials,
                                   unsigned long long* host_flags, unsigned long long seq, hipStream_t stream) {
  hipLaunchKernelGGL(gicp_cost_kernel, dim3(blocks), dim3(256), 0, stream, src, n_s, tgt, keys, thr, T, base,
                     maha6, host_partials, host_flags, seq);
  return hipGetLastError();
}

hipError_t launch_gicp_server(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                              const Xform& base, const double* maha6, double* host_partials, unsigned long long* host_flags,
                              unsigned int* cmd, unsigned int first_seq, unsigned int seq_hi, hipStream_t stream) {
  static const int stamps = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_GICP_TIMING"); return e && std::atoi(e) != 0 ? 1 : 0; }();
  // every lane's share fits one quad: up to 256 workgroups x 1024 points (ICPGPU_GICP_RESIDENT_MAX: tuning switch; 0 = never)
  static const int resident_max = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_GICP_RESIDENT_MAX"); return e ? std::atoi(e) : 262144; }();
  if ((long long)blocks * 1024 >= n_s && n_s <= resident_max)
    hipLaunchKernelGGL(gicp_server_kernel<true>, dim3(blocks), dim3(256), 0, stream, src, n_s, tgt, keys, thr, base, maha6,
                       host_partials, host_flags, cmd, first_seq, seq_hi, stamps);
  else
    hipLaunchKernelGGL(gicp_server_kernel<false>, dim3(blocks), dim3(256), 0, stream, src, n_s, tgt, keys, thr, base, maha6,
                       host_partials, host_flags, cmd, first_seq, seq_hi, stamps);
  return hipGetLastError();
}

// host side of a granule: true and the value if it carries number `seq` and its own checksum
bool gicp_granule_read(const volatile unsigned long long* g, unsigned long long seq, double* value) {
  unsigned long long bits;
  if (!mailbox_read(g, seq, &bits)) return false;
  std::memcpy(value, &bits, sizeof bits);
  return true;
}

}  // namespace icpgpu
