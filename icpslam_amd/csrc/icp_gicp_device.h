// icp_gicp_device.h -- what one GICP evaluation is made of, shared by the evaluation kernels (icp_gicp.hip) and the device
// solver (icp_gicp_solve_device.h) (internal): the accumulator of a lane, a lane's four correspondences, the workgroup
// reduction, and the granule helpers.
#pragma once

#include <hip/hip_runtime.h>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

// ---- one BFGS evaluation ---------------------------------------------------------------------------------------
// terms: 0 = m, 1 = sum r^T M r, 2..4 = sum M r, 5..13 = sum (base p)(M r)^T (row-major), 14 = sum d2 of the NN sweep
// ---- order-independent sums ----------------------------------------------------------------------------------------
// BFGS is a chaotic consumer: one ulp in a cost or gradient sum can change a line-search decision, and the outer loop's
// delta < 1 stop sits on a 1e-6 m threshold.  With plain float64 sums the GPU (per-lane partial sums, trees) and the
// oracle (one sequential sum, like PCL) agreed to the last bit on most pairs but ended up to 6 cm apart on 2 % of 1 000
// random pairs (scripts/gicp_campaign.py).  So the 13 real sums of an evaluation (f, g_t, R) are accumulated as
// double-double numbers everywhere -- error-free TwoSum per term in the lane, double-double adds across lanes, waves,
// workgroups and on the host; the oracle keeps a three-fold expansion over its sequential loop -- and rounded to
// float64 once at the end.  Either way the result is the correctly rounded exact sum unless that sum lies within
// ~1e-30 (relative to the sum of magnitudes) of a rounding boundary: the order of summation no longer matters.
// (DD, two_sum, dd_add_term, dd_add: icp_dd.h)

// Sixteen double-double numbers added as a BALANCED TREE (depth 4) rather than one after the other: the same fifteen additions,
// but four dependent ones instead of fifteen -- a dependent float64 operation costs a wave 8-10 cycles, an independent one 4
// (round 4: a workgroup's two reduction stages 1.55 -> 0.9 us).  The order of these additions does not matter to the result (the
// sums are exact to ~1e-30: see above), which is what makes them comparable bit for bit with the oracle in the first place.
__host__ __device__ __forceinline__ DD dd_sum16(const DD* x) {
  DD a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = dd_add(x[2 * i], x[2 * i + 1]);
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = dd_add(a[2 * i], a[2 * i + 1]);
  a[0] = dd_add(a[0], a[1]);
  a[1] = dd_add(a[2], a[3]);
  return dd_add(a[0], a[1]);
}

constexpr int kGicpSums = 13;  // f, g_t(3), R(9): terms 1..13 of the layout above

struct GicpAcc {
  double m, d2;       // count and sum of the sweep's d2 (sums of floats: exact in float64 at these sizes)
  DD s[kGicpSums];
};

// Four correspondences of a lane (positions i0, i0 + stride, ...): everything an evaluation reads from memory.  Their loads
// are issued together: key -> (target point, Mahalanobis matrix) is a dependent chain of random reads, and one after the
// other they made the evaluation 14-16 us long (latency, not bandwidth).
struct GicpQuad {
  bool use[4];
  float d2[4];
  float4 s[4], q[4];
  double M[4][6];
};
__device__ __forceinline__ void gicp_load_quad(GicpQuad& L, int i0, int stride, const float4* __restrict__ src, int n_s,
                                               const float4* __restrict__ tgt, const unsigned long long* __restrict__ keys,
                                               float thr, const double* __restrict__ maha6) {
  unsigned long long key[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + u * stride;
    key[u] = i < n_s ? keys[i] : kEmptyKey;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = min(i0 + u * stride, n_s - 1);
    const unsigned int j = (unsigned int)key[u];
    L.d2[u] = __uint_as_float((unsigned int)(key[u] >> 32));
    L.use[u] = j != 0xFFFFFFFFu && L.d2[u] < thr;
    L.s[u] = src[i];
    L.q[u] = tgt[L.use[u] ? j : 0u];
#pragma unroll
    for (int k = 0; k < 6; ++k) L.M[u][k] = maha6[(size_t)i * 6 + k];
  }
}
__device__ __forceinline__ void gicp_add_quad(GicpAcc& acc, const GicpQuad& L, const Xform& T, const Xform& base) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (!L.use[u]) continue;
    const float4 s = L.s[u], q = L.q[u];
    float px, py, pz, bx, by, bz;
    xform_point(T, s.x, s.y, s.z, px, py, pz);
    xform_point(base, s.x, s.y, s.z, bx, by, bz);
    const double r0 = (double)(px - q.x), r1 = (double)(py - q.y), r2 = (double)(pz - q.z);
    const double t0 = L.M[u][0] * r0 + L.M[u][1] * r1 + L.M[u][2] * r2;
    const double t1 = L.M[u][1] * r0 + L.M[u][3] * r1 + L.M[u][4] * r2;
    const double t2 = L.M[u][2] * r0 + L.M[u][4] * r1 + L.M[u][5] * r2;
    acc.m += 1.0;
    dd_add_term(acc.s[0], r0 * t0 + r1 * t1 + r2 * t2);
    dd_add_term(acc.s[1], t0);
    dd_add_term(acc.s[2], t1);
    dd_add_term(acc.s[3], t2);
    const double pb[3] = {(double)bx, (double)by, (double)bz};
    const double tt[3] = {t0, t1, t2};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) dd_add_term(acc.s[4 + 3 * r + c], pb[r] * tt[c]);
    acc.d2 += (double)L.d2[u];
  }
}
__device__ __forceinline__ void gicp_clear(GicpAcc& acc) {
  acc.m = acc.d2 = 0.0;
#pragma unroll
  for (int k = 0; k < kGicpSums; ++k) acc.s[k].hi = acc.s[k].lo = 0.0;
}

__device__ __forceinline__ void gicp_accumulate(GicpAcc& acc, const float4* __restrict__ src, int n_s,
                                                const float4* __restrict__ tgt,
                                                const unsigned long long* __restrict__ keys, float thr, const Xform& T,
                                                const Xform& base, const double* __restrict__ maha6, int wid = (int)blockIdx.x,
                                                int nw = (int)gridDim.x) {
  gicp_clear(acc);
  const int stride = nw * 256;
  for (int i0 = wid * 256 + threadIdx.x; i0 < n_s; i0 += 4 * stride) {
    GicpQuad L;
    gicp_load_quad(L, i0, stride, src, n_s, tgt, keys, thr, maha6);
    gicp_add_quad(acc, L, T, base);
  }
}

// Workgroup reduction of the lanes' accumulators into partials[block * kGicpPartialStride + ...] as four 64-byte ANSWER LINES of
// seven values + one tag (word 8 L + 7): value 0 = m, 1..13 = the sums' high parts, 14 = sum d2, 15..27 = their low parts.  The 13 double-double sums go through LDS: thread
// (sum, chunk) adds the 16 lanes of its chunk in lane order, then thread `sum` adds the 16 chunk results in order.
// md (nullable): the workgroup's m and sum d2 from an EARLIER evaluation of the same correspondences (they do not depend on the
// state): md[2] != 0 means md[0], md[1] are valid and the two wave reductions (twelve dependent cross-lane steps) are skipped;
// otherwise they are computed and left there (thread kGicpSums keeps them).
__device__ __forceinline__ void gicp_block_reduce_store(const GicpAcc& acc, double* __restrict__ partials, unsigned long long tag,
                                                        double* md = nullptr) {
  __shared__ DD s_lane[kGicpSums][16][17];  // [sum][lane % 16][lane / 16], rows padded: neither the writes (a lane per
                                            // thread) nor the reads (a chunk per thread) pile up on one LDS bank
  __shared__ DD s_chunk[kGicpSums][16];
  __shared__ double s_md[2][4];
#pragma unroll
  for (int k = 0; k < kGicpSums; ++k) s_lane[k][threadIdx.x & 15][threadIdx.x >> 4] = acc.s[k];
  const bool have_md = md && md[2] != 0.0;  // (workgroup-uniform: every thread holds the same flag)
  if (!have_md) {
    const double m = wave_sum(acc.m), d2 = wave_sum(acc.d2);
    if ((threadIdx.x & 63) == 0) {
      s_md[0][threadIdx.x >> 6] = m;
      s_md[1][threadIdx.x >> 6] = d2;
    }
  }
  __syncthreads();
  if (threadIdx.x < kGicpSums * 16) {
    const int k = threadIdx.x >> 4, c = threadIdx.x & 15;
    DD x[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) x[l] = s_lane[k][l][c];  // lanes 16c .. 16c+15, in lane order; 16 independent reads, then the tree
    const DD v = dd_sum16(x);
    s_chunk[k][c] = v;
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * kGicpPartialStride;
  if (threadIdx.x < 64) {
    // wave 0: lane s < 13 adds the chunks of sum s, lane 13 has m and sum d2; then the 28 results are dealt out as four ANSWER
    // LINES of 64 bytes (icp_kernels.h: kGicpLine*): lanes 8 L .. 8 L + 6 hold values 7 L .. 7 L + 6, lane 8 L + 7 the line's tag =
    // (evaluation number << 24) | the XOR of the values' 24-bit folds, and ONE 8-byte store instruction of 32 lanes writes the
    // workgroup's whole answer -- four 64-byte requests towards the host where the 16-byte {value, tag} pairs of rounds 2-4
    // took seven (the answers of a run's workgroups reach the host over 1.2-2 us, the largest single item of an evaluation's
    // wall time, and the host's poll looks at 4 tags per workgroup instead of 28).  A line is valid or recognisably not in
    // whatever order its bytes become visible, exactly like a pair.
    DD v{0.0, 0.0};
    double m = 0.0, d2 = 0.0;
    if (threadIdx.x < kGicpSums) {
      DD x[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) x[c] = s_chunk[threadIdx.x][c];
      v = dd_sum16(x);
    } else if (threadIdx.x == kGicpSums) {
      m = have_md ? md[0] : (s_md[0][0] + s_md[0][1]) + (s_md[0][2] + s_md[0][3]);
      d2 = have_md ? md[1] : (s_md[1][0] + s_md[1][1]) + (s_md[1][2] + s_md[1][3]);
      if (md) {
        md[0] = m;
        md[1] = d2;
      }
    }
    const int lane = (int)threadIdx.x, pos = lane & 7;
    const int slot = 7 * (lane >> 3) + pos;  // value number (pos < 7): 0 = m, 1..13 = high parts, 14 = sum d2, 15..27 = low parts
    const double from_hi = __shfl(v.hi, min(max(slot - 1, 0), kGicpSums - 1), 64), from_lo = __shfl(v.lo, min(max(slot - 15, 0), kGicpSums - 1), 64);
    const double from_m = __shfl(m, kGicpSums, 64), from_d2 = __shfl(d2, kGicpSums, 64);
    const double value = slot == 0 ? from_m : slot <= 13 ? from_hi : slot == 14 ? from_d2 : from_lo;
    const unsigned long long bits = pos < 7 ? (unsigned long long)__double_as_longlong(value) : 0ull;
    unsigned int fold = (unsigned int)((bits ^ (bits >> 24) ^ (bits >> 48)) & 0xFFFFFFull);
    fold ^= (unsigned int)__shfl_xor((int)fold, 1, 64);
    fold ^= (unsigned int)__shfl_xor((int)fold, 2, 64);
    fold ^= (unsigned int)__shfl_xor((int)fold, 4, 64);  // every lane of the line: the XOR of its seven folds
    const unsigned long long word = pos < 7 ? bits : (((tag & ~kMailboxReleaseBit) << 24) | (unsigned long long)fold);
    unsigned long long* w = reinterpret_cast<unsigned long long*>(out) + lane;
    // (ASSUMPTION of the classic form, gfx9 hardware rather than the HIP memory model: the values of a line are stored by lanes
    //  8 L .. 8 L + 6 and its tag by lane 8 L + 7 of the SAME wave; a release fence is executed wave-wide on this hardware
    //  (s_waitcnt + write-back), so the tag lane's release also orders the other lanes' stores.  The model only promises that for
    //  the storing lane itself.  The default form below does not depend on it -- a line carries its own checksum -- and
    //  tests/test_gpu_mailbox.py runs both forms against each other.)
    if (tag & kMailboxReleaseBit) {  // the classic form: values, system-scope release, tags
      if (lane < 8 * kGicpLines && pos < 7) __hip_atomic_store(w, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __atomic_thread_fence(__ATOMIC_RELEASE);
      if (lane < 8 * kGicpLines && pos == 7) __hip_atomic_store(w, word, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if (lane < 8 * kGicpLines) {
      __hip_atomic_store(w, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // written through to system memory (sc0 sc1)
    }
  }
  if (md) md[2] = 1.0;
}

// ---- granules: {value, tag} pairs that validate themselves (icp_kernels.h: mailbox_tag) -----------------------------------------
__device__ __forceinline__ unsigned long long granule_tag(unsigned long long seq, unsigned long long bits) { return mailbox_tag(seq, bits); }
__device__ __forceinline__ void granule_store(unsigned long long* g, double value, unsigned long long seq) {
  store_result_pair(g, (unsigned long long)__double_as_longlong(value), seq);   // (host-visible results: seq may carry the release bit)
}

}  // namespace
}  // namespace icpgpu
