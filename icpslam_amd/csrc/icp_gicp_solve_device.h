// icp_gicp_solve_device.h -- the device solver of the GICP mode (internal): the body every solve kernel runs.  The units that
// instantiate its kernels: icp_gicp_solve.hip (the resident single-run variants), icp_gicp_solve_streamed.hip (shares larger than
// one quad per lane) and icp_gicp_solve_batch.hip (several runs in one launch).
//
// ---- the device solver (round 4) --------------------------------------------------------------------------------------------
// What the reference runs per scan (icp_odometer.cpp:188-198) is ~5 outer iterations of ~35 DEPENDENT cost evaluations each; with
// the BFGS on the host every one of them was a host <-> device round trip (7.6 us wall for 1.4 us of device work: 1.3 of the
// pipeline's 2.2 ms per scan).  gicp_solve_kernel runs the WHOLE inner minimisation of an outer iteration on the device: the
// host queues it behind the search and the Mahalanobis kernels and polls ONE result.
//
//   * Every workgroup holds its share of the correspondences in registers (RESIDENT; streamed from memory when the share is
//     larger than one quad per lane) and runs the SAME solver redundantly -- icp_gicp_solver_impl.h, the source the host
//     fallback instantiates: same operations, same order, correctly rounded sines and cosines (icp_trig.h), so every lane of
//     every workgroup takes the same decisions and the bits equal the host path's and the oracle's.
//   * One evaluation = one hop: each workgroup reduces its share (double-double, two LDS stages), PUBLISHES 28 granules --
//     {value, tag}, one 16-byte write-through store each, tag = evaluation number and a checksum of the value's bits, so a
//     granule is valid or recognisably not, whatever the order its halves become visible in -- into its slot of a fine-grained
//     device buffer, and wave 0 of EVERY workgroup GATHERS all slots (4 lanes per sum, every load of a round in flight at
//     once), merges them in double-double (order-independent to ~1e-30) and hands the 15 numbers to the workgroup through LDS.
//     There is no master and no command hop: the next state is computed everywhere at once.
//   * Slots are double-buffered by the evaluation number's parity: a workgroup can run at most one evaluation ahead of the
//     slowest one (it needs everybody's partials of evaluation k to start k + 1).
//   * Nobody waits for ever: 50 ms without a granule ends the run with kDeviceError everywhere (the host falls back to its own
//     solver); the workgroups are co-resident by construction (one per CU, at most the context's share of the chip).
#pragma once

#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_gicp_device.h"
#include "icp_gicp_solver_impl.h"
#include "icp_kernels.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int kSolveLocalBlocks = 32;  // CUs of one XCD: the most workgroups of the one-XCD variant
constexpr int kSolveGranules = 28;  // per workgroup and parity: 13 sums' high parts, their low parts, m, sum d2
constexpr int kSolveOut = 20;       // host granules: status, x[6], m, sum d2, f, evaluations, inner iterations done

struct GicpSolveArgs {
  const float4* src;
  int n_s;
  const float4* tgt;
  const unsigned long long* keys;
  float thr;
  Xform base;
  float guess[16];
  const double* maha6;
  double x0[6];
  unsigned long long* slots;     // [2][gridDim.x][kSolveGranules] granules (2 words each), fine-grained device memory
  unsigned long long* host_out;  // kSolveOut granules in the host mailbox
  unsigned long long seq0;       // evaluation e of this run carries the number seq0 + e; the result carries seq0
  unsigned long long host_seq;   // seq0, with kMailboxReleaseBit if the host mailbox is in release mode
  int max_inner;
  double gradient_tol;
  // one-XCD variant (LOCAL): `workers` participants, all on XCD `xcc_want`, exchange their granules through that XCD's L2
  int workers;
  int xcc_want;
  unsigned long long* owner;     // [kGicpDirectBlocks]: worker index -> number of the run that claimed it
};

// The six sine / cosine pairs of a state, six lanes at a time: lane l (mod 8) evaluates argument l, the results come back through
// v_readlane (every group of eight lanes computes the same six, so lanes 0..5 of the wave serve everybody).  Same function, same
// bits as the host's one-after-the-other loop (gicp::trig6), a sixth of the instructions on the critical path.
__device__ __forceinline__ gicp::Trig6 trig6_lanes(const gicp::V6& x, const double (*table)[4]) {
  double a[6];
  gicp::trig6_arguments(x, a);
  const int l = (int)threadIdx.x & 7;
  double arg = a[0];
  arg = l == 1 ? a[1] : arg;
  arg = l == 2 ? a[2] : arg;
  arg = l == 3 ? a[3] : arg;
  arg = l == 4 ? a[4] : arg;
  arg = l >= 5 ? a[5] : arg;
  double sv, cv;
  trig::sincos_cr_with(table, arg, &sv, &cv);
  double s6[6], c6[6];
  s6[0] = readlane_f64(sv, 0); c6[0] = readlane_f64(cv, 0);
  s6[1] = readlane_f64(sv, 1); c6[1] = readlane_f64(cv, 1);
  s6[2] = readlane_f64(sv, 2); c6[2] = readlane_f64(cv, 2);
  s6[3] = readlane_f64(sv, 3); c6[3] = readlane_f64(cv, 3);
  s6[4] = readlane_f64(sv, 4); c6[4] = readlane_f64(cv, 4);
  s6[5] = readlane_f64(sv, 5); c6[5] = readlane_f64(cv, 5);
  gicp::Trig6 t;
  gicp::trig6_from(s6, c6, t);
  return t;
}

// LOCAL: the workgroups of the run sit on ONE XCD (each has checked its own XCC id), so a granule travels through the L2 they
// share -- a plain 16-byte store (stays in L2) and L1-bypassing loads (sc1, served by L2): ~0.3 us per hop instead of the
// ~1 us of a trip through the fabric to fine-grained memory and back.  Not LOCAL: any placement, write-through stores and
// system-scope loads on fine-grained memory.  The protocol (self-validating granules, double buffer, timeouts) is the same.
template <bool LOCAL>
__device__ __forceinline__ void granule_publish(unsigned long long* g, double value, unsigned long long seq) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(value);
  if constexpr (LOCAL) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u64x2*>(g) = u64x2{bits, granule_tag(seq, bits)};
  } else {
    store_pair_system(g, bits, granule_tag(seq, bits));
  }
}
template <bool LOCAL>
__device__ __forceinline__ unsigned long long granule_word(const unsigned long long* p) {
  if constexpr (LOCAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

#if defined(ICPGPU_DEV_SWITCHES)
#define SOLVE_CLOCK() ((long long)wall_clock64())   // development flavour: phase times of an evaluation (six clock reads of ~0.15 us each)
#else
#define SOLVE_CLOCK() (0ll)
#endif

template <bool RESIDENT, bool LOCAL>
struct DeviceEval {
  const GicpSolveArgs& A;
  const GicpQuad& mine;
  int wid, nw;         // this workgroup's index among the run's workgroups, and their number
  double* s_sums;      // LDS: the 15 numbers of an evaluation
  int* s_ok;           // LDS: the gather's verdict
  const double (*s_table)[4];  // LDS: icp_trig.h's table
  unsigned long long n_eval = 0;
  double m = 0.0, d2 = 0.0;
  double dbg_raw[4] = {0, 0, 0, 0};
  long long t_apply = 0, t_acc = 0, t_pub = 0, t_gather = 0, t_grad = 0;  // phase times (100 MHz ticks), development
  unsigned long long n_pass = 0;  // gather passes (development)
  double md[3] = {0.0, 0.0, 0.0};  // this workgroup's m and sum d2 (the same at every evaluation of the run)
  double dbg = 0.0;    // on a gather timeout: evaluation * 1e6 + the first missing workgroup * 1e3 + quantity (host_out granule 11)

  __device__ __forceinline__ bool operator()(const gicp::V6& x, gicp::Eval& out) {
    const long long c0 = SOLVE_CLOCK();
    const gicp::Trig6 tr = trig6_lanes(x, s_table);
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = A.guess[i];
    gicp::apply_state(T, x, tr);
    Xform Tx;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) Tx.m[4 * r + c] = T[c * 4 + r];
    const long long c1 = SOLVE_CLOCK();
    GicpAcc acc;
    if constexpr (RESIDENT) {
      gicp_clear(acc);
      gicp_add_quad(acc, mine, Tx, A.base);
    } else {
      gicp_accumulate(acc, A.src, A.n_s, A.tgt, A.keys, A.thr, Tx, A.base, A.maha6, wid, nw);
    }
    const long long c2 = SOLVE_CLOCK();
    ++n_eval;
    const unsigned long long seq = A.seq0 + n_eval;
    const int B = nw;
    unsigned long long* parity = A.slots + (size_t)(n_eval & 1ull) * (size_t)B * kSolveGranules * 2;
    publish(acc, parity + (size_t)wid * kSolveGranules * 2, seq);
    const long long c3 = SOLVE_CLOCK();
    gather(parity, B, seq);
    __syncthreads();
    const long long c4 = SOLVE_CLOCK();
    const bool ok = *s_ok != 0;
    double s[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) s[k] = s_sums[k];
    __syncthreads();  // (the LDS words are rewritten by the next evaluation)
    if (!ok) return false;
    m = s[0];
    d2 = s[14];
    gicp::eval_from_sums(tr, s, out);
    const long long c5 = SOLVE_CLOCK();
    t_apply += c1 - c0;
    t_acc += c2 - c1;
    t_pub += c3 - c2;
    t_gather += c4 - c3;
    t_grad += c5 - c4;
    return true;
  }

  // workgroup reduction of the lanes' accumulators (the two LDS stages of gicp_block_reduce_store), then 28 granules
  __device__ __forceinline__ void publish(const GicpAcc& acc, unsigned long long* slot, unsigned long long seq) {
    __shared__ DD s_lane[kGicpSums][16][17];
    __shared__ DD s_chunk[kGicpSums][16];
    __shared__ double s_md[2][4];
#pragma unroll
    for (int k = 0; k < kGicpSums; ++k) s_lane[k][threadIdx.x & 15][threadIdx.x >> 4] = acc.s[k];
    const bool have_md = md[2] != 0.0;
    if (!have_md) {
      const double wm = wave_sum(acc.m), wd = wave_sum(acc.d2);
      if ((threadIdx.x & 63) == 0) {
        s_md[0][threadIdx.x >> 6] = wm;
        s_md[1][threadIdx.x >> 6] = wd;
      }
    }
    __syncthreads();
    if (threadIdx.x < kGicpSums * 16) {
      const int k = threadIdx.x >> 4, c = threadIdx.x & 15;
      DD x[16];
#pragma unroll
      for (int l = 0; l < 16; ++l) x[l] = s_lane[k][l][c];
      const DD v = dd_sum16(x);
      s_chunk[k][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < kGicpSums) {
      DD x[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) x[c] = s_chunk[threadIdx.x][c];
      const DD v = dd_sum16(x);
      granule_publish<LOCAL>(slot + 2 * threadIdx.x, v.hi, seq);
      granule_publish<LOCAL>(slot + 2 * (kGicpSums + threadIdx.x), v.lo, seq);
    } else if (threadIdx.x == kGicpSums) {
      if (!have_md) {
        md[0] = (s_md[0][0] + s_md[0][1]) + (s_md[0][2] + s_md[0][3]);
        md[1] = (s_md[1][0] + s_md[1][1]) + (s_md[1][2] + s_md[1][3]);
      }
      granule_publish<LOCAL>(slot + 2 * 26, md[0], seq);
      granule_publish<LOCAL>(slot + 2 * 27, md[1], seq);
    }
    md[2] = 1.0;
  }

  // wave 0: lane = (quantity q = lane / 4, part p = lane % 4) merges the workgroups p, p + 4, ... of quantity q, then the four
  // parts are combined by two exchanges; quantities 0..12 are the double-double sums, 13 = m, 14 = sum d2 (plain sums of
  // integers / of floats: exact in float64 at these sizes).  s_sums[0] = m, [1..13] = the sums rounded once, [14] = sum d2.
  __device__ __forceinline__ void gather(const unsigned long long* parity, int B, unsigned long long seq) {
    if (threadIdx.x >= 64) return;
    const int q = (int)threadIdx.x >> 2, p = (int)threadIdx.x & 3;
    const bool active = q < 15;
    const int g_hi = q < kGicpSums ? q : (q == 13 ? 26 : 27);
    const bool two = q < kGicpSums;
    const int g_lo = two ? kGicpSums + q : g_hi;  // (quantities without a low part read their one granule twice)
    DD v{0.0, 0.0};
    bool failed = false;
    const long long patience = 5000000;  // 50 ms of the 100 MHz wall clock
    constexpr int R = 8;                 // workgroups per lane and round: 2 R loads in flight
    for (int b0 = p; b0 < B && !failed; b0 += 4 * R) {
      double hi[R], lo[R];
      unsigned int have = 0u, want = 0u;
#pragma unroll
      for (int u = 0; u < R; ++u) {
        hi[u] = lo[u] = 0.0;
        if (active && b0 + 4 * u < B) want |= 1u << u;
      }
      long long t0 = 0;
      for (unsigned pass = 0; have != want; ++pass) {
        ++n_pass;
        // every load of the round is issued before any is looked at (addresses clamped to the last workgroup: no branches
        // between the loads), then the granules are validated; what is not there yet is read again
        unsigned long long hb[R], ht[R], lb[R], lt[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
          hb[u] = ht[u] = lb[u] = lt[u] = 0ull;
          if (b0 - p + 4 * u >= B) continue;  // (wave-uniform: nobody's u-th workgroup of this round exists)
          const int b = min(b0 + 4 * u, B - 1);
          const unsigned long long* slot = parity + (size_t)b * kSolveGranules * 2;
          hb[u] = granule_word<LOCAL>(slot + 2 * g_hi);
          ht[u] = granule_word<LOCAL>(slot + 2 * g_hi + 1);
          lb[u] = granule_word<LOCAL>(slot + 2 * g_lo);
          lt[u] = granule_word<LOCAL>(slot + 2 * g_lo + 1);
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
          const bool ok = ht[u] == granule_tag(seq, hb[u]) && (!two || lt[u] == granule_tag(seq, lb[u]));
          if (ok && (((want & ~have) >> u) & 1u)) {
            hi[u] = __longlong_as_double((long long)hb[u]);
            lo[u] = two ? __longlong_as_double((long long)lb[u]) : 0.0;
            have |= 1u << u;
          }
        }
        if (have != want && (pass & 31u) == 31u) {  // (the clock is a memory instruction: not in every pass)
          const long long now = (long long)wall_clock64();
          if (t0 == 0) t0 = now;
          if (now - t0 <= patience) continue;
          failed = true;
          int miss = 0;
#pragma unroll
          for (int u = R - 1; u >= 0; --u)
            if (((want & ~have) >> u) & 1u) miss = b0 + 4 * u;
          dbg = (double)n_eval * 1e6 + (double)miss * 1e3 + (double)q;
          break;
        }
      }
      {  // the round's (up to) eight workgroups as a tree (absent ones are zeros), then onto the running sum
        DD t[R];
#pragma unroll
        for (int u = 0; u < R; ++u) t[u] = ((want >> u) & 1u) ? DD{hi[u], lo[u]} : DD{0.0, 0.0};
#pragma unroll
        for (int u = 0; u < R / 2; ++u) t[u] = dd_add(t[2 * u], t[2 * u + 1]);
#pragma unroll
        for (int u = 0; u < R / 4; ++u) t[u] = dd_add(t[2 * u], t[2 * u + 1]);
        v = dd_add(v, dd_add(t[0], t[1]));
      }
    }
    // combine the four parts (TwoSum is symmetric in its arguments: all four lanes end with the same bits)
#pragma unroll
    for (int d = 1; d <= 2; d <<= 1) {
      DD o;
      o.hi = __shfl_xor(v.hi, d, 64);
      o.lo = __shfl_xor(v.lo, d, 64);
      v = dd_add(v, o);
    }
    const bool any_failed = __any(failed ? 1 : 0) != 0;
    if (any_failed) {  // the lowest failing lane's record to lane 0
      const unsigned long long mask = __ballot(failed ? 1 : 0);
      const int src_lane = __ffsll((long long)mask) - 1;
      dbg = __shfl(dbg, src_lane, 64);
      for (int k = 0; k < 4; ++k) dbg_raw[k] = __shfl(dbg_raw[k], src_lane, 64);
    }
    if (active && p == 0) s_sums[q < kGicpSums ? 1 + q : (q == 13 ? 0 : 14)] = v.hi + v.lo;
    if (threadIdx.x == 0) *s_ok = any_failed ? 0 : 1;
  }
};

// The body of a run: `bx` of `n_launched` workgroups (blockIdx.x / gridDim.x of the single-run launch; in a batched launch the
// run's own numbers).
template <bool RESIDENT, bool LOCAL>
__device__ __forceinline__ void gicp_solve_body(const GicpSolveArgs& A, int bx, int n_launched) {
  __shared__ double s_sums[16];
  __shared__ int s_ok;
  __shared__ double s_table[128][4];
  // (Measured and dropped in round 5: s_setprio 3 for this latency-bound wave and the evaluation server's -- no effect on an
  //  evaluation's time, alone or with eight registrations in flight: profiles/r05_gicp_batch.txt.)
  const long long t_kernel0 = (long long)wall_clock64();
  int wid = bx, nw = n_launched;
  if constexpr (LOCAL) {
    // Eight times the workgroups the run needs are launched; a workgroup takes part iff the hardware says it sits on XCD
    // xcc_want -- round-robin dispatch puts workgroup b on XCD b % 8, so those are the ones with one residue and b / 8 numbers
    // them 0 .. workers - 1, but NOTHING relies on that: a worker index is claimed (atomic exchange of the run's number), a
    // second claimant leaves, and an index nobody claims makes the gathers time out -- the host then uses the variant that
    // works under any placement.
    unsigned int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if ((int)(xcc & 0xFu) != A.xcc_want) return;
    wid = bx >> 3;
    nw = A.workers;
    if (wid >= nw) return;
    __shared__ int s_mine;
    if (threadIdx.x == 0) s_mine = atomicExch(&A.owner[wid], A.seq0) != A.seq0 ? 1 : 0;
    __syncthreads();
    if (!s_mine) return;
  }
  {
    const double (*src_table)[4] = trig::trig_table();
    for (int i = threadIdx.x; i < 512; i += 256) s_table[i >> 2][i & 3] = src_table[i >> 2][i & 3];
    __syncthreads();
  }
  GicpQuad mine;
  if constexpr (RESIDENT)
    gicp_load_quad(mine, wid * 256 + threadIdx.x, nw * 256, A.src, A.n_s, A.tgt, A.keys, A.thr, A.maha6);
  DeviceEval<RESIDENT, LOCAL> ev{A, mine, wid, nw, s_sums, &s_ok, s_table};
  gicp::V6 x;
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = A.x0[i];
  gicp::Eval probe;
  int status;
  double f_last = 0.0;
  if (!ev(x, probe)) {
    status = gicp::kDeviceError;
  } else if (!(ev.m >= 4.0)) {
    status = gicp::kNotEnoughPoints;  // PCL: NotEnoughPointsException (fewer than 4 correspondences)
  } else {
    const double m0 = ev.m, d20 = ev.d2;
    status = (int)gicp::minimize(ev, x, A.max_inner, A.gradient_tol, &probe);
    ev.m = m0;  // (the correspondences do not change during a run: every evaluation counts the same m and sum d2)
    ev.d2 = d20;
  }
  f_last = probe.f;
  if (wid == 0 && threadIdx.x == 0) {
    unsigned long long* o = A.host_out;
    granule_store(o + 2 * 1, x[0], A.host_seq);
    granule_store(o + 2 * 2, x[1], A.host_seq);
    granule_store(o + 2 * 3, x[2], A.host_seq);
    granule_store(o + 2 * 4, x[3], A.host_seq);
    granule_store(o + 2 * 5, x[4], A.host_seq);
    granule_store(o + 2 * 6, x[5], A.host_seq);
    granule_store(o + 2 * 7, ev.m, A.host_seq);
    granule_store(o + 2 * 8, ev.d2, A.host_seq);
    granule_store(o + 2 * 9, f_last, A.host_seq);
    granule_store(o + 2 * 10, (double)ev.n_eval, A.host_seq);
    granule_store(o + 2 * 11, ev.dbg, A.host_seq);
    if (ev.dbg != 0.0) {
      for (int k = 0; k < 4; ++k) granule_store(o + 2 * (12 + k), ev.dbg_raw[k], A.host_seq);
      for (int k = 16; k < 18; ++k) granule_store(o + 2 * k, 0.0, A.host_seq);
    } else {  // development: phase times in microseconds, packed two to a granule (apply | accumulate, publish | gather, gradient | total)
      const long long t_all = (long long)wall_clock64() - t_kernel0;
      granule_store(o + 2 * 12, (double)ev.t_apply * 0.01, A.host_seq);
      granule_store(o + 2 * 13, (double)ev.t_acc * 0.01, A.host_seq);
      granule_store(o + 2 * 14, (double)ev.t_pub * 0.01, A.host_seq);
      granule_store(o + 2 * 15, (double)ev.t_gather * 0.01, A.host_seq);
      granule_store(o + 2 * 16, (double)ev.t_grad * 0.01, A.host_seq);
      granule_store(o + 2 * 17, (double)t_all * 0.01, A.host_seq);
    }
    granule_store(o + 2 * 18, (double)ev.n_pass, A.host_seq);
    granule_store(o + 2 * 19, 0.0, A.host_seq);
    granule_store(o + 2 * 0, (double)status, A.host_seq);
  }
}

template <bool RESIDENT, bool LOCAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gicp_solve_kernel(GicpSolveArgs A) {
  gicp_solve_body<RESIDENT, LOCAL>(A, (int)blockIdx.x, (int)gridDim.x);
}

// a run's argument block from a launcher's plain parameters (seq0 may carry kMailboxReleaseBit; the one-XCD fields: none)
inline GicpSolveArgs gicp_solve_args(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                                     const Xform& base, const float guess[16], const double* maha6, const double x0[6],
                                     unsigned long long* slots, unsigned long long* host_out, unsigned long long seq0, int max_inner,
                                     double gradient_tol) {
  GicpSolveArgs A;
  A.src = src;
  A.n_s = n_s;
  A.tgt = tgt;
  A.keys = keys;
  A.thr = thr;
  A.base = base;
  for (int i = 0; i < 16; ++i) A.guess[i] = guess[i];
  A.maha6 = maha6;
  for (int i = 0; i < 6; ++i) A.x0[i] = x0[i];
  A.slots = slots;
  A.host_out = host_out;
  A.seq0 = seq0 & ~kMailboxReleaseBit;
  A.host_seq = seq0;
  A.max_inner = max_inner;
  A.gradient_tol = gradient_tol;
  A.workers = blocks;
  A.xcc_want = 0;
  A.owner = nullptr;
  return A;
}

}  // namespace

// gicp_solve_kernel<false, false> (icp_gicp_solve_streamed.hip), for launch_gicp_solve: not one of the library's symbols
__attribute__((visibility("hidden"))) hipError_t launch_gicp_solve_streamed(int blocks, const float4* src, int n_s, const float4* tgt,
                                                                            const unsigned long long* keys, float thr, const Xform& base,
                                                                            const float guess[16], const double* maha6, const double x0[6],
                                                                            unsigned long long* slots, unsigned long long* host_out,
                                                                            unsigned long long seq0, int max_inner, double gradient_tol,
                                                                            hipStream_t stream);

}  // namespace icpgpu
