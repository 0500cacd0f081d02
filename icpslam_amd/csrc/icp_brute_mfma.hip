// icp_brute_mfma.hip -- brute-force exact nearest neighbour on the MATRIX cores (row a2 of SURVEY.md section 8(a);
// north_star's LDS-tiled brute force, the arithmetic of PCL's CorrespondenceEstimation::determineCorrespondences reached from
// /root/reference/src/icpslam/icp_odometer.cpp:198 and src/icpslam/octree_mapper.cpp:114).
//
// Why: the plain-VALU kernel (icp_kernels.hip) needs 7 vector instructions per (source, target) pair and sits at 79 % of
// what the vector ALUs can issue -- 62 TFLOP/s by the 8 flop / pair convention, 40 % of the chip's f32 peak, because that
// peak (157.3 TFLOP/s) is only reachable with packed or matrix f32 (v_pk_fma_f32 issues at half rate on gfx950: the packed
// variant of the VALU kernel measured +-3 %).  The f32 MFMA runs at the full 157.3 TFLOP/s and is bit-for-bit an fmaf
// chain (MI355X guide), but the contract's distance |q - p|^2 = fma(dz, dz, fma(dy, dy, dx * dx)) is a function of
// DIFFERENCES, not a contraction over (source, target) -- so the matrix cores cannot produce it.  They can produce a
// certified LOWER BOUND of it for 32 x 32 pairs at a time, and nearly every pair is settled by that bound alone
// (icp_bound_device.h: the statement, the key and bound rules, the error budget behind kTau):
//
//   centre c: the workgroup's first source (its 256 sources are neighbours in space, they come in cell order)
//   s_ij = fma(1, |v_j|^2 - tau_j, fma(-2uz, vz, fma(-2uy, vy, (-2ux) vx)))      two v_mfma_f32_32x32x2_f32, K = 4
//
// For targets in arbitrary order the bound improves ~ln(N) times per source, so the exact path runs for ~20 of 200 000 targets;
// everything else costs two MFMAs per 1024 pairs plus ~20 vector instructions per tile.  The result is the exact key -- same
// bits as the VALU kernel and the oracle.
//
// This kernel runs only where brute_variant = 2 asks for it (the default from 8192 x 8192 points on is icp_brute_bf16.hip):
// tests/test_gpu_brute_edges.py holds its keys to the oracle's bit for bit at every boundary of its launch arithmetic (sources
// 1 .. 8193, targets around every step and tile, several tiles per split, a non-finite target in every row of a step, ties
// across every seam, degenerate centres, seeded sweeps) and reads from the ICPGPU_DEBUG line that it is this kernel that ran;
// tests/test_gpu_brute_bf16.py compares it with the bf16 and the VALU kernel on seven clouds of 9 000 - 90 000 points, and
// tests/history_model.py runs it among a context's histories.  (test_gpu_parity.py, test_gpu_grid.py and test_gpu_fullsize.py
// run the default variant: since the default changed they exercise the bf16 kernel or the VALU kernel, not this one.)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "icp_bound_device.h"
#include "icp_env.h"

namespace icpgpu {
namespace {

constexpr int MF_BLOCK = kMfmaShape.block;   // 4 waves
constexpr int MF_TILE = kMfmaShape.tile;     // target points per LDS tile (16 KiB), shared by the 4 waves

// G groups of 32 sources per wave (both half-waves hold the same 32 sources; each sees 16 of a tile's 32 targets)
template <int G, bool PIPE>
__device__ __forceinline__ void nn_brute_mfma_body(const float4* __restrict__ src_sorted, int n_q,
                                                   const float4* __restrict__ tgt, int n_t, const Xform& T,
                                                   int tgt_per_split, int splits, unsigned long long* __restrict__ keys,
                                                   const unsigned long long* __restrict__ seed, int debug_no_exact) {
  // a target tile in LDS, twice: the raw points (for the exact evaluations) and the MFMA's A operands, ready to use --
  // (vx, vy) and (vz, |v|^2 - tau) -- computed ONCE per tile and workgroup instead of per wave and step (16 vector
  // instructions per step less; measured effect on the sweep: within noise -- the kernel sits at 1.55-1.6x the time its MFMAs
  // alone would take whatever else is trimmed, profiles/r02_brute_force_mfma.txt).
  __shared__ float4 tile[MF_TILE];
  __shared__ float2 a01s[MF_TILE], a23s[MF_TILE];
  __shared__ float s_centre[4];
  __shared__ float s_pmax[MF_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;

  float px[G], py[G], pz[G];
  int orig[G];
  bool valid[G];
  load_wave_sources<G>(src_sorted, n_q, T, (blockIdx.x * (MF_BLOCK / 64) + wave) * (32 * G), col, px, py, pz, orig, valid);
  // the workgroup's centre: its first source (sources arrive in cell order: the other 32 G x 4 - 1 are close by)
  if (threadIdx.x == 0) {
    s_centre[0] = px[0];
    s_centre[1] = py[0];
    s_centre[2] = pz[0];
  }
  __syncthreads();
  const float cx = s_centre[0], cy = s_centre[1], cz = s_centre[2];
  // B operands (K x N = sources): lane supplies B[k = half][n = col] -- first MFMA k = 0, 1 = (-2ux, -2uy), second
  // k = 2, 3 = (-2uz, 1)
  float b01[G], b23[G], p2[G], pmax2 = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float ux = px[g] - cx, uy = py[g] - cy, uz = pz[g] - cz;
    b01[g] = half ? -2.0f * uy : -2.0f * ux;
    b23[g] = half ? 1.0f : -2.0f * uz;
    p2[g] = len2(ux, uy, uz);
    pmax2 = fmaxf(pmax2, p2[g]);
  }
  pmax2 = workgroup_max<MF_BLOCK>(pmax2, s_pmax, lane, wave);

  unsigned long long best[G];
  float bound[G];
#pragma unroll
  for (int g = 0; g < G; ++g) seed_brute(seed, orig[g], tgt, n_t, px[g], py[g], pz[g], p2[g], best[g], bound[g]);

  const int j0 = blockIdx.y * tgt_per_split;
  const int j1 = min(n_t, j0 + tgt_per_split);
  // target tiles: the NEXT tile's global loads are in flight (in registers) while this one is being worked on
  float4 nxt[MF_TILE / MF_BLOCK];
#pragma unroll
  for (int u = 0; u < MF_TILE / MF_BLOCK; ++u) nxt[u] = tgt[min(j0 + u * MF_BLOCK + (int)threadIdx.x, n_t - 1)];
  for (int jt = j0; jt < j1; jt += MF_TILE) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < MF_TILE / MF_BLOCK; ++u) {
      const int k = u * MF_BLOCK + threadIdx.x;
      const float4 q = nxt[u];
      tile[k] = q;
      // A operands (M x K = targets): row k supplies (vx, vy | vz, |v|^2 - tau); a row past the end can never undercut a bound
      const float vx = q.x - cx, vy = q.y - cy, vz = q.z - cz;
      const float q2 = len2(vx, vy, vz);
      const bool real = jt + k < j1;
      a01s[k] = real ? make_float2(vx, vy) : make_float2(0.f, 0.f);
      a23s[k] = real ? make_float2(vz, q2 - (pmax2 + q2) * kTau) : make_float2(0.f, INFINITY);
    }
    __syncthreads();
    if (jt + MF_TILE < j1) {
#pragma unroll
      for (int u = 0; u < MF_TILE / MF_BLOCK; ++u) nxt[u] = tgt[min(jt + MF_TILE + u * MF_BLOCK + (int)threadIdx.x, n_t - 1)];
    }
    const int lim = min(MF_TILE, j1 - jt);
    const float* __restrict__ a01p = reinterpret_cast<const float*>(a01s) + half;
    const float* __restrict__ a23p = reinterpret_cast<const float*>(a23s) + half;
    // One step = 32 targets against the wave's 32 G sources: 2 G MFMAs, then the fold of their 16 G values per lane.  The
    // steps are SOFTWARE-PIPELINED (PIPE): the MFMAs of step k + 1 are issued into a second accumulator set before step k's
    // values are folded, so the ~27 vector instructions of a fold run under the wave's OWN matrix work -- round 2's counters
    // showed matrix and vector time adding up (64 % + 27 %) instead of overlapping when a wave folds right behind its MFMAs
    // and leaves the overlap to the other waves of the SIMD.
    auto issue = [&](floatx16 (&acc)[G], int st) {
      const float a01 = a01p[2 * (st + col)], a23 = a23p[2 * (st + col)];  // lane supplies A[m = col][k = half]
      // all the groups' first MFMAs, then the second ones (each depends on its first: interleaved, neither waits)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const floatx16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a01, b01[g], zero, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a23, b23[g], acc[g], 0, 0, 0);
    };
    auto fold_step = [&](floatx16 (&acc)[G], int st) {
      // every accumulator is first read by an instruction the compiler can see (icp_bound_device.h, the fold): a readfirstlane
      __builtin_amdgcn_sched_barrier(0);
      int touched = 0;
#pragma unroll
      for (int g = 0; g < G; ++g) touched |= __builtin_amdgcn_readfirstlane(__float_as_int(acc[g][15]));
      asm volatile("" ::"s"(touched));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float mn = fold(acc[g], min3f(acc[g][14], acc[g][15], acc[g][15]));
        // rare: some lane's bound is undercut -- those targets are evaluated exactly
        if (!debug_no_exact && __ballot(mn <= bound[g])) recheck_brute(acc[g], half, tile, st, lim, jt, px[g], py[g], pz[g], p2[g], best[g], bound[g]);
      }
    };
    if (PIPE) {
      floatx16 acc_a[G], acc_b[G];
      issue(acc_a, 0);
      for (int st = 0;; st += 64) {
        const bool more_b = st + 32 < lim;
        if (more_b) issue(acc_b, st + 32);
        fold_step(acc_a, st);
        if (!more_b) break;
        const bool more_a = st + 64 < lim;
        if (more_a) issue(acc_a, st + 64);
        fold_step(acc_b, st + 32);
        if (!more_a) break;
      }
    } else {
      for (int st = 0; st < lim; st += 32) {
        floatx16 acc[G];
        issue(acc, st);
        fold_step(acc, st);
      }
    }
  }

#pragma unroll
  for (int g = 0; g < G; ++g) {
    const unsigned long long k = merge_halves(best[g]);
    if (half == 0 && valid[g]) write_key(keys, orig[g], k, splits);
  }
}

template <int G, bool PIPE>
__global__ __launch_bounds__(MF_BLOCK) void nn_brute_mfma_kernel(const float4* __restrict__ src_sorted, int n_q,
                                                                 const float4* __restrict__ tgt, int n_t, Xform T,
                                                                 int tgt_per_split, int splits,
                                                                 unsigned long long* __restrict__ keys,
                                                                 const unsigned long long* __restrict__ seed, int debug_no_exact) {
  nn_brute_mfma_body<G, PIPE>(src_sorted, n_q, tgt, n_t, T, tgt_per_split, splits, keys, seed, debug_no_exact);
}

// the pipelined body held to 128 registers (four waves per SIMD instead of three; a few spills in return) -- ICPGPU_MFMA_PIPE=2
template <int G>
__global__ __launch_bounds__(MF_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void nn_brute_mfma_capped_kernel(
    const float4* __restrict__ src_sorted, int n_q, const float4* __restrict__ tgt, int n_t, Xform T, int tgt_per_split,
    int splits, unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ seed, int debug_no_exact) {
  nn_brute_mfma_body<G, true>(src_sorted, n_q, tgt, n_t, T, tgt_per_split, splits, keys, seed, debug_no_exact);
}

}  // namespace

// The launch shape: ICPGPU_MFMA_G (sources per wave / 32: 2 or 4) and ICPGPU_MFMA_WAVES (target waves per SIMD the splits aim
// at) are experiments, read once per process.
MatrixNnPlan plan_nn_brute_mfma(int n_q, int n_t, int num_cus) {
  static const int g_env = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_MFMA_G"); return e ? atoi(e) : kMfmaShape.g; }();
  static const int waves_env = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_MFMA_WAVES"); return e ? atoi(e) : kMatrixNnWavesPerSimd; }();
  return matrix_nn_plan(n_q, n_t, num_cus, {g_env == 4 ? 4 : 2, MF_TILE, MF_BLOCK}, waves_env);
}

int matrix_nn_no_exact() {
  static const int no_exact = [] {
    if (!ICPGPU_DEV_ENV("ICPGPU_MFMA_NO_EXACT")) return 0;
    fprintf(stderr, "[icpgpu] WARNING: ICPGPU_MFMA_NO_EXACT is set -- the matrix-core search skips its exact path, every brute-force result "
                    "of this process is WRONG (a timing experiment's switch, never a production setting)\n");
    return 1;
  }();
  return no_exact;
}

// src_sorted: the source in cell order with the ORIGINAL index in .w (what the grid machinery's sorted copy holds); keys are
// written at the original indices and must be pre-filled with kEmptyKey (points missing from src_sorted -- the non-finite ones
// -- stay unmatched, and target splits merge by atomic min).
// seed (optional, n_s keys indexed like `keys`): every source's neighbour from an earlier sweep over the SAME target array.
hipError_t launch_nn_brute_mfma(const float4* src_sorted, int n_q, const float4* tgt, int n_t, const Xform& T, int num_cus,
                                unsigned long long* keys, const unsigned long long* seed, hipStream_t stream) {
  if (n_q <= 0 || n_t <= 0) return hipSuccess;
  const MatrixNnPlan plan = plan_nn_brute_mfma(n_q, n_t, num_cus);
  static const int pipe_env = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_MFMA_PIPE"); return e ? atoi(e) : 0; }();
  auto launch = [&](auto kernel) { launch_matrix_nn(kernel, plan, stream, src_sorted, n_q, tgt, n_t, T, keys, seed); };
  if (plan.g == 4) {
    if (pipe_env) launch(nn_brute_mfma_kernel<4, true>);
    else launch(nn_brute_mfma_kernel<4, false>);
  } else {
    if (pipe_env == 2) launch(nn_brute_mfma_capped_kernel<2>);
    else if (pipe_env) launch(nn_brute_mfma_kernel<2, true>);
    else launch(nn_brute_mfma_kernel<2, false>);
  }
  return hipGetLastError();
}

}  // namespace icpgpu
