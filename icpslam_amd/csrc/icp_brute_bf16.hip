// icp_brute_bf16.hip -- brute-force exact nearest neighbour, the lower bound on the bf16 matrix path (row a2 of SURVEY.md
// section 8(a); north_star's LDS-tiled brute force, the arithmetic of PCL's CorrespondenceEstimation::determineCorrespondences
// reached from /root/reference/src/icpslam/icp_odometer.cpp:198 and src/icpslam/octree_mapper.cpp:114).
//
// Why a second matrix-core kernel: on gfx950 an f32 MFMA and the ordinary vector instructions of the same SIMD do not run side
// by side (scripts/probes/mfma_coissue.cpp, profiles/r03_mfma_coissue.txt: 4 f32 MFMAs + 32 v_fma_f32 take the SUM of their
// times, in one wave or in two), so icp_brute_mfma.hip's two f32 MFMAs + ~13 vector instructions per 1024 pairs cannot pass
// ~71 % of the f32 peak whatever the schedule.  bf16 MFMAs DO overlap with vector work, and one v_mfma_f32_32x32x16_bf16
// (K = 16, 34 cycles) does what the two f32 MFMAs (K = 2 + 2, 128 cycles) do if the operands are split:
//
//   u = p - c, v = q - c (c: centre of the workgroup's sources);  U = -2u
//   x = xh + xl + r,  xh = bf16(x), xl = bf16(x - xh)  (round to nearest even, v_cvt_pk_bf16_f32; |r| <= 2^-16 |x|)
//   s_ij = sum over the coordinates of (Uh + Ul)(vh + vl) -- four exact bf16 x bf16 products each, 12 of the 16 K slots --
//          + (S_h + S_l) * 1,   S = |v|^2 - tau_j  (2 more slots; 2 unused)
//   tau_j = 2^-13 (P^2 + |v_j|^2),  P = max |u| of the workgroup
//   =>  s_ij <= |q_j - p_i|^2 - |u_i|^2   for every pair: exactly the f32 kernel's statement with a wider tau.
//
// The key and bound rules, the operand records, the fold and the error budget behind tau = 2^-13 are icp_bound_device.h's,
// shared with the f32 kernel and the tile search: each lane keeps the best EXACT key per source and the bound B = its distance
// - |u|^2 (+ margin); only a lane that sees s <= B evaluates those targets exactly.  The result is the exact key -- same bits as
// the VALU kernel and the oracle.  Because tau grows with P^2, the sources come in MORTON order of their grid cells
// (launch_morton_order below: a workgroup's 256 sources sit within 1-4 m of each other instead of the 1-40 m of x-fastest cell
// order) and the centre is the middle of their bounding box.  ICPGPU_MFMA_CHECK_BOUND=1 (an instantiation of its own, CHECK)
// measures the bound on every pair; tests/test_gpu_brute_edges.py and tests/test_gpu_brute_bf16.py hold the keys to the oracle's.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "icp_bound_device.h"
#include "icp_env.h"
#include "icp_grid_device.h"

namespace icpgpu {
namespace {

// G groups of 32 sources per wave (both half-waves hold the same 32 sources; each sees 16 of a step's 32 targets); TILE
// targets per LDS tile; BLOCK threads per workgroup (the A operands of a tile are built once per workgroup: the more sources
// share them, the less they cost per pair)
template <int G, int TILE, int BLOCK, bool CHECK>
__device__ __forceinline__ void nn_brute_bf16_body(const float4* __restrict__ src_sorted, int n_q, const float4* __restrict__ tgt,
                                                   int n_t, const Xform& T, int tgt_per_split, int splits,
                                                   unsigned long long* __restrict__ keys,
                                                   const unsigned long long* __restrict__ seed, int flags,
                                                   unsigned long long* __restrict__ check) {
  // a target tile in LDS, twice: the raw points (for the exact evaluations) and the MFMA's A operands, ready to use: per
  // target one 16-byte record for the lanes of each half-wave (K slots 0-7: x and y products; 8-15: z products and S)
  __shared__ float4 tile[TILE];
  __shared__ uint4 aop[2 * TILE];
  __shared__ float s_box[BLOCK / 64][6];
  __shared__ float s_pmax[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;
  const bool no_exact = flags & 1;

  float px[G], py[G], pz[G];
  int orig[G];
  bool valid[G];
  load_wave_sources<G>(src_sorted, n_q, T, (blockIdx.x * (BLOCK / 64) + wave) * (32 * G), col, px, py, pz, orig, valid);
  // the workgroup's centre: the middle of its sources' bounding box (they come in Morton order: close together)
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int g = 0; g < G; ++g) {
    lo[0] = fminf(lo[0], px[g]); hi[0] = fmaxf(hi[0], px[g]);
    lo[1] = fminf(lo[1], py[g]); hi[1] = fmaxf(hi[1], py[g]);
    lo[2] = fminf(lo[2], pz[g]); hi[2] = fmaxf(hi[2], pz[g]);
  }
  workgroup_box<BLOCK>(lo, hi, s_box, lane, wave);
  const float cx = 0.5f * lo[0] + 0.5f * hi[0], cy = 0.5f * lo[1] + 0.5f * hi[1], cz = 0.5f * lo[2] + 0.5f * hi[2];
  uint4 bop[G];
  float p2[G], pmax2 = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float ux = px[g] - cx, uy = py[g] - cy, uz = pz[g] - cz;
    p2[g] = len2(ux, uy, uz);
    pmax2 = fmaxf(pmax2, p2[g]);
    bop[g] = bf16_source_operand(ux, uy, uz, half);
  }
  pmax2 = workgroup_max<BLOCK>(pmax2, s_pmax, lane, wave);

  unsigned long long best[G];
  float bound[G];
#pragma unroll
  for (int g = 0; g < G; ++g) seed_brute(seed, orig[g], tgt, n_t, px[g], py[g], pz[g], p2[g], best[g], bound[g]);

  const int j0 = blockIdx.y * tgt_per_split;
  const int j1 = min(n_t, j0 + tgt_per_split);
  unsigned long long n_violations = 0;
  float worst_ratio = 0.f;
  // target tiles: the NEXT tile's global loads are in flight (in registers) while this one is being worked on
  float4 nxt[TILE / BLOCK];
#pragma unroll
  for (int u = 0; u < TILE / BLOCK; ++u) nxt[u] = tgt[min(j0 + u * BLOCK + (int)threadIdx.x, n_t - 1)];
  for (int jt = j0; jt < j1; jt += TILE) {
    __syncthreads();
    const bool whole = jt + TILE <= j1;  // (uniform) only a split's last tile has rows past the end
#pragma unroll
    for (int u = 0; u < TILE / BLOCK; ++u) {
      const int k = u * BLOCK + threadIdx.x;
      const float4 q = nxt[u];
      tile[k] = q;
      uint4 r0, r1;
      bf16_target_records(q.x - cx, q.y - cy, q.z - cz, pmax2, r0, r1);
      if (!whole && jt + k >= j1) bf16_padding_records(r0, r1);
      aop[k] = r0;
      aop[TILE + k] = r1;
    }
    __syncthreads();
    if (jt + TILE < j1) {
#pragma unroll
      for (int u = 0; u < TILE / BLOCK; ++u) nxt[u] = tgt[min(jt + TILE + u * BLOCK + (int)threadIdx.x, n_t - 1)];
    }
    const int lim = min(TILE, j1 - jt);
    const uint4* __restrict__ arow = aop + half * TILE + col;
    const float minus_inf = opaque_minus_inf();

    // One step = 32 targets against the wave's 32 G sources: G MFMAs, then the fold of their 16 G values per lane.
    auto issue = [&](floatx16 (&acc)[G], const uint4& a) {  // a: this lane's A[m = col][k = 8 half .. 8 half + 7] of the step
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const floatx16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bop[g]), zero, 0, 0, 0);
      }
    };
    auto fold_step = [&](floatx16 (&acc)[G], int st) {
      float tail[G], mn[G];
      first_read_tails<G>(acc, minus_inf, tail);
      bool hit = false;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        mn[g] = fold(acc[g], tail[g]);
        hit |= mn[g] <= bound[g];
      }
      if (CHECK) {  // (test mode: its own instantiation) every pair exactly: does its bound allow what its own distance would need?
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const floatx16 d = acc[g];
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int row = row_of(v, half);
            if (st + row < lim && valid[g]) {
              const float4 t = tile[st + row];
              const float e = dist2(t.x, t.y, t.z, px[g], py[g], pz[g]);
              if (e < INFINITY) {
                if (d[v] > bound_of(e, p2[g])) ++n_violations;
                const float scale = pmax2 + len2(t.x - cx, t.y - cy, t.z - cz);
                if (scale >= kTinyScale) {
                  // how far the value WITHOUT tau lies above the truth, in units of (P^2 + |v|^2): must stay well below tau
                  const double over = ((double)d[v] + (double)scale * (double)kTauBf16) - ((double)e - (double)p2[g]);
                  worst_ratio = fmaxf(worst_ratio, (float)(over / (double)scale));
                }
              }
            }
          }
        }
      }
      if (!no_exact && __ballot(hit)) {  // rare: some lane's bound is undercut -- those targets are evaluated exactly
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (__ballot(mn[g] <= bound[g])) recheck_brute(acc[g], half, tile, st, lim, jt, px[g], py[g], pz[g], p2[g], best[g], bound[g]);
        }
      }
    };
    // two steps per trip; the A operands of a step are read from LDS one step ahead (the read's latency passes under the
    // fold before it instead of in front of the MFMAs); rows up to the end of the tile always hold valid records
    uint4 a0 = arow[0];
    for (int st = 0; st < lim; st += 64) {
      floatx16 acc[G];
      const uint4 a1 = arow[st + 32];
      issue(acc, a0);
      fold_step(acc, st);
      a0 = arow[(st + 64) & (TILE - 1)];
      if (st + 32 < lim) {
        issue(acc, a1);
        fold_step(acc, st + 32);
      }
    }
  }

  if (CHECK) {
    if (n_violations) atomicAdd(&check[0], n_violations);
    if (worst_ratio > 0.f) atomicMax(reinterpret_cast<unsigned int*>(&check[1]), __float_as_uint(worst_ratio));
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const unsigned long long k = merge_halves(best[g]);
    if (half == 0 && valid[g]) write_key(keys, orig[g], k, splits);
  }
}

template <int G, int TILE, int BLOCK, bool CHECK = false>
__global__ __launch_bounds__(BLOCK) void nn_brute_bf16_kernel(const float4* __restrict__ src_sorted, int n_q,
                                                                 const float4* __restrict__ tgt, int n_t, Xform T,
                                                                 int tgt_per_split, int splits,
                                                                 unsigned long long* __restrict__ keys,
                                                                 const unsigned long long* __restrict__ seed, int flags,
                                                                 unsigned long long* __restrict__ check) {
  nn_brute_bf16_body<G, TILE, BLOCK, CHECK>(src_sorted, n_q, tgt, n_t, T, tgt_per_split, splits, keys, seed, flags, check);
}

// ---- Morton order of a grid's sorted copy ----------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int spread10(unsigned int x) {  // 10 bits -> every third bit
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

__global__ __launch_bounds__(256) void morton_keys_kernel(const float4* __restrict__ sorted, int n, GridDesc g, int shift,
                                                          int* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = sorted[i];
  int cx, cy, cz;
  cell_of(g, p.x, p.y, p.z, cx, cy, cz);
  cx = min(max(cx, 0), g.nx - 1) >> shift;
  cy = min(max(cy, 0), g.ny - 1) >> shift;
  cz = min(max(cz, 0), g.nz - 1) >> shift;
  keys[i] = (int)(spread10((unsigned int)cx) | (spread10((unsigned int)cy) << 1) | (spread10((unsigned int)cz) << 2));
  vals[i] = i;
}

__global__ __launch_bounds__(256) void morton_gather_kernel(const float4* __restrict__ sorted, const int* __restrict__ order, int n,
                                                            float4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = sorted[order[i]];
}

}  // namespace

size_t morton_order_work_ints(int n) { return 4 * (size_t)n + radix_sort_scratch_ints(n); }

// out[0..n) = sorted[0..n) (a grid's cell-ordered copy: finite points, original index in .w) reordered by the Morton code of
// their cells (cells merged 2^shift to a side until every axis fits 10 bits); stable: ties keep the cell order
hipError_t launch_morton_order(const float4* sorted, int n, const GridDesc& g, int* work, float4* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  int shift = 0;
  while (((g.nx - 1) >> shift) > 1023 || ((g.ny - 1) >> shift) > 1023 || ((g.nz - 1) >> shift) > 1023) ++shift;
  int* keys = work;               // 2 n: input half, output half
  int* vals = work + 2 * (size_t)n;
  int* scratch = work + 4 * (size_t)n;
  hipLaunchKernelGGL(morton_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, sorted, n, g, shift, keys, vals);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = launch_radix_sort_pairs(keys, vals, n, 30, scratch, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(morton_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, sorted, vals + n, n, out);
  return hipGetLastError();
}

// The launch shape.  check: the test mode (ICPGPU_MFMA_CHECK_BOUND) has its own instantiation, one shape.  Experiments, read
// once per process: ICPGPU_BF16_G (sources per wave / 32: 2 or 4), ICPGPU_BF16_TILE (512 / 1024), ICPGPU_BF16_BLOCK (256 / 512),
// ICPGPU_MFMA_WAVES (target waves per SIMD the splits aim at).
MatrixNnPlan plan_nn_brute_bf16(int n_q, int n_t, int num_cus, bool check) {
  static const int g_env = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BF16_G"); return e ? atoi(e) : kBf16Shape.g; }();
  static const int tile_env = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BF16_TILE"); return e ? atoi(e) : kBf16Shape.tile; }();
  static const int block_env = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BF16_BLOCK"); return e ? atoi(e) : kBf16Shape.block; }();
  static const int waves_env = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_MFMA_WAVES"); return e ? atoi(e) : kMatrixNnWavesPerSimd; }();
  const MatrixNnShape s = {g_env == 4 ? 4 : 2, tile_env == 1024 ? 1024 : 512, block_env == 512 ? 512 : 256};
  return matrix_nn_plan(n_q, n_t, num_cus, check ? kBf16CheckShape : s, waves_env);
}

// src_sorted: the source in MORTON order with the ORIGINAL index in .w (launch_morton_order); keys are written at the original
// indices and must be pre-filled with kEmptyKey (points missing from src_sorted -- the non-finite ones -- stay unmatched, and
// target splits merge by atomic min).  seed (optional, n_s keys indexed like `keys`): every source's neighbour from an earlier
// sweep over the SAME target array.  check (optional: 2 x u64, zeroed by the caller): ICPGPU_MFMA_CHECK_BOUND's counters.
hipError_t launch_nn_brute_bf16(const float4* src_sorted, int n_q, const float4* tgt, int n_t, const Xform& T, int num_cus,
                                unsigned long long* keys, const unsigned long long* seed, unsigned long long* check,
                                hipStream_t stream) {
  if (n_q <= 0 || n_t <= 0) return hipSuccess;
  const MatrixNnPlan plan = plan_nn_brute_bf16(n_q, n_t, num_cus, check != nullptr);
  auto launch = [&](auto kernel) { launch_matrix_nn(kernel, plan, stream, src_sorted, n_q, tgt, n_t, T, keys, seed, check); };
  if (check) {
    static_assert(kBf16CheckShape.g == 2 && kBf16CheckShape.tile == 512 && kBf16CheckShape.block == 256, "the one CHECK instantiation");
    launch(nn_brute_bf16_kernel<2, 512, 256, true>);
    return hipGetLastError();
  }
  const int sel = (plan.g == 4 ? 4 : 0) | (plan.tile == 1024 ? 2 : 0) | (plan.block == 512 ? 1 : 0);
  switch (sel) {
    case 0: launch(nn_brute_bf16_kernel<2, 512, 256>); break;
    case 1: launch(nn_brute_bf16_kernel<2, 512, 512>); break;
    case 2: launch(nn_brute_bf16_kernel<2, 1024, 256>); break;
    case 3: launch(nn_brute_bf16_kernel<2, 1024, 512>); break;
    case 4: launch(nn_brute_bf16_kernel<4, 512, 256>); break;
    case 5: launch(nn_brute_bf16_kernel<4, 512, 512>); break;
    case 6: launch(nn_brute_bf16_kernel<4, 1024, 256>); break;
    default: launch(nn_brute_bf16_kernel<4, 1024, 512>); break;
  }
  return hipGetLastError();
}

}  // namespace icpgpu
