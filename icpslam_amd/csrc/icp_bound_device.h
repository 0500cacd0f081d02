// icp_bound_device.h -- the certified lower bound of the matrix-core searches, stated ONCE for its three kernel units:
// icp_brute_bf16.hip (brute force, bf16 matrix path), icp_brute_mfma.hip (brute force, f32 MFMA) and icp_tile.hip (grid search,
// bf16 matrix path).  What decides their correctness lives here; the units keep what differs (the choice of centre, the f32
// operands, the step loops and their pipelining, the bound-check mode, everything the tile search does with the grid).
//
// The statement.  With a centre c per workgroup, u = p - c (sources), v = q - c (targets):
//   |q - p|^2 - |u|^2 = |v|^2 - 2 u.v                                   (exact in real arithmetic)
//   s_ij = (-2 u_i).v_j + (|v_j|^2 - tau_j),   tau_j = tau (P^2 + |v_j|^2),   P = max |u| of the workgroup
//   =>  s_ij <= |q_j - p_i|^2 - |u_i|^2   for every pair, if tau covers every rounding on the way.
// Each lane keeps, per source, the best EXACT key found so far (key_of: contract arithmetic on the original coordinates, lowest
// index among ties) and the bound B = its distance - |u|^2, widened (bound_of).  A target can only beat or tie the best if
// s_ij <= B; the 16 values a lane receives from a 32 x 32 step (row_of) are folded with v_min3 and compared once; only a lane
// that sees s <= B evaluates those targets exactly and tightens its bound.  The result is the exact key.
//
// Error budget, f32 MFMA (kTau = 2^-18; two v_mfma_f32_32x32x2_f32, bit for bit an fmaf chain), in units of 2^-24 = one float
// rounding, relative to the magnitudes named:
//   u and v are rounded differences (1 each, of |u|, |v|): moves |v - u|^2 by <= 2 |q-p| (|u| + |v|) 2^-24 sqrt(3)
//   |v|^2 by three roundings (3 of |v|^2); the four fused steps of the chain (4 of 2|u||v| + |v|^2)
//   sum <= 2^-24 * 16 (P + |v|)^2 <= 2^-24 * 32 (P^2 + |v|^2) = 2^-19 (P^2 + |v|^2); tau carries a further factor 2.
//
// Error budget, bf16 (kTauBf16 = 2^-13; one v_mfma_f32_32x32x16_bf16 on split operands: x = xh + xl + r, xh = bf16(x),
// xl = bf16(x - xh), round to nearest even, |r| <= 2^-16 |x|; s_ij = sum over the coordinates of (Uh + Ul)(vh + vl), U = -2u --
// four exact bf16 x bf16 products each, 12 of the 16 K slots -- + (S_h + S_l) * 1, S = |v|^2 - tau_j, 2 more slots), relative to
// (P^2 + |v|^2):
//   operand splits: |u.v - (uh + ul).(vh + vl)| <= (2^-16 + 2^-16)|u||v| per sum, times 2: 2^-14 |u||v| <= 2^-15 (P^2 + |v|^2)
//   S = S_h + S_l + r, |r| <= 2^-16 |S| <= 2^-16 |v|^2 (+ tau);  the MFMA's own accumulation: MEASURED (round 4,
//   scripts/probes/mfma_accum.cpp, profiles/r04_mfma_accumulation.txt: 8192 MFMAs x 1024 outputs against the exact sums, operands
//   chosen to cancel in the 14 K slots used here, exponent spreads up to 30 binades): the adder aligns to the largest product and
//   drops what lies 2^-21 .. 2^-24 below it -- worst |error| = 2^-21.9 of the sum of the |products| (2^-20.8 of the largest
//   one).  The |products| of a bound add up to <= 2 |u||v| (1 + 2^-7) + |v|^2 + tau <= 2 (P^2 + |v|^2), so the accumulation costs
//   <= 2^-20.9 (P^2 + |v|^2); the budget keeps the 2^-17 it assumed until then (a factor 15 above the measurement); the f32
//   budget above for the rounded differences and |v|^2: 2^-19.
//   Sum < 1.9 x 2^-15; tau = 2^-13 leaves a factor two.  MEASURED, not only argued: ICPGPU_MFMA_CHECK_BOUND=1 evaluates every
//   pair exactly and counts the pairs whose bound exceeds what their own distance allows (must be 0) and the worst
//   (s + tau - truth) / (P^2 + |v|^2) seen (tests/test_gpu_brute_bf16.py and a campaign of 4000 random clouds: 1.8e-5 = 2^-15.8
//   at worst against tau = 2^-13).
//
// Anonymous namespace, as icp_wave.h: every unit compiles its own copy into its kernels.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include "icp_device.h"
#include "icp_kernels.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr float kTau = 3.814697265625e-06f;       // 2^-18: the f32 bound
constexpr float kTauBf16 = 1.220703125e-04f;      // 2^-13: the bf16 bound
constexpr float kTinyScale = 1e-18f;              // P^2 + |v|^2 below this: products near the denormal range, no bf16 bound claimed
constexpr float kBoundMargin = 9.5367431640625e-07f;  // 2^-20: the rounding of |u|^2 and of the bound's own subtraction

__device__ __forceinline__ float min3f(float a, float b, float c) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float len2(float x, float y, float z) { return __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)); }

// everything that can still beat or tie a neighbour at distance e has |q - p|^2 - |u|^2 <= e - |u|^2: the bound, widened for the
// rounding of p2 = |u|^2 and of this subtraction
__device__ __forceinline__ float bound_of(float e, float p2) { return __builtin_fmaf(e + p2, kBoundMargin, e - p2); }
__device__ __forceinline__ unsigned long long key_of(float e, unsigned int index) {
  return ((unsigned long long)__float_as_uint(e) << 32) | index;
}
// the target row of a step that accumulator value v (0..15) of a lane in half-wave `half` belongs to (its source: column lane & 31)
__device__ __forceinline__ int row_of(int v, int half) { return 8 * (v >> 2) + 4 * half + (v & 3); }

// ---- the source side -------------------------------------------------------------------------------------------------------
// sources of a wave: group g, column col, first source q0 (transformed: the contract's p = T * s); orig: the index in .w
template <int G>
__device__ __forceinline__ void load_wave_sources(const float4* __restrict__ src_sorted, int n_q, const Xform& T, int q0, int col,
                                                  float (&px)[G], float (&py)[G], float (&pz)[G], int (&orig)[G], bool (&valid)[G]) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int k = q0 + g * 32 + col;
    valid[g] = k < n_q;
    const float4 s = src_sorted[min(k, n_q - 1)];
    xform_point(T, s.x, s.y, s.z, px[g], py[g], pz[g]);
    orig[g] = __float_as_int(s.w);
  }
}

// P^2 of the WORKGROUP (tau is shared by its waves) from every lane's largest |u|^2; s_pmax: BLOCK / 64 floats of LDS.  (fmaxf
// drops a NaN: a NaN source never matches anything, its s_ij are NaN.)
template <int BLOCK>
__device__ __forceinline__ float workgroup_max(float pmax2, float (&s_pmax)[BLOCK / 64], int lane, int wave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pmax2 = fmaxf(pmax2, __shfl_xor(pmax2, off, 64));
  if (lane == 0) s_pmax[wave] = pmax2;
  __syncthreads();
  pmax2 = s_pmax[0];
#pragma unroll
  for (int w = 1; w < BLOCK / 64; ++w) pmax2 = fmaxf(pmax2, s_pmax[w]);
  return pmax2;
}

// a lane's box [lo, hi] becomes the workgroup's; s_box: BLOCK / 64 x 6 floats of LDS
template <int BLOCK>
__device__ __forceinline__ void workgroup_box(float (&lo)[3], float (&hi)[3], float (*s_box)[6], int lane, int wave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s_box[wave][a] = lo[a];
      s_box[wave][3 + a] = hi[a];
    }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = s_box[0][a];
    hi[a] = s_box[0][3 + a];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) {
      lo[a] = fminf(lo[a], s_box[w][a]);
      hi[a] = fmaxf(hi[a], s_box[w][3 + a]);
    }
  }
}

// ---- bf16 operands -----------------------------------------------------------------------------------------------------------
// two floats -> two bf16 (round to nearest even) in one dword, `lo` in the low half: v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned int pack_bf16(float lo, float hi) {
  const floatx2 f = {lo, hi};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(f, bf16x2));
}
__device__ __forceinline__ float bf16_lo(unsigned int p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf16_hi(unsigned int p) { return __uint_as_float(p & 0xffff0000u); }
__device__ __forceinline__ unsigned int dup_lo(unsigned int p) { return __builtin_amdgcn_perm(p, p, 0x01000100u); }
__device__ __forceinline__ unsigned int dup_hi(unsigned int p) { return __builtin_amdgcn_perm(p, p, 0x03020302u); }

// B operand (K x N = sources) of the source at u = p - c: the lanes of half 0 supply K slots 0-7, those of half 1 slots 8-15 (two
// bf16 per dword):  half 0: (Uxh, Uxl) (Uxh, Uxl) (Uyh, Uyl) (Uyh, Uyl)      half 1: (Uzh, Uzl) (Uzh, Uzl) (1, 1) (0, 0)
__device__ __forceinline__ uint4 bf16_source_operand(float ux, float uy, float uz, int half) {
  const float Ux = -2.0f * ux, Uy = -2.0f * uy, Uz = -2.0f * uz;
  const unsigned int hxy = pack_bf16(Ux, Uy), lxy = pack_bf16(Ux - bf16_lo(hxy), Uy - bf16_hi(hxy));
  const unsigned int hz = pack_bf16(Uz, 1.0f), lz = pack_bf16(Uz - bf16_lo(hz), 0.0f);
  const unsigned int dx = (hxy & 0xffffu) | (lxy << 16), dy = (hxy >> 16) | (lxy & 0xffff0000u);
  const unsigned int dz = (hz & 0xffffu) | (lz << 16);
  return half ? make_uint4(dz, dz, 0x3F803F80u, 0u) : make_uint4(dx, dx, dy, dy);
}

// A operands (M x K = targets) of the target at v = q - c, one 16-byte record for the lanes of each half-wave (K slots 0-7: x and
// y products; 8-15: z products and S):  (vxh, vxh) (vxl, vxl) (vyh, vyh) (vyl, vyl) | (vzh, vzh) (vzl, vzl) (Sh, Sl) (0, 0)
// (scale tiny: the products sit near the denormal range, where the matrix path may flush -- such a target is simply always
// evaluated exactly; a NaN scale keeps its NaN)
__device__ __forceinline__ void bf16_target_records(float vx, float vy, float vz, float pmax2, uint4& r0, uint4& r1) {
  const float q2 = len2(vx, vy, vz);
  const float scale = pmax2 + q2;
  const float S = scale < kTinyScale ? -INFINITY : q2 - scale * kTauBf16;
  const unsigned int hxy = pack_bf16(vx, vy), lxy = pack_bf16(vx - bf16_lo(hxy), vy - bf16_hi(hxy));
  const unsigned int hzs = pack_bf16(vz, S), lzs = pack_bf16(vz - bf16_lo(hzs), isinf(S) ? 0.0f : S - bf16_hi(hzs));
  r0 = make_uint4(dup_lo(hxy), dup_lo(lxy), dup_hi(hxy), dup_hi(lxy));
  r1 = make_uint4(dup_lo(hzs), dup_lo(lzs), (hzs >> 16) | (lzs & 0xffff0000u), 0u);
}
// a row past the end can never undercut a bound: S = +inf
__device__ __forceinline__ void bf16_padding_records(uint4& r0, uint4& r1) {
  r0 = make_uint4(0u, 0u, 0u, 0u);
  r1 = make_uint4(0u, 0u, 0x00007F80u, 0u);
}

// ---- the seed rule of the brute-force kernels ---------------------------------------------------------------------------------
// Nothing known: the empty key and an infinite bound.  Seed (optional): the neighbour this source found in the previous sweep
// over the same target.  It is a target point whatever the transform is now, so its exact key is a valid candidate and its
// distance a valid bound from the first tile on: in an ICP iteration nearly nothing undercuts it (without a seed the bound
// improves ~ln(N) times per source).
__device__ __forceinline__ void seed_brute(const unsigned long long* __restrict__ seed, int orig, const float4* __restrict__ tgt,
                                           int n_t, float px, float py, float pz, float p2, unsigned long long& best, float& bound) {
  best = kEmptyKey;
  bound = INFINITY;
  if (seed) {
    const unsigned int j = (unsigned int)seed[orig];
    if (j < (unsigned int)n_t) {
      const float4 t = tgt[j];
      const float e = dist2(t.x, t.y, t.z, px, py, pz);
      if (e < INFINITY) {
        best = key_of(e, j);
        bound = bound_of(e, p2);
      }
    }
  }
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------
// The folds are v_min3_f32 by hand (fminf on MFMA outputs makes the compiler canonicalise every operand first: 6 extra
// instructions per fold).  Inline assembly is opaque to the compiler's hazard recogniser, which is what inserts the wait states
// between an MFMA and the first vector read of its result -- so every accumulator is FIRST read by an instruction the compiler
// can see (it waits there), between two scheduling barriers: nothing may be scheduled across.  The f32 kernel does that with a
// readfirstlane of its own; the bf16 kernels with first_read_tails below, which does a fold's work too: v_med3_f32(a, b, -inf)
// = min(a, b); with a NaN among its operands the hardware returns their min3 = -inf, i.e. the step of a non-finite target goes
// through the exact path (where its NaN / inf distance never wins) instead of being dropped -- correct, and rare.
__device__ __forceinline__ float opaque_minus_inf() {  // (a literal -inf makes the compiler rewrite the v_med3 as a canonicalising minimum)
  float minus_inf;
  asm volatile("v_mov_b32 %0, 0xff800000" : "=v"(minus_inf));
  return minus_inf;
}
template <int G>
__device__ __forceinline__ void first_read_tails(const floatx16 (&acc)[G], float minus_inf, float (&tail)[G]) {
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < G; ++g) tail[g] = __builtin_amdgcn_fmed3f(acc[g][14], acc[g][15], minus_inf);
  __builtin_amdgcn_sched_barrier(0);
}
// the five partial minima of a lane's 16 values (tail = the minimum of d[14], d[15]): part[k] covers d[3k .. 3k + 2], part[4]
// d[12 .. 15].  A NaN (a non-finite point) is dropped by the minimum and fails the comparison with the bound.
__device__ __forceinline__ void fold_parts(const floatx16& d, float tail, float (&part)[5]) {
  part[0] = min3f(d[0], d[1], d[2]);
  part[1] = min3f(d[3], d[4], d[5]);
  part[2] = min3f(d[6], d[7], d[8]);
  part[3] = min3f(d[9], d[10], d[11]);
  part[4] = min3f(d[12], d[13], tail);
}
__device__ __forceinline__ float fold_min(const float (&part)[5]) { return min3f(min3f(part[0], part[1], part[2]), part[3], part[4]); }
__device__ __forceinline__ float fold(const floatx16& d, float tail) {
  float part[5];
  fold_parts(d, tail, part);
  return fold_min(part);
}

// ---- the exact re-check ----------------------------------------------------------------------------------------------------------
// (brute force) the values of one accumulator that undercut the bound of its source: their targets -- rows st + row_of(v) of
// the tile, below lim; index jt + st + row -- are evaluated exactly.  NaN and inf distances never win (the VALU kernel's rule).
__device__ __forceinline__ void recheck_brute(const floatx16& d, int half, const float4* tile, int st, int lim, int jt, float px,
                                              float py, float pz, float p2, unsigned long long& best, float& bound) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    if (d[v] <= bound) {
      const int row = row_of(v, half);
      if (st + row < lim) {
        const float4 t = tile[st + row];
        const float e = dist2(t.x, t.y, t.z, px, py, pz);
        const unsigned long long key = key_of(e, (unsigned int)(jt + st + row));
        if (e < INFINITY && key < best) {
          best = key;
          bound = bound_of(e, p2);
        }
      }
    }
  }
}

// ---- the end -----------------------------------------------------------------------------------------------------------------
// the two half-waves hold the same sources: the smaller of their keys, in both
__device__ __forceinline__ unsigned long long merge_halves(unsigned long long best) {
  const unsigned long long other = shfl_xor_u64(best, 32);
  return other < best ? other : best;
}
// under the source's original index; target splits merge by atomic minimum (keys pre-filled with kEmptyKey)
__device__ __forceinline__ void write_key(unsigned long long* __restrict__ keys, int orig, unsigned long long k, int splits) {
  if (splits > 1) atomicMin(&keys[orig], k);
  else keys[orig] = k;
}

}  // namespace
}  // namespace icpgpu
