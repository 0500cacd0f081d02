// icp_reject.hip -- device side of the correspondence rejectors (pcl::registration::CorrespondenceRejectorMedianDistance,
// ...Trimmed, ...OneToOne; PCL 1.8): stages that run between a key-writing correspondence search and the keys reduction of the
// method, and REWRITE KEYS -- a rejected pair's key becomes kEmptyKey, so the reductions behind them run unchanged.
//
// A pair is ALIVE when its key names a target and its d2 (the key's high word) passes the gate, d2 <= thr -- the predicate of
// reduce_kernel and p2plane_reduce_kernel.  Every kernel here judges keys by it, so a search may leave anything it likes in the
// keys of points beyond the gate.
//
//   Order statistic (median, trimmed).  d2 >= 0, so its float bit pattern orders as an unsigned integer: an MSB-first radix select
//   over three histograms of integer counts (digits of 11, 11 and 10 bits).  reject_hist_kernel<P> counts digit P of the alive
//   pairs whose higher digits equal the ones selected so far; each workgroup counts in LDS and adds its non-zero bins to the
//   stage's histogram in device memory (integer atomics commute: the same counts from run to run).  Nothing is handed from one
//   launch to the next but the histograms: every workgroup re-derives the rank k (from the first histogram's total: n / 2, or
//   the trimmed rule's m - 1) and the digits selected so far by scanning the histograms in front of it (2048 counts each: 8 KiB
//   out of L2).  reject_cut_apply_kernel derives the cut the same way and empties every alive key above it.
//   One-to-one.  reject_winner_kernel: 64-bit atomicMin of (d2 bits << 32 | source index) into winners[target index] (all ones
//   before); reject_winner_apply_kernel keeps a pair iff it is its target's winner.
//
//   Surface normal.  reject_normal_kernel: one launch; per alive pair the source's normal (coalesced) rotated by the iteration's T
//   (xform_normal) and the gathered target normal; the pair stays iff (double)dot > threshold (normal_dot: float32, strict; a NaN
//   dot is rejected).  8 B + 16 B + 16 B read per alive pair, 8 B written per rejected pair.
//
// Per stage: 4 launches (order statistic), 2 (one-to-one) or 1 (surface normal); 8 B read per pair and pass, 8 B written per rejected pair by the
// apply pass; 8 B per target point set and 8 B per alive pair updated for the winner array.  The statistics of a stage (pairs
// in, pairs out, the cut's bits) stay in device memory behind its histograms (RejectState) until the host asks for them.
#include "icp_device.h"
#include "icp_kernels.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int RJ_BLOCK = 256;
constexpr int kRejectMaxBlocks = 1024;

__device__ __forceinline__ bool key_alive(unsigned long long key, float thr) {
  return (unsigned int)key != 0xFFFFFFFFu && __uint_as_float((unsigned int)(key >> 32)) <= thr;
}

// digit P of a d2 pattern, and the bits above digit P
template <int P>
__device__ __forceinline__ unsigned int digit_of(unsigned int bits) {
  return P == 0 ? bits >> 21 : P == 1 ? (bits >> 10) & 2047u : bits & 1023u;
}
template <int P>
__device__ __forceinline__ unsigned int above_of(unsigned int bits) {
  return P == 0 ? 0u : P == 1 ? bits >> 21 : bits >> 10;
}

// The whole workgroup: the bin of hist[0 .. nbins) that holds rank k (0-based) of its counts, the rank within that bin, and the
// total.  found = false when k >= total.  nbins is a multiple of RJ_BLOCK.
struct BinPick {
  unsigned int bin, k_in_bin, total;
  bool found;
};
__device__ BinPick pick_bin(const unsigned int* __restrict__ hist, int nbins, unsigned int k) {
  __shared__ unsigned int scan[RJ_BLOCK];
  __shared__ unsigned int res[2];
  const int per = nbins / RJ_BLOCK, t = threadIdx.x;
  unsigned int mine = 0;
  for (int b = 0; b < per; ++b) mine += hist[t * per + b];
  __syncthreads();  // (scan / res may still be read from an earlier call)
  scan[t] = mine;
  if (t == 0) res[0] = 0xFFFFFFFFu;
  __syncthreads();
  for (int off = 1; off < RJ_BLOCK; off <<= 1) {  // inclusive scan, Hillis-Steele
    const unsigned int v = t >= off ? scan[t - off] : 0u;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const unsigned int incl = scan[t], excl = incl - mine;
  if (k >= excl && k < incl) {  // exactly one thread
    unsigned int run = excl;
    for (int b = 0; b < per; ++b) {
      const unsigned int cnt = hist[t * per + b];
      if (k < run + cnt) {
        res[0] = (unsigned int)(t * per + b);
        res[1] = k - run;
        break;
      }
      run += cnt;
    }
  }
  __syncthreads();
  BinPick p;
  p.total = scan[RJ_BLOCK - 1];
  p.found = res[0] != 0xFFFFFFFFu;
  p.bin = res[0];
  p.k_in_bin = res[1];
  return p;
}

// the rank (0-based) of the cut among n alive pairs; false = the stage keeps nothing (n = 0, or the trimmed rule's m = 0)
__device__ __forceinline__ bool rank_of_cut(const RejectStage& S, unsigned int n, unsigned int& k) {
  if (n == 0) return false;
  if (S.kind == kRejectMedian) {
    k = n / 2;  // nth_element at size() / 2
    return true;
  }
  // CorrespondenceRejectorTrimmed: min(n, max(min_correspondences, (unsigned)(overlap_ratio * (float)n))), the product in float32
  unsigned int m = (unsigned int)__fmul_rn(S.ratio, (float)n);
  if (m < S.min_corr) m = S.min_corr;
  if (m > n) m = n;
  if (m == 0) return false;
  k = m - 1;
  return true;
}

// The digits selected by the histograms in front of pass P (the whole workgroup; the same answer in every workgroup).
// prefix = the selected digits as the high bits of the pattern; k = the rank within what is left; go = false: nothing to select.
template <int P>
__device__ bool select_so_far(const unsigned int* state, const RejectStage& S, unsigned int& prefix, unsigned int& k,
                              unsigned int& n_in) {
  prefix = 0;
  k = 0;
  n_in = 0;
  if (P == 0) return true;
  BinPick a = pick_bin(state + kRejectHist0, 2048, 0u);  // (the total; the rank needs it first)
  n_in = a.total;
  if (!rank_of_cut(S, n_in, k)) return false;
  a = pick_bin(state + kRejectHist0, 2048, k);
  prefix = a.bin;
  k = a.k_in_bin;
  if (P == 1) return true;
  a = pick_bin(state + kRejectHist1, 2048, k);
  prefix = (prefix << 11) | a.bin;
  k = a.k_in_bin;
  if (P == 2) return true;
  a = pick_bin(state + kRejectHist2, 1024, k);
  prefix = (prefix << 10) | a.bin;
  k = a.k_in_bin;
  return true;
}

template <int P>
__global__ __launch_bounds__(RJ_BLOCK) void reject_hist_kernel(const unsigned long long* __restrict__ keys, int n, float thr, RejectStage S,
                                                               unsigned int* state) {
  constexpr int kBins = P == 2 ? 1024 : 2048;
  __shared__ unsigned int bins[kBins];
  for (int b = threadIdx.x; b < kBins; b += RJ_BLOCK) bins[b] = 0u;
  unsigned int prefix, k, n_in;
  const bool go = select_so_far<P>(state, S, prefix, k, n_in);  // (uniform; ends on a barrier, so the zeroes above are visible)
  if (!go) return;
  __syncthreads();
  for (int i = blockIdx.x * RJ_BLOCK + threadIdx.x; i < n; i += gridDim.x * RJ_BLOCK) {
    const unsigned long long key = keys[i];
    const unsigned int bits = (unsigned int)(key >> 32);
    if (key_alive(key, thr) && above_of<P>(bits) == prefix) atomicAdd(&bins[digit_of<P>(bits)], 1u);
  }
  __syncthreads();
  unsigned int* hist = state + (P == 0 ? kRejectHist0 : P == 1 ? kRejectHist1 : kRejectHist2);
  for (int b = threadIdx.x; b < kBins; b += RJ_BLOCK)
    if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

__global__ __launch_bounds__(RJ_BLOCK) void reject_cut_apply_kernel(unsigned long long* __restrict__ keys, int n, float thr, RejectStage S,
                                                                    unsigned int* state) {
  unsigned int cut_bits, k, n_in;
  const bool have_cut = select_so_far<3>(state, S, cut_bits, k, n_in);
  // median: keep (double)d2 <= (double)median * factor; trimmed: keep d2 <= the m-th smallest (ties at the cut all stay)
  const double cut = __uint_as_float(cut_bits);
  const double limit = S.kind == kRejectMedian ? cut * S.factor : cut;
  unsigned int kept = 0;
  for (int i = blockIdx.x * RJ_BLOCK + threadIdx.x; i < n; i += gridDim.x * RJ_BLOCK) {
    const unsigned long long key = keys[i];
    if (!key_alive(key, thr)) continue;
    const bool keep = have_cut && (double)__uint_as_float((unsigned int)(key >> 32)) <= limit;
    if (keep) kept += 1;
    else keys[i] = kEmptyKey;
  }
  block_count_add(kept, state + kRejectStats + 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state[kRejectStats + 0] = n_in;
    state[kRejectStats + 2] = have_cut ? cut_bits : 0u;
  }
}

__global__ __launch_bounds__(RJ_BLOCK) void reject_winner_kernel(const unsigned long long* __restrict__ keys, int n, float thr, int n_t,
                                                                 unsigned long long* __restrict__ winners, unsigned int* __restrict__ state) {
  unsigned int alive = 0;
  for (int i = blockIdx.x * RJ_BLOCK + threadIdx.x; i < n; i += gridDim.x * RJ_BLOCK) {
    const unsigned long long key = keys[i];
    const unsigned int j = (unsigned int)key;
    if (!key_alive(key, thr) || j >= (unsigned int)n_t) continue;
    alive += 1;
    atomicMin(&winners[j], (key & 0xFFFFFFFF00000000ull) | (unsigned long long)(unsigned int)i);
  }
  block_count_add(alive, state + kRejectStats + 0);
}

__global__ __launch_bounds__(RJ_BLOCK) void reject_winner_apply_kernel(unsigned long long* __restrict__ keys, int n, float thr, int n_t,
                                                                       const unsigned long long* __restrict__ winners,
                                                                       unsigned int* __restrict__ state) {
  unsigned int kept = 0;
  for (int i = blockIdx.x * RJ_BLOCK + threadIdx.x; i < n; i += gridDim.x * RJ_BLOCK) {
    const unsigned long long key = keys[i];
    const unsigned int j = (unsigned int)key;
    if (!key_alive(key, thr)) continue;
    if (j < (unsigned int)n_t && winners[j] == ((key & 0xFFFFFFFF00000000ull) | (unsigned long long)(unsigned int)i)) kept += 1;
    else keys[i] = kEmptyKey;
  }
  block_count_add(kept, state + kRejectStats + 1);
}

__global__ __launch_bounds__(RJ_BLOCK) void reject_normal_kernel(unsigned long long* __restrict__ keys, int n, float thr, int n_t,
                                                                 const float4* __restrict__ src_normals,
                                                                 const float4* __restrict__ tgt_normals, Xform T, double threshold,
                                                                 unsigned int* __restrict__ state) {
  unsigned int alive = 0, kept = 0;
  for (int i = blockIdx.x * RJ_BLOCK + threadIdx.x; i < n; i += gridDim.x * RJ_BLOCK) {
    const unsigned long long key = keys[i];
    if (!key_alive(key, thr)) continue;
    alive += 1;
    const unsigned int j = (unsigned int)key;
    bool keep = false;
    if (j < (unsigned int)n_t) {
      const float4 a = src_normals[i], b = tgt_normals[j];
      float n1x, n1y, n1z;
      xform_normal(T, a.x, a.y, a.z, n1x, n1y, n1z);
      keep = (double)normal_dot(n1x, n1y, n1z, b.x, b.y, b.z) > threshold;
    }
    if (keep) kept += 1;
    else keys[i] = kEmptyKey;
  }
  block_count_add(alive, state + kRejectStats + 0);
  block_count_add(kept, state + kRejectStats + 1);
}

__global__ __launch_bounds__(RJ_BLOCK) void reject_unpack_kernel(const unsigned long long* __restrict__ keys, int n, float thr,
                                                                 int32_t* __restrict__ idx, float* __restrict__ d2) {
  const int i = blockIdx.x * RJ_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  const bool alive = key_alive(key, thr);
  idx[i] = alive ? (int32_t)(unsigned int)key : -1;
  d2[i] = alive ? __uint_as_float((unsigned int)(key >> 32)) : __uint_as_float(0x7F800000u);
}

int reject_blocks(int n) {
  int blocks = (n + 4 * RJ_BLOCK - 1) / (4 * RJ_BLOCK);  // ~4 pairs per lane
  if (blocks > kRejectMaxBlocks) blocks = kRejectMaxBlocks;
  return blocks < 1 ? 1 : blocks;
}

}  // namespace

hipError_t launch_reject_chain(unsigned long long* keys, int n_s, int n_t, float thr, const RejectStage* stages, int n_stages,
                               unsigned int* state, unsigned long long* winners, hipStream_t stream, const float4* src_normals,
                               const float4* tgt_normals, const Xform* T) {
  if (n_stages <= 0) return hipSuccess;
  if (n_stages > kRejectMaxStages) return hipErrorInvalidValue;
  for (int s = 0; s < n_stages; ++s)
    if (stages[s].kind == kRejectSampleConsensus) return hipErrorInvalidValue;  // (the host's stage: the caller splits the chain around it)
  hipError_t e = hipMemsetAsync(state, 0, (size_t)n_stages * kRejectStateInts * sizeof(unsigned int), stream);
  if (e != hipSuccess) return e;
  const dim3 grid(reject_blocks(n_s)), block(RJ_BLOCK);
  for (int s = 0; s < n_stages; ++s) {
    const RejectStage& S = stages[s];
    unsigned int* st = state + (size_t)s * kRejectStateInts;
    if (S.kind == kRejectOneToOne) {
      if (n_t > 0 && (e = hipMemsetAsync(winners, 0xFF, (size_t)n_t * sizeof(unsigned long long), stream)) != hipSuccess) return e;
      hipLaunchKernelGGL(reject_winner_kernel, grid, block, 0, stream, keys, n_s, thr, n_t, winners, st);
      hipLaunchKernelGGL(reject_winner_apply_kernel, grid, block, 0, stream, keys, n_s, thr, n_t, winners, st);
    } else if (S.kind == kRejectSurfaceNormal) {
      if (!T || (n_s > 0 && n_t > 0 && (!src_normals || !tgt_normals))) return hipErrorInvalidValue;
      hipLaunchKernelGGL(reject_normal_kernel, grid, block, 0, stream, keys, n_s, thr, n_t, src_normals, tgt_normals, *T, S.factor, st);
    } else {
      hipLaunchKernelGGL(reject_hist_kernel<0>, grid, block, 0, stream, keys, n_s, thr, S, st);
      hipLaunchKernelGGL(reject_hist_kernel<1>, grid, block, 0, stream, keys, n_s, thr, S, st);
      hipLaunchKernelGGL(reject_hist_kernel<2>, grid, block, 0, stream, keys, n_s, thr, S, st);
      hipLaunchKernelGGL(reject_cut_apply_kernel, grid, block, 0, stream, keys, n_s, thr, S, st);
    }
  }
  return hipGetLastError();
}

hipError_t launch_reject_unpack(const unsigned long long* keys, int n, float thr, int32_t* idx, float* d2, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(reject_unpack_kernel, dim3((n + RJ_BLOCK - 1) / RJ_BLOCK), dim3(RJ_BLOCK), 0, stream, keys, n, thr, idx, d2);
  return hipGetLastError();
}

}  // namespace icpgpu
