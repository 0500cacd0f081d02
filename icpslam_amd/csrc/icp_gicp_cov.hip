// icp_gicp_cov.hip -- computeCovariances of the GICP mode, and the point-to-plane mode's surface
// normals from the same patches: per point the 20 smallest (d2, index) keys of its own cloud, the covariance in double from float
// products, its smallest singular direction u, C = I - (1 - 1e-3) u u^T (== U diag(1, 1, 1e-3) U^T).  The streaming kernel, the
// selecting form, its far field and the finish kernels are described where they stand.  (One evaluation: icp_gicp.hip.)
#include <math.h>
#include <algorithm>
#include <cstdlib>

#include "icp_env.h"
#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int GK = kGicpK;  // 20

// Left singular vectors of a symmetric 3x3 (row-major), columns by decreasing singular value: Eigen::JacobiSVD<Matrix3d>(A,
// ComputeFullU).matrixU() as the CPU checker restates it for computeCovariances (Eigen 3.3's two-sided Jacobi iteration on the
// scaled matrix, pairs (1,0) (2,0) (2,1), a pair rotated while an off-diagonal exceeds 2 eps x the largest diagonal met so far,
// real_2x2_jacobi_svd + makeJacobi, diagonal signs into U, descending selection sort) -- OPERATION FOR OPERATION: on a patch
// with two (nearly) equal singular values the vectors are whatever the method's rounding makes them, and a regularised
// covariance that differs in its 10th digit is a different optimisation problem for the chaotic BFGS that follows.
// Until round 3 both sides ran a one-sided iteration whose stopping rule was relative to each column pair: 0.6 % of a scan's
// patches (near-planar: the third column is noise) hovered at it for all 60 sweeps and every wave waited for such a lane
// (136 us per 22k-point cloud); Eigen's rule is relative to the LARGEST singular value and ends after 2-4 sweeps.
constexpr int kSvdMaxSweeps = 64;  // (Eigen has no cap; this one only guards non-finite input, the checker has the same)
__device__ __forceinline__ void svd_rot_rows(double* W, int p, int q, double c, double s) {
  if (c == 1.0 && s == 0.0) return;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double xi = W[3 * p + i], yi = W[3 * q + i];
    W[3 * p + i] = c * xi + s * yi;
    W[3 * q + i] = -s * xi + c * yi;
  }
}
__device__ __forceinline__ void svd_rot_cols(double* W, int p, int q, double c, double s) {
  if (c == 1.0 && s == 0.0) return;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double xi = W[3 * i + p], yi = W[3 * i + q];
    W[3 * i + p] = c * xi - s * yi;
    W[3 * i + q] = s * xi + c * yi;
  }
}
__device__ void svd3_left_vectors(const double A[9], double U[9]) {
  const double kMin = 2.2250738585072014e-308, kEps = 2.220446049250313e-16;  // DBL_MIN, DBL_EPSILON
  double scale = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i)
    if (fabs(A[i]) > scale) scale = fabs(A[i]);
  if (scale == 0.0) scale = 1.0;
  double W[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    W[i] = A[i] / scale;
    U[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
  const double precision = 2.0 * kEps;
  double max_diag = fmax(fabs(W[0]), fmax(fabs(W[4]), fabs(W[8])));
  for (int sweep = 0; sweep < kSvdMaxSweeps; ++sweep) {
    bool finished = true;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 0 ? 1 : 2, q = pq == 2 ? 1 : 0;  // (1,0) (2,0) (2,1)
      const double threshold = fmax(kMin, precision * max_diag);
      if (!(fabs(W[3 * p + q]) > threshold || fabs(W[3 * q + p]) > threshold)) continue;
      finished = false;
      double m00 = W[3 * p + p], m01 = W[3 * p + q], m10 = W[3 * q + p], m11 = W[3 * q + q];
      double c1, s1;
      const double t = m00 + m11, d = m10 - m01;
      if (fabs(d) < kMin) {
        s1 = 0.0;
        c1 = 1.0;
      } else {
        const double u = t / d, tmp = sqrt(1.0 + u * u);
        s1 = 1.0 / tmp;
        c1 = u / tmp;
      }
      if (!(c1 == 1.0 && s1 == 0.0)) {
        const double a0 = m00, a1 = m01, b0 = m10, b1 = m11;
        m00 = c1 * a0 + s1 * b0;
        m01 = c1 * a1 + s1 * b1;
        m10 = -s1 * a0 + c1 * b0;
        m11 = -s1 * a1 + c1 * b1;
      }
      double cr, sr;
      const double deno = 2.0 * fabs(m01);
      if (deno < kMin) {
        cr = 1.0;
        sr = 0.0;
      } else {
        const double tau = (m00 - m11) / deno, w = sqrt(tau * tau + 1.0);
        const double tt = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
        const double sign_t = tt > 0.0 ? 1.0 : -1.0, n = 1.0 / sqrt(tt * tt + 1.0);
        sr = -sign_t * (m01 / fabs(m01)) * fabs(tt) * n;
        cr = n;
      }
      const double cl = c1 * cr - s1 * (-sr), sl = c1 * (-sr) + s1 * cr;
      svd_rot_rows(W, p, q, cl, sl);
      svd_rot_cols(U, p, q, cl, -sl);
      svd_rot_cols(W, p, q, cr, sr);
      max_diag = fmax(max_diag, fmax(fabs(W[3 * p + p]), fabs(W[3 * q + q])));
    }
    if (finished) break;
  }
  double sv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double a = fabs(W[4 * i]);
    sv[i] = a * scale;
    if (a != 0.0) {
      const double f = W[4 * i] / a;
#pragma unroll
      for (int r = 0; r < 3; ++r) U[3 * r + i] *= f;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    int pos = i;
#pragma unroll
    for (int k = i + 1; k < 3; ++k)
      if (sv[k] > sv[pos]) pos = k;
    if (sv[pos] == 0.0) break;
    if (pos != i) {
      const double ts = sv[i];
      sv[i] = sv[pos];
      sv[pos] = ts;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double tu = U[3 * r + i];
        U[3 * r + i] = U[3 * r + pos];
        U[3 * r + pos] = tu;
      }
    }
  }
}

// ---- computeCovariances -----------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_lds_handover();
__device__ __forceinline__ void cov_emit(const unsigned long long* top, double* scratch, const float4* __restrict__ cloud, int i, double* __restrict__ cov6, int lane);

// (list, optional: the points gicp_cov_select_kernel left over -- list[0 .. *list_n); without it every point of the cloud)
__global__ __launch_bounds__(256) void gicp_cov_kernel(const float4* __restrict__ cloud, int n,
                                                       const float4* __restrict__ sorted, const int* __restrict__ cell_start, GridDesc g,
                                                       double* __restrict__ cov6, const int* __restrict__ list,
                                                       const int* __restrict__ list_n) {
  __shared__ unsigned long long s_key[4][GK];  // per-wave staging of the top-20 while it is re-ranked
  __shared__ int s_pos[4][GK];
  __shared__ double s_scratch[4][9 * GK + 9];  // cov_emit's terms and sums
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // one wave per point; with a list: a few hundred waves walk it (it is short or empty: an empty launch sized for the cloud cost 4.6 us)
  for (int slot = blockIdx.x * 4 + wv;; slot += gridDim.x * 4) {
  int i = slot;
  if (list) {
    if (slot >= *list_n) return;
    i = list[slot];
  }
  if (i >= n) return;
  const float4 s = cloud[i];
  bool have_patch = false;
  if (finite3(s.x, s.y, s.z)) {
    int cx, cy, cz;
    cell_of(g, s.x, s.y, s.z, cx, cy, cz);
    const int span = max(g.nx, max(g.ny, g.nz));
    unsigned long long mykey = kEmptyKey;  // lanes 0..19: the running top-20 (unordered)
    int mypos = -1;
    for (int rho = 1;; rho *= 2) {
      mykey = kEmptyKey;
      mypos = -1;
      unsigned long long kth = kEmptyKey;  // largest key among the 20 slots
      const int side = 2 * rho + 1, nrows = side * side;
      const int x0 = max(cx - rho, 0), x1 = min(cx + rho, g.nx - 1);
      const float inv_side = 1.0f / (float)side;
      for (int rb = 0; rb < nrows; rb += 64) {
        const int r = rb + lane;
        const int zr = (int)(((float)r + 0.5f) * inv_side), yr = r - zr * side;
        const int yy = cy + yr - rho, zz = cz + zr - rho;
        int lo = 0, len = 0;
        if (r < nrows && x0 <= x1 && yy >= 0 && yy < g.ny && zz >= 0 && zz < g.nz) {
          const int row = zz * g.sz + yy * g.sy;
          lo = cell_start[row + x0];
          len = cell_start[row + x1 + 1] - lo;
        }
        // The batch's rows as ONE list of candidates, 64 per chunk (round 4; until then one row -- ~24 candidates at cells sized for
        // ~8 points then -- per chunk, later two): an exclusive scan of the row lengths over the lanes, and every lane of a chunk finds
        // the row of its entry by a binary search over those offsets (six lane reads).  A merge round's ~100 fixed instructions
        // are then spent on 64 candidates, not on 24.
        int incl = len;
        ICPGPU_WAVE_INCLUSIVE_SCAN(incl, lane);
        const int start = incl - len, total = __shfl(incl, 63, 64);
        for (int c0 = 0; c0 < total; c0 += 64) {  // wave-uniform
          {
            const int e = c0 + lane;
            int rr = 0;  // the LAST lane whose offset is <= e (empty rows share their successor's offset: the successor wins)
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) {
              const int probe = rr + step;
              const int sp = __shfl(start, probe & 63, 64);
              if (probe < 64 && sp <= e) rr = probe;
            }
            const int rlo = __shfl(lo, rr, 64), rst = __shfl(start, rr, 64);
            unsigned long long ckey = kEmptyKey;
            const int cpos = rlo + (e - rst);
            if (e < total) {
              const float4 q = sorted[cpos];
              const float d = dist2(q.x, q.y, q.z, s.x, s.y, s.z);
              ckey = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(q.w);
            }
            const unsigned long long better = __ballot(ckey < kth);
            if (better) {  // wave-uniform
              // Merge the chunk's improving candidates into the sorted top-20 (lanes 0..19) by RANK: keys are distinct
              // (the index is part of the key), so "how many keys of the union are smaller than mine" is my slot.
              // ~80 + 6 * popcount(better) instructions per chunk, against ~40 per candidate for one-at-a-time insertion
              // (measured: covariances of a 200k-point cloud 4.75 -> 4.25 ms; most of the kernel's time is the row walk).
              int rank_top = (int)lane;  // slots below me among the current top keys (they are sorted); lanes < GK only
              int rank_cand = 0;
              for (unsigned long long m = better; m; m &= m - 1) {
                const int j = __ffsll((long long)m) - 1;
                const unsigned long long bk = readlane_u64(ckey, j);
                rank_top += bk < mykey ? 1 : 0;
                rank_cand += bk < ckey ? 1 : 0;
              }
#pragma unroll
              for (int j = 0; j < GK; ++j) rank_cand += readlane_u64(mykey, j) < ckey ? 1 : 0;  // empty slots hold the maximum key
              if (lane < GK) {
                s_key[wv][lane] = kEmptyKey;
                s_pos[wv][lane] = -1;
              }
              if (lane < GK && mykey != kEmptyKey && rank_top < GK) {
                s_key[wv][rank_top] = mykey;
                s_pos[wv][rank_top] = mypos;
              }
              if (((better >> lane) & 1ull) && rank_cand < GK) {
                s_key[wv][rank_cand] = ckey;
                s_pos[wv][rank_cand] = cpos;
              }
              if (lane < GK) {
                mykey = s_key[wv][lane];
                mypos = s_pos[wv][lane];
              }
              kth = readlane_u64(mykey, GK - 1);
            }
          }
        }
      }
      const float safe = (float)rho * g.h * kGridSafety;
      const bool full = kth != kEmptyKey;  // all 20 slots filled
      if ((full && __uint_as_float((unsigned int)(kth >> 32)) <= safe * safe) || rho >= span) break;
    }
    // Lanes 0..19 hold the neighbours in key order (every merge hands lane r the key of rank r): staged in LDS in that order,
    // their moments are the selecting kernels' (cov_emit: sequential sums, the oracle's order), handed to gicp_cov_finish_kernel.
    if (__popcll(__ballot(lane < GK && mypos >= 0)) == GK) {
      if (lane < GK) s_key[wv][lane] = mykey;
      wave_lds_handover();
      cov_emit(s_key[wv], s_scratch[wv], cloud, i, cov6, lane);
      have_patch = true;
    }
  }
  if (!have_patch && lane < 6)  // marker: identity covariance
    cov6[(size_t)i * 6 + lane] = lane == 0 ? __longlong_as_double(0x7FF8000000000000ll) : (lane == 3 || lane == 5 ? 1.0 : 0.0);
  if (!list) return;
  }
}

// ---- shared by the selecting kernels: from a list of >= 20 keys to the covariance ---------------------------------------------
constexpr int CS = 4;            // 256 keys per level in registers (a scan filtered at 0.2 m has ~60 inside a level's radius)
constexpr int CS_LIST = 64 * CS;

// Lanes of ONE wave hand data to each other through LDS below (a list appended to by some lanes and read by others).  The LDS
// operations of a wave complete in order, so no instruction is needed -- but the memory model orders one lane's stores before
// another lane's loads only across a synchronisation: a wavefront-scope release / acquire fence pair around a wave barrier says so
// (no instruction beyond, at most, a wait for the LDS counter).
__device__ __forceinline__ void wave_lds_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// buf[0 .. fill): distinct keys (d2 bits << 32 | index), all <= cap_key, 20 <= fill <= CS_LIST; one wave.  On return lanes 0..19
// of `top` (LDS, 20 words) hold the 20 smallest in ascending order.  The threshold is lowered on the float distance while that
// separates, then by bisection on the 64-bit keys themselves (dozens of equal distances: the index part decides) -- keys are
// distinct, so a threshold with 20..64 keys below it always exists.
__device__ __forceinline__ void cov_pick20(unsigned long long* buf, unsigned long long* top, int fill, unsigned long long cap_key, int lane,
                                           unsigned long long lane_lt, int& probes, int& ranked) {
  unsigned long long K[CS];
  const int nreg = (fill + 63) >> 6;  // wave-uniform: registers in use
  wave_lds_handover();  // (the list was appended to by whichever lanes found the keys)
#pragma unroll
  for (int m = 0; m < CS; ++m) K[m] = (m < nreg && m * 64 + lane < fill) ? buf[m * 64 + lane] : kEmptyKey;
  auto count_le = [&](unsigned long long T) {
    int c = 0;
#pragma unroll
    for (int m = 0; m < CS; ++m)
      if (m < nreg) c += __popcll(__ballot(K[m] <= T));
    return c;
  };
  // lower the threshold until 20 .. 64 keys pass: [T_lo: fewer than 20 (at most the key 0 itself), T: at least 20]
  unsigned long long T_lo = 0ull, T = cap_key;
  int c_lo = 0, c_hi = fill;
  bool by_key = false;
  for (int probe = 0; c_hi > 64; ++probe) {
    unsigned long long Tm = 0ull;
    if (!by_key) {
      // interpolate for ~40 on d2 (the first probes), bisect afterwards
      const float lo_f = __uint_as_float((unsigned int)(T_lo >> 32)), hi_f = __uint_as_float((unsigned int)(T >> 32));
      float mid = probe < 6 ? lo_f + (hi_f - lo_f) * ((40.0f - (float)c_lo) / (float)(c_hi - c_lo)) : 0.5f * (lo_f + hi_f);
      if (!(mid > lo_f && mid < hi_f)) mid = 0.5f * (lo_f + hi_f);
      if (probe >= 12 || !(mid > lo_f && mid < hi_f)) by_key = true;  // (adjacent floats: more than 44 keys at one distance)
      else Tm = ((unsigned long long)__float_as_uint(mid) << 32) | 0xFFFFFFFFull;
    }
    if (by_key) Tm = T_lo + ((T - T_lo) >> 1);  // strictly inside: T - T_lo >= 2 while more than one key lies between them
    probes += 1;
    const int cm = count_le(Tm);
    if (cm < GK) {
      T_lo = Tm;
      c_lo = cm;
    } else {
      T = Tm;
      c_hi = cm;
    }
  }
  // compact the passing keys, one per lane (the list is in registers: its first 64 entries are free again)
  unsigned long long k = K[0];  // (a list of one register's length that passes whole is in place already)
  if (!(nreg == 1 && c_hi == fill)) {
    wave_lds_handover();  // (every lane has its part of the list in registers before the buffer is written again)
    int base = 0;
#pragma unroll
    for (int m = 0; m < CS; ++m)
      if (m < nreg) {
        const unsigned long long b = __ballot(K[m] <= T);
        if (K[m] <= T) buf[base + __popcll(b & lane_lt)] = K[m];
        base += __popcll(b);
      }
    wave_lds_handover();
    k = lane < c_hi ? buf[lane] : kEmptyKey;
  }
  int rank = 0;
  const int c8 = c_hi & ~7;
  for (int j = 0; j < c8; j += 8) {  // wave-uniform addresses: broadcast reads, eight in flight
    unsigned long long v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = buf[j + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) rank += v[u] < k ? 1 : 0;
  }
  for (int j = c8; j < c_hi; ++j) rank += buf[j] < k ? 1 : 0;
  if (lane < c_hi && rank < GK) top[rank] = k;
  wave_lds_handover();  // (top[] is read by lanes 0..19 next: cov_emit)
  ranked = c_hi;
}

// Lanes 0..19 of `top` hold the neighbours in key order: mean and second moments (float products widened to double) as the oracle
// and PCL's computeCovariances form them -- each of the nine sums added from zero ONE TERM AFTER ANOTHER in key order, by one lane
// over the terms in LDS -- and one lane per covariance entry does its three divisions.  The order matters: where a patch straddles
// a coordinate plane the terms span many binades and the double sums round (a wave butterfly's sums differed from
// the oracle's on ~1 point in 10^5: scripts/cov_campaign.py).  One wave; `scratch`: 189 doubles of LDS (the selecting
// kernels pass the key list's buffer: the list is dead).  gicp_cov_kernel emits through here too.
__device__ __forceinline__ void cov_emit(const unsigned long long* top, double* scratch, const float4* __restrict__ cloud, int i,
                                         double* __restrict__ cov6, int lane) {
  double* term = scratch;  // [9][20]
  if (lane < GK) {
    const float4 q = cloud[(unsigned int)top[lane]];  // (the grid's sorted copy holds the same coordinates under the same index)
    term[0 * GK + lane] = (double)q.x;
    term[1 * GK + lane] = (double)q.y;
    term[2 * GK + lane] = (double)q.z;
    term[3 * GK + lane] = (double)(q.x * q.x);  // (the second moments in the order of the triangle's entries)
    term[4 * GK + lane] = (double)(q.y * q.x);
    term[5 * GK + lane] = (double)(q.z * q.x);
    term[6 * GK + lane] = (double)(q.y * q.y);
    term[7 * GK + lane] = (double)(q.z * q.y);
    term[8 * GK + lane] = (double)(q.z * q.z);
  }
  double* sums = term + 9 * GK;  // [9]
  wave_lds_handover();
  if (lane < 9) {
    const volatile double* v = term + lane * GK;  // (volatile: read in the order of use -- all twenty at once cost 40 registers)
    double sum = 0.0;
#pragma unroll
    for (int l = 0; l < GK; ++l) sum += v[l];
    sums[lane] = sum;
  }
  wave_lds_handover();
  if (lane < 6) {
    // entry e = (row r, column c) of the upper triangle: (0,0) (1,0) (2,0) (1,1) (2,1) (2,2), second moments at sums[3 + e]
    const int r = lane == 0 ? 0 : (lane == 1 || lane == 3 ? 1 : 2), cidx = lane < 3 ? 0 : (lane < 5 ? 1 : 2);
    const double kk = (double)GK;
    const double mr = sums[r] / kk, mc = sums[cidx] / kk;
    cov6[(size_t)i * 6 + lane] = sums[3 + lane] / kk - mr * mc;
  }
}

// The points the selecting kernel's cubes do not reach cheaply -- isolated far-field points whose 20th neighbour is metres away: cube
// radii 8, 16, ... cells are hundreds to thousands of rows walked in one dependent chain (27 row batches, ~65 us, for a point
// certified at radius 16; a handful of them per scan set the kernel's duration) -- and the rare ones its caps cannot settle
// (hundreds of points at one distance).  Here a WORKGROUP takes such a point and looks at the whole cloud (a filtered scan: ~23k
// points, 23 per thread): a pass collects the keys under a cap into the list; the first cap extrapolates the count the last cube
// found inside its radius (neighbours on a surface grow with d2) to ~60, later ones interpolate between the caps tried -- usually
// one pass -- and when float distances no longer separate, the caps become 64-bit keys and are bisected as such (keys are distinct:
// that always ends).  Then the same selection and sums as above.  Exact whatever the caps were: every point of the cloud is looked
// at; a cloud with fewer than 20 finite points gets the identity marker, as in gicp_cov_kernel.  It is also the whole covariance
// pass of a cloud the k-NN grid refuses (thousands of points in one cell of the largest table: gicp_cov_all_far_kernel queues every
// point).  Clouds above kGicpCovFarMost points keep the streaming kernel for these points.
// far_list entries: point index | code << 20; code 0..19 = the keys the last cube found inside r_tried, 31 = no such knowledge.
constexpr int kCovFarLevel = 4;  // the last cube radius (cells) the selecting kernel tries before it hands a point over
constexpr int kCovFarNoHint = 31;
__global__ __launch_bounds__(1024) void gicp_cov_far_kernel(const float4* __restrict__ cloud, int n, double* __restrict__ cov6, float r_tried,
                                                            const int* __restrict__ far_list, const int* __restrict__ far_n) {
  __shared__ unsigned long long s_buf[CS_LIST];
  __shared__ unsigned long long s_top[GK];
  __shared__ int s_count;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned long long lane_lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  auto key_of = [](float d2, unsigned int idx) -> unsigned long long { return ((unsigned long long)__float_as_uint(d2) << 32) | idx; };
  for (int slot = blockIdx.x; slot < *far_n; slot += gridDim.x) {
    const int packed = far_list[slot];
    const int i = packed & 0xFFFFF, code = (packed >> 20) & 31;
    const float4 s = cloud[i];
    // the keys <= cap: their number, the first CS_LIST of them in s_buf (any order: they are ranked later)
    auto pass = [&](unsigned long long cap) -> int {
      __syncthreads();
      if (tid == 0) s_count = 0;
      __syncthreads();
      for (int j0 = 0; j0 < n; j0 += 8192) {  // block-uniform; eight loads in flight per thread
        float4 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = j0 + u * 1024 + tid;
          q[u] = j < n ? cloud[j] : make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = j0 + u * 1024 + tid;
          const unsigned long long key = key_of(dist2(q[u].x, q[u].y, q[u].z, s.x, s.y, s.z), (unsigned int)j);
          const bool in = finite3(q[u].x, q[u].y, q[u].z) && key <= cap;  // (the grid's sorted copy leaves non-finite points out: so do we)
          const unsigned long long b = __ballot(in);
          if (b) {  // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_count, __popcll(b));
            base = __shfl(base, 0, 64);
            const int at = base + __popcll(b & lane_lt);
            if (in && at < CS_LIST) s_buf[at] = key;
          }
        }
      }
      __syncthreads();
      return s_count;
    };
    // [lo: fewer than 20 keys (the key 0 alone at most), hi: more than the list holds]
    const bool hint = code != kCovFarNoHint;
    unsigned long long lo = hint ? key_of(r_tried * r_tried, 0xFFFFFFFFu) : 0ull, hi = 0ull;
    int n_lo = hint ? code : 0, n_hi = 0, fill = 0;
    unsigned long long cap = key_of(r_tried * r_tried * (hint ? 60.0f / (float)max(code, 2) : 1.0f), 0xFFFFFFFFu);
    bool settled = false, by_key = false;
    for (int pass_no = 0; pass_no < 200; ++pass_no) {
      fill = pass(cap);
      if (fill >= GK && fill <= CS_LIST) {
        settled = true;
        break;
      }
      if (fill < GK) {
        lo = cap;
        n_lo = fill;
      } else {
        hi = cap;
        n_hi = fill;
      }
      if (n_hi == 0) {  // nothing above yet: grow (by the same rule)
        const float c = __uint_as_float((unsigned int)(cap >> 32));
        float next = c * (fill < 5 ? 8.0f : 60.0f / (float)fill);
        if (!(next > c)) next = c > 0.0f ? c * 2.0f : 1.0e-12f;
        if (!(next < 3.0e38f)) break;  // fewer than 20 finite points in the cloud
        cap = key_of(next, 0xFFFFFFFFu);
        continue;
      }
      if (!by_key) {
        const float lo_f = __uint_as_float((unsigned int)(lo >> 32)), hi_f = __uint_as_float((unsigned int)(hi >> 32));
        float mid = pass_no < 8 ? lo_f + (hi_f - lo_f) * ((60.0f - (float)n_lo) / (float)(n_hi - n_lo)) : 0.5f * (lo_f + hi_f);
        if (!(mid > lo_f && mid < hi_f)) mid = 0.5f * (lo_f + hi_f);
        if (pass_no >= 40 || !(mid > lo_f && mid < hi_f)) by_key = true;  // hundreds of keys at one distance: the index part decides
        else cap = key_of(mid, 0xFFFFFFFFu);
      }
      if (by_key) cap = lo + ((hi - lo) >> 1);
    }
    if (tid < 64) {  // one wave finishes
      if (settled) {
        int probes = 0, ranked = 0;
        cov_pick20(s_buf, s_top, fill, cap, lane, lane_lt, probes, ranked);
        cov_emit(s_top, reinterpret_cast<double*>(s_buf), cloud, i, cov6, lane);
      } else if (lane < 6) {  // (the marker of an identity covariance, as gicp_cov_kernel writes it for a cloud of fewer than 20 points)
        cov6[(size_t)i * 6 + lane] = lane == 0 ? __longlong_as_double(0x7FF8000000000000ll) : (lane == 3 || lane == 5 ? 1.0 : 0.0);
      }
    }
  }
}

// every finite point of the cloud onto the far-field kernel's list (no hint), the marker for the others: the covariance pass of a
// cloud that has no grid
__global__ __launch_bounds__(256) void gicp_cov_all_far_kernel(const float4* __restrict__ cloud, int n, double* __restrict__ cov6,
                                                               int* __restrict__ far_list, int* __restrict__ far_n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 s = cloud[i];
  if (finite3(s.x, s.y, s.z)) {
    far_list[atomicAdd(far_n, 1)] = i | (kCovFarNoHint << 20);
  } else {
    double* c = cov6 + (size_t)i * 6;
    c[0] = __longlong_as_double(0x7FF8000000000000ll);
    c[1] = c[2] = c[4] = 0.0;
    c[3] = c[5] = 1.0;
  }
}

// computeCovariances, the SELECTING form (round 6).  gicp_cov_kernel above streams candidates 64 at a time into a running top-20 and
// pays ~100 + 6 x (improving candidates) instructions per chunk -- 460 for the first chunk of every level, when all 64 improve --
// in ONE dependent chain per point; a dense corner of a scan (a thousand candidates in the first cube) kept a wave for 30 us.
// Here a level's candidates (the cube of radius rho cells around the point) are only EVALUATED, and the keys (d2 bits << 32 |
// index) that lie within a distance cap -- the level's certified radius to begin with -- are appended to a per-wave LDS list:
//   * a level succeeds iff >= 20 keys lie within its certified radius (the 20th neighbour is then known to be the true one); a
//     level that fails has cost nothing but the evaluations;
//   * a list that overflows (> 256 keys inside the radius: a dense corner) is collected again under a smaller cap, aimed at ~128
//     keys by interpolating on d2 (neighbours on a surface grow linearly with it);
//   * from the list, held in registers, a threshold is lowered the same way until 20..64 keys pass; those are compacted into one
//     lane each and ranked by counting (keys are distinct): ranks 0..19 are the neighbours, in key order.
// The next chunk's load is in flight while a chunk is processed, and rows are found by counting over at most 25 lane reads instead
// of a six-step search through the LDS crossbar: the kernel is a latency chain per point, not an issue problem (23k waves for 8k
// slots).  Same neighbours, same order, same sums as gicp_cov_kernel (tests/test_gpu_gicp.py compares the covariances bit for bit
// with it and with the oracle).  A point whose caps do not settle (dozens of equal distances) or whose search reaches the whole
// grid goes on a list, and gicp_cov_kernel finishes the list.
template <bool STATS>
#if defined(ICPGPU_COV_WAVES8)  // A/B build: 64 registers (a few spilled) for 8 waves per SIMD instead of 72 for 7 (no difference measured)
__attribute__((amdgpu_waves_per_eu(8, 8)))
#else
__attribute__((amdgpu_waves_per_eu(7, 8)))  // (left alone the compiler spreads to 108 registers: 4 waves per SIMD for a latency-bound kernel)
#endif
__global__ __launch_bounds__(256) void gicp_cov_select_kernel(const float4* __restrict__ cloud, int n,
                                                              const float4* __restrict__ sorted,
                                                              const int* __restrict__ cell_start, GridDesc g,
                                                              double* __restrict__ cov6, int* __restrict__ list,
                                                              int* __restrict__ list_n, int far_ok, int* __restrict__ far_list,
                                                              int* __restrict__ far_n, unsigned long long* __restrict__ stats) {
#define CS_STAT(k, v) do { if (STATS && lane == 0) atomicAdd(stats + (k), (unsigned long long)(v)); } while (0)
  __shared__ unsigned long long s_buf[4][CS_LIST];
  __shared__ unsigned long long s_top[4][GK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;  // one wave per point
  if (i >= n) return;
  const float4 s = cloud[i];
  if (!finite3(s.x, s.y, s.z)) {  // (as gicp_cov_kernel: the marker of an identity covariance)
    if (lane < 6) cov6[(size_t)i * 6 + lane] = lane == 0 ? __longlong_as_double(0x7FF8000000000000ll) : (lane == 3 || lane == 5 ? 1.0 : 0.0);
    return;
  }
  int cx, cy, cz;
  cell_of(g, s.x, s.y, s.z, cx, cy, cz);
  const int span = max(g.nx, max(g.ny, g.nz));
  const unsigned long long lane_lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  unsigned long long* buf = s_buf[wv];
  bool done = false, give_up = false, go_far = false;
  int last_seen = 0;  // keys inside the radius of the last level that failed
  for (int rho = 1; !done && !give_up; rho *= 2) {
    if (far_ok && rho > kCovFarLevel) {  // wave-uniform
      go_far = true;
      break;
    }
    const int side = 2 * rho + 1, nrows = side * side;
    const int x0 = max(cx - rho, 0), x1 = min(cx + rho, g.nx - 1);
    const float inv_side = 1.0f / (float)side;
    const float safe = (float)rho * g.h * kGridSafety;
    const float safe_sq = safe * safe;
    // One pass over the level's candidates: the keys with d2 <= cap into buf (the first CS_LIST of them), their number returned.
    // Under a cap below the level's radius only the cells the cap's ball reaches are read (box pruning on the SAME float cell
    // coordinates that binned the points, which are monotone in x: a point within sqrt(cap) of s cannot lie in a skipped cell).
    // A list that overflows ends the pass at once (levels of one row batch): `est` then extrapolates the count from the share of
    // the candidates seen so far -- a guide for the next cap, not a result.
    auto collect = [&](float cap, int& est) -> int {
      int fill = 0;
      const float r_cap = sqrtf(cap) * 1.0001f + g.h * 0.03125f;
      const int xa = (int)fmaxf(floorf((s.x - r_cap - g.ox) * g.inv_h), -4.0f), xb = (int)fminf(floorf((s.x + r_cap - g.ox) * g.inv_h), 1048576.0f);
      const int ya = (int)fmaxf(floorf((s.y - r_cap - g.oy) * g.inv_h), -4.0f), yb = (int)fminf(floorf((s.y + r_cap - g.oy) * g.inv_h), 1048576.0f);
      const int za = (int)fmaxf(floorf((s.z - r_cap - g.oz) * g.inv_h), -4.0f), zb = (int)fminf(floorf((s.z + r_cap - g.oz) * g.inv_h), 1048576.0f);
      const int xx0 = max(x0, xa), xx1 = min(x1, xb);
      for (int rb = 0; rb < nrows; rb += 64) {
        const int r = rb + lane;
        const int zr = (int)(((float)r + 0.5f) * inv_side), yr = r - zr * side;
        const int yy = cy + yr - rho, zz = cz + zr - rho;
        int lo = 0, len = 0;
        if (r < nrows && xx0 <= xx1 && yy >= max(0, ya) && yy <= min(g.ny - 1, yb) && zz >= max(0, za) && zz <= min(g.nz - 1, zb)) {
          const int row = zz * g.sz + yy * g.sy;
          lo = cell_start[row + xx0];
          len = cell_start[row + xx1 + 1] - lo;
        }
        int incl = len;
        ICPGPU_WAVE_INCLUSIVE_SCAN(incl, lane);
        const int start = incl - len, total = __shfl(incl, 63, 64);
        if (nrows <= 64 && total < GK) {  // fewer than 20 points in reach: nothing to evaluate
          est = total;
          return total;
        }
        const int rows_here = min(nrows - rb, 64);
        // entry e of the batch's candidate list lives in the LAST row whose offset is <= e (empty rows share their successor's
        // offset: the successor wins) -- (rows with offset <= e) - 1, counted over lane reads when the rows are few
        auto locate = [&](int e) -> int {
          int rr = 0;
          if (rows_here <= 25) {
            for (int j = 1; j < rows_here; ++j) rr += __builtin_amdgcn_readlane(start, j) <= e ? 1 : 0;
          } else {
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) {
              const int probe = rr + step;
              const int sp = __shfl(start, probe & 63, 64);
              if (probe < 64 && sp <= e) rr = probe;
            }
          }
          return __shfl(lo, rr, 64) + (e - __shfl(start, rr, 64));
        };
        // (locate() moves data between lanes: every lane of the wave takes part in it, only the load is conditional)
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        int at0 = locate(lane);
        if (lane < total) q = sorted[at0];
        for (int c0 = 0; c0 < total; c0 += 64) {  // wave-uniform
          const float4 cur = q;
          const bool live = c0 + lane < total;
          if (c0 + 64 < total) {  // wave-uniform: the next chunk's load, in flight during this one
            const int at1 = locate(c0 + 64 + lane);
            if (c0 + 64 + lane < total) q = sorted[at1];
          }
          const float d = dist2(cur.x, cur.y, cur.z, s.x, s.y, s.z);
          const bool pass = live && d <= cap;
          const unsigned long long b = __ballot(pass);
          const int at = fill + __popcll(b & lane_lt);
          if (pass && at < CS_LIST) buf[at] = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(cur.w);
          fill += __popcll(b);
          if (fill > CS_LIST && nrows <= 64) {  // wave-uniform: overflow
            const int seen = min(c0 + 64, total);
            est = (int)fminf((float)fill * ((float)total / (float)seen), 1.0e9f);
            return fill;
          }
        }
      }
      est = fill;
      return fill;
    };
    CS_STAT(2, 1);
    // the level's radius first; a list that overflows (a dense corner) again under smaller caps, [lo_c: fewer than 20 keys, hi_c: more
    // than the list holds], aimed at ~100 keys by interpolating on d2
    float cap = safe_sq, lo_c = 0.0f, hi_c = safe_sq;
    int fill = 0, est = 0, n_lo = 0, n_hi = 0;
    bool level_fails = false;
    for (int pass_no = 0;; ++pass_no) {
      fill = collect(cap, est);
      if (pass_no == 0 && fill < GK) {  // the level cannot certify 20 neighbours
        level_fails = true;
        break;
      }
      if (fill >= GK && fill <= CS_LIST) break;
      if (pass_no == 0) CS_STAT(3, 1);
      if (fill < GK) {
        lo_c = cap;
        n_lo = fill;
      } else {
        hi_c = cap;
        n_hi = est;
      }
      float mid = pass_no < 4 ? lo_c + (hi_c - lo_c) * ((100.0f - (float)n_lo) / (float)(n_hi - n_lo)) : 0.5f * (lo_c + hi_c);
      if (!(mid > lo_c && mid < hi_c)) mid = 0.5f * (lo_c + hi_c);
      if (pass_no >= 12 || !(mid > lo_c && mid < hi_c)) {
        give_up = true;
        CS_STAT(4, 1);
        break;
      }
      cap = mid;
    }
    if (level_fails) {
      last_seen = fill;
      if (rho >= span) { give_up = true; CS_STAT(5, 1); }  // (the whole grid has been looked at: gicp_cov_kernel's closing rule applies)
      continue;
    }
    if (give_up) break;
    CS_STAT(1, fill);
    int probes = 0, ranked = 0;
    cov_pick20(buf, s_top[wv], fill, ((unsigned long long)__float_as_uint(cap) << 32) | 0xFFFFFFFFull, lane, lane_lt, probes, ranked);
    done = true;
    CS_STAT(6, probes);
    CS_STAT(7, ranked);
    CS_STAT(0, 1);
    CS_STAT(8 + min(31 - __clz(rho), 7), 1);  // histogram of the level that succeeded: rho = 1, 2, 4, ... 128+
  }
#undef CS_STAT
  if (!done) {
    // far_ok (clouds up to kGicpCovFarMost points): whatever is not done -- no cube of up to kCovFarLevel cells certified the point,
    // the caps did not settle -- goes to gicp_cov_far_kernel; in larger clouds to gicp_cov_kernel
    if (lane == 0) {
      if (go_far) far_list[atomicAdd(far_n, 1)] = i | (last_seen << 20);  // (i < kGicpCovFarMost, last_seen < 20)
      else if (far_ok) far_list[atomicAdd(far_n, 1)] = i | (kCovFarNoHint << 20);  // caps that did not settle, the whole grid searched
      else list[atomicAdd(list_n, 1)] = i;
    }
    return;
  }
  cov_emit(s_top[wv], reinterpret_cast<double*>(buf), cloud, i, cov6, lane);
}

// The 3x3 decomposition, ONE LANE PER POINT: inside the search kernel every lane of the wave repeated it (several thousand
// double-precision instructions per point, the largest part of that kernel's time); here 64 points share a wave.
// (zero2, optional: the two list counters of launch_gicp_covariances, left zero for the next cloud -- every kernel that reads them has run)
__global__ __launch_bounds__(256) void gicp_cov_finish_kernel(int n, double* __restrict__ cov6, int* __restrict__ zero2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (zero2 && i == 0) zero2[0] = zero2[1] = 0;
  if (i >= n) return;
  double* c = cov6 + (size_t)i * 6;
  const double a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3], a4 = c[4], a5 = c[5];
  double C[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
  if (a0 == a0) {  // not the marker
    const double A[9] = {a0, a1, a2, a1, a3, a4, a2, a4, a5};
    double U[9];
    svd3_left_vectors(A, U);
    // C = sum_k v_k u_k u_k^T with v = (1, 1, epsilon): the loop of PCL's computeCovariances, in its order
    const int rr[6] = {0, 1, 2, 1, 2, 2}, cc[6] = {0, 0, 0, 1, 1, 2};  // (0,0) (1,0) (2,0) (1,1) (2,1) (2,2)
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double v = (k == 2) ? kGicpEpsilon : 1.0;
        acc += v * U[3 * rr[e] + k] * U[3 * cc[e] + k];
      }
      C[e] = acc;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = C[k];
}

// The point-to-plane mode's surface normals (icp_p2plane.hip): the same raw covariance and the same
// svd3_left_vectors as gicp_cov_finish_kernel, but instead of the regularised covariance the third column of U -- the direction
// computeCovariances scales by epsilon -- rounded to float and turned towards the viewpoint (0, 0, 0) as PCL's
// flipNormalTowardsViewpoint does: cos = ((vx nx + vy ny) + vz nz) in float with v = 0 - p, flipped when cos < 0.  Marker points
// (non-finite, or a cloud of fewer than 20 finite points) get (NaN, NaN, NaN, 0).  cov6 is left holding the raw covariances.
__global__ __launch_bounds__(256) void gicp_normal_finish_kernel(const float4* __restrict__ cloud, int n, const double* __restrict__ cov6,
                                                                 float4* __restrict__ normals, int* __restrict__ zero2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (zero2 && i == 0) zero2[0] = zero2[1] = 0;
  if (i >= n) return;
  const double* c = cov6 + (size_t)i * 6;
  const double a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3], a4 = c[4], a5 = c[5];
  float4 out = make_float4(__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000), 0.0f);
  if (a0 == a0) {  // not the marker
    const double A[9] = {a0, a1, a2, a1, a3, a4, a2, a4, a5};
    double U[9];
    svd3_left_vectors(A, U);
    float nx = (float)U[2], ny = (float)U[5], nz = (float)U[8];
    const float4 p = cloud[i];
    const float vx = __fsub_rn(0.0f, p.x), vy = __fsub_rn(0.0f, p.y), vz = __fsub_rn(0.0f, p.z);
    const float cos_theta = __fadd_rn(__fadd_rn(__fmul_rn(vx, nx), __fmul_rn(vy, ny)), __fmul_rn(vz, nz));
    if (cos_theta < 0.0f) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    out = make_float4(nx, ny, nz, 0.0f);
  }
  normals[i] = out;
}

}  // namespace

// list (optional): 2 n + 2 ints of scratch -- with it the selecting kernel runs first, the far-field kernel takes what that one hands
// over (clouds up to kGicpCovFarMost points; in larger ones gicp_cov_kernel finishes the list); without it gicp_cov_kernel does
// every point, as until round 5.
hipError_t launch_gicp_covariances(const float4* cloud, int n, const float4* sorted, const int* cell_start,
                                   const GridDesc& g, double* cov6, hipStream_t stream, int* list, bool list_counters_zero,
                                   float4* normals) {
  if (n <= 0) return hipSuccess;
  // development flavour, ICPGPU_COV_SELECT=0: the streaming kernel for every point
  static const bool select = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_COV_SELECT"); return !e || atoi(e) != 0; }();
  if (list && select) {
    if (!list_counters_zero) {  // (a fresh buffer; afterwards the finish kernel leaves them zero: one launch less per cloud)
      hipError_t e = hipMemsetAsync(list, 0, 2 * sizeof(int), stream);
      if (e != hipSuccess) return e;
    }
    // development flavour, ICPGPU_COV_STATS=1: what the selecting kernel did with the cloud (a synchronising print per cloud)
    static const bool want_stats = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_COV_STATS"); return e && atoi(e) != 0; }();
    unsigned long long* d_stats = nullptr;
    if (want_stats && hipMalloc(reinterpret_cast<void**>(&d_stats), 16 * sizeof(unsigned long long)) == hipSuccess)
      (void)hipMemsetAsync(d_stats, 0, 16 * sizeof(unsigned long long), stream);
    // list layout: [0] streaming count, [1] far count, [2 .. 2 + n) streaming list, [2 + n .. 2 + 2n) far list
    const int far_ok = n <= kGicpCovFarMost ? 1 : 0;
    int* far_list = list + 2 + n;
    if (d_stats)
      hipLaunchKernelGGL(gicp_cov_select_kernel<true>, dim3((n + 3) / 4), dim3(256), 0, stream, cloud, n, sorted, cell_start, g, cov6, list + 2, list, far_ok,
                         far_list, list + 1, d_stats);
    else
      hipLaunchKernelGGL(gicp_cov_select_kernel<false>, dim3((n + 3) / 4), dim3(256), 0, stream, cloud, n, sorted, cell_start, g, cov6, list + 2, list, far_ok,
                         far_list, list + 1, d_stats);
    if (far_ok)  // (the first cap: the radius the last cube tried has already failed)
      hipLaunchKernelGGL(gicp_cov_far_kernel, dim3(std::min(n, 256)), dim3(1024), 0, stream, cloud, n, cov6, (float)kCovFarLevel * g.h * kGridSafety, far_list,
                         list + 1);
    if (d_stats) {
      unsigned long long h[16];
      (void)hipStreamSynchronize(stream);
      (void)hipMemcpy(h, d_stats, sizeof(h), hipMemcpyDeviceToHost);
      (void)hipFree(d_stats);
      fprintf(stderr, "[icpgpu] covariances of %d points (cells of %.3f m): %llu selected (%.1f levels, %.0f keys inside the certified radius, %.2f threshold probes, %.1f keys ranked "
                      "each), %llu dense corners collected again; handed on: %llu caps not settled, %llu whole grid searched\n", n, (double)g.h, h[0],
              (double)h[2] / (double)(h[0] ? h[0] : 1), (double)h[1] / (double)(h[0] ? h[0] : 1), (double)h[6] / (double)(h[0] ? h[0] : 1),
              (double)h[7] / (double)(h[0] ? h[0] : 1), h[3], h[4], h[5]);
      int h_lists[2] = {0, 0};
      (void)hipMemcpy(h_lists, list, sizeof(h_lists), hipMemcpyDeviceToHost);
      fprintf(stderr, "[icpgpu]   handed over: %d to the far-field kernel, %d to the streaming kernel (before the far-field kernel ran)\n", h_lists[1], h_lists[0]);
      fprintf(stderr, "[icpgpu]   points by the cube radius (in cells) that certified them: 1: %llu, 2: %llu, 4: %llu, 8: %llu, 16: %llu, 32: %llu, 64: %llu, more: %llu\n", h[8],
              h[9], h[10], h[11], h[12], h[13], h[14], h[15]);
    }
    // (with the far-field kernel nothing is left over: it settles every point it is handed)
    if (!far_ok) hipLaunchKernelGGL(gicp_cov_kernel, dim3(std::min((n + 3) / 4, 128)), dim3(256), 0, stream, cloud, n, sorted, cell_start, g, cov6, list + 2, list);
  } else {
    hipLaunchKernelGGL(gicp_cov_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, cloud, n, sorted, cell_start, g, cov6, nullptr, nullptr);
  }
  if (normals)  // (the point-to-plane mode: normals instead of regularised covariances; cov6 keeps the raw ones)
    hipLaunchKernelGGL(gicp_normal_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud, n, cov6, normals,
                       (list && select) ? list : nullptr);
  else
    hipLaunchKernelGGL(gicp_cov_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, cov6, (list && select) ? list : nullptr);
  return hipGetLastError();
}

// The covariances of a cloud WITHOUT a grid (the k-NN grid refuses a cloud whose densest cell of the largest table holds thousands of
// points): every finite point through the far-field kernel's whole-cloud passes.  n <= kGicpCovFarMost; list as above.
hipError_t launch_gicp_covariances_brute(const float4* cloud, int n, double* cov6, hipStream_t stream, int* list, bool list_counters_zero,
                                         float4* normals) {
  if (n <= 0) return hipSuccess;
  if (n > kGicpCovFarMost || !list) return hipErrorInvalidValue;
  if (!list_counters_zero) {
    hipError_t e = hipMemsetAsync(list, 0, 2 * sizeof(int), stream);
    if (e != hipSuccess) return e;
  }
  int* far_list = list + 2 + n;
  hipLaunchKernelGGL(gicp_cov_all_far_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud, n, cov6, far_list, list + 1);
  hipLaunchKernelGGL(gicp_cov_far_kernel, dim3(std::min(n, 1024)), dim3(1024), 0, stream, cloud, n, cov6, 0.05f, far_list, list + 1);
  if (normals)
    hipLaunchKernelGGL(gicp_normal_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud, n, cov6, normals, list);
  else
    hipLaunchKernelGGL(gicp_cov_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, cov6, list);
  return hipGetLastError();
}

}  // namespace icpgpu
