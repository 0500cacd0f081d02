// icp_ndt.hip -- device side of the NDT mode: pcl::NormalDistributionsTransform with pcl::VoxelGridCovariance (PCL 1.8).
//
// Cell build, once per target cloud and resolution (host: icpgpu_ndt.cpp, ensure_ndt_cells):
//   ndt_key_kernel       the voxel filter's cell key of every point (icp_voxel.hip: voxel_key_kernel's arithmetic, operation for
//                        operation), then launch_radix_sort_pairs (stable: a cell's points stay in input order)
//   ndt_flag_kernel      first sorted position of every cell; an exclusive scan numbers the cells
//   ndt_cell_kernel      one lane per cell: float sums in input order -> the voxel filter's centroid; double S = sum x and
//                        Q = sum x x^T in input order -> mean, PCL's covariance, a cyclic Jacobi eigen-decomposition in double,
//                        the eigenvalue floor, icov = cov^-1 (cofactors) and the validity test
//   ndt_compact_kernel   the valid cells, in key order: key, float4 centroid, {mean(3), icov(6)} as 10 doubles, n
//   ndt_stats_kernel     one workgroup: number of valid cells and the largest distance, in cell units, by which a valid cell's
//                        float centroid lies outside its own cell (the derivative pass widens its stencil by it: exact search)
// Derivative pass, once per evaluation (PCL's computeDerivatives):
//   ndt_deriv_kernel     one lane per source point: q = T * x (float, xform_point), every valid cell whose centroid c has float
//                        (dx^2 + dy^2) + dz^2 <= r^2 (the cells come from a per-axis range of lattice indices and a binary search of
//                        the sorted keys per (y, z) row), then per pair PCL's updateDerivatives in double: 29 terms per lane
//                        (pairs, score, gradient 6, Hessian upper triangle 21), one partial per workgroup (fixed shuffle + LDS tree)
//   ndt_grad_kernel      the More-Thuente line search's trial pass (ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE): the same lane, pair
//                        arithmetic and tree for the first 8 terms only (pairs, score, gradient), without A, M and the Hessian --
//                        its 8 sums are the bits of ndt_deriv_kernel's first 8 at the same pose (both are ndt_pass<>)
//   p2plane_final_kernel (icp_p2plane.hip, launch_terms29_final) adds the partials in a fixed order into the result mailbox
#include <math.h>

#include "icp_device.h"
#include "icp_jacobi3.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

constexpr int kNdtSentinel = 0x7FFFFFFF;  // key of points that are not binned (non-finite): sorts last
constexpr int ND_BLOCK = 256;
constexpr int kNdtMaxBlocks = 1024;

__global__ __launch_bounds__(256) void ndt_key_kernel(const float4* __restrict__ pts, int n, float inv_leaf, int minb_x, int minb_y,
                                                      int minb_z, int mul_y, int mul_z, int* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  int key = kNdtSentinel;
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const int ix = (int)floorf(p.x * inv_leaf) - minb_x;
    const int iy = (int)floorf(p.y * inv_leaf) - minb_y;
    const int iz = (int)floorf(p.z * inv_leaf) - minb_z;
    key = ix + iy * mul_y + iz * mul_z;
  }
  keys[i] = key;
  vals[i] = i;
}

__global__ __launch_bounds__(256) void ndt_flag_kernel(const int* __restrict__ keys, int n, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = keys[i];
  flags[i] = (k != kNdtSentinel && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

// (the cells' eigen-decomposition, jacobi3: icp_jacobi3.h -- shared with icp_normals.hip)

// one lane per cell (the first sorted position of its points); every cell's record goes to slot slots[i]
__global__ __launch_bounds__(256) void ndt_cell_kernel(const float4* __restrict__ pts, const int* __restrict__ keys,
                                                       const int* __restrict__ vals, const int* __restrict__ flags,
                                                       const int* __restrict__ slots, int n, NdtLattice L, int* __restrict__ valid,
                                                       int* __restrict__ ckey, float4* __restrict__ cent, double* __restrict__ gauss,
                                                       int* __restrict__ npts, double* __restrict__ excess) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const int k = keys[i];
  float ax = 0.f, ay = 0.f, az = 0.f;
  double S[3] = {0.0, 0.0, 0.0}, Q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // the cell's points eight at a time: their keys, indices and coordinates are independent loads; the sums take them in order
  int j = i;
  for (bool more = true; more;) {
    int kk[8], vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = min(j + u, n - 1);
      kk[u] = keys[idx];
      vv[u] = vals[idx];
    }
    float4 pp[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pp[u] = pts[vv[u]];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (more && j < n && kk[u] == k) {
        const float4 p = pp[u];
        ax += p.x;
        ay += p.y;
        az += p.z;
        const double x[3] = {(double)p.x, (double)p.y, (double)p.z};
        S[0] += x[0];
        S[1] += x[1];
        S[2] += x[2];
        Q[0] += x[0] * x[0];
        Q[1] += x[0] * x[1];
        Q[2] += x[0] * x[2];
        Q[3] += x[1] * x[1];
        Q[4] += x[1] * x[2];
        Q[5] += x[2] * x[2];
        ++j;
      } else {
        more = false;
      }
    }
  }
  const int cnt = j - i;
  const float fc = (float)cnt;
  const float4 c = make_float4(ax / fc, ay / fc, az / fc, 1.0f);
  const int slot = slots[i];
  ckey[slot] = k;
  cent[slot] = c;
  npts[slot] = cnt;
  int ok = 0;
  double* g = gauss + (size_t)slot * kNdtGaussDoubles;
  const double nd = (double)cnt;
  const double m[3] = {S[0] / nd, S[1] / nd, S[2] / nd};
  for (int a = 0; a < 3; ++a) g[a] = m[a];
  if (cnt >= kNdtMinPoints) {
    // cov = ((Q - 2 (S m^T)) / n + m m^T) * ((n - 1) / n), entry by entry as Eigen evaluates PCL's expression; the LOWER
    // triangle's entries (row >= column: S_row m_col), the ones SelfAdjointEigenSolver reads, mirrored
    const double f = (nd - 1.0) / nd;
    const int ri[6] = {0, 0, 0, 1, 1, 2}, ci[6] = {0, 1, 2, 1, 2, 2};
    double cov[3][3];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const int r = ri[e], cc = ci[e];
      const double v = ((Q[e] - 2.0 * (S[cc] * m[r])) / nd + m[cc] * m[r]) * f;
      cov[r][cc] = cov[cc][r] = v;
    }
    double a[3][3], V[3][3];
    for (int r = 0; r < 3; ++r)
      for (int cc = 0; cc < 3; ++cc) a[r][cc] = cov[r][cc];
    jacobi3(a, V);
    // eigenvalues ascending (the order SelfAdjointEigenSolver returns them in), eigenvectors with them
    double lam[3] = {a[0][0], a[1][1], a[2][2]};
    int ord[3] = {0, 1, 2};
    for (int x = 0; x < 2; ++x)
      for (int y = 0; y < 2 - x; ++y)
        if (lam[ord[y + 1]] < lam[ord[y]]) {
          const int t = ord[y];
          ord[y] = ord[y + 1];
          ord[y + 1] = t;
        }
    double l0 = lam[ord[0]], l1 = lam[ord[1]];
    const double l2 = lam[ord[2]];
    if (!(l0 < 0.0 || l1 < 0.0 || l2 <= 0.0)) {
      const double floor_l = kNdtEigRatio * l2;
      if (l0 < floor_l) {
        l0 = floor_l;
        if (l1 < floor_l) l1 = floor_l;
        const double ls[3] = {l0, l1, l2};
        for (int r = 0; r < 3; ++r)
          for (int cc = 0; cc < 3; ++cc) {
            double s = 0.0;
            for (int e = 0; e < 3; ++e) s += V[r][ord[e]] * ls[e] * V[cc][ord[e]];
            cov[r][cc] = s;
          }
      }
      // icov = cov^-1 by cofactors of the (possibly rebuilt) covariance
      const double c00 = cov[1][1] * cov[2][2] - cov[1][2] * cov[2][1];
      const double c01 = cov[1][2] * cov[2][0] - cov[1][0] * cov[2][2];
      const double c02 = cov[1][0] * cov[2][1] - cov[1][1] * cov[2][0];
      const double det = cov[0][0] * c00 + cov[0][1] * c01 + cov[0][2] * c02;
      const double ic[6] = {c00 / det,
                            (cov[0][2] * cov[2][1] - cov[0][1] * cov[2][2]) / det,
                            (cov[0][1] * cov[1][2] - cov[0][2] * cov[1][1]) / det,
                            (cov[0][0] * cov[2][2] - cov[0][2] * cov[2][0]) / det,
                            (cov[0][2] * cov[1][0] - cov[0][0] * cov[1][2]) / det,
                            (cov[0][0] * cov[1][1] - cov[0][1] * cov[1][0]) / det};
      ok = 1;
      for (int e = 0; e < 6; ++e) {
        g[3 + e] = ic[e];
        if (!isfinite(ic[e])) ok = 0;
      }
    }
  }
  valid[slot] = ok;
  // how far (cell units) the float centroid lies outside the cell its points were keyed to
  const int ix = k % L.mul_y, iy = (k / L.mul_y) % L.divb[1], iz = k / L.mul_z;
  const int cell[3] = {ix + L.minb[0], iy + L.minb[1], iz + L.minb[2]};
  const float cf[3] = {c.x, c.y, c.z};
  double ex = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double u = (double)cf[a] * L.inv_leaf;
    ex = fmax(ex, fmax((double)cell[a] - u, u - ((double)cell[a] + 1.0)));
  }
  excess[slot] = ex;
}

__global__ __launch_bounds__(256) void ndt_compact_kernel(const int* __restrict__ valid, const int* __restrict__ vslots, int n,
                                                          const int* __restrict__ ckey, const float4* __restrict__ cent,
                                                          const double* __restrict__ gauss, const int* __restrict__ npts,
                                                          int* __restrict__ out_key, float4* __restrict__ out_cent,
                                                          double* __restrict__ out_gauss, int* __restrict__ out_n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !valid[i]) return;
  const int d = vslots[i];
  out_key[d] = ckey[i];
  out_cent[d] = cent[i];
  out_n[d] = npts[i];
#pragma unroll
  for (int e = 0; e < kNdtGaussDoubles; ++e) out_gauss[(size_t)d * kNdtGaussDoubles + e] = gauss[(size_t)i * kNdtGaussDoubles + e];
}

// stats[0] = valid cells, stats[1..2] = the largest excess of a valid cell (double bits)
__global__ __launch_bounds__(1024) void ndt_stats_kernel(const int* __restrict__ valid, const int* __restrict__ vslots,
                                                         const double* __restrict__ excess, int n, int* __restrict__ stats) {
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024)
    if (valid[i]) m = fmax(m, excess[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
  __shared__ double w[16];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; ++i) m = fmax(m, w[i]);
    stats[0] = n > 0 ? vslots[n - 1] + valid[n - 1] : 0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(m);
    stats[1] = (int)(unsigned int)b;
    stats[2] = (int)(unsigned int)(b >> 32);
  }
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// first position in keys[lo, hi) whose key is >= k
__device__ __forceinline__ int lower_bound_key(const int* __restrict__ keys, int lo, int hi, int k) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// per-axis range of lattice indices (absolute) that may hold a cell whose centroid lies within the radius of q (exact: see DESIGN.md)
__device__ __forceinline__ bool axis_range(float q, const NdtLattice& L, const NdtPass& P, int a, int& lo, int& hi) {
  const double qd = (double)q;
  double flo = ceil((qd - P.r_wide) * L.inv_leaf - 1.0 - P.excess - 1e-9);
  double fhi = floor((qd + P.r_wide) * L.inv_leaf + P.excess + 1e-9);
  const double cmin = (double)L.minb[a], cmax = (double)(L.minb[a] + L.divb[a] - 1);
  flo = fmax(flo, cmin);
  fhi = fmin(fhi, cmax);
  if (!(flo <= fhi)) return false;
  lo = (int)flo;
  hi = (int)fhi;
  return true;
}

// One lane per source point; kHessian: the 29 sums of computeDerivatives, else the first kNdtGradTerms of them (pairs, score,
// gradient) with the same per-point arithmetic and the same reduction tree, so those 8 are the same bits in both passes.
template <bool kHessian>
__device__ __forceinline__ void ndt_pass(const float4* __restrict__ src, int n_s, const Xform& T, const NdtLattice& L, const NdtPass& P,
                                         const int* __restrict__ ckey, const float4* __restrict__ cent, const double* __restrict__ gauss,
                                         int n_cells, double* __restrict__ partials) {
  constexpr int NT = kHessian ? kNdtTerms : kNdtGradTerms;
  constexpr int NP = kHessian ? 17 : 5;  // per-point sums: pairs, score, b (3) [, A (6), M (6)]
  double acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = 0.0;
  // (one lane per point: dealing a point's stencil rows out to 2, 4 or 8 lanes measured 1.0x, 1.5x, 2.4x SLOWER on 200k points)
  const int stride = gridDim.x * ND_BLOCK;
  for (int i = blockIdx.x * ND_BLOCK + threadIdx.x; i < n_s; i += stride) {
    const float4 s = src[i];
    float q[3];
    xform_point(T, s.x, s.y, s.z, q[0], q[1], q[2]);
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
    int lo[3], hi[3];
    if (!axis_range(q[0], L, P, 0, lo[0], hi[0]) || !axis_range(q[1], L, P, 1, lo[1], hi[1]) || !axis_range(q[2], L, P, 2, lo[2], hi[2]))
      continue;
    // Per pair (q' = q - mean, icq = icov q', w = d1 d2 e) PCL adds w (q'^T icov J_k) to g_k and
    // w (-d2 (q'^T icov J_k)(q'^T icov J_l) + q'^T icov H_kl + J_l^T icov J_k) to H_kl.  J and H depend on the point alone, so the
    // point's pairs are summed first -- b = sum w icq, A = sum w icov, M = sum w icq icq^T -- and then g = J^T b,
    // H_kl = -d2 J_k^T M J_l + b . H_kl + J_l^T A J_k: the same sums, ~60 flops per pair instead of ~300
    double pt[NP];  // pairs, score, b (3), A (6: xx xy xz yy yz zz), M (6)
#pragma unroll
    for (int k = 0; k < NP; ++k) pt[k] = 0.0;
    int pos = 0;
    for (int iz = lo[2]; iz <= hi[2]; ++iz)
      for (int iy = lo[1]; iy <= hi[1]; ++iy) {
        const int row = (iy - L.minb[1]) * L.mul_y + (iz - L.minb[2]) * L.mul_z;
        const int k0 = row + (lo[0] - L.minb[0]), k1 = row + (hi[0] - L.minb[0]);
        // rows are visited in ascending key order: the search starts where the previous row's ended
        for (int j = pos = lower_bound_key(ckey, pos, n_cells, k0); j < n_cells && ckey[j] <= k1; ++j) {
          const float4 c = cent[j];
          const float dx = q[0] - c.x, dy = q[1] - c.y, dz = q[2] - c.z;
          const float d2 = (dx * dx + dy * dy) + dz * dz;
          if (!(d2 <= P.r2f)) continue;
          const double* gm = gauss + (size_t)j * kNdtGaussDoubles;
          const double qp[3] = {(double)q[0] - gm[0], (double)q[1] - gm[1], (double)q[2] - gm[2]};
          const double ic[6] = {gm[3], gm[4], gm[5], gm[6], gm[7], gm[8]};
          const double icq[3] = {(ic[0] * qp[0] + ic[1] * qp[1]) + ic[2] * qp[2], (ic[1] * qp[0] + ic[3] * qp[1]) + ic[4] * qp[2],
                                 (ic[2] * qp[0] + ic[4] * qp[1]) + ic[5] * qp[2]};
          const double e = exp(-P.d2 * dot3(qp, icq) / 2.0);
          const double de = P.d2 * e;
          if (de > 1.0 || de < 0.0 || de != de) continue;
          const double w = de * P.d1;
          pt[0] += 1.0;
          pt[1] += -P.d1 * e;
#pragma unroll
          for (int a = 0; a < 3; ++a) pt[2 + a] += w * icq[a];
          if constexpr (kHessian) {
#pragma unroll
            for (int a = 0; a < 6; ++a) pt[5 + a] += w * ic[a];
            const double wq[3] = {w * icq[0], w * icq[1], w * icq[2]};
            pt[11] += wq[0] * icq[0];
            pt[12] += wq[0] * icq[1];
            pt[13] += wq[0] * icq[2];
            pt[14] += wq[1] * icq[1];
            pt[15] += wq[1] * icq[2];
            pt[16] += wq[2] * icq[2];
          }
        }
      }
    if (pt[0] == 0.0) continue;
    // computePointDerivatives(x): the angular columns of J and the angular blocks of H, from the untransformed point (double)
    const double x[3] = {(double)s.x, (double)s.y, (double)s.z};
    double J[6][3];  // J[k] = d(T x)/dp_k
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) J[k][a] = k == a ? 1.0 : 0.0;
    J[3][0] = 0.0;
    J[3][1] = dot3(x, P.j_ang[0]);
    J[3][2] = dot3(x, P.j_ang[1]);
    J[4][0] = dot3(x, P.j_ang[2]);
    J[4][1] = dot3(x, P.j_ang[3]);
    J[4][2] = dot3(x, P.j_ang[4]);
    J[5][0] = dot3(x, P.j_ang[5]);
    J[5][1] = dot3(x, P.j_ang[6]);
    J[5][2] = dot3(x, P.j_ang[7]);
    acc[0] += pt[0];
    acc[1] += pt[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[2 + k] += dot3(J[k], pt + 2);
    if constexpr (kHessian) {
      // Hb[0..5] = the blocks a, b, c, d, e, f: H(3,3) = a, H(3,4) = b, H(3,5) = c, H(4,4) = d, H(4,5) = e, H(5,5) = f
      double Hb[6][3];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        Hb[b][0] = 0.0;
        Hb[b][1] = dot3(x, P.h_ang[2 * b]);
        Hb[b][2] = dot3(x, P.h_ang[2 * b + 1]);
      }
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int a = 0; a < 3; ++a) Hb[3 + b][a] = dot3(x, P.h_ang[6 + 3 * b + a]);
      const double A[3][3] = {{pt[5], pt[6], pt[7]}, {pt[6], pt[8], pt[9]}, {pt[7], pt[9], pt[10]}};
      const double M[3][3] = {{pt[11], pt[12], pt[13]}, {pt[12], pt[14], pt[15]}, {pt[13], pt[15], pt[16]}};
      double AJ[6][3], MJ[6][3];
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          AJ[k][r] = dot3(A[r], J[k]);
          MJ[k][r] = dot3(M[r], J[k]);
        }
      int t = 8;
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int l = k; l < 6; ++l, ++t) {
          double h = -P.d2 * dot3(J[l], MJ[k]);
          if (k >= 3) h += dot3(pt + 2, Hb[k == 3 ? l - 3 : (k == 4 ? 3 + (l - 4) : 5)]);
          h += dot3(J[l], AJ[k]);
          acc[t] += h;
        }
    }
  }
  // fixed-order block reduction: shuffle tree per wave, then the four waves in order; partials keep kNdtTerms doubles per
  // workgroup in both passes (the final kernel reads the first NT columns)
  __shared__ double wsum[ND_BLOCK / 64][NT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) wsum[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NT) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < ND_BLOCK / 64; ++w) v += wsum[w][threadIdx.x];
    partials[(size_t)blockIdx.x * kNdtTerms + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(ND_BLOCK) void ndt_deriv_kernel(const float4* __restrict__ src, int n_s, Xform T, NdtLattice L, NdtPass P,
                                                             const int* __restrict__ ckey, const float4* __restrict__ cent,
                                                             const double* __restrict__ gauss, int n_cells,
                                                             double* __restrict__ partials) {
  ndt_pass<true>(src, n_s, T, L, P, ckey, cent, gauss, n_cells, partials);
}

// the More-Thuente line search's trial pass: score and gradient only (no A, M or Hessian)
__global__ __launch_bounds__(ND_BLOCK) void ndt_grad_kernel(const float4* __restrict__ src, int n_s, Xform T, NdtLattice L, NdtPass P,
                                                            const int* __restrict__ ckey, const float4* __restrict__ cent,
                                                            const double* __restrict__ gauss, int n_cells,
                                                            double* __restrict__ partials) {
  ndt_pass<false>(src, n_s, T, L, P, ckey, cent, gauss, n_cells, partials);
}

}  // namespace

hipError_t launch_ndt_keys(const float4* pts, int n, const NdtLattice& L, int* keys, int* vals, int* temp, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(ndt_key_kernel, dim3(blocks), dim3(256), 0, stream, pts, n, L.inv_leaf_f, L.minb[0], L.minb[1], L.minb[2], L.mul_y,
                     L.mul_z, keys, vals);
  // the voxel filter's key width (icp_voxel.hip: launch_voxel_grid): the bits of the cell indices + one, so the sentinel sorts last
  unsigned int end_bit = 1;
  const long long ncells = (long long)L.divb[0] * L.divb[1] * L.divb[2];
  while (end_bit < 31 && (1ll << end_bit) < ncells) ++end_bit;
  end_bit = end_bit < 31 ? end_bit + 1 : 31;
  return launch_radix_sort_pairs(keys, vals, n, end_bit, temp, stream);
}

hipError_t launch_ndt_cells(const float4* pts, int n, const NdtLattice& L, const int* sorted_keys, const int* sorted_vals, int* flags,
                            int* slots, int* temp, int* valid, int* vslots, int* ckey, float4* cent, double* gauss, int* npts,
                            double* excess, int* out_key, float4* out_cent, double* out_gauss, int* out_n, int* stats,
                            hipStream_t stream) {
  if (n <= 0) return hipMemsetAsync(stats, 0, 3 * sizeof(int), stream);
  const int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(ndt_flag_kernel, dim3(blocks), dim3(256), 0, stream, sorted_keys, n, flags);
  hipError_t e = launch_exclusive_scan(flags, slots, n, temp, stream);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(valid, 0, (size_t)n * sizeof(int), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(ndt_cell_kernel, dim3(blocks), dim3(256), 0, stream, pts, sorted_keys, sorted_vals, flags, slots, n, L, valid, ckey,
                     cent, gauss, npts, excess);
  if ((e = launch_exclusive_scan(valid, vslots, n, temp, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(ndt_compact_kernel, dim3(blocks), dim3(256), 0, stream, valid, vslots, n, ckey, cent, gauss, npts, out_key, out_cent,
                     out_gauss, out_n);
  hipLaunchKernelGGL(ndt_stats_kernel, dim3(1), dim3(1024), 0, stream, valid, vslots, excess, n, stats);
  return hipGetLastError();
}

int ndt_blocks(int n_s) {
  int blocks = (n_s + ND_BLOCK - 1) / ND_BLOCK;
  if (blocks > kNdtMaxBlocks) blocks = kNdtMaxBlocks;
  return blocks < 1 ? 1 : blocks;
}

hipError_t launch_ndt_derivatives(const float4* src, int n_s, const Xform& T, const NdtLattice& L, const NdtPass& P, const int* ckey,
                                  const float4* cent, const double* gauss, int n_cells, double* partials, double* sums_out,
                                  unsigned long long* flags, unsigned long long seq, hipStream_t stream, bool hessian) {
  const int blocks = ndt_blocks(n_s);
  if (n_s > 0 && n_cells > 0) {
    if (hessian)
      hipLaunchKernelGGL(ndt_deriv_kernel, dim3(blocks), dim3(ND_BLOCK), 0, stream, src, n_s, T, L, P, ckey, cent, gauss, n_cells, partials);
    else
      hipLaunchKernelGGL(ndt_grad_kernel, dim3(blocks), dim3(ND_BLOCK), 0, stream, src, n_s, T, L, P, ckey, cent, gauss, n_cells, partials);
  } else {
    const hipError_t e = hipMemsetAsync(partials, 0, (size_t)blocks * kNdtTerms * sizeof(double), stream);
    if (e != hipSuccess) return e;
  }
  return launch_terms29_final(partials, blocks, sums_out, flags, seq, stream, hessian ? kNdtTerms : kNdtGradTerms);
}

}  // namespace icpgpu
