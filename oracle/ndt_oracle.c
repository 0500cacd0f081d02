/*
 * ndt_oracle.c -- CPU ORACLE for the NDT mode.  TEST INFRASTRUCTURE ONLY.
 *
 *      ***  PARITY UNPINNED  ***   (see icp_oracle.h)
 *
 * Restates pcl::NormalDistributionsTransform over pcl::VoxelGridCovariance (PCL 1.8) from DESIGN.md f6, independently of
 * tests/ndt_restated.py (which it is pinned to in tests/test_ndt_oracle.py) and of the kernels:
 *   transform     T(p) = Translation3f * AngleAxisf(X) * AngleAxisf(Y) * AngleAxisf(Z) in float; sinf / cosf are the binary128
 *                 values rounded once to float.  The angle terms j_ang / h_ang are built in long double from binary128 sin / cos
 *                 rounded to double, with PCL's |angle| < 1e-4 -> cos 1, sin 0.
 *   cells         the contract arithmetic, bit for bit: float keys, a stable sort, float sums and double S / Q in input order,
 *                 PCL's covariance from the lower triangle.  Then, in binary128: a cyclic Jacobi run to convergence (not the
 *                 device's 8 sweeps), the eigenvalues, the validity and floor decisions with their margin, the floored
 *                 covariance's inverse rounded to double, and the eigen residual.  Each cell also reports e, how far (cell units)
 *                 its float centroid lies outside the cell its points were keyed to.
 *   derivatives   neighbourhoods from the float predicate (dx^2 + dy^2) + dz^2 <= float(r^2) on the float transform, found
 *                 WITHOUT keys or e: brute force over every centroid, or a hash of centroid positions (buckets of 2 r); the pair
 *                 in PCL's per-pair form (updateDerivatives) in long double with expl; a point's pairs summed in long double,
 *                 the points in binary128.  mag[k] is the same sum with every factor replaced by its absolute value: the
 *                 scale of a tolerance.
 * Built with -ffp-contract=off: every float operation of the contract happens as written (fmaf where the contract has one).
 */
#include <float.h>
#include <math.h>
#include <quadmath.h>
#include <stdlib.h>
#include <string.h>

#include "icp_oracle.h"

typedef __float128 f128;

/* ------------------------------------------------------------------------------------------ */
/* transform and angle terms                                                                   */
/* ------------------------------------------------------------------------------------------ */

static void angle_axis_f(float angle, int axis, float R[3][3]) {
  const f128 a = (f128)angle;
  const float s = (float)sinq(a), c = (float)cosq(a); /* one rounding from binary128 */
  float ax[3] = {0.f, 0.f, 0.f};
  ax[axis] = 1.f;
  float sa[3], ca[3];
  for (int k = 0; k < 3; ++k) {
    sa[k] = s * ax[k];
    ca[k] = (1.f - c) * ax[k];
  }
  /* Eigen's AngleAxis::toRotationMatrix */
  for (int i = 0; i < 3; ++i) R[i][i] = ca[i] * ax[i] + c;
  R[0][1] = ca[0] * ax[1] - sa[2];
  R[1][0] = ca[0] * ax[1] + sa[2];
  R[0][2] = ca[0] * ax[2] + sa[1];
  R[2][0] = ca[0] * ax[2] - sa[1];
  R[1][2] = ca[1] * ax[2] - sa[0];
  R[2][1] = ca[1] * ax[2] + sa[0];
}

static void matmul3f(const float A[3][3], const float B[3][3], float C[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}

void orc_ndt_transform(const double p[6], float T[16]) {
  float Rx[3][3], Ry[3][3], Rz[3][3], A[3][3], R[3][3];
  angle_axis_f((float)p[3], 0, Rx);
  angle_axis_f((float)p[4], 1, Ry);
  angle_axis_f((float)p[5], 2, Rz);
  matmul3f(Rx, Ry, A);
  matmul3f(A, Rz, R);
  memset(T, 0, 16 * sizeof(float));
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = R[r][c];
  T[12] = (float)p[0];
  T[13] = (float)p[1];
  T[14] = (float)p[2];
  T[15] = 1.f;
}

/* PCL's j_ang_a .. h (8 x 3) and h_ang_a2 .. f3 (15 x 3) from the sines and cosines.  neg = -1: the terms; neg = +1 with
 * |sin|, |cos|: every factor by its magnitude (the bound of mag[]). */
static void angle_tables(long double cx, long double sx, long double cy, long double sy, long double cz, long double sz,
                         long double neg, long double j[8][3], long double h[15][3]) {
  const long double n = neg;
  const long double J[8][3] = {{n * sx * sz + cx * sy * cz, n * sx * cz + n * cx * sy * sz, n * cx * cy},
                               {cx * sz + sx * sy * cz, cx * cz + n * sx * sy * sz, n * sx * cy},
                               {n * sy * cz, sy * sz, cy},
                               {sx * cy * cz, n * sx * cy * sz, sx * sy},
                               {n * cx * cy * cz, cx * cy * sz, n * cx * sy},
                               {n * cy * sz, n * cy * cz, 0.0L},
                               {cx * cz + n * sx * sy * sz, n * cx * sz + n * sx * sy * cz, 0.0L},
                               {sx * cz + cx * sy * sz, cx * sy * cz + n * sx * sz, 0.0L}};
  const long double H[15][3] = {{n * cx * sz + n * sx * sy * cz, n * cx * cz + sx * sy * sz, sx * cy},  /* a2 */
                                {n * sx * sz + cx * sy * cz, n * cx * sy * sz + n * sx * cz, n * cx * cy}, /* a3 */
                                {cx * cy * cz, n * cx * cy * sz, cx * sy},                        /* b2 */
                                {sx * cy * cz, n * sx * cy * sz, sx * sy},                        /* b3 */
                                {n * sx * cz + n * cx * sy * sz, sx * sz + n * cx * sy * cz, 0.0L},  /* c2 */
                                {cx * cz + n * sx * sy * sz, n * sx * sy * cz + n * cx * sz, 0.0L},  /* c3 */
                                {n * cy * cz, cy * sz, n * sy},                                   /* d1 */
                                {n * sx * sy * cz, sx * sy * sz, sx * cy},                        /* d2 */
                                {cx * sy * cz, n * cx * sy * sz, n * cx * cy},                    /* d3 */
                                {sy * sz, sy * cz, 0.0L},                                         /* e1 */
                                {n * sx * cy * sz, n * sx * cy * cz, 0.0L},                       /* e2 */
                                {cx * cy * sz, cx * cy * cz, 0.0L},                               /* e3 */
                                {n * cy * cz, cy * sz, 0.0L},                                     /* f1 */
                                {n * cx * sz + n * sx * sy * cz, n * cx * cz + sx * sy * sz, 0.0L},  /* f2 */
                                {n * sx * sz + cx * sy * cz, n * cx * sy * sz + n * sx * cz, 0.0L}}; /* f3 */
  memcpy(j, J, sizeof J);
  memcpy(h, H, sizeof H);
}

/* sin / cos of each angle: binary128 rounded to double, or (cos 1, sin 0) under the small-angle rule */
static void angle_sincos(const double p[6], double c[3], double s[3]) {
  for (int a = 0; a < 3; ++a) {
    if (fabs(p[3 + a]) < 10e-5) {
      c[a] = 1.0;
      s[a] = 0.0;
    } else {
      c[a] = (double)cosq((f128)p[3 + a]);
      s[a] = (double)sinq((f128)p[3 + a]);
    }
  }
}

void orc_ndt_angle_terms(const double p[6], double j_out[24], double h_out[45]) {
  double c[3], s[3];
  angle_sincos(p, c, s);
  long double j[8][3], h[15][3];
  angle_tables(c[0], s[0], c[1], s[1], c[2], s[2], -1.0L, j, h);
  for (int i = 0; i < 24; ++i) j_out[i] = (double)j[i / 3][i % 3];
  for (int i = 0; i < 45; ++i) h_out[i] = (double)h[i / 3][i % 3];
}

/* ------------------------------------------------------------------------------------------ */
/* cells                                                                                       */
/* ------------------------------------------------------------------------------------------ */

/* cyclic Jacobi in binary128, swept until the off-diagonal part vanishes against the diagonal (or no rotation changes
 * anything); a's diagonal -> eigenvalues, v's columns -> eigenvectors.  ORC_NDT_JACOBI_SWEEPS caps the sweeps (default: none). */
#ifndef ORC_NDT_JACOBI_SWEEPS
#define ORC_NDT_JACOBI_SWEEPS 100
#endif
static void jacobi3q(f128 a[3][3], f128 v[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1 : 0;
  for (int sweep = 0; sweep < ORC_NDT_JACOBI_SWEEPS; ++sweep) {
    const f128 off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const f128 dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (off == 0 || off <= 1e-70Q * dia) break;
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
      const f128 apq = a[p][q];
      if (apq == 0) continue;
      const f128 theta = (a[q][q] - a[p][p]) / (2 * apq);
      const f128 t = (theta >= 0 ? 1 : -1) / (fabsq(theta) + sqrtq(theta * theta + 1));
      const f128 c = 1 / sqrtq(t * t + 1), s = t * c;
      const f128 arp = a[r][p], arq = a[r][q];
      a[p][p] -= t * apq;
      a[q][q] += t * apq;
      a[p][q] = a[q][p] = 0;
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
      for (int k = 0; k < 3; ++k) {
        const f128 vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
      }
    }
  }
}

static int cmp_u64(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : x > y;
}

/* the eigen part of one cell of n >= 6 points: decisions, margin, icov, residual */
static void cell_gaussian(orc_ndt_cell* o) {
  const double* C = o->cov;
  f128 a[3][3], V[3][3];
  double amax = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      a[r][c] = (f128)C[3 * r + c];
      amax = fmax(amax, fabs(C[3 * r + c]));
    }
  jacobi3q(a, V);
  f128 l[3] = {a[0][0], a[1][1], a[2][2]};
  int ord[3] = {0, 1, 2};
  for (int x = 0; x < 2; ++x)
    for (int y = 0; y < 2 - x; ++y)
      if (l[ord[y + 1]] < l[ord[y]]) {
        const int t = ord[y];
        ord[y] = ord[y + 1];
        ord[y + 1] = t;
      }
  /* residual: max over eigenpairs of |A v - l v|, and of |V^T V - I|, against max |A| */
  f128 res = 0;
  for (int e = 0; e < 3; ++e)
    for (int r = 0; r < 3; ++r) {
      f128 av = 0;
      for (int c = 0; c < 3; ++c) av += (f128)C[3 * r + c] * V[c][e];
      const f128 d = fabsq(av - l[e] * V[r][e]);
      if (d > res) res = d;
    }
  f128 orth = 0;
  for (int e = 0; e < 3; ++e)
    for (int f = 0; f < 3; ++f) {
      f128 d = 0;
      for (int k = 0; k < 3; ++k) d += V[k][e] * V[k][f];
      d = fabsq(d - (e == f ? 1 : 0));
      if (d > orth) orth = d;
    }
  o->resid = amax > 0.0 ? fmax((double)(res / (f128)amax), (double)orth) : (double)orth;
  const f128 l0 = l[ord[0]], l1 = l[ord[1]], l2 = l[ord[2]];
  for (int e = 0; e < 3; ++e) o->eig[e] = (double)l[ord[e]];
  const f128 big = fmaxq(fabsq(l0), fabsq(l2));
  f128 margin = big > 0 ? fabsq(l0) / big : 0;   /* validity: l0 < 0 (l1 < 0 implies it) or l2 <= 0 */
  if (big > 0 && fabsq(l2) / big < margin) margin = fabsq(l2) / big;
  const int valid = !(l0 < 0 || l1 < 0 || l2 <= 0);
  o->valid = valid;
  o->floored = 0;
  if (valid) {
    const f128 fl = (f128)0.01 * l2; /* (the double constant, exactly) */
    f128 ls[3] = {l0, l1, l2};
    const f128 m0 = fabsq(l0 - fl) / big;
    if (m0 < margin) margin = m0;
    if (l0 < fl) {
      o->floored = 1;
      ls[0] = fl;
      const f128 m1 = fabsq(l1 - fl) / big;
      if (m1 < margin) margin = m1;
      if (l1 < fl) {
        o->floored = 2;
        ls[1] = fl;
      }
    }
    /* icov = V diag(1 / l) V^T of the (floored) covariance */
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        f128 s = 0;
        for (int e = 0; e < 3; ++e) s += V[r][ord[e]] * V[c][ord[e]] / ls[e];
        o->icov[3 * r + c] = (double)s;
      }
    for (int e = 0; e < 9; ++e)
      if (!isfinite(o->icov[e])) o->valid = 0;
  }
  o->margin = (double)margin;
}

long orc_ndt_cells(const float* pts_xyzw, size_t n, double resolution, orc_ndt_lattice* L, orc_ndt_cell** out) {
  memset(L, 0, sizeof *L);
  *out = NULL;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  size_t n_fin = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* p = pts_xyzw + 4 * i;
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) continue;
    ++n_fin;
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], p[a]);
      hi[a] = fmaxf(hi[a], p[a]);
    }
  }
  if (n_fin == 0) return 0;
  /* the voxel filter's lattice at leaf = (float) resolution, float arithmetic */
  const float inv = 1.0f / (float)resolution;
  double dd[3], db[3];
  for (int a = 0; a < 3; ++a) {
    dd[a] = (double)((long long)((hi[a] - lo[a]) * inv) + 1);
    L->minb[a] = (int32_t)floorf(lo[a] * inv);
    db[a] = (double)((long long)floorf(hi[a] * inv) - L->minb[a] + 1);
    L->divb[a] = (int32_t)db[a];
  }
  if (dd[0] * dd[1] * dd[2] > 2147483647.0 || db[0] * db[1] * db[2] > 2147483647.0) return -1;
  L->has_cells = 1;
  L->mul_y = L->divb[0];
  L->mul_z = L->divb[0] * L->divb[1];
  L->inv_leaf_f = inv;
  /* keys, then (key, index) sorted: a stable order */
  uint64_t* ki = malloc(n_fin * sizeof *ki);
  if (!ki) return -2;
  size_t m = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* p = pts_xyzw + 4 * i;
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) continue;
    long long ijk[3];
    for (int a = 0; a < 3; ++a) ijk[a] = (long long)floorf(p[a] * inv) - L->minb[a];
    const long long key = ijk[0] + ijk[1] * L->mul_y + ijk[2] * (long long)L->mul_z;
    ki[m++] = ((uint64_t)key << 32) | (uint64_t)i;
  }
  qsort(ki, m, sizeof *ki, cmp_u64);
  size_t n_cells = 0;
  for (size_t s = 0; s < m; ++s)
    if (s == 0 || (ki[s] >> 32) != (ki[s - 1] >> 32)) ++n_cells;
  orc_ndt_cell* cells = calloc(n_cells ? n_cells : 1, sizeof *cells);
  if (!cells) {
    free(ki);
    return -2;
  }
  const double inv_d = (double)inv;
  size_t ci = 0;
  for (size_t s = 0; s < m;) {
    size_t e = s;
    const uint64_t key = ki[s] >> 32;
    while (e < m && (ki[e] >> 32) == key) ++e;
    orc_ndt_cell* o = &cells[ci++];
    o->key = (int32_t)key;
    o->n = (int32_t)(e - s);
    float fs[3] = {0.f, 0.f, 0.f};
    double S[3] = {0.0, 0.0, 0.0}, Q[3][3] = {{0.0}};
    for (size_t t = s; t < e; ++t) {
      const float* p = pts_xyzw + 4 * (ki[t] & 0xFFFFFFFFu);
      for (int a = 0; a < 3; ++a) {
        fs[a] += p[a];
        S[a] += (double)p[a];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c) Q[r][c] += (double)p[r] * (double)p[c];
    }
    const float fn = (float)o->n;
    for (int a = 0; a < 3; ++a) o->centroid[a] = fs[a] / fn;
    o->centroid[3] = 1.f;
    const double nd = (double)o->n;
    for (int a = 0; a < 3; ++a) o->mean[a] = S[a] / nd;
    /* e: the first point's cell (all of them share it) against the float centroid */
    const float* p0 = pts_xyzw + 4 * (ki[s] & 0xFFFFFFFFu);
    double ex = 0.0;
    for (int a = 0; a < 3; ++a) {
      const double cell = (double)floorf(p0[a] * inv);
      const double u = (double)o->centroid[a] * inv_d;
      ex = fmax(ex, fmax(cell - u, u - (cell + 1.0)));
    }
    o->excess = ex;
    for (int k = 0; k < 9; ++k) o->cov[k] = o->icov[k] = NAN;
    for (int k = 0; k < 3; ++k) o->eig[k] = NAN;
    o->margin = INFINITY;
    o->resid = 0.0;
    if (o->n >= 6) {
      /* ((Q - 2 S_c m_r) / n + m_c m_r) (n - 1) / n for row r <= column c: the lower triangle's products, mirrored */
      const double f = (nd - 1.0) / nd;
      for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c) {
          const double v = ((Q[r][c] - 2.0 * (S[c] * o->mean[r])) / nd + o->mean[c] * o->mean[r]) * f;
          o->cov[3 * r + c] = o->cov[3 * c + r] = v;
        }
      cell_gaussian(o);
    }
    if (o->valid && ex > L->max_excess) L->max_excess = ex;
    s = e;
  }
  free(ki);
  *out = cells;
  return (long)n_cells;
}

void orc_ndt_free(void* p) { free(p); }

/* ------------------------------------------------------------------------------------------ */
/* neighbourhoods and derivatives                                                              */
/* ------------------------------------------------------------------------------------------ */

typedef struct {
  int64_t b[3];
  int32_t idx;
} bucket_entry;

static int cmp_bucket(const void* x, const void* y) {
  const bucket_entry *a = x, *b = y;
  for (int k = 2; k >= 0; --k)
    if (a->b[k] != b->b[k]) return a->b[k] < b->b[k] ? -1 : 1;
  return a->idx < b->idx ? -1 : a->idx > b->idx;
}

/* first entry >= (bz, by, bx) */
static size_t bucket_lower(const bucket_entry* e, size_t m, int64_t bx, int64_t by, int64_t bz) {
  size_t lo = 0, hi = m;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    const int64_t* b = e[mid].b;
    const int less = b[2] != bz ? b[2] < bz : (b[1] != by ? b[1] < by : b[0] < bx);
    if (less) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

static int cmp_i32(const void* a, const void* b) {
  const int32_t x = *(const int32_t*)a, y = *(const int32_t*)b;
  return x < y ? -1 : x > y;
}

int orc_ndt_derivatives(const float* cent_xyzw, const double* mean3, const double* icov6, size_t m, const float* src_xyzw,
                        size_t n_s, const double p[6], double resolution, double outlier_ratio, int search,
                        double sums[ORC_NDT_TERMS], double mag[ORC_NDT_TERMS], int64_t stats[4], int32_t* pair_pt,
                        int32_t* pair_cell, size_t pair_cap) {
  /* the Gauss constants in double, as computeTransformation forms them */
  const double c1 = 10.0 * (1.0 - outlier_ratio), c2 = outlier_ratio / (resolution * resolution * resolution);
  const double d3 = -log(c2), gd1 = -log(c1 + c2) - d3;
  const double gd2 = -2.0 * log((-log(c1 * exp(-0.5) + c2) - d3) / gd1);
  const long double d1 = gd1, d2 = gd2;
  const float r2f = (float)(resolution * resolution);
  float T[16];
  orc_ndt_transform(p, T);
  double c[3], s[3];
  angle_sincos(p, c, s);
  long double ja[8][3], ha[15][3], jm[8][3], hm[15][3];
  angle_tables(c[0], s[0], c[1], s[1], c[2], s[2], -1.0L, ja, ha);
  angle_tables(fabs(c[0]), fabs(s[0]), fabs(c[1]), fabs(s[1]), fabs(c[2]), fabs(s[2]), 1.0L, jm, hm);
  f128 acc[ORC_NDT_TERMS], accm[ORC_NDT_TERMS];
  for (int k = 0; k < ORC_NDT_TERMS; ++k) acc[k] = accm[k] = 0;
  int64_t n_pairs = 0, n_skip = 0, n_near = 0;
  /* the position hash: buckets of 2 r' (r' = r (1 + 1e-5) bounds |c - q| per axis for every pair the float test accepts) */
  const double rw = resolution * (1.0 + 1e-5), bs = 2.0 * rw;
  bucket_entry* hb = NULL;
  int64_t bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
  if (search == ORC_NDT_SEARCH_HASH && m > 0) {
    hb = malloc(m * sizeof *hb);
    if (!hb) return -2;
    for (size_t j = 0; j < m; ++j) {
      for (int a = 0; a < 3; ++a) {
        hb[j].b[a] = (int64_t)floor((double)cent_xyzw[4 * j + a] / bs);
        if (j == 0 || hb[j].b[a] < bmin[a]) bmin[a] = hb[j].b[a];
        if (j == 0 || hb[j].b[a] > bmax[a]) bmax[a] = hb[j].b[a];
      }
      hb[j].idx = (int32_t)j;
    }
    qsort(hb, m, sizeof *hb, cmp_bucket);
  }
  int32_t* cand = malloc((m ? m : 1) * sizeof *cand);
  if (!cand) {
    free(hb);
    return -2;
  }
  for (size_t i = 0; i < n_s; ++i) {
    const float* x = src_xyzw + 4 * i;
    float q[3];
    for (int r = 0; r < 3; ++r) q[r] = fmaf(T[8 + r], x[2], fmaf(T[4 + r], x[1], fmaf(T[r], x[0], T[12 + r])));
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
    /* candidates */
    size_t nc = 0;
    if (search == ORC_NDT_SEARCH_HASH) {
      int64_t blo[3], bhi[3];
      int empty = 0;
      for (int a = 0; a < 3; ++a) {
        double fl = floor(((double)q[a] - rw) / bs), fh = floor(((double)q[a] + rw) / bs);
        fl = fmax(fl, (double)bmin[a]);
        fh = fmin(fh, (double)bmax[a]);
        if (!(fl <= fh)) empty = 1;
        blo[a] = empty ? 0 : (int64_t)fl;
        bhi[a] = empty ? -1 : (int64_t)fh;
      }
      if (empty || !hb) continue;
      for (int64_t bz = blo[2]; bz <= bhi[2]; ++bz)
        for (int64_t by = blo[1]; by <= bhi[1]; ++by)
          for (size_t t = bucket_lower(hb, m, blo[0], by, bz); t < m && hb[t].b[2] == bz && hb[t].b[1] == by && hb[t].b[0] <= bhi[0];
               ++t)
            cand[nc++] = hb[t].idx;
      qsort(cand, nc, sizeof *cand, cmp_i32);
    } else {
      for (size_t j = 0; j < m; ++j) cand[nc++] = (int32_t)j;
    }
    /* the point's derivatives (computePointDerivatives), terms and magnitudes */
    const long double xv[3] = {x[0], x[1], x[2]}, xa[3] = {fabsl(xv[0]), fabsl(xv[1]), fabsl(xv[2])};
    long double J[6][3] = {{0}}, Ja[6][3] = {{0}}, Hx[6][6][3] = {{{0}}}, Hxa[6][6][3] = {{{0}}};
    for (int k = 0; k < 3; ++k) J[k][k] = Ja[k][k] = 1.0L;
#define DOT(v, t) ((v)[0] * (t)[0] + (v)[1] * (t)[1] + (v)[2] * (t)[2])
    const int jmap[8][2] = {{3, 1}, {3, 2}, {4, 0}, {4, 1}, {4, 2}, {5, 0}, {5, 1}, {5, 2}};
    for (int t = 0; t < 8; ++t) {
      J[jmap[t][0]][jmap[t][1]] = DOT(xv, ja[t]);
      Ja[jmap[t][0]][jmap[t][1]] = DOT(xa, jm[t]);
    }
    /* H(3,3) = a, H(3,4) = b, H(3,5) = c, H(4,4) = d, H(4,5) = e, H(5,5) = f; a, b, c have a zero x entry */
    const int blk[6][2] = {{3, 3}, {3, 4}, {3, 5}, {4, 4}, {4, 5}, {5, 5}};
    for (int b = 0; b < 6; ++b) {
      long double v[3], va[3];
      for (int r = 0; r < 3; ++r) {
        if (b < 3) {
          v[r] = r == 0 ? 0.0L : DOT(xv, ha[2 * b + r - 1]);
          va[r] = r == 0 ? 0.0L : DOT(xa, hm[2 * b + r - 1]);
        } else {
          v[r] = DOT(xv, ha[6 + 3 * (b - 3) + r]);
          va[r] = DOT(xa, hm[6 + 3 * (b - 3) + r]);
        }
      }
      for (int r = 0; r < 3; ++r) {
        Hx[blk[b][0]][blk[b][1]][r] = Hx[blk[b][1]][blk[b][0]][r] = v[r];
        Hxa[blk[b][0]][blk[b][1]][r] = Hxa[blk[b][1]][blk[b][0]][r] = va[r];
      }
    }
    long double pa[ORC_NDT_TERMS] = {0}, pm[ORC_NDT_TERMS] = {0}; /* the point's pairs, long double; into binary128 per point */
    for (size_t t = 0; t < nc; ++t) {
      const size_t j = (size_t)cand[t];
      const float* cc = cent_xyzw + 4 * j;
      const float dx = q[0] - cc[0], dy = q[1] - cc[1], dz = q[2] - cc[2];
      const float dd = (dx * dx + dy * dy) + dz * dz;
      if (fabsf(dd - r2f) <= 1e-12f * r2f) ++n_near;
      if (!(dd <= r2f)) continue;
      const double* mu = mean3 + 3 * j;
      const double* i6 = icov6 + 6 * j;
      const long double ic[3][3] = {{i6[0], i6[1], i6[2]}, {i6[1], i6[3], i6[4]}, {i6[2], i6[4], i6[5]}};
      long double ica[3][3];
      for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) ica[r][k] = fabsl(ic[r][k]);
      const long double qp[3] = {(long double)q[0] - mu[0], (long double)q[1] - mu[1], (long double)q[2] - mu[2]};
      const long double qa[3] = {fabsl(qp[0]), fabsl(qp[1]), fabsl(qp[2])};
      long double icq[3], icqa[3];
      for (int r = 0; r < 3; ++r) {
        icq[r] = DOT(ic[r], qp);
        icqa[r] = DOT(ica[r], qa);
      }
      const long double e = expl(-d2 * DOT(qp, icq) / 2.0L);
      const long double de = d2 * e;
      if (fabsl(de - 1.0L) <= 1e-12L) ++n_near;
      if (de > 1.0L || de < 0.0L || de != de) {
        ++n_skip;
        continue;
      }
      if (pair_pt && (size_t)n_pairs < pair_cap) {
        pair_pt[n_pairs] = (int32_t)i;
        pair_cell[n_pairs] = (int32_t)j;
      }
      ++n_pairs;
      const long double w = de * d1, wa = fabsl(w);
      /* updateDerivatives, pair by pair */
      long double cJ[6][3], cJa[6][3], aq[6], aqa[6];
      for (int k = 0; k < 6; ++k) {
        for (int r = 0; r < 3; ++r) {
          cJ[k][r] = DOT(ic[r], J[k]);
          cJa[k][r] = DOT(ica[r], Ja[k]);
        }
        aq[k] = DOT(qp, cJ[k]);
        aqa[k] = DOT(qa, cJa[k]);
      }
      pa[0] += 1;
      pm[0] += 1;
      pa[1] += -d1 * e;
      pm[1] += fabsl(d1) * e;
      for (int k = 0; k < 6; ++k) {
        pa[2 + k] += w * aq[k];
        pm[2 + k] += wa * aqa[k];
      }
      int tt = 8;
      for (int k = 0; k < 6; ++k)
        for (int l = k; l < 6; ++l, ++tt) {
          const long double h = -d2 * aq[k] * aq[l] + DOT(icq, Hx[k][l]) + DOT(J[l], cJ[k]);
          const long double ha_ = fabsl(d2) * aqa[k] * aqa[l] + DOT(icqa, Hxa[k][l]) + DOT(Ja[l], cJa[k]);
          pa[tt] += w * h;
          pm[tt] += wa * ha_;
        }
    }
    for (int k = 0; k < ORC_NDT_TERMS; ++k) {
      acc[k] += (f128)pa[k];
      accm[k] += (f128)pm[k];
    }
#undef DOT
  }
  free(cand);
  free(hb);
  for (int k = 0; k < ORC_NDT_TERMS; ++k) {
    sums[k] = (double)acc[k];
    mag[k] = (double)accm[k];
  }
  stats[0] = n_pairs;
  stats[1] = n_skip;
  stats[2] = n_near;
  stats[3] = n_pairs + n_skip;
  return 0;
}
