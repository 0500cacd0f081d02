/*
 * p2plane_oracle.c -- CPU ORACLE for the point-to-plane mode.  TEST INFRASTRUCTURE ONLY.
 *
 *      ***  PARITY UNPINNED  ***   (see icp_oracle.h)
 *
 * Restates pcl::IterativeClosestPointWithNormals with pcl::registration::TransformationEstimationPointToPlaneLLS of PCL 1.8.x
 * from DESIGN.md section 3's P2PLANE contract:
 *   correspondences      : orc_nn's keys (d2, lowest index) under the float transform, kept when (double)d2 <= r^2
 *   estimateRigidTransformation: per kept pair with a finite normal the float terms
 *                            a = nz sy - ny sz,  b = nx sz - nz sx,  c = ny sx - nx sy,
 *                            r = ((((nx dx + ny dy) + nz dz) - nx sx) - ny sy) - nz sz
 *                          each operation rounded to float on its own, widened; the 29 float64 sums n, sum d2, the upper
 *                          triangle of A^T A over (a, b, c, nx, ny, nz) and A^T r
 *   solve                : ATA.inverse() by Eigen's PartialPivLU, x = inv * ATb, constructTransformationMatrix
 *   loop                 : the point-to-point loop of orc_icp_align (chain, DefaultConvergenceCriteria, forced iterations)
 * Summation: ORC_P2PLANE_SUMS_EXACT rounds each sum once from the exact sum of its terms (an error-free expansion, Shewchuk's
 * grow-expansion as in gicp_oracle.c's TwoSum cascade, carried to as many components as the terms need); every term is a
 * product of two floats and so exact in float64.  ORC_P2PLANE_SUMS_SEQUENTIAL is PCL's plain float64 loop in source order.
 */
#include <float.h>
#include <math.h>
#include <quadmath.h>
#include <stdlib.h>
#include <string.h>

#include "icp_oracle.h"
#include "oracle_internal.h"

/* ------------------------------------------------------------------------------------------ */
/* the 29 sums (exact: the xsum expansion of oracle_internal.h)                                */
/* ------------------------------------------------------------------------------------------ */

static int finite3f(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

/* the terms of one kept pair: t[29] (t[0] = 1, t[1] = d2); returns 0 when the normal is not finite (only t[0], t[1] set) */
static int pair_terms(const float* s, const float* d, const float* nrm, float d2, double t[29]) {
  t[0] = 1.0;
  t[1] = (double)d2;
  if (!finite3f(nrm)) return 0;
  const float nx = nrm[0], ny = nrm[1], nz = nrm[2];
  const float sx = s[0], sy = s[1], sz = s[2];
  float u, v;
  u = nz * sy;
  v = ny * sz;
  const float a = u - v;
  u = nx * sz;
  v = nz * sx;
  const float b = u - v;
  u = ny * sx;
  v = nx * sy;
  const float c = u - v;
  float r = nx * d[0];
  u = ny * d[1];
  r = r + u;
  u = nz * d[2];
  r = r + u;
  u = nx * sx;
  r = r - u;
  u = ny * sy;
  r = r - u;
  u = nz * sz;
  r = r - u;
  const double w[6] = {(double)a, (double)b, (double)c, (double)nx, (double)ny, (double)nz};
  int k = 2;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) t[k++] = w[i] * w[j];
  for (int i = 0; i < 6; ++i) t[23 + i] = w[i] * (double)r;
  return 1;
}

int orc_p2plane_sums(const float* src, size_t n_s, const float* tgt, const float* nrm, const float T[16], const int32_t* idx,
                     const float* d2, double max_dist, int mode, double sums[ORC_P2PLANE_TERMS]) {
  const double r2 = max_dist * max_dist;
  xsum* acc = NULL;
  if (mode != ORC_P2PLANE_SUMS_SEQUENTIAL) {
    acc = (xsum*)malloc(ORC_P2PLANE_TERMS * sizeof(xsum));
    if (!acc) return -1;
    for (int k = 0; k < ORC_P2PLANE_TERMS; ++k) xsum_init(&acc[k]);
  }
  for (int k = 0; k < ORC_P2PLANE_TERMS; ++k) sums[k] = 0.0;
  for (size_t i = 0; i < n_s; ++i) {
    if (idx[i] < 0 || !((double)d2[i] <= r2)) continue;
    float s[4];
    orc_transform_cloud(src + 4 * i, 1, T, s);
    double t[ORC_P2PLANE_TERMS];
    const int full = pair_terms(s, tgt + 4 * (size_t)idx[i], nrm + 4 * (size_t)idx[i], d2[i], t);
    const int nt = full ? ORC_P2PLANE_TERMS : 2;
    for (int k = 0; k < nt; ++k) {
      if (mode == ORC_P2PLANE_SUMS_SEQUENTIAL)
        sums[k] += t[k];
      else
        xsum_add(&acc[k], mode == ORC_P2PLANE_SUMS_ABS ? fabs(t[k]) : t[k]);
    }
  }
  if (acc) {
    for (int k = 0; k < ORC_P2PLANE_TERMS; ++k) sums[k] = xsum_value(&acc[k]);
    free(acc);
  }
  return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* the 6 x 6 solve                                                                             */
/* ------------------------------------------------------------------------------------------ */

static void identity16(double M[16]) {
  for (int i = 0; i < 16; ++i) M[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

/* binary128 rounded once; beyond |x| > 2^19 (never a rotation angle) DESIGN.md section 3 leaves them to the platform's libm */
static void sincos_rounded_once(double x, double* s, double* c) {
  if (fabs(x) <= 524288.0) {
    *s = (double)sinq((__float128)x);
    *c = (double)cosq((__float128)x);
  } else {
    *s = sin(x);
    *c = cos(x);
  }
}

int orc_p2plane_solve(const double sums[ORC_P2PLANE_TERMS], double Tk[16]) {
  identity16(Tk);
  /* ATA from its upper triangle (row by row), ATb */
  double lu[6][6], rhs[6];
  int k = 2;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      lu[i][j] = sums[k];
      lu[j][i] = sums[k];
      ++k;
    }
  for (int i = 0; i < 6; ++i) rhs[i] = sums[23 + i];

  /* PartialPivLU (unblocked at this size): for each column the first row of the largest magnitude at or below the
   * diagonal is the pivot; rows swapped; the column below divided by the pivot; the trailing block takes the rank-1 update */
  int row_of[6];
  for (int i = 0; i < 6; ++i) row_of[i] = i;
  for (int col = 0; col < 6; ++col) {
    int piv = col;
    double big = fabs(lu[col][col]);
    for (int r = col + 1; r < 6; ++r) {
      const double m = fabs(lu[r][col]);
      if (m > big) {
        big = m;
        piv = r;
      }
    }
    if (!(big != 0.0) || isnan(big)) return -1; /* singular (a zero or NaN pivot) */
    if (piv != col) {
      double tmp[6];
      memcpy(tmp, lu[col], sizeof tmp);
      memcpy(lu[col], lu[piv], sizeof tmp);
      memcpy(lu[piv], tmp, sizeof tmp);
      const int t = row_of[col];
      row_of[col] = row_of[piv];
      row_of[piv] = t;
    }
    for (int r = col + 1; r < 6; ++r) lu[r][col] = lu[r][col] / lu[col][col];
    for (int r = col + 1; r < 6; ++r)
      for (int c = col + 1; c < 6; ++c) lu[r][c] = lu[r][c] - lu[r][col] * lu[col][c];
  }

  /* inverse: solve L U X = P I one column of X at a time, forward then backward substitution, each row's products
   * subtracted in increasing column order */
  double inv[6][6];
  for (int c = 0; c < 6; ++c) {
    double z[6];
    for (int r = 0; r < 6; ++r) z[r] = (row_of[r] == c) ? 1.0 : 0.0;
    for (int r = 1; r < 6; ++r)
      for (int j = 0; j < r; ++j) z[r] = z[r] - lu[r][j] * z[j];
    for (int r = 5; r >= 0; --r) {
      for (int j = r + 1; j < 6; ++j) z[r] = z[r] - lu[r][j] * z[j];
      z[r] = z[r] / lu[r][r];
    }
    for (int r = 0; r < 6; ++r) inv[r][c] = z[r];
  }
  double x[6];
  for (int r = 0; r < 6; ++r) {
    double acc = 0.0;
    for (int j = 0; j < 6; ++j) acc = acc + inv[r][j] * rhs[j];
    if (!isfinite(acc)) return -1;
    x[r] = acc;
  }

  /* constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz), sines and cosines correctly rounded */
  double sa, ca, sb, cb, sg, cg;
  sincos_rounded_once(x[0], &sa, &ca);
  sincos_rounded_once(x[1], &sb, &cb);
  sincos_rounded_once(x[2], &sg, &cg);
  double M[16] = {0};
#define AT(r, c) M[(c) * 4 + (r)]
  AT(0, 0) = cg * cb;
  AT(0, 1) = -sg * ca + cg * sb * sa;
  AT(0, 2) = sg * sa + cg * sb * ca;
  AT(1, 0) = sg * cb;
  AT(1, 1) = cg * ca + sg * sb * sa;
  AT(1, 2) = -cg * sa + sg * sb * ca;
  AT(2, 0) = -sb;
  AT(2, 1) = cb * sa;
  AT(2, 2) = cb * ca;
  AT(0, 3) = x[3];
  AT(1, 3) = x[4];
  AT(2, 3) = x[5];
  AT(3, 3) = 1.0;
#undef AT
  memcpy(Tk, M, sizeof M);
  return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* Registration::align                                                                         */
/* ------------------------------------------------------------------------------------------ */

static void mat4_mul_cm(const double A[16], const double B[16], double C[16]) {
  double R[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += A[k * 4 + r] * B[c * 4 + k];
      R[c * 4 + r] = s;
    }
  memcpy(C, R, sizeof R);
}

int orc_p2plane_align(const float* src, size_t n_s, const float* tgt, size_t n_t, const float* nrm_in, const orc_params* P,
                      const float* guess, float* out_xyzw, int want_fitness, orc_result* res, orc_p2plane_trace* trace) {
  if (!P || !res) return -1;
  memset(res, 0, sizeof(*res));
  double final[16];
  identity16(final);
  for (int i = 0; i < 16; ++i) res->T[i] = (float)final[i];
  res->fitness = NAN;
  res->convergence_state = ORC_NOT_CONVERGED;
  if (n_t == 0 || !tgt) { /* setInputTarget refuses an empty target: align returns with identity */
    if (out_xyzw && n_s) orc_transform_cloud(src, n_s, res->T, out_xyzw);
    return 0;
  }
  if (guess)
    for (int i = 0; i < 16; ++i) final[i] = (double)guess[i];
  float finalf[16];
  for (int i = 0; i < 16; ++i) finalf[i] = (float)final[i];

  float* nrm_est = NULL;
  const float* nrm = nrm_in;
  if (!nrm) {
    nrm_est = (float*)malloc(n_t * 4 * sizeof(float));
    if (!nrm_est) return -1;
    orc_gicp_normals(tgt, n_t, P->arith, nrm_est);
    nrm = nrm_est;
  }
  const size_t nalloc = n_s ? n_s : 1;
  float* X = (float*)malloc(nalloc * 4 * sizeof(float));
  int32_t* idx = (int32_t*)malloc(nalloc * sizeof(int32_t));
  float* d2 = (float*)malloc(nalloc * sizeof(float));
  void* tree = P->nn_mode == ORC_NN_KDTREE ? orc_kd_build(tgt, n_t, P->arith) : NULL;

  const double rotation_thr = 1.0 - P->transformation_epsilon, translation_thr = P->transformation_epsilon;
  double mse_prev = DBL_MAX, mse = 0.0;
  int nr_iter = 0, converged = 0, state = ORC_NOT_CONVERGED;
  unsigned n_corr = 0;
  for (;;) {
    if (tree) {
      orc_transform_cloud(src, n_s, finalf, X);
      for (size_t i = 0; i < n_s; ++i) orc_kd_nearest(tree, X + 4 * i, &idx[i], &d2[i]);
    } else {
      orc_nn(src, n_s, tgt, n_t, finalf, ORC_NN_BRUTE, P->arith, idx, d2);
    }
    double sums[ORC_P2PLANE_TERMS];
    orc_p2plane_sums(src, n_s, tgt, nrm, finalf, idx, d2, P->max_correspondence_distance, ORC_P2PLANE_SUMS_EXACT, sums);
    n_corr = (unsigned)sums[0];
    if ((int)n_corr < P->min_correspondences) {
      state = ORC_NO_CORRESPONDENCES;
      converged = 0;
      break;
    }
    double Tk[16];
    if (orc_p2plane_solve(sums, Tk) != 0) { /* singular: stop with the last finite transform */
      state = ORC_NOT_CONVERGED;
      converged = 0;
      break;
    }
    if (trace) {
      orc_p2plane_trace* tr = &trace[nr_iter];
      memcpy(tr->final, final, sizeof(tr->final));
      memcpy(tr->Tk, Tk, sizeof(tr->Tk));
      memcpy(tr->sums, sums, sizeof(tr->sums));
      tr->n_corr = n_corr;
    }
    mat4_mul_cm(Tk, final, final);
    for (int i = 0; i < 16; ++i) finalf[i] = (float)final[i];
    mse = sums[1] / sums[0];
    if (trace) trace[nr_iter].mse = mse;
    ++nr_iter;
    /* DefaultConvergenceCriteria::hasConverged, as orc_icp_align */
    converged = 0;
    if (nr_iter >= P->max_iterations) {
      converged = 1;
      state = ORC_ITERATIONS;
    } else if (!P->force_iterations) {
      const double cos_angle = 0.5 * (Tk[0] + Tk[5] + Tk[10] - 1.0);
      const double tsq = Tk[12] * Tk[12] + Tk[13] * Tk[13] + Tk[14] * Tk[14];
      if (cos_angle >= rotation_thr && tsq <= translation_thr) {
        converged = 1;
        state = ORC_TRANSFORM;
      } else if (fabs(mse - mse_prev) < 1e-12) {
        converged = 1;
        state = ORC_ABS_MSE;
      } else if (fabs(mse - mse_prev) / mse_prev < P->euclidean_fitness_epsilon) {
        converged = 1;
        state = ORC_REL_MSE;
      }
      mse_prev = mse;
    }
    if (converged) break;
  }
  for (int i = 0; i < 16; ++i) res->T[i] = finalf[i];
  res->converged = converged;
  res->iterations = nr_iter;
  res->convergence_state = state;
  res->n_correspondences = n_corr;
  res->mse_last = mse;
  if (out_xyzw) orc_transform_cloud(src, n_s, finalf, out_xyzw);
  if (want_fitness) res->fitness = orc_fitness(src, n_s, tgt, n_t, finalf, DBL_MAX, P->nn_mode, P->arith);
  if (tree) orc_kd_free(tree);
  free(X);
  free(idx);
  free(d2);
  free(nrm_est);
  return 0;
}
