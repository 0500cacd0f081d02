/* oracle_internal.h -- shared between the oracle's translation units (test infrastructure only). */
#ifndef ORACLE_INTERNAL_H
#define ORACLE_INTERNAL_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
void* orc_kd_build(const float* pts_xyzw, size_t n, int arith);
void orc_kd_free(void* tree);
void orc_kd_nearest(const void* tree, const float* q, int32_t* idx, float* d2);
/* the k smallest (d2, index) keys in ascending order; returns how many were found (min(k, n)) */
int orc_kd_knn(const void* tree, const float* q, int k, int32_t* idx, float* d2);
void orc_svd3(const double A[9], double U[9], double s[3], double V[9]);

/* ---- exact sums (p2plane_oracle.c, icp_oracle.c) ---- */
/* a non-overlapping expansion: the exact sum of every finite term added so far is p[0] + ... + p[n - 1] (increasing
 * magnitude).  Non-finite terms are added plainly into `special` and decide the value (inf, or NaN for inf - inf). */
typedef struct {
  double p[96];
  int n;
  double special;
  int has_special;
} xsum;

static inline void xsum_init(xsum* s) {
  s->n = 0;
  s->special = 0.0;
  s->has_special = 0;
}

static inline void xsum_add(xsum* s, double x) {
  if (!isfinite(x)) {
    s->special += x;
    s->has_special = 1;
    return;
  }
  int m = 0;
  for (int i = 0; i < s->n; ++i) {
    double y = s->p[i];
    if (fabs(x) < fabs(y)) {
      const double t = x;
      x = y;
      y = t;
    }
    const double hi = x + y;
    const double lo = y - (hi - x);
    if (lo != 0.0) s->p[m++] = lo;
    x = hi;
  }
  s->p[m++] = x;
  s->n = m;
}

/* the expansion rounded once to nearest, ties to even: add from the top until a sum is inexact, then settle a tie the
 * remaining components decide (the correction the rounding of hi + lo cannot see) */
static inline double xsum_value(const xsum* s) {
  if (s->has_special) return s->special;
  int n = s->n;
  if (n == 0) return 0.0;
  double hi = s->p[--n], lo = 0.0;
  while (n > 0) {
    const double x = hi, y = s->p[--n];
    hi = x + y;
    lo = y - (hi - x);
    if (lo != 0.0) break;
  }
  if (n > 0 && ((lo < 0.0 && s->p[n - 1] < 0.0) || (lo > 0.0 && s->p[n - 1] > 0.0))) {
    const double y = 2.0 * lo, x = hi + y;
    if (y == x - hi) hi = x;
  }
  return hi;
}
#endif
