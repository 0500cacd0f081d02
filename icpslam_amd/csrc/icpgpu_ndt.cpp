// icpgpu_ndt.cpp -- NDT registration behind icpgpu_align (method ICPGPU_NDT): pcl::NormalDistributionsTransform with
// pcl::VoxelGridCovariance (PCL 1.8), the other standard scan matcher for 3D LIDAR odometry.  The target's cells (one Gaussian per
// voxel of >= 6 points) are built on the device once per target cloud and resolution (icp_ndt.hip); every Newton iteration is
// one derivative pass (ndt_deriv_kernel + the fixed-order final sum into the result mailbox) -> the host solves the 6 x 6 system
// by a pseudo-inverse, takes PCL 1.8's step (computeStepLengthMT without a More-Thuente trial: DESIGN.md) and builds the float
// transform of the new pose.  Opt-in per context (icpgpu_set_ndt_line_search): the More-Thuente line search with its loop running,
// whose loop trials are score-and-gradient passes (ndt_grad_kernel).  The contract, rule by rule, is DESIGN.md's NDT section.
#include "icp_ctx.h"
#include "icp_voxel_plan.h"
#include "icp_trig.h"

namespace icpgpu_impl {

namespace {

struct GaussConst {
  double d1, d2;
};

// PCL 1.8 NormalDistributionsTransform::computeTransformation: the Gauss fitting constants (Magnusson 2009, eq. 6.8)
GaussConst gauss_constants(double resolution, double outlier_ratio) {
  const double c1 = 10.0 * (1.0 - outlier_ratio);
  const double c2 = outlier_ratio / (resolution * resolution * resolution);
  const double d3 = -std::log(c2);
  GaussConst g;
  g.d1 = -std::log(c1 + c2) - d3;
  g.d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / g.d1);
  return g;
}

// computeAngleDerivatives: PCL's j_ang_a .. h and h_ang_a2 .. f3 at the angles of p, in double, |angle| < 1e-4 -> cos 1, sin 0
void angle_terms(const double p[6], NdtPass& P) {
  double s[3], c[3];
  for (int a = 0; a < 3; ++a) {
    if (std::fabs(p[3 + a]) < 10e-5) {
      c[a] = 1.0;
      s[a] = 0.0;
    } else {
      trig::sincos_cr(p[3 + a], &s[a], &c[a]);
    }
  }
  const double cx = c[0], sx = s[0], cy = c[1], sy = s[1], cz = c[2], sz = s[2];
  const double j[8][3] = {{-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy},
                          {cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy},
                          {-sy * cz, sy * sz, cy},
                          {sx * cy * cz, -sx * cy * sz, sx * sy},
                          {-cx * cy * cz, cx * cy * sz, -cx * sy},
                          {-cy * sz, -cy * cz, 0.0},
                          {cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0.0},
                          {sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0.0}};
  const double h[15][3] = {{-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, sx * cy},   // a2
                           {-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, -cx * cy},  // a3
                           {cx * cy * cz, -cx * cy * sz, cx * sy},                        // b2
                           {sx * cy * cz, -sx * cy * sz, sx * sy},                        // b3
                           {-sx * cz - cx * sy * sz, sx * sz - cx * sy * cz, 0.0},        // c2
                           {cx * cz - sx * sy * sz, -sx * sy * cz - cx * sz, 0.0},        // c3
                           {-cy * cz, cy * sz, -sy},                                      // d1
                           {-sx * sy * cz, sx * sy * sz, sx * cy},                        // d2
                           {cx * sy * cz, -cx * sy * sz, -cx * cy},                       // d3
                           {sy * sz, sy * cz, 0.0},                                       // e1
                           {-sx * cy * sz, -sx * cy * cz, 0.0},                           // e2
                           {cx * cy * sz, cx * cy * cz, 0.0},                             // e3
                           {-cy * cz, cy * sz, 0.0},                                      // f1
                           {-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, 0.0},       // f2
                           {-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, 0.0}};      // f3
  std::memcpy(P.j_ang, j, sizeof j);
  std::memcpy(P.h_ang, h, sizeof h);
}

// Eigen's AngleAxisf(angle, unit axis).toRotationMatrix() in float, row-major 3x3
void angle_axis_f(float angle, int axis, float R[3][3]) {
  float s, c;
  trig::sincosf_cr(angle, &s, &c);
  const float ax[3] = {axis == 0 ? 1.f : 0.f, axis == 1 ? 1.f : 0.f, axis == 2 ? 1.f : 0.f};
  const float sa[3] = {s * ax[0], s * ax[1], s * ax[2]};
  const float ca[3] = {(1.f - c) * ax[0], (1.f - c) * ax[1], (1.f - c) * ax[2]};
  for (int i = 0; i < 3; ++i) R[i][i] = ca[i] * ax[i] + c;
  R[0][1] = ca[0] * ax[1] - sa[2];
  R[1][0] = ca[0] * ax[1] + sa[2];
  R[0][2] = ca[0] * ax[2] + sa[1];
  R[2][0] = ca[0] * ax[2] - sa[1];
  R[1][2] = ca[1] * ax[2] - sa[0];
  R[2][1] = ca[1] * ax[2] + sa[0];
}

void mul3f(const float A[3][3], const float B[3][3], float C[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}

}  // namespace

// Translation3f(p0..2) * AngleAxisf(p3, X) * AngleAxisf(p4, Y) * AngleAxisf(p5, Z) -> column-major float[16]
void ndt_transform_float(const double p[6], float T[16]) {
  float Rx[3][3], Ry[3][3], Rz[3][3], A[3][3], R[3][3];
  angle_axis_f((float)p[3], 0, Rx);
  angle_axis_f((float)p[4], 1, Ry);
  angle_axis_f((float)p[5], 2, Rz);
  mul3f(Rx, Ry, A);
  mul3f(A, Rz, R);
  for (int i = 0; i < 16; ++i) T[i] = 0.f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = R[r][c];
  T[12] = (float)p[0];
  T[13] = (float)p[1];
  T[14] = (float)p[2];
  T[15] = 1.f;
}

// p0 of computeTransformation: the guess's translation and eulerAngles(0, 1, 2) of its rotation, as floats (Vector3f), in double
void ndt_initial_pose(const float* guess, double p[6]) {
  if (!guess) {
    for (int k = 0; k < 6; ++k) p[k] = 0.0;
    return;
  }
  double m[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m[r][c] = (double)guess[c * 4 + r];
  // Eigen's MatrixBase::eulerAngles(0, 1, 2): i = 0, j = 1, k = 2, odd = 0
  double r0 = std::atan2(m[1][2], m[2][2]), r1;
  const double c2 = std::hypot(m[0][0], m[0][1]);
  if (r0 > 0.0) {
    r0 = r0 - M_PI;
    r1 = std::atan2(-m[0][2], -c2);
  } else {
    r1 = std::atan2(-m[0][2], c2);
  }
  const double s1 = std::sin(r0), c1 = std::cos(r0);
  const double r2 = std::atan2(s1 * m[2][0] - c1 * m[1][0], c1 * m[1][1] - s1 * m[2][1]);
  const double ang[3] = {-r0, -r1, -r2};
  for (int k = 0; k < 3; ++k) {
    p[k] = (double)guess[12 + k];
    p[3 + k] = (double)(float)ang[k];
  }
}

// H x = b for symmetric H (6 x 6) as JacobiSVD<Matrix6d>::solve: singular values <= sigma_max * 6 * 2^-52 count as zero.  For a
// symmetric matrix the singular values are |eigenvalues|: a cyclic Jacobi eigen-decomposition gives the pseudo-inverse directly.
static void pinv_solve6(const double H[6][6], const double b[6], double x[6]) {
  double a[6][6], v[6][6];
  bool finite = true;
  for (int i = 0; i < 6; ++i) {
    finite = finite && std::isfinite(b[i]);
    for (int j = 0; j < 6; ++j) {
      a[i][j] = H[i][j];
      v[i][j] = i == j ? 1.0 : 0.0;
      finite = finite && std::isfinite(H[i][j]);
    }
  }
  if (!finite) {  // (JacobiSVD of a matrix with a NaN or an infinity: a NaN solution)
    for (int i = 0; i < 6; ++i) x[i] = NAN;
    return;
  }
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < 6; ++i) {
      diag += a[i][i] * a[i][i];
      for (int j = i + 1; j < 6; ++j) off += a[i][j] * a[i][j];
    }
    if (!(off > 1e-60 * diag) || !std::isfinite(off)) break;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; ++k) {  // columns p, q of a
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {  // rows p, q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        a[p][q] = a[q][p] = 0.0;
        for (int k = 0; k < 6; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
  double smax = 0.0;
  bool nan = false;
  for (int i = 0; i < 6; ++i) {
    if (a[i][i] != a[i][i]) nan = true;
    smax = std::max(smax, std::fabs(a[i][i]));
  }
  const double thr = std::max(smax * 6.0 * std::ldexp(1.0, -52), DBL_MIN);
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  if (nan) {
    for (int i = 0; i < 6; ++i) x[i] = NAN;
    return;
  }
  for (int e = 0; e < 6; ++e) {
    const double lam = a[e][e];
    if (!(std::fabs(lam) > thr)) continue;
    double vb = 0.0;
    for (int k = 0; k < 6; ++k) vb += v[k][e] * b[k];
    const double f = vb / lam;
    for (int k = 0; k < 6; ++k) x[k] += v[k][e] * f;
  }
}

// The Newton direction of computeTransformation from an evaluation's 29 sums: delta = pseudo-inverse(H) (-g).  NDT_ZERO / NDT_NAN:
// |delta| is 0 / NaN, PCL returns.  Else d = delta / |delta|, flipped when -(g . d) > 0 so that it descends, *norm = |delta|,
// *d_phi_0 = -(g . d) before the flip (exactly 0: no descent, PCL's step is 0).
enum { NDT_STEP = 0, NDT_ZERO = 1, NDT_NAN = 2 };
static int ndt_direction(const double sums[kNdtTerms], double d[6], double* norm_out, double* d_phi_0_out) {
  double H[6][6], g[6], b[6];
  for (int k = 0; k < 6; ++k) g[k] = sums[2 + k];
  for (int i = 0, t = 8; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++t) H[i][j] = H[j][i] = sums[t];
  for (int k = 0; k < 6; ++k) b[k] = -g[k];
  pinv_solve6(H, b, d);
  double nn = 0.0;
  for (int k = 0; k < 6; ++k) nn += d[k] * d[k];
  const double norm = std::sqrt(nn);
  *norm_out = norm;
  *d_phi_0_out = 0.0;
  if (norm == 0.0) return NDT_ZERO;
  if (norm != norm) return NDT_NAN;
  for (int k = 0; k < 6; ++k) d[k] /= norm;
  double gd = 0.0;
  for (int k = 0; k < 6; ++k) gd += g[k] * d[k];
  const double d_phi_0 = -gd;
  *d_phi_0_out = d_phi_0;
  if (d_phi_0 > 0.0)
    for (int k = 0; k < 6; ++k) d[k] = -d[k];
  return NDT_STEP;
}

// One Newton step of computeTransformation from an evaluation's 29 sums at p (PCL 1.8; computeStepLengthMT's line search makes no
// More-Thuente trial: interval_converged starts true).  NDT_STEP: p_out = p + a d^, *step = a, T_out = T(p_out) (when g . d^ is
// exactly 0: a = 0, p_out = p, T_out = T(p), and no evaluation follows); NDT_ZERO / NDT_NAN: |delta| is 0 / NaN, PCL returns.
int ndt_step_impl(const double sums[kNdtTerms], const double p[6], double step_size, double eps, double p_out[6], double* step,
                  float T_out[16], bool* evaluate) {
  double d[6], norm, d_phi_0;
  const int st = ndt_direction(sums, d, &norm, &d_phi_0);
  for (int k = 0; k < 6; ++k) p_out[k] = p[k];
  *step = 0.0;
  *evaluate = false;
  ndt_transform_float(p, T_out);
  if (st != NDT_STEP) return st;
  if (d_phi_0 == 0.0) return NDT_STEP;  // step 0: p stays, nothing is evaluated
  double a = std::min(norm, step_size);
  a = std::max(a, eps / 2.0);
  for (int k = 0; k < 6; ++k) p_out[k] = p[k] + d[k] * a;
  *step = a;
  *evaluate = true;
  ndt_transform_float(p_out, T_out);
  return NDT_STEP;
}

// ---- the More-Thuente line search (ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE): computeStepLengthMT with its loop running ----------------
// The rule is DESIGN.md's (f6, "More-Thuente step rule"); the sequence of trial steps is a function of the observed (phi, phi')
// alone, so the host replays it without a device (icpgpu_ndt_line_search_replay) and tests/ndt_line_search_restated.py restates it.
namespace mt {

constexpr double kMu = 1e-4, kNu = 0.9;
constexpr int kMaxLoopTrials = 10;

struct Search {
  double phi_0, d_phi_0, step_max, step_min;
  double a_l = 0.0, f_l = 0.0, g_l = 0.0, a_u = 0.0, f_u = 0.0, g_u = 0.0;
  bool open = true, interval_converged = false;
  int trials = 0;       // observed trials, the first included
  int loop_trials = 0;  // observed trials of the loop (PCL's step_iterations)
  double a_t = 0.0;     // the pending trial's step; after an exit, the accepted step
  int final_trial = -1;
  double a_prev = 0.0;  // the last observed trial's step
};

double psi(double a, double f_a, double f_0, double g_0) { return f_a - f_0 - kMu * g_0 * a; }  // auxilaryFunction_PsiMT
double dpsi(double g_a, double g_0) { return g_a - kMu * g_0; }                                  // auxilaryFunction_dPsiMT

double clamp_step(double a, double step_max, double step_min) {
  a = std::min(a, step_max);
  return std::max(a, step_min);
}

// trialValueSelectionMT (More & Thuente 1994, its four cases; the cubic and quadratic minimisers of Sun & Yuan 2006, 2.4.52 / 2.4.56,
// 2.4.2 and 2.4.5)
double trial_value(double a_l, double f_l, double g_l, double a_u, double f_u, double g_u, double a_t, double f_t, double g_t) {
  if (f_t > f_l) {  // case 1
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
    if (std::fabs(a_c - a_l) < std::fabs(a_q - a_l)) return a_c;
    return 0.5 * (a_q + a_c);
  }
  if (g_t * (a_l - a_t) > 0) {  // case 2
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    if (std::fabs(a_c - a_t) >= std::fabs(a_s - a_t)) return a_c;
    return a_s;
  }
  if (std::fabs(g_t) <= std::fabs(g_l)) {  // case 3
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    const double a_t_next = std::fabs(a_c - a_t) < std::fabs(a_s - a_t) ? a_c : a_s;
    if (a_t > a_l) return std::min(a_t + 0.66 * (a_u - a_t), a_t_next);
    return std::max(a_t + 0.66 * (a_u - a_t), a_t_next);
  }
  // case 4
  const double z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u;
  const double w = std::sqrt(z * z - g_t * g_u);
  return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w);
}

// updateIntervalMT: cases U1 / a, U2 / b, U3 / c; true = the interval has converged
bool update_interval(double& a_l, double& f_l, double& g_l, double& a_u, double& f_u, double& g_u, double a_t, double f_t, double g_t) {
  if (f_t > f_l) {
    a_u = a_t;
    f_u = f_t;
    g_u = g_t;
    return false;
  }
  if (g_t * (a_l - a_t) > 0) {
    a_l = a_t;
    f_l = f_t;
    g_l = g_t;
    return false;
  }
  if (g_t * (a_l - a_t) < 0) {
    a_u = a_l;
    f_u = f_l;
    g_u = g_l;
    a_l = a_t;
    f_l = f_t;
    g_l = g_t;
    return false;
  }
  return true;
}

// phi_0 = -score at x, d_phi_0 = -(g . d) < 0 (d already descends), step_init = |delta|; -> the first trial's step in S.a_t
void start(Search& S, double phi_0, double d_phi_0, double step_init, double step_max, double step_min) {
  S = Search{};
  S.phi_0 = phi_0;
  S.d_phi_0 = d_phi_0;
  S.step_max = step_max;
  S.step_min = step_min;
  S.f_l = S.f_u = psi(0.0, phi_0, phi_0, d_phi_0);
  S.g_l = S.g_u = dpsi(d_phi_0, d_phi_0);
  S.interval_converged = (step_max - step_min) < 0;  // (PCL 1.8 tests > 0: always true, so its loop never runs)
  S.a_t = clamp_step(step_init, step_max, step_min);
}

// the pending trial (step S.a_t) observed phi_t, d_phi_t -> ICPGPU_NDT_MT_TRIAL (S.a_t = the next trial's step) or an exit
// (S.a_t = the accepted step, S.final_trial = its index)
int observe(Search& S, double phi_t, double d_phi_t) {
  const int k = S.trials++;
  const double a_t = S.a_t;
  if (!std::isfinite(phi_t) || !std::isfinite(d_phi_t)) {  // (deviation: PCL leaves it undefined)
    if (k == 0) {  // the first trial stands, as under PCL 1.8's rule; the next Newton solve sees its sums
      S.final_trial = 0;
    } else {       // the previous trial stands
      S.final_trial = k - 1;
      S.a_t = S.a_prev;
    }
    return ICPGPU_NDT_MT_NON_FINITE;
  }
  S.a_prev = a_t;
  const double psi_t = psi(a_t, phi_t, S.phi_0, S.d_phi_0);
  const double d_psi_t = dpsi(d_phi_t, S.d_phi_0);
  if (k > 0) {
    if (S.open && (psi_t <= 0 && d_psi_t >= 0)) {
      S.open = false;
      S.f_l = S.f_l + S.phi_0 - kMu * S.d_phi_0 * S.a_l;
      S.g_l = S.g_l + kMu * S.d_phi_0;
      S.f_u = S.f_u + S.phi_0 - kMu * S.d_phi_0 * S.a_u;
      S.g_u = S.g_u + kMu * S.d_phi_0;
    }
    S.interval_converged = S.open ? update_interval(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, a_t, psi_t, d_psi_t)
                                  : update_interval(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, a_t, phi_t, d_phi_t);
    ++S.loop_trials;
  }
  S.final_trial = k;
  if (psi_t <= 0 && d_phi_t <= -kNu * S.d_phi_0) return ICPGPU_NDT_MT_WOLFE;
  if (S.interval_converged) return ICPGPU_NDT_MT_INTERVAL;
  if (S.loop_trials >= kMaxLoopTrials) return ICPGPU_NDT_MT_TRIAL_CAP;
  double next = S.open ? trial_value(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, a_t, psi_t, d_psi_t)
                       : trial_value(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, a_t, phi_t, d_phi_t);
  next = clamp_step(next, S.step_max, S.step_min);
  if (next != next) return ICPGPU_NDT_MT_NAN_STEP;  // (deviation: the search ends at this trial)
  S.final_trial = -1;
  S.a_t = next;
  return ICPGPU_NDT_MT_TRIAL;
}

}  // namespace mt

// The target's cells at the context's resolution: built when the target version or the resolution changed
static int ensure_ndt_cells(icpgpu_ctx* c) {
  auto& N = c->ndt;
  if (N.version == c->tgt_version && N.resolution == c->ndt_resolution && N.key.ptr) return ICPGPU_OK;
  N.version = 0;
  N.n_cells = 0;
  N.excess = 0.0;
  const int n = (int)c->tgt.n;
  int rc;
  for (DeviceBuf* b : {&N.key, &N.centroid, &N.gauss_c, &N.n_points})
    if ((rc = ensure(c, *b, 16))) return rc;  // (never null, even without a cell)
  if ((rc = ensure(c, N.stats, 8 * sizeof(int)))) return rc;
  if (n > 0) {
    int* d_box = static_cast<int*>(N.stats.ptr);
    HIP_TRY(c, launch_bbox(c->tgt.data(), n, d_box, c->stream));
    int hv[6];
    if ((rc = fetch_ints(c, d_box, 6, hv))) return rc;
    float lo[3], hi[3];
    decode_bbox(hv, lo, hi);
    if (lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]) {  // (no finite point: no cell)
      // the voxel filter's arithmetic (icpgpu_voxel.cpp) at leaf = resolution
      const float leaf = (float)c->ndt_resolution;
      const float inv = 1.0f / leaf;
      NdtLattice L{};
      // the voxel filter's plan (icp_voxel_plan.h: exact staged products, no out-of-range cast); what PCL would pass through, and an
      // index that wraps, are refused here
      long long ncells = 0;
      if (voxel_grid_plan(lo, hi, inv, L.minb, L.divb, &ncells) != kVoxelPlanDirect)
        return fail(c, ICPGPU_ERR_INVALID_ARG, "NDT: the cell index overflows at resolution %g for this target", c->ndt_resolution);
      L.mul_y = L.divb[0];
      L.mul_z = L.divb[0] * L.divb[1];
      L.inv_leaf_f = inv;
      L.inv_leaf = (double)inv;
      const size_t nn = (size_t)n;
      const size_t temp_ints = std::max(radix_sort_scratch_ints(n), exclusive_scan_scratch_ints(n));
      if ((rc = ensure(c, N.keys, 2 * nn * sizeof(int))) || (rc = ensure(c, N.vals, 2 * nn * sizeof(int))) ||
          (rc = ensure(c, N.flags, nn * sizeof(int))) || (rc = ensure(c, N.slots, nn * sizeof(int))) ||
          (rc = ensure(c, N.temp, temp_ints * sizeof(int))) || (rc = ensure(c, N.valid, nn * sizeof(int))) ||
          (rc = ensure(c, N.vslots, nn * sizeof(int))) || (rc = ensure(c, N.ckey, nn * sizeof(int))) ||
          (rc = ensure(c, N.cent, nn * sizeof(float4))) || (rc = ensure(c, N.gauss, nn * kNdtGaussDoubles * sizeof(double))) ||
          (rc = ensure(c, N.npts, nn * sizeof(int))) || (rc = ensure(c, N.cell_excess, nn * sizeof(double))) ||
          (rc = ensure(c, N.key, nn * sizeof(int))) || (rc = ensure(c, N.centroid, nn * sizeof(float4))) ||
          (rc = ensure(c, N.gauss_c, nn * kNdtGaussDoubles * sizeof(double))) || (rc = ensure(c, N.n_points, nn * sizeof(int))))
        return rc;
      int* keys = static_cast<int*>(N.keys.ptr);
      int* vals = static_cast<int*>(N.vals.ptr);
      int* temp = static_cast<int*>(N.temp.ptr);
      HIP_TRY(c, launch_ndt_keys(c->tgt.data(), n, L, keys, vals, temp, c->stream));
      int* stats = static_cast<int*>(N.stats.ptr);
      HIP_TRY(c, launch_ndt_cells(c->tgt.data(), n, L, keys + n, vals + n, static_cast<int*>(N.flags.ptr), static_cast<int*>(N.slots.ptr),
                                  temp, static_cast<int*>(N.valid.ptr), static_cast<int*>(N.vslots.ptr), static_cast<int*>(N.ckey.ptr),
                                  static_cast<float4*>(N.cent.ptr), static_cast<double*>(N.gauss.ptr), static_cast<int*>(N.npts.ptr),
                                  static_cast<double*>(N.cell_excess.ptr), static_cast<int*>(N.key.ptr), static_cast<float4*>(N.centroid.ptr),
                                  static_cast<double*>(N.gauss_c.ptr), static_cast<int*>(N.n_points.ptr), stats, c->stream));
      int st[3];
      if ((rc = fetch_ints(c, stats, 3, st))) return rc;
      const unsigned long long bits = (unsigned long long)(unsigned int)st[1] | ((unsigned long long)(unsigned int)st[2] << 32);
      N.n_cells = st[0];
      std::memcpy(&N.excess, &bits, sizeof bits);
      N.L = L;
    }
  }
  N.version = c->tgt_version;
  N.resolution = c->ndt_resolution;
  return ICPGPU_OK;
}

// one derivative pass at the float transform T and the pose p: the 29 sums (computeDerivatives) -> sums (host); without hessian the
// trial pass, whose 8 sums (pairs, score, gradient) are the first 8 of the 29 -- sums[8..28] are left as they were
static int ndt_evaluate(icpgpu_ctx* c, const float T[16], const double p[6], double sums[kNdtTerms], bool mailbox, bool hessian = true) {
  const int n_s = (int)c->src.n;
  int rc = ensure(c, c->ndt_partials, (size_t)ndt_blocks(n_s) * kNdtTerms * sizeof(double));
  if (rc) return rc;
  NdtPass P{};
  const double r = c->ndt_resolution;
  const GaussConst G = gauss_constants(r, c->ndt_outlier_ratio);
  P.r_wide = r * (1.0 + 1e-6);
  P.excess = c->ndt.excess;
  P.d1 = G.d1;
  P.d2 = G.d2;
  P.r2f = (float)(r * r);
  angle_terms(p, P);
  const auto& N = c->ndt;
  const unsigned long long seq = mailbox ? ++c->sums_seq : 0;
  HIP_TRY(c, launch_ndt_derivatives(c->src.data(), n_s, to_xform(T), N.L, P, static_cast<const int*>(N.key.ptr),
                                    static_cast<const float4*>(N.centroid.ptr), static_cast<const double*>(N.gauss_c.ptr), N.n_cells,
                                    static_cast<double*>(c->ndt_partials.ptr), mailbox ? nullptr : static_cast<double*>(c->sums.ptr),
                                    mailbox ? c->h_flags_dev : nullptr, mailbox ? wire_seq(c, seq) : 0, c->stream, hessian));
  c->prof.reduce_launches += 1;
  const int terms = hessian ? kNdtTerms : kNdtGradTerms;
  if (mailbox) {
    if ((rc = wait_flags(c, c->h_flags, terms, seq))) return rc;
    for (int k = 0; k < terms; ++k) {
      const unsigned long long bits = c->h_flags[2 * k];
      std::memcpy(&sums[k], &bits, sizeof bits);
    }
    return ICPGPU_OK;
  }
  HIP_TRY(c, hipMemcpyAsync(sums, c->sums.ptr, terms * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ICPGPU_OK;
}

// -(g . d) from an evaluation's gradient
static double ndt_d_phi(const double sums[kNdtTerms], const double d[6]) {
  double gd = 0.0;
  for (int k = 0; k < 6; ++k) gd += sums[2 + k] * d[k];
  return -gd;
}

// One Newton step under the More-Thuente rule: the direction as ndt_step_impl's, then computeStepLengthMT with its
// loop running.  The first trial is a 29-term pass (PCL's computeDerivatives with the Hessian), every loop trial a trial pass (score
// and gradient); when the search ends on a loop trial, one 29-term pass at that trial's pose gives the Hessian (PCL's
// computeHessian).  On NDT_STEP: p, Tf and sums are those of the accepted trial and *a its step (a = 0 and nothing changes when
// g . d is exactly 0).
static int ndt_step_mt(icpgpu_ctx* c, int iteration, double eps, double p[6], float Tf[16], double sums[kNdtTerms], double* a, int* st) {
  double d[6], norm, d_phi_0;
  *a = 0.0;
  *st = ndt_direction(sums, d, &norm, &d_phi_0);
  if (*st != NDT_STEP || d_phi_0 == 0.0) return ICPGPU_OK;
  if (d_phi_0 > 0.0) d_phi_0 = -d_phi_0;  // (ndt_direction flipped d)
  struct Trial {
    double x[6];
    float T[16];
    double sums[kNdtTerms];
  } cur{}, prev{};
  mt::Search S;
  mt::start(S, -sums[1], d_phi_0, norm, c->ndt_step_size, eps / 2.0);
  int rc, exit;
  do {
    const bool first = S.trials == 0;
    prev = cur;
    for (int k = 0; k < 6; ++k) cur.x[k] = p[k] + d[k] * S.a_t;
    ndt_transform_float(cur.x, cur.T);
    if ((rc = ndt_evaluate(c, cur.T, cur.x, cur.sums, true, /*hessian=*/first))) return rc;
    const double phi_t = -cur.sums[1], d_phi_t = ndt_d_phi(cur.sums, d);
    c->ndt_trace.push_back({iteration, S.a_t, phi_t, d_phi_t});
    exit = mt::observe(S, phi_t, d_phi_t);
  } while (exit == ICPGPU_NDT_MT_TRIAL);
  const Trial& acc = S.final_trial == S.trials - 1 ? cur : prev;
  std::memcpy(p, acc.x, sizeof acc.x);
  std::memcpy(Tf, acc.T, sizeof acc.T);
  std::memcpy(sums, acc.sums, sizeof acc.sums);
  if (S.final_trial > 0 && (rc = ndt_evaluate(c, Tf, p, sums, true, /*hessian=*/true))) return rc;
  *a = S.a_t;
  return ICPGPU_OK;
}

int align_ndt(icpgpu_ctx* c, const float* guess, float* out_xyzw, int want_fitness, icpgpu_result* res) {
  const auto t_start = std::chrono::steady_clock::now();
  int rc = call_begin(c, res);
  if (rc) return rc;
  c->ndt_probability = NAN;
  c->ndt_trace.clear();
  float Tf[16];
  for (int i = 0; i < 16; ++i) Tf[i] = guess ? guess[i] : (i % 5 == 0 ? 1.f : 0.f);
  const int n_s = (int)c->src.n, n_t = (int)c->tgt.n;
  bool converged = false;
  int nr = 0, state = ICPGPU_NOT_CONVERGED;
  unsigned n_corr = 0;
  if (n_t == 0) {  // PCL: setInputTarget refuses an empty target, align() leaves converged_ = false and T = identity
    for (int i = 0; i < 16; ++i) Tf[i] = i % 5 == 0 ? 1.f : 0.f;
  } else {
    if ((rc = ensure_ndt_cells(c))) return rc;
    const icpgpu_params& P = c->params;
    const double eps = P.transformation_epsilon;
    double p[6], sums[kNdtTerms];
    ndt_initial_pose(guess, p);
    if ((rc = ndt_evaluate(c, Tf, p, sums, true))) return rc;
    n_corr = (unsigned)sums[0];
    if (n_corr == 0) {  // no pair at p0: delta is 0, PCL returns converged with the guess
      converged = true;
      state = ICPGPU_CONV_NO_CORRESPONDENCES;
    } else {
      const bool more_thuente = c->ndt_line_search == ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE;
      for (;;) {
        double p_new[6], a;
        float T_new[16];
        bool evaluate = false;
        int st;
        if (more_thuente) {
          if ((rc = ndt_step_mt(c, nr, eps, p, Tf, sums, &a, &st))) return rc;
          n_corr = (unsigned)sums[0];
        } else {
          st = ndt_step_impl(sums, p, c->ndt_step_size, eps, p_new, &a, T_new, &evaluate);
        }
        if (st == NDT_ZERO) {
          converged = true;
          state = ICPGPU_CONV_TRANSFORM;
          break;
        }
        if (st == NDT_NAN) {  // the last finite transform stays
          converged = false;
          state = ICPGPU_NOT_CONVERGED;
          break;
        }
        if (evaluate) {
          std::memcpy(p, p_new, sizeof p);
          std::memcpy(Tf, T_new, sizeof Tf);
          if ((rc = ndt_evaluate(c, Tf, p, sums, true))) return rc;
          n_corr = (unsigned)sums[0];
        }
        c->prof.iterations += 1;
        const bool cap = nr > P.max_iterations;
        if (cap || (nr && std::fabs(a) < eps)) {
          converged = true;
          state = cap ? ICPGPU_CONV_ITERATIONS : ICPGPU_CONV_TRANSFORM;
          ++nr;
          break;
        }
        ++nr;
      }
    }
    c->ndt_probability = sums[1] / (double)n_s;
  }
  record_result(c, res, Tf, converged, nr, state, n_corr, /*mse=*/NAN);  // (NDT has no mean squared error to report)
  const bool fitness = want_fitness && n_t > 0;
  // the fitness sweep wants the search grid, which nothing of NDT has asked for (built, on a target's first call, ahead of the cloud)
  if (fitness && (rc = ensure_grid(c, gate_threshold(c)))) return rc;
  return cloud_then_fitness(c, to_xform(Tf), out_xyzw, fitness, res, t_start);
}

}  // namespace icpgpu_impl

using namespace icpgpu_impl;

extern "C" {

int icpgpu_set_ndt_params(icpgpu_ctx* c, double resolution, double step_size, double outlier_ratio) {
  if (!c) return fail(nullptr, ICPGPU_ERR_INVALID_ARG, "null context");
  if (!(resolution > 0.0) || !std::isfinite(resolution)) return fail(c, ICPGPU_ERR_INVALID_ARG, "NDT: resolution must be positive");
  if (!(step_size > 0.0) || !std::isfinite(step_size)) return fail(c, ICPGPU_ERR_INVALID_ARG, "NDT: step size must be positive");
  if (!(outlier_ratio > 0.0 && outlier_ratio < 1.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "NDT: outlier ratio must lie in (0, 1)");
  c->ndt_resolution = resolution;
  c->ndt_step_size = step_size;
  c->ndt_outlier_ratio = outlier_ratio;
  return ICPGPU_OK;
}

int icpgpu_get_ndt_params(const icpgpu_ctx* c, double* resolution, double* step_size, double* outlier_ratio) {
  if (!c) return ICPGPU_ERR_INVALID_ARG;
  if (resolution) *resolution = c->ndt_resolution;
  if (step_size) *step_size = c->ndt_step_size;
  if (outlier_ratio) *outlier_ratio = c->ndt_outlier_ratio;
  return ICPGPU_OK;
}

int icpgpu_ndt_transformation_probability(const icpgpu_ctx* c, double* out) {
  if (!c || !out) return ICPGPU_ERR_INVALID_ARG;
  *out = c->ndt_probability;
  return ICPGPU_OK;
}

int icpgpu_ndt_cells(icpgpu_ctx* c, size_t capacity, float* centroid_xyzw, double* mean3, double* icov6, int32_t* n_points,
                     size_t* n_cells) {
  ENTER(c);
  if (!n_cells) return fail(c, ICPGPU_ERR_INVALID_ARG, "null argument");
  *n_cells = 0;
  if (!c->tgt.set) return fail(c, ICPGPU_ERR_NO_INPUT, "ndt_cells: no target set");
  int rc = ensure_ndt_cells(c);
  if (rc) return rc;
  const auto& N = c->ndt;
  const size_t n = (size_t)N.n_cells;
  *n_cells = n;
  if (n > capacity || n == 0) return ICPGPU_OK;  // (the count alone: size the buffers and call again)
  if (centroid_xyzw) HIP_TRY(c, hipMemcpyAsync(centroid_xyzw, N.centroid.ptr, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  if (n_points) HIP_TRY(c, hipMemcpyAsync(n_points, N.n_points.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  std::vector<double> g;
  if (mean3 || icov6) {
    g.resize(n * kNdtGaussDoubles);
    HIP_TRY(c, hipMemcpyAsync(g.data(), N.gauss_c.ptr, g.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n && !g.empty(); ++i) {
    if (mean3)
      for (int a = 0; a < 3; ++a) mean3[3 * i + a] = g[i * kNdtGaussDoubles + a];
    if (icov6)
      for (int e = 0; e < 6; ++e) icov6[6 * i + e] = g[i * kNdtGaussDoubles + 3 + e];
  }
  return ICPGPU_OK;
}

int icpgpu_ndt_derivatives(icpgpu_ctx* c, const double p[6], double sums[29]) {
  ENTER(c);
  if (!p || !sums) return fail(c, ICPGPU_ERR_INVALID_ARG, "null argument");
  if (!c->src.set || !c->tgt.set) return fail(c, ICPGPU_ERR_NO_INPUT, "ndt_derivatives: source and target must be set first");
  int rc = ensure_ndt_cells(c);
  if (rc) return rc;
  if ((rc = ensure(c, c->sums, kNdtTerms * sizeof(double)))) return rc;
  float T[16];
  ndt_transform_float(p, T);
  return ndt_evaluate(c, T, p, sums, /*mailbox=*/false);
}

int icpgpu_ndt_step(const double sums[29], const double p[6], double step_size, double eps, double p_out[6], double* step,
                    float T_out[16]) {
  if (!sums || !p || !p_out || !step || !T_out) return ICPGPU_ERR_INVALID_ARG;
  bool evaluate;
  return ndt_step_impl(sums, p, step_size, eps, p_out, step, T_out, &evaluate);
}

int icpgpu_set_ndt_line_search(icpgpu_ctx* c, int mode) {
  if (!c) return fail(nullptr, ICPGPU_ERR_INVALID_ARG, "null context");
  if (mode != ICPGPU_NDT_LINE_SEARCH_PCL18 && mode != ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "NDT: unknown line search %d", mode);
  c->ndt_line_search = mode;
  return ICPGPU_OK;
}

int icpgpu_get_ndt_line_search(const icpgpu_ctx* c, int* mode) {
  if (!c || !mode) return ICPGPU_ERR_INVALID_ARG;
  *mode = c->ndt_line_search;
  return ICPGPU_OK;
}

int icpgpu_ndt_gradient(icpgpu_ctx* c, const double p[6], double sums[8]) {
  ENTER(c);
  if (!p || !sums) return fail(c, ICPGPU_ERR_INVALID_ARG, "null argument");
  if (!c->src.set || !c->tgt.set) return fail(c, ICPGPU_ERR_NO_INPUT, "ndt_gradient: source and target must be set first");
  int rc = ensure_ndt_cells(c);
  if (rc) return rc;
  if ((rc = ensure(c, c->sums, kNdtTerms * sizeof(double)))) return rc;
  float T[16];
  ndt_transform_float(p, T);
  double all[kNdtTerms];
  if ((rc = ndt_evaluate(c, T, p, all, /*mailbox=*/false, /*hessian=*/false))) return rc;
  std::memcpy(sums, all, kNdtGradTerms * sizeof(double));
  return ICPGPU_OK;
}

int icpgpu_ndt_line_search_replay(double phi_0, double d_phi_0, double step_init, double step_max, double step_min, const double* phi,
                                  const double* d_phi, int n, double* step, int* trial) {
  if (!step || !trial || n < 0 || (n > 0 && (!phi || !d_phi))) return ICPGPU_ERR_INVALID_ARG;
  if (!std::isfinite(phi_0) || !(d_phi_0 < 0.0) || !std::isfinite(d_phi_0)) return ICPGPU_ERR_INVALID_ARG;
  mt::Search S;
  mt::start(S, phi_0, d_phi_0, step_init, step_max, step_min);
  int st = ICPGPU_NDT_MT_TRIAL;
  for (int k = 0; k < n; ++k) {
    if (st != ICPGPU_NDT_MT_TRIAL) return ICPGPU_ERR_INVALID_ARG;  // (an observation after the search has ended)
    st = mt::observe(S, phi[k], d_phi[k]);
  }
  *step = S.a_t;
  *trial = st == ICPGPU_NDT_MT_TRIAL ? n : S.final_trial;
  return st;
}

int icpgpu_ndt_line_search_trace(const icpgpu_ctx* c, size_t capacity, int32_t* iteration, double* step, double* phi, double* d_phi,
                                 size_t* n_trials) {
  if (!c || !n_trials) return ICPGPU_ERR_INVALID_ARG;
  const size_t n = c->ndt_trace.size();
  *n_trials = n;
  if (n > capacity) return ICPGPU_OK;  // (the count alone: size the buffers and call again)
  for (size_t i = 0; i < n; ++i) {
    const auto& t = c->ndt_trace[i];
    if (iteration) iteration[i] = t.iteration;
    if (step) step[i] = t.a;
    if (phi) phi[i] = t.phi;
    if (d_phi) d_phi[i] = t.dphi;
  }
  return ICPGPU_OK;
}

}  // extern "C"
