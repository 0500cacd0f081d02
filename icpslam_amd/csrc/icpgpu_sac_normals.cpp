// icpgpu_sac_normals.cpp -- host side of the segmentation from normals (pcl::SACSegmentationFromNormals with SACMODEL_NORMAL_PLANE /
// SACMODEL_CYLINDER and SAC_RANSAC; rules: include/icpgpu.h "segmentation from normals"; kernels: icp_sac_normals.hip).
//
// The sequential RANSAC loop runs HERE over counts the device takes 64 hypotheses at a time, as the plane segmentation's does
// (icpgpu_sac.cpp), and the result lives in the same state (icpgpu_ctx::sac, model != 0): it is "the last segmentation", whichever call
// made it, and icpgpu_sac_extract works on it.  The cylinder's Gauss-Newton runs here too, over 21 sums a device pass hands it.
#include "icp_ctx.h"
#include "icp_sac_normals.h"

namespace icpgpu_impl {
namespace {

using icpgpu::kSacnCylinder;
using icpgpu::kSacnCylTerms;
using icpgpu::kSacnPlane;

// the chart of the cylinder's refinement: e the coordinate with the largest |dir_e| (the lowest index among equals), ia < ib the
// other two; p = (P_ia, P_ib, D_ia, D_ib, r) with P_e = Ke and D_e = 1
struct Chart {
  int e, ia, ib;
  double Ke;
};
void chart_axis(const Chart& ch, const double p[5], double P[3], double D[3]) {
  P[ch.ia] = p[0], P[ch.ib] = p[1], P[ch.e] = ch.Ke;
  D[ch.ia] = p[2], D[ch.ib] = p[3], D[ch.e] = 1.0;
}

// the Gauss-Newton step of the 21 sums: (J^T J) delta = -J^T rho by Cholesky.  false: a pivot that is not > 0.
bool cyl_step(const double S[kSacnCylTerms], double delta[5]) {
  double A[5][5], L[5][5] = {};
  int k = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = i; j < 5; ++j) A[i][j] = A[j][i] = S[k++];
  for (int j = 0; j < 5; ++j) {
    double s = A[j][j];
    for (int q = 0; q < j; ++q) s -= L[j][q] * L[j][q];
    if (!(s > 0.0)) return false;
    L[j][j] = std::sqrt(s);
    for (int i = j + 1; i < 5; ++i) {
      double u = A[i][j];
      for (int q = 0; q < j; ++q) u -= L[i][q] * L[j][q];
      L[i][j] = u / L[j][j];
    }
  }
  double y[5];
  for (int i = 0; i < 5; ++i) {
    double u = -S[15 + i];
    for (int q = 0; q < i; ++q) u -= L[i][q] * y[q];
    y[i] = u / L[i][i];
  }
  for (int i = 4; i >= 0; --i) {
    double u = y[i];
    for (int q = i + 1; q < 5; ++q) u -= L[q][i] * delta[q];
    delta[i] = u / L[i][i];
  }
  return true;
}

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_sac_segmentation_from_normals(icpgpu_ctx* c, int model, const float* normals_nxyzc, double distance_threshold, double normal_distance_weight,
                                         double radius_min, double radius_max, int max_iterations, double probability, uint64_t seed,
                                         int optimize_coefficients, const double* axis3, double eps_angle, float coeff7[7], int32_t* n_coeff,
                                         size_t* n_inliers, int32_t* iterations, int32_t* found) {
  ENTER(c);
  auto& S = c->search;
  auto& K = c->sac;
  K.have = false;
  if (coeff7)
    for (int a = 0; a < 7; ++a) coeff7[a] = 0.f;
  if (n_coeff) *n_coeff = 0;
  if (n_inliers) *n_inliers = 0;
  if (iterations) *iterations = 0;
  if (found) *found = 0;
  const char* who = "sac_segmentation_from_normals";
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: no search cloud (icpgpu_search_set_input)", who);
  if (model != kSacnPlane && model != kSacnCylinder) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: model %d is neither NORMAL_PLANE nor CYLINDER", who, model);
  if (!normals_nxyzc) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: null normals", who);
  if (!std::isfinite(distance_threshold) || distance_threshold < 0.0)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: distance_threshold must be finite and >= 0", who);
  if (!(normal_distance_weight >= 0.0 && normal_distance_weight <= 1.0))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: normal_distance_weight must be inside [0, 1]", who);
  if (!std::isfinite(radius_min) || !std::isfinite(radius_max) || radius_min < 0.0 || radius_max < 0.0 ||
      (radius_max < radius_min && !(radius_min == 0.0 && radius_max == 0.0)))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: radius limits must be finite, >= 0 and ordered (or both 0)", who);
  if (max_iterations < 0 || max_iterations > ICPGPU_SAC_MAX_ITERATIONS)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: max_iterations %d outside 0..%d", who, max_iterations, ICPGPU_SAC_MAX_ITERATIONS);
  if (!(probability > 0.0 && probability < 1.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: probability must be inside (0, 1)", who);
  double axis[3] = {0.0, 0.0, 0.0}, cos_eps = 0.0;
  if (axis3) {
    if (model == kSacnPlane) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: NORMAL_PLANE takes no axis", who);
    if (!std::isfinite(axis3[0]) || !std::isfinite(axis3[1]) || !std::isfinite(axis3[2])) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: the axis must be finite", who);
    const double len = std::sqrt((axis3[0] * axis3[0] + axis3[1] * axis3[1]) + axis3[2] * axis3[2]);
    if (!(len > 0.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: the axis has zero length", who);
    if (!std::isfinite(eps_angle) || eps_angle < 0.0) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: eps_angle must be finite and >= 0", who);
    for (int a = 0; a < 3; ++a) axis[a] = axis3[a] / len;
    cos_eps = std::cos(eps_angle);
  }
  if (!coeff7 || !n_coeff || !n_inliers || !iterations || !found) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: null output pointer", who);

  const size_t n = S.n;
  const int ni = (int)n;
  const float thr = sac_threshold_image(distance_threshold);
  const float weight = (float)normal_distance_weight;
  const int size = model == kSacnPlane ? 3 : 2, nc = model == kSacnPlane ? 4 : 7;
  K.model = model;
  K.n_coeff = nc;
  K.n = n;
  K.thr = thr;
  K.found = 0;
  K.iterations = 0;
  K.best_t = -1;
  K.n_inliers = K.n_unrefined = 0;
  K.waits = 0;
  K.cyl_passes = K.cyl_stop = 0;
  K.counts.clear();
  K.cyl_sums.clear();
  for (int a = 0; a < 3; ++a) K.sample[a] = -1;
  for (int a = 0; a < 4; ++a) K.coeff[a] = K.coeff_unrefined[a] = 0.f;
  for (int a = 0; a < 7; ++a) K.coeff7[a] = K.coeff7_unrefined[a] = 0.f;
  for (int a = 0; a < 9; ++a) K.moments[a] = 0.0;

  int rc;
  int best_count = 0;
  float best_K[3] = {0.f, 0.f, 0.f};  // the best sample's first point (a cylinder's record carries it)
  if (n > 0 && max_iterations > 0) {
    if ((rc = ensure(c, K.nbatch, sizeof(SacnBatch)))) return rc;
    if ((rc = ensure(c, K.normals, n * sizeof(float4)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(K.normals.ptr, normals_nxyzc, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    SacnBatch* d_batch = K.nbatch.as<SacnBatch>();
    SacnBatch hb;
    double k = INFINITY;
    int t = 0;
    for (;; ++t) {
      if (t >= max_iterations || (double)t >= k) break;
      const int h = t % kSacBatch;
      if (h == 0) {  // the loop goes on into the next batch: take it
        HIP_TRY(c, launch_sacn_batch(S.cloud.data(), K.normals.as<const float4>(), ni, model, (unsigned long long)seed, t, max_iterations,
                                     axis3 != nullptr, axis, cos_eps, radius_min, radius_max, thr, weight, d_batch, c->stream));
        if ((rc = copy_to_host(c, &hb, d_batch, sizeof hb))) return rc;
        ++K.waits;
      }
      const int cnt = hb.count[h];
      if (cnt < -1 || cnt > ni) return fail(c, ICPGPU_ERR_HIP, "%s: hypothesis %d counts %d of %d points (internal error)", who, t, cnt, ni);
      K.counts.push_back(cnt);
      if (cnt > 0 && cnt > best_count) {
        best_count = cnt;
        K.best_t = t;
        for (int a = 0; a < 3; ++a) K.sample[a] = a < size ? hb.sample[h][a] : -1;
        for (int a = 0; a < nc; ++a) K.coeff7_unrefined[a] = hb.rec[h][a];
        for (int a = 0; a < 3; ++a) best_K[a] = hb.rec[h][12 + a];
        const double w = (double)cnt / (double)n;
        double p = 1.0 - (size == 3 ? w * w * w : w * w);
        p = std::max(p, DBL_EPSILON);
        p = std::min(p, 1.0 - DBL_EPSILON);
        k = std::log(1.0 - probability) / std::log(p);
      }
    }
    K.iterations = t;
  }

  if (K.best_t >= 0) {
    if (K.sample[0] < 0 || K.sample[0] >= ni) return fail(c, ICPGPU_ERR_HIP, "%s: sample %d of %d points (internal error)", who, K.sample[0], ni);
    if ((rc = ensure_compaction(c, K.sel, n))) return rc;
    if ((rc = ensure(c, K.ints, 4 * sizeof(int)))) return rc;
    if ((rc = ensure(c, K.sums, kSacnCylTerms * sizeof(double)))) return rc;
    const Compaction& C = K.sel;
    const float4* normals = K.normals.as<const float4>();
    auto select = [&](const float* co) {
      return launch_sacn_select(S.cloud.data(), normals, ni, model, co, thr, weight, C.flags.as<int>(), C.pos.as<int>(), C.scan.as<int>(),
                                C.kept.as<int>(), K.ints.as<int>(), c->stream);
    };
    K.found = 1;
    K.n_unrefined = (size_t)best_count;  // (the selection below is the counting kernel's own test: the same number)
    for (int a = 0; a < 7; ++a) K.coeff7[a] = K.coeff7_unrefined[a];
    HIP_TRY(c, select(K.coeff7_unrefined));
    int m = best_count;
    bool reselect = false;
    if (optimize_coefficients && model == kSacnPlane && best_count >= 3) {
      double sums[12];
      HIP_TRY(c, launch_sac_sums(S.cloud.data(), ni, C.kept.as<int>(), best_count, K.sample[0], K.sums.as<double>(), c->stream));
      if ((rc = copy_to_host(c, sums, K.sums.ptr, sizeof sums))) return rc;
      ++K.waits;
      for (int a = 0; a < 9; ++a) K.moments[a] = sums[a];
      sac_refine_plane(sums, sums + 9, best_count, K.coeff7_unrefined, K.coeff7);
      reselect = true;
    } else if (optimize_coefficients && model == kSacnCylinder && best_count >= 5) {
      const float* u = K.coeff7_unrefined;
      Chart ch;
      ch.e = 0;
      if (std::fabs(u[4]) > std::fabs(u[3 + ch.e])) ch.e = 1;
      if (std::fabs(u[5]) > std::fabs(u[3 + ch.e])) ch.e = 2;
      ch.ia = ch.e == 0 ? 1 : 0;
      ch.ib = ch.e == 2 ? 1 : 2;
      ch.Ke = (double)best_K[ch.e];
      const double de = (double)u[3 + ch.e], s = ch.Ke - (double)u[ch.e];
      double p[5], P[3], D[3];
      p[2] = (double)u[3 + ch.ia] / de, p[3] = (double)u[3 + ch.ib] / de;
      p[0] = (double)u[ch.ia] + (s / de) * (double)u[3 + ch.ia], p[1] = (double)u[ch.ib] + (s / de) * (double)u[3 + ch.ib];
      p[4] = (double)u[6];
      auto pass = [&](const double q[5], double out[kSacnCylTerms]) -> int {
        chart_axis(ch, q, P, D);
        hipError_t e = launch_sacn_cyl_sums(S.cloud.data(), ni, C.kept.as<int>(), best_count, P, D, ch.ia, ch.ib, q[4], K.sums.as<double>(), c->stream);
        if (e != hipSuccess) return fail(c, ICPGPU_ERR_HIP, "%s: the refinement's pass failed: %s", who, hipGetErrorString(e));
        const int r = copy_to_host(c, out, K.sums.ptr, kSacnCylTerms * sizeof(double));
        if (r) return r;
        ++K.waits;
        ++K.cyl_passes;
        K.cyl_sums.insert(K.cyl_sums.end(), out, out + kSacnCylTerms);
        return 0;
      };
      double cur[kSacnCylTerms], next[kSacnCylTerms];
      if ((rc = pass(p, cur))) return rc;
      for (;;) {
        if (K.cyl_passes >= ICPGPU_SAC_CYLINDER_ITERATIONS) { K.cyl_stop = ICPGPU_SAC_STOP_PASSES; break; }
        double delta[5], trial[5];
        if (!cyl_step(cur, delta)) { K.cyl_stop = ICPGPU_SAC_STOP_CHOLESKY; break; }
        double big = 0.0, scale = 0.0;
        bool finite = true;
        for (int a = 0; a < 5; ++a) {
          trial[a] = p[a] + delta[a];
          finite = finite && std::isfinite(trial[a]);
          big = std::max(big, std::fabs(delta[a]));
          scale = std::max(scale, std::fabs(p[a]));
        }
        if (!finite) { K.cyl_stop = ICPGPU_SAC_STOP_NOT_FINITE; break; }
        if (big <= 1e-12 * (1.0 + scale)) { K.cyl_stop = ICPGPU_SAC_STOP_SMALL_STEP; break; }
        if ((rc = pass(trial, next))) return rc;
        if (!(next[20] < cur[20])) { K.cyl_stop = ICPGPU_SAC_STOP_NO_DECREASE; break; }
        for (int a = 0; a < 5; ++a) p[a] = trial[a];
        for (int a = 0; a < kSacnCylTerms; ++a) cur[a] = next[a];
      }
      chart_axis(ch, p, P, D);
      const double len = std::sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
      const double sign = u[3 + ch.e] < 0.f ? -1.0 : 1.0;
      for (int a = 0; a < 3; ++a) K.coeff7[a] = (float)P[a], K.coeff7[3 + a] = (float)(sign * (D[a] / len));
      K.coeff7[6] = (float)std::fabs(p[4]);
      reselect = true;
    }
    if (reselect) {
      HIP_TRY(c, select(K.coeff7));
      if ((rc = fetch_ints(c, K.ints.as<int>(), 1, &m))) return rc;
      ++K.waits;
      if (m < 0 || m > ni) return fail(c, ICPGPU_ERR_HIP, "%s: %d inliers of %d points (internal error)", who, m, ni);
    }
    K.n_inliers = (size_t)m;
  }
  K.have = true;
  for (int a = 0; a < 7; ++a) coeff7[a] = K.coeff7[a];
  *n_coeff = K.found ? nc : 0;
  *n_inliers = K.n_inliers;
  *iterations = K.iterations;
  *found = K.found;
  return ICPGPU_OK;
}

int icpgpu_sac_normals_fetch(icpgpu_ctx* c, size_t capacity_inliers, size_t capacity_counts, int32_t* inliers, int32_t* counts, int32_t best_sample3[3],
                             int32_t* best_t, float coeff_unrefined7[7], size_t* n_unrefined_inliers, double moments9[9],
                             double* cylinder_sums, int32_t* cylinder_passes, int32_t* cylinder_stop) {
  ENTER(c);
  const auto& K = c->sac;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_normals_fetch: no result (icpgpu_sac_segmentation_from_normals)");
  if (K.model == 0) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_normals_fetch: the last segmentation is a plane segmentation (icpgpu_sac_fetch)");
  if ((inliers && K.n_inliers > capacity_inliers) || (counts && K.counts.size() > capacity_counts))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_normals_fetch: %zu inliers and %zu counts, room for %zu and %zu", K.n_inliers, K.counts.size(),
                capacity_inliers, capacity_counts);
  if (inliers && K.n_inliers) {
    const int rc = copy_to_host(c, inliers, K.sel.kept.ptr, K.n_inliers * sizeof(int32_t));
    if (rc) return rc;
  }
  if (counts && !K.counts.empty()) std::memcpy(counts, K.counts.data(), K.counts.size() * sizeof(int32_t));
  if (best_sample3)
    for (int a = 0; a < 3; ++a) best_sample3[a] = K.sample[a];
  if (best_t) *best_t = K.best_t;
  if (coeff_unrefined7)
    for (int a = 0; a < 7; ++a) coeff_unrefined7[a] = K.coeff7_unrefined[a];
  if (n_unrefined_inliers) *n_unrefined_inliers = K.n_unrefined;
  if (moments9)
    for (int a = 0; a < 9; ++a) moments9[a] = K.moments[a];
  if (cylinder_sums) {
    for (int a = 0; a < kSacnCylTerms * ICPGPU_SAC_CYLINDER_ITERATIONS; ++a) cylinder_sums[a] = 0.0;
    if (!K.cyl_sums.empty()) std::memcpy(cylinder_sums, K.cyl_sums.data(), K.cyl_sums.size() * sizeof(double));
  }
  if (cylinder_passes) *cylinder_passes = K.cyl_passes;
  if (cylinder_stop) *cylinder_stop = K.cyl_stop;
  return ICPGPU_OK;
}

int icpgpu_sac_normals_stats(const icpgpu_ctx* c, int32_t* host_waits) {
  if (!c || !c->sac.have || c->sac.model == 0) return ICPGPU_ERR_INVALID_ARG;
  if (host_waits) *host_waits = c->sac.waits;
  return ICPGPU_OK;
}

}  // extern "C"
