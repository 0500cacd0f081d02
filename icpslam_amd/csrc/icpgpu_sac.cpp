// icpgpu_sac.cpp -- host side of the plane segmentation (pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE and
// SAC_RANSAC, pcl::ExtractIndices over its result; rules: include/icpgpu.h "plane segmentation"; kernels: icp_sac.hip).
//
// The sequential RANSAC loop runs HERE, over counts the device takes 64 hypotheses at a time: one wait per batch, and a batch is
// launched only when the loop has not stopped before its first hypothesis.  Everything the call writes on the device is the
// segmentation state's own (icpgpu_ctx::sac), so no other call's result meets it.
#include "icp_ctx.h"
#include "icp_jacobi3.h"

namespace icpgpu_impl {

// (both shared with the segmentation from normals, icpgpu_sac_normals.cpp: declared in icp_ctx.h)
// the smallest float32 that is not below t (t >= 0, finite): for every float32 f, f < it <=> (double)f < t
float sac_threshold_image(double t) {
  float f = (float)t;
  if ((double)f < t) f = std::nextafterf(f, INFINITY);
  return f;
}

// the refinement's host half: the nine sums about K over m inliers -> the refined coefficients (rule: include/icpgpu.h)
void sac_refine_plane(const double S[9], const double K[3], int m, const float unrefined[4], float out[4]) {
  const double dm = (double)m;
  const double mx = S[6] / dm, my = S[7] / dm, mz = S[8] / dm;
  double a[3][3], V[3][3];
  a[0][0] = S[0] / dm - mx * mx;
  a[0][1] = a[1][0] = S[1] / dm - mx * my;
  a[0][2] = a[2][0] = S[2] / dm - mx * mz;
  a[1][1] = S[3] / dm - my * my;
  a[1][2] = a[2][1] = S[4] / dm - my * mz;
  a[2][2] = S[5] / dm - mz * mz;
  jacobi3(a, V);
  int col = 0;  // the smallest diagonal entry, the lowest index among equals
  if (a[1][1] < a[col][col]) col = 1;
  if (a[2][2] < a[col][col]) col = 2;
  float nx = (float)V[0][col], ny = (float)V[1][col], nz = (float)V[2][col];
  const float cs = (nx * unrefined[0] + ny * unrefined[1]) + nz * unrefined[2];
  if (cs < 0.f) nx = -nx, ny = -ny, nz = -nz;
  const double cx = K[0] + mx, cy = K[1] + my, cz = K[2] + mz;
  out[0] = nx, out[1] = ny, out[2] = nz;
  out[3] = (float)-(((double)nx * cx + (double)ny * cy) + (double)nz * cz);
}

}  // namespace icpgpu_impl

extern "C" {

int icpgpu_sac_plane_segmentation(icpgpu_ctx* c, double distance_threshold, int max_iterations, double probability, uint64_t seed,
                                  int optimize_coefficients, const double* axis3, double eps_angle, float coeff4[4], size_t* n_inliers,
                                  int32_t* iterations, int32_t* found) {
  ENTER(c);
  auto& S = c->search;
  auto& K = c->sac;
  K.have = false;
  K.model = 0;  // (a plane result: icpgpu_sac_normals.cpp sets its own)
  if (coeff4) coeff4[0] = coeff4[1] = coeff4[2] = coeff4[3] = 0.f;
  if (n_inliers) *n_inliers = 0;
  if (iterations) *iterations = 0;
  if (found) *found = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: no search cloud (icpgpu_search_set_input)");
  if (!std::isfinite(distance_threshold) || distance_threshold < 0.0)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: distance_threshold must be finite and >= 0");
  if (max_iterations < 0 || max_iterations > ICPGPU_SAC_MAX_ITERATIONS)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: max_iterations %d outside 0..%d", max_iterations, ICPGPU_SAC_MAX_ITERATIONS);
  if (!(probability > 0.0 && probability < 1.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: probability must be inside (0, 1)");
  double axis[3] = {0.0, 0.0, 0.0}, cos_eps = 0.0;
  if (axis3) {
    if (!std::isfinite(axis3[0]) || !std::isfinite(axis3[1]) || !std::isfinite(axis3[2]))
      return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: the axis must be finite");
    const double len = std::sqrt((axis3[0] * axis3[0] + axis3[1] * axis3[1]) + axis3[2] * axis3[2]);
    if (!(len > 0.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: the axis has zero length");
    if (!std::isfinite(eps_angle) || eps_angle < 0.0) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: eps_angle must be finite and >= 0");
    for (int a = 0; a < 3; ++a) axis[a] = axis3[a] / len;
    cos_eps = std::cos(eps_angle);
  }
  if (!coeff4 || !n_inliers || !iterations || !found) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_plane_segmentation: null output pointer");

  const size_t n = S.n;
  const int ni = (int)n;
  const float thr = sac_threshold_image(distance_threshold);
  K.n = n;
  K.thr = thr;
  K.found = 0;
  K.iterations = 0;
  K.best_t = -1;
  K.n_inliers = K.n_unrefined = 0;
  K.waits = 0;
  K.counts.clear();
  for (int a = 0; a < 3; ++a) K.sample[a] = -1;
  for (int a = 0; a < 4; ++a) K.coeff[a] = K.coeff_unrefined[a] = 0.f;
  for (int a = 0; a < 9; ++a) K.moments[a] = 0.0;

  int rc;
  int best_count = 0;
  if (n > 0 && max_iterations > 0) {
    if ((rc = ensure(c, K.batch, sizeof(SacBatch)))) return rc;
    SacBatch* d_batch = K.batch.as<SacBatch>();
    SacBatch hb;
    double k = INFINITY;
    int t = 0;
    for (;; ++t) {
      if (t >= max_iterations || (double)t >= k) break;
      const int h = t % kSacBatch;
      if (h == 0) {  // the loop goes on into the next batch: take it
        HIP_TRY(c, launch_sac_batch(S.cloud.data(), ni, (unsigned long long)seed, t, max_iterations, axis3 != nullptr, axis, cos_eps, thr, d_batch,
                                    c->stream));
        if ((rc = copy_to_host(c, &hb, d_batch, sizeof hb))) return rc;
        ++K.waits;
      }
      const int cnt = hb.count[h];
      if (cnt < -1 || cnt > ni) return fail(c, ICPGPU_ERR_HIP, "sac_plane_segmentation: hypothesis %d counts %d of %d points (internal error)", t, cnt, ni);
      K.counts.push_back(cnt);
      if (cnt > 0 && cnt > best_count) {
        best_count = cnt;
        K.best_t = t;
        for (int a = 0; a < 3; ++a) K.sample[a] = hb.sample[h][a];
        K.coeff_unrefined[0] = hb.plane[h].x, K.coeff_unrefined[1] = hb.plane[h].y, K.coeff_unrefined[2] = hb.plane[h].z,
        K.coeff_unrefined[3] = hb.plane[h].w;
        const double w = (double)cnt / (double)n;
        double p = 1.0 - w * w * w;
        p = std::max(p, DBL_EPSILON);
        p = std::min(p, 1.0 - DBL_EPSILON);
        k = std::log(1.0 - probability) / std::log(p);
      }
    }
    K.iterations = t;
  }

  if (K.best_t >= 0) {
    if (K.sample[0] < 0 || K.sample[0] >= ni) return fail(c, ICPGPU_ERR_HIP, "sac_plane_segmentation: sample %d of %d points (internal error)", K.sample[0], ni);
    if ((rc = ensure_compaction(c, K.sel, n))) return rc;
    if ((rc = ensure(c, K.ints, 4 * sizeof(int)))) return rc;
    if ((rc = ensure(c, K.sums, 12 * sizeof(double)))) return rc;
    const Compaction& C = K.sel;
    K.found = 1;
    K.n_unrefined = (size_t)best_count;  // (the selection below is the counting kernel's own test: the same number)
    for (int a = 0; a < 4; ++a) K.coeff[a] = K.coeff_unrefined[a];
    HIP_TRY(c, launch_sac_select(S.cloud.data(), ni, K.coeff_unrefined, thr, C.flags.as<int>(), C.pos.as<int>(), C.scan.as<int>(), C.kept.as<int>(),
                                 K.ints.as<int>(), c->stream));
    int m = best_count;
    if (optimize_coefficients && best_count >= 3) {
      double sums[12];
      HIP_TRY(c, launch_sac_sums(S.cloud.data(), ni, C.kept.as<int>(), best_count, K.sample[0], K.sums.as<double>(), c->stream));
      if ((rc = copy_to_host(c, sums, K.sums.ptr, sizeof sums))) return rc;
      ++K.waits;
      for (int a = 0; a < 9; ++a) K.moments[a] = sums[a];
      sac_refine_plane(sums, sums + 9, best_count, K.coeff_unrefined, K.coeff);
      HIP_TRY(c, launch_sac_select(S.cloud.data(), ni, K.coeff, thr, C.flags.as<int>(), C.pos.as<int>(), C.scan.as<int>(), C.kept.as<int>(),
                                   K.ints.as<int>(), c->stream));
      if ((rc = fetch_ints(c, K.ints.as<int>(), 1, &m))) return rc;
      ++K.waits;
      if (m < 0 || m > ni) return fail(c, ICPGPU_ERR_HIP, "sac_plane_segmentation: %d inliers of %d points (internal error)", m, ni);
    }
    K.n_inliers = (size_t)m;
  }
  K.have = true;
  for (int a = 0; a < 4; ++a) coeff4[a] = K.coeff[a];
  *n_inliers = K.n_inliers;
  *iterations = K.iterations;
  *found = K.found;
  return ICPGPU_OK;
}

int icpgpu_sac_fetch(icpgpu_ctx* c, size_t capacity_inliers, size_t capacity_counts, int32_t* inliers, int32_t* counts, int32_t best_sample3[3],
                     int32_t* best_t, float coeff_unrefined4[4], double moments9[9], size_t* n_unrefined_inliers) {
  ENTER(c);
  const auto& K = c->sac;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_fetch: no result (icpgpu_sac_plane_segmentation)");
  if (K.model != 0) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_fetch: the last segmentation is from normals (icpgpu_sac_normals_fetch)");
  if ((inliers && K.n_inliers > capacity_inliers) || (counts && K.counts.size() > capacity_counts))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_fetch: %zu inliers and %zu counts, room for %zu and %zu", K.n_inliers, K.counts.size(), capacity_inliers,
                capacity_counts);
  if (inliers && K.n_inliers) {
    const int rc = copy_to_host(c, inliers, K.sel.kept.ptr, K.n_inliers * sizeof(int32_t));
    if (rc) return rc;
  }
  if (counts && !K.counts.empty()) std::memcpy(counts, K.counts.data(), K.counts.size() * sizeof(int32_t));
  if (best_sample3)
    for (int a = 0; a < 3; ++a) best_sample3[a] = K.sample[a];
  if (best_t) *best_t = K.best_t;
  if (coeff_unrefined4)
    for (int a = 0; a < 4; ++a) coeff_unrefined4[a] = K.coeff_unrefined[a];
  if (moments9)
    for (int a = 0; a < 9; ++a) moments9[a] = K.moments[a];
  if (n_unrefined_inliers) *n_unrefined_inliers = K.n_unrefined;
  return ICPGPU_OK;
}

int icpgpu_sac_stats(const icpgpu_ctx* c, int32_t* host_waits) {
  if (!c || !c->sac.have) return ICPGPU_ERR_INVALID_ARG;
  if (host_waits) *host_waits = c->sac.waits;
  return ICPGPU_OK;
}

}  // extern "C"

namespace icpgpu_impl {
namespace {

// pcl::ExtractIndices over the last segmentation: the cloud's points in (negative = 0) or not in (1) the inliers, in cloud order, written
// by the compaction's last kernel into the pinned staging buffer.  One wait: the count.
int sac_extract(icpgpu_ctx* c, int negative, float* out_xyzw, const float** view_xyzw, bool view, size_t* n_out) {
  auto& S = c->search;
  auto& K = c->sac;
  if (view && view_xyzw) *view_xyzw = nullptr;
  if (n_out) *n_out = 0;
  if (!n_out || (view && !view_xyzw)) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_extract: null argument");
  if (!K.have || !S.set || K.n != S.n) return fail(c, ICPGPU_ERR_INVALID_ARG, "sac_extract: no result (icpgpu_sac_plane_segmentation)");
  const size_t n = K.n, want = negative ? n - K.n_inliers : K.n_inliers;
  if (want == 0) return ICPGPU_OK;
  const int ni = (int)n;
  int rc;
  Compaction& C = K.ext;
  if ((rc = ensure_compaction(c, C, n))) return rc;
  if ((rc = ensure(c, K.ints, 4 * sizeof(int)))) return rc;
  if ((rc = ensure_stage(c, want * sizeof(float4), /*any_size=*/true))) return rc;
  int* d_count = K.ints.as<int>() + 1;
  if (K.model != 0)  // (a result from normals: its kept inlier list says which points)
    HIP_TRY(c, launch_sacn_list_flags(K.sel.kept.as<int>(), (int)K.n_inliers, ni, negative != 0, C.flags.as<int>(), c->stream));
  else
    HIP_TRY(c, launch_sac_flags(S.cloud.data(), ni, K.coeff, K.thr, K.found != 0, negative != 0, C.flags.as<int>(), c->stream));
  HIP_TRY(c, launch_compact(C.flags.as<int>(), ni, C.pos.as<int>(), C.scan.as<int>(), C.kept.as<int>(), d_count, S.cloud.data(),
                            static_cast<float4*>(c->h_stage_dev), c->stream));
  int m = 0;
  if ((rc = fetch_ints(c, d_count, 1, &m))) return rc;
  if ((size_t)m != want) return fail(c, ICPGPU_ERR_HIP, "sac_extract: %d points extracted, %zu expected (internal error)", m, want);
  if (view) *view_xyzw = static_cast<const float*>(c->h_stage);
  else if (out_xyzw) std::memcpy(out_xyzw, c->h_stage, want * sizeof(float4));
  *n_out = want;
  return ICPGPU_OK;
}

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_sac_extract(icpgpu_ctx* c, int negative, float* out_xyzw, size_t* n_out) {
  ENTER(c);
  return sac_extract(c, negative, out_xyzw, nullptr, false, n_out);
}

int icpgpu_sac_extract_view(icpgpu_ctx* c, int negative, const float** view_xyzw, size_t* n_out) {
  ENTER(c);
  return sac_extract(c, negative, nullptr, view_xyzw, true, n_out);
}

}  // extern "C"
