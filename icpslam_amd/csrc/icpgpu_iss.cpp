// icpgpu_iss.cpp -- host side of the intrinsic shape signature keypoints (pcl::ISSKeypoint3D without border estimation; rules:
// include/icpgpu.h "ISS keypoints"; kernels: icp_iss.hip).  The call works on the search cloud and its grid (icpgpu_search.cpp) and
// writes nothing but the ISS state's own buffers: the search state's scratch, and so a later search, normal estimation, FPFH,
// clustering or segmentation, never meets it.  One wait: the count.
#include "icp_ctx.h"

namespace icpgpu_impl {
namespace {

// the cube of `shells` cells around a point's cell contains its ball (shells * h * kGridSafety >= radius: the grid search's bound);
// a ball of more than kSearchRadiusShells cells, and every ball of a cloud without a grid, is searched by a sweep (-1): the rule of
// icpgpu_search_radius
int shells_of(const icpgpu_ctx* c, double radius) {
  const auto& S = c->search;
  if (!(S.n && S.grid.usable)) return -1;
  const double s = std::ceil(radius / ((double)S.grid.g.h * (double)kGridSafety));
  return s <= (double)kSearchRadiusShells ? (int)s : -1;
}

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_iss_keypoints(icpgpu_ctx* c, double salient_radius, double non_max_radius, double gamma_21, double gamma_32, int min_neighbors,
                         size_t* n_keypoints) {
  ENTER(c);
  auto& S = c->search;
  auto& K = c->iss;
  K.have = false;
  K.waits = 0;
  if (n_keypoints) *n_keypoints = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: no search cloud (icpgpu_search_set_input)");
  if (!(std::isfinite(salient_radius) && salient_radius > 0.0) || !(std::isfinite(non_max_radius) && non_max_radius > 0.0))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: both radii must be finite and > 0 (salient %g, non-max %g)", salient_radius, non_max_radius);
  if (!std::isfinite(gamma_21) || !std::isfinite(gamma_32)) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: the gammas must be finite");
  if (min_neighbors < 0) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: min_neighbors %d < 0", min_neighbors);
  if (!n_keypoints) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: null n_keypoints");
  const size_t n = S.n, m = std::max<size_t>(n, 1);
  int rc;
  if ((rc = ensure(c, K.n_salient, m * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, K.scatter, m * 6 * sizeof(double)))) return rc;
  if ((rc = ensure(c, K.eig, m * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(c, K.saliency, m * sizeof(double)))) return rc;
  for (DeviceBuf* b : {&K.flags, &K.pos, &K.kept})
    if ((rc = ensure(c, *b, m * sizeof(int)))) return rc;
  if ((rc = ensure(c, K.scan, exclusive_scan_scratch_ints((int)m) * sizeof(int)))) return rc;
  if ((rc = ensure(c, K.points, m * sizeof(float4)))) return rc;
  if ((rc = ensure(c, K.ints, 4 * sizeof(int)))) return rc;
  const bool grid = n && S.grid.usable;
  const float4* sorted = grid ? static_cast<const float4*>(S.grid.sorted.ptr) : nullptr;
  const int* cell_start = grid ? static_cast<const int*>(S.grid.cell_start.ptr) : nullptr;
  const GridDesc g = grid ? S.grid.g : GridDesc{};
  const float r2_salient = (float)(salient_radius * salient_radius), r2_non_max = (float)(non_max_radius * non_max_radius);
  int* d_count = static_cast<int*>(K.ints.ptr);
  HIP_TRY(c, launch_iss_keypoints(S.cloud.data(), (int)n, S.n_finite > 0, sorted, cell_start, g, shells_of(c, salient_radius), r2_salient,
                                  shells_of(c, non_max_radius), r2_non_max, min_neighbors, gamma_21, gamma_32,
                                  static_cast<int32_t*>(K.n_salient.ptr), static_cast<double*>(K.scatter.ptr), static_cast<double*>(K.eig.ptr),
                                  static_cast<double*>(K.saliency.ptr), static_cast<int*>(K.flags.ptr), static_cast<int*>(K.pos.ptr),
                                  static_cast<int*>(K.scan.ptr), static_cast<float4*>(K.points.ptr), static_cast<int*>(K.kept.ptr), d_count,
                                  c->stream));
  int count = 0;
  if ((rc = fetch_ints(c, d_count, 1, &count))) return rc;
  K.waits = 1;
  if (count < 0 || (size_t)count > n) return fail(c, ICPGPU_ERR_HIP, "iss_keypoints: %d keypoints of %zu points (internal error)", count, n);
  K.n = n;
  K.n_keypoints = (size_t)count;
  K.have = true;
  *n_keypoints = K.n_keypoints;
  return ICPGPU_OK;
}

int icpgpu_iss_fetch(icpgpu_ctx* c, size_t capacity_keypoints, int32_t* keypoint_index, float* keypoints_xyzw, int32_t* n_salient, double* scatter6,
                     double* eigenvalues3, double* saliency) {
  ENTER(c);
  const auto& K = c->iss;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_fetch: no result (icpgpu_iss_keypoints)");
  if ((keypoint_index || keypoints_xyzw) && K.n_keypoints > capacity_keypoints)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_fetch: %zu keypoints, room for %zu", K.n_keypoints, capacity_keypoints);
  const Delivery first[3] = {{keypoint_index, K.kept.ptr, keypoint_index ? K.n_keypoints * sizeof(int32_t) : 0},
                             {keypoints_xyzw, K.points.ptr, keypoints_xyzw ? K.n_keypoints * sizeof(float4) : 0},
                             {n_salient, K.n_salient.ptr, n_salient ? K.n * sizeof(int32_t) : 0}};
  int rc;
  if ((rc = deliver(c, first, 3))) return rc;
  const Delivery second[3] = {{scatter6, K.scatter.ptr, scatter6 ? K.n * 6 * sizeof(double) : 0},
                              {eigenvalues3, K.eig.ptr, eigenvalues3 ? K.n * 3 * sizeof(double) : 0},
                              {saliency, K.saliency.ptr, saliency ? K.n * sizeof(double) : 0}};
  return deliver(c, second, 3);
}

int icpgpu_iss_stats(const icpgpu_ctx* c, int32_t* host_waits) {
  if (!c || !c->iss.have) return ICPGPU_ERR_INVALID_ARG;
  if (host_waits) *host_waits = c->iss.waits;
  return ICPGPU_OK;
}

}  // extern "C"
