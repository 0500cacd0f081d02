// icpgpu_iss.cpp -- host side of the intrinsic shape signature keypoints (pcl::ISSKeypoint3D; rules: include/icpgpu.h "ISS
// keypoints"; kernels: icp_iss.hip, icp_boundary.hip).  The calls work on the search cloud and its grid (icpgpu_search.cpp).  Without
// border estimation a call writes nothing but the ISS state's own buffers and waits once, for the count.  With it
// (icpgpu_iss_keypoints_border, border_radius > 0) the border radius's rows -- and the normal radius's, when the normals are computed
// -- go through the search calls' scratch, as a radius search's do, at one more wait each; the normals, the edge and border flags and
// everything else the result consists of stay in the ISS state's own buffers.
#include "icp_ctx.h"

namespace icpgpu_impl {
namespace {

// both compute calls; border_radius == 0: no border estimation (normals, normal_radius and angle_threshold are not looked at)
int iss_compute(icpgpu_ctx* c, double salient_radius, double non_max_radius, double gamma_21, double gamma_32, int min_neighbors,
                double border_radius, double angle_threshold, const float* normals_nxyzc, double normal_radius, size_t* n_keypoints) {
  auto& S = c->search;
  auto& K = c->iss;
  K.have = false;
  K.with_border = false;
  K.waits = 0;
  if (n_keypoints) *n_keypoints = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: no search cloud (icpgpu_search_set_input)");
  if (!(std::isfinite(border_radius) && border_radius >= 0.0))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: border_radius must be finite and >= 0 (%g)", border_radius);
  const bool with_border = border_radius > 0.0;
  if (with_border) {
    if (!(std::isfinite(angle_threshold) && angle_threshold > 0.0 && angle_threshold <= M_PI))
      return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: angle_threshold %g outside (0, pi]", angle_threshold);
    if (!normals_nxyzc && !(std::isfinite(normal_radius) && normal_radius > 0.0))
      return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_keypoints: border estimation needs normals or a finite normal_radius > 0 (%g)", normal_radius);
  }
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
  if ((rc = ensure_compaction(c, K.comp, m))) return rc;
  if ((rc = ensure(c, K.points, m * sizeof(float4)))) return rc;
  if ((rc = ensure(c, K.ints, 4 * sizeof(int)))) return rc;
  const SearchView v = view_of(c);
  const float r2_salient = (float)(salient_radius * salient_radius), r2_non_max = (float)(non_max_radius * non_max_radius);
  int waits = 1;
  const int32_t* d_border = nullptr;
  if (with_border) {
    if ((rc = ensure(c, K.normals, m * sizeof(float4)))) return rc;
    if ((rc = ensure(c, K.edge, m * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, K.border, m * sizeof(int32_t)))) return rc;
    HIP_TRY(c, hipMemsetAsync(K.edge.ptr, 0, m * sizeof(int32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(K.border.ptr, 0, m * sizeof(int32_t), c->stream));
    if (n) {
      float4* d_normals = K.normals.as<float4>();
      const float origin[3] = {0.f, 0.f, 0.f};
      NeighbourRows rows;
      if (normals_nxyzc) {
        HIP_TRY(c, hipMemcpyAsync(d_normals, normals_nxyzc, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
      } else {  // icpgpu_normal_estimation(NULL, n, 0, normal_radius, NULL)'s normals, kept on the device
        if ((rc = neighbour_rows(c, "iss_keypoints", v.cloud, n, 0, normal_radius, rows))) return rc;
        ++waits;
        HIP_TRY(c, launch_normals_from_rows(v.cloud, v.n, v.cloud, v.n, rows.idx, rows.n_found, rows.k, rows.row_start, origin, d_normals, nullptr, c->stream));
      }
      if ((rc = neighbour_rows(c, "iss_keypoints", v.cloud, n, 0, border_radius, rows))) return rc;
      ++waits;
      HIP_TRY(c, launch_boundary_from_rows(v.cloud, v.n, d_normals, v.cloud, v.n, rows.idx, rows.n_found, rows.k, rows.row_start, min_neighbors,
                                           std::cos(angle_threshold), nullptr, K.edge.as<int32_t>(), nullptr, nullptr, c->stream));
      HIP_TRY(c, launch_iss_border(v.cloud, v.n, v.sorted, v.cell_start, v.g, v.shells(border_radius), (float)(border_radius * border_radius),
                                   K.edge.as<const int32_t>(), K.border.as<int32_t>(), c->stream));
    }
    d_border = K.border.as<const int32_t>();
  }
  HIP_TRY(c, launch_iss_keypoints(v.cloud, v.n, v.n_eval > 0, v.sorted, v.cell_start, v.g, v.shells(salient_radius), r2_salient,
                                  v.shells(non_max_radius), r2_non_max, min_neighbors, gamma_21, gamma_32, d_border, K.n_salient.as<int32_t>(),
                                  K.scatter.as<double>(), K.eig.as<double>(), K.saliency.as<double>(), K.comp.flags.as<int>(), K.comp.pos.as<int>(),
                                  K.comp.scan.as<int>(), K.points.as<float4>(), K.comp.kept.as<int>(), K.ints.as<int>(), c->stream));
  int count = 0;
  if ((rc = fetch_ints(c, K.ints.as<int>(), 1, &count))) return rc;
  K.waits = waits;
  if (count < 0 || (size_t)count > n) return fail(c, ICPGPU_ERR_HIP, "iss_keypoints: %d keypoints of %zu points (internal error)", count, n);
  K.n = n;
  K.n_keypoints = (size_t)count;
  K.with_border = with_border;
  K.have = true;
  *n_keypoints = K.n_keypoints;
  return ICPGPU_OK;
}

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_iss_keypoints(icpgpu_ctx* c, double salient_radius, double non_max_radius, double gamma_21, double gamma_32, int min_neighbors,
                         size_t* n_keypoints) {
  ENTER(c);
  return iss_compute(c, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, 0.0, 0.0, nullptr, 0.0, n_keypoints);
}

int icpgpu_iss_keypoints_border(icpgpu_ctx* c, double salient_radius, double non_max_radius, double gamma_21, double gamma_32, int min_neighbors,
                                double border_radius, double angle_threshold, const float* normals_nxyzc, double normal_radius,
                                size_t* n_keypoints) {
  ENTER(c);
  return iss_compute(c, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, border_radius, angle_threshold, normals_nxyzc,
                     normal_radius, n_keypoints);
}

// zeros after a call without border estimation
int icpgpu_iss_fetch_border(icpgpu_ctx* c, int32_t* edge, int32_t* border) {
  ENTER(c);
  const auto& K = c->iss;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_fetch_border: no result (icpgpu_iss_keypoints, icpgpu_iss_keypoints_border)");
  if (!K.with_border) {
    if (edge) std::memset(edge, 0, K.n * sizeof(int32_t));
    if (border) std::memset(border, 0, K.n * sizeof(int32_t));
    return ICPGPU_OK;
  }
  const Delivery out[2] = {{edge, K.edge.ptr, edge ? K.n * sizeof(int32_t) : 0}, {border, K.border.ptr, border ? K.n * sizeof(int32_t) : 0}};
  return deliver(c, out, 2);
}

int icpgpu_iss_fetch(icpgpu_ctx* c, size_t capacity_keypoints, int32_t* keypoint_index, float* keypoints_xyzw, int32_t* n_salient, double* scatter6,
                     double* eigenvalues3, double* saliency) {
  ENTER(c);
  const auto& K = c->iss;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_fetch: no result (icpgpu_iss_keypoints)");
  if ((keypoint_index || keypoints_xyzw) && K.n_keypoints > capacity_keypoints)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "iss_fetch: %zu keypoints, room for %zu", K.n_keypoints, capacity_keypoints);
  const Delivery first[3] = {{keypoint_index, K.comp.kept.ptr, keypoint_index ? K.n_keypoints * sizeof(int32_t) : 0},
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
