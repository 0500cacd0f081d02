// icpgpu_boundary.cpp -- host side of pcl::BoundaryEstimation over the search cloud (rules: include/icpgpu.h "boundary estimation";
// kernel: icp_boundary.hip).  The neighbour rows never leave the device: the search's launchers write them into the search state's
// buffers, as for icpgpu_normal_estimation, and boundary_from_rows_kernel reads them there.  One wait per call with k (deliver), two
// with a radius: the totals that size the rows, then the results.
#include "icp_ctx.h"

extern "C" {

int icpgpu_boundary_estimation(icpgpu_ctx* c, const float* normals_nxyzc, const float* queries_xyzw, size_t n_q, int k, double radius,
                               double angle_threshold, uint8_t* boundary, int32_t* n_neighbours, int32_t* n_directions, int32_t* witness) {
  ENTER(c);
  auto& S = c->search;
  const float4* d_queries = nullptr;
  int rc;
  const bool by_k = k != 0, by_radius = radius != 0.0;
  if (by_k == by_radius) return fail(c, ICPGPU_ERR_INVALID_ARG, "boundary_estimation: exactly one of k and radius must be set (k %d, radius %g)", k, radius);
  if (by_k && (k < 1 || k > ICPGPU_SEARCH_MAX_K)) return fail(c, ICPGPU_ERR_INVALID_ARG, "boundary_estimation: k %d outside 1..%d", k, ICPGPU_SEARCH_MAX_K);
  if (by_radius && !(std::isfinite(radius) && radius > 0.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "boundary_estimation: radius must be finite and > 0");
  if (!(std::isfinite(angle_threshold) && angle_threshold > 0.0 && angle_threshold <= M_PI))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "boundary_estimation: angle_threshold %g outside (0, pi]", angle_threshold);
  if ((rc = stage_queries(c, "boundary_estimation", queries_xyzw, n_q, d_queries))) return rc;
  if (n_q == 0) return ICPGPU_OK;
  if (!normals_nxyzc) return fail(c, ICPGPU_ERR_INVALID_ARG, "boundary_estimation: null normals for %zu queries", n_q);
  if (!boundary) return fail(c, ICPGPU_ERR_INVALID_ARG, "boundary_estimation: null result pointer");
  if ((rc = ensure(c, S.bnd_normals, n_q * sizeof(float4)))) return rc;
  if ((rc = ensure(c, S.bnd_flags, n_q * sizeof(uint8_t)))) return rc;
  if ((rc = ensure(c, S.bnd_dirs, n_q * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, S.bnd_witness, n_q * sizeof(int32_t)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(S.bnd_normals.ptr, normals_nxyzc, n_q * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  const SearchView v = view_of(c);
  const double cos_threshold = std::cos(angle_threshold);
  const float4* d_normals = static_cast<const float4*>(S.bnd_normals.ptr);
  uint8_t* d_flags = static_cast<uint8_t*>(S.bnd_flags.ptr);
  int32_t* d_dirs = static_cast<int32_t*>(S.bnd_dirs.ptr);
  int32_t* d_witness = static_cast<int32_t*>(S.bnd_witness.ptr);
  const void* d_counts = nullptr;
  if (by_k) {
    const size_t cells = n_q * (size_t)k;
    if ((rc = ensure(c, S.idx, cells * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, S.d2, cells * sizeof(float)))) return rc;
    if ((rc = ensure(c, S.n_found, n_q * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, S.far, (n_q + 2) * sizeof(int)))) return rc;
    HIP_TRY(c, launch_search_knn(d_queries, (int)n_q, v.cloud, v.n, v.sorted, v.cell_start, v.g, k, static_cast<int32_t*>(S.idx.ptr),
                                 static_cast<float*>(S.d2.ptr), static_cast<int32_t*>(S.n_found.ptr), static_cast<int*>(S.far.ptr), c->stream));
    HIP_TRY(c, launch_boundary_from_rows(d_queries, (int)n_q, d_normals, v.cloud, v.n, static_cast<const int32_t*>(S.idx.ptr),
                                         static_cast<const int32_t*>(S.n_found.ptr), k, nullptr, 3, cos_threshold, d_flags, nullptr, d_dirs, d_witness,
                                         c->stream));
    d_counts = S.n_found.ptr;
  } else {
    if ((rc = radius_rows_on_device(c, "boundary_estimation", d_queries, n_q, radius))) return rc;
    HIP_TRY(c, launch_boundary_from_rows(d_queries, (int)n_q, d_normals, v.cloud, v.n, static_cast<const int32_t*>(S.idx.ptr), nullptr, 0,
                                         static_cast<const int*>(S.row_start.ptr), 3, cos_threshold, d_flags, nullptr, d_dirs, d_witness, c->stream));
    d_counts = S.counts.ptr;
  }
  const Delivery out[4] = {{boundary, d_flags, n_q * sizeof(uint8_t)},
                           {n_neighbours, d_counts, n_neighbours ? n_q * sizeof(int32_t) : 0},
                           {n_directions, d_dirs, n_directions ? n_q * sizeof(int32_t) : 0},
                           {witness, d_witness, witness ? n_q * sizeof(int32_t) : 0}};
  return deliver(c, out, 4);
}

}  // extern "C"
