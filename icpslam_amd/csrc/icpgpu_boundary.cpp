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
  if ((rc = check_k_or_radius(c, "boundary_estimation", k, 1, radius))) return rc;
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
  NeighbourRows rows;
  if ((rc = neighbour_rows(c, "boundary_estimation", d_queries, n_q, k, radius, rows))) return rc;
  uint8_t* d_flags = S.bnd_flags.as<uint8_t>();
  int32_t* d_dirs = S.bnd_dirs.as<int32_t>();
  int32_t* d_witness = S.bnd_witness.as<int32_t>();
  HIP_TRY(c, launch_boundary_from_rows(d_queries, (int)n_q, S.bnd_normals.as<const float4>(), v.cloud, v.n, rows.idx, rows.n_found, rows.k, rows.row_start,
                                       3, std::cos(angle_threshold), d_flags, nullptr, d_dirs, d_witness, c->stream));
  const Delivery out[4] = {{boundary, d_flags, n_q * sizeof(uint8_t)},
                           {n_neighbours, rows.counts, n_neighbours ? n_q * sizeof(int32_t) : 0},
                           {n_directions, d_dirs, n_directions ? n_q * sizeof(int32_t) : 0},
                           {witness, d_witness, witness ? n_q * sizeof(int32_t) : 0}};
  return deliver(c, out, 4);
}

}  // extern "C"
