// icpgpu_mls.cpp -- host side of the moving least squares projection over the search cloud (pcl::MovingLeastSquares, UpsamplingMethod
// NONE; rules: include/icpgpu.h "moving least squares"; kernels: icp_mls.hip).  The radius rows never leave the device: the search's
// launchers write them into the search state's buffers, as for icpgpu_normal_estimation, and the kernels read them there; everything
// the call keeps lives in the MLS state's own buffers.  Two waits per call: the totals that size the rows, then the results -- the
// kept count travels with them.
#include "icp_ctx.h"

extern "C" {

int icpgpu_moving_least_squares(icpgpu_ctx* c, const float* queries_xyzw, size_t n_q, double radius, int order, double sqr_gauss_param,
                                float* out_xyzw, float* out_nxyzc, int32_t* out_index, size_t* n_out) {
  ENTER(c);
  auto& M = c->mls;
  M.have = false;
  M.waits = 0;
  if (n_out) *n_out = 0;
  if (!(std::isfinite(radius) && radius > 0.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "moving_least_squares: radius must be finite and > 0");
  if (order < 0 || order > ICPGPU_MLS_MAX_ORDER)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "moving_least_squares: order %d outside 0..%d", order, ICPGPU_MLS_MAX_ORDER);
  if (!(sqr_gauss_param == 0.0 || (std::isfinite(sqr_gauss_param) && sqr_gauss_param > 0.0)))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "moving_least_squares: sqr_gauss_param must be 0 or finite and > 0 (%g)", sqr_gauss_param);
  const float4* d_queries = nullptr;
  int rc;
  if ((rc = stage_queries(c, "moving_least_squares", queries_xyzw, n_q, d_queries))) return rc;
  if (n_q && (!out_xyzw || !out_index || !n_out)) return fail(c, ICPGPU_ERR_INVALID_ARG, "moving_least_squares: null out_xyzw, out_index or n_out");
  if (n_q == 0) {
    M.n_q = M.n_out = 0;
    M.have = true;
    return ICPGPU_OK;
  }
  const double s = sqr_gauss_param == 0.0 ? radius * radius : sqr_gauss_param;
  for (DeviceBuf* b : {&M.n_neighbours, &M.status})
    if ((rc = ensure(c, *b, n_q * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, M.plane, n_q * 7 * sizeof(double)))) return rc;
  if ((rc = ensure(c, M.coeff, n_q * 10 * sizeof(double)))) return rc;
  if ((rc = ensure(c, M.sums, n_q * 9 * sizeof(double)))) return rc;
  if ((rc = ensure(c, M.frame, n_q * 12 * sizeof(double)))) return rc;
  if ((rc = ensure(c, M.fit, std::max<size_t>(n_q * icpgpu::mls_fit_doubles(order), 1) * sizeof(double)))) return rc;
  for (DeviceBuf* b : {&M.points, &M.normals, &M.out_points, &M.out_normals})
    if ((rc = ensure(c, *b, n_q * sizeof(float4)))) return rc;
  if ((rc = ensure_compaction(c, M.comp, n_q))) return rc;
  if ((rc = ensure(c, M.ints, 4 * sizeof(int)))) return rc;
  const SearchView v = view_of(c);
  NeighbourRows rows;
  if ((rc = neighbour_rows(c, "moving_least_squares", d_queries, n_q, 0, radius, rows))) return rc;
  HIP_TRY(c, launch_mls(d_queries, (int)n_q, v.cloud, v.n, rows.idx, rows.row_start, order, s, M.n_neighbours.as<int32_t>(), M.sums.as<double>(),
                        M.frame.as<double>(), M.fit.as<double>(), M.status.as<int32_t>(), M.plane.as<double>(), M.coeff.as<double>(),
                        M.points.as<float4>(), M.normals.as<float4>(), M.comp.flags.as<int>(), M.comp.pos.as<int>(), M.comp.scan.as<int>(),
                        M.comp.kept.as<int>(), M.ints.as<int>(), M.out_points.as<float4>(), M.out_normals.as<float4>(), c->stream));
  // n_q slots of each array arrive with the count; the first n_out of them reach the caller, whose arrays stay untouched beyond
  M.h_points.resize(n_q * 4);
  M.h_index.resize(n_q);
  if (out_nxyzc) M.h_normals.resize(n_q * 4);
  int count = 0;
  const Delivery out[4] = {{&count, M.ints.ptr, sizeof count},
                           {M.h_points.data(), M.out_points.ptr, n_q * sizeof(float4)},
                           {M.h_index.data(), M.comp.kept.ptr, n_q * sizeof(int32_t)},
                           {M.h_normals.data(), M.out_normals.ptr, out_nxyzc ? n_q * sizeof(float4) : 0}};
  if ((rc = deliver(c, out, 4))) return rc;
  if (count < 0 || (size_t)count > n_q) return fail(c, ICPGPU_ERR_HIP, "moving_least_squares: %d of %zu queries kept (internal error)", count, n_q);
  const size_t kept = (size_t)count;
  if (kept) {
    std::memcpy(out_xyzw, M.h_points.data(), kept * sizeof(float4));
    std::memcpy(out_index, M.h_index.data(), kept * sizeof(int32_t));
    if (out_nxyzc) std::memcpy(out_nxyzc, M.h_normals.data(), kept * sizeof(float4));
  }
  M.n_q = n_q;
  M.n_out = kept;
  M.waits = 2;
  M.have = true;
  *n_out = kept;
  return ICPGPU_OK;
}

int icpgpu_mls_fetch(icpgpu_ctx* c, size_t capacity, int32_t* status, int32_t* n_neighbours, double* plane7, double* coeff10) {
  ENTER(c);
  const auto& M = c->mls;
  if (!M.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "mls_fetch: no result (icpgpu_moving_least_squares)");
  if (capacity < M.n_q) return fail(c, ICPGPU_ERR_INVALID_ARG, "mls_fetch: %zu queries, room for %zu", M.n_q, capacity);
  const Delivery out[4] = {{status, M.status.ptr, status ? M.n_q * sizeof(int32_t) : 0},
                           {n_neighbours, M.n_neighbours.ptr, n_neighbours ? M.n_q * sizeof(int32_t) : 0},
                           {plane7, M.plane.ptr, plane7 ? M.n_q * 7 * sizeof(double) : 0},
                           {coeff10, M.coeff.ptr, coeff10 ? M.n_q * 10 * sizeof(double) : 0}};
  return deliver(c, out, 4);
}

int icpgpu_mls_stats(const icpgpu_ctx* c, int32_t* host_waits) {
  if (!c || !c->mls.have) return ICPGPU_ERR_INVALID_ARG;
  if (host_waits) *host_waits = c->mls.waits;
  return ICPGPU_OK;
}

}  // extern "C"
