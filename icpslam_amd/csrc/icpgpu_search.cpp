// icpgpu_search.cpp -- host side of the neighbour search (pcl::search::KdTree / pcl::KdTreeFLANN: nearestKSearch, radiusSearch;
// rules: include/icpgpu.h "neighbour search"; kernels: icp_search.hip) and of what runs over the search cloud: normal estimation
// (icp_normals.hip), fast point feature histograms (icp_fpfh.hip) and euclidean clustering (icp_cluster.hip).  The steps every stage
// over the search cloud takes are stated here once and declared in icp_ctx.h: view_of (the cloud as a kernel sees it, with the
// shells rule; also icpgpu_iss.cpp and icpgpu_feature.cpp's alignment), stage_queries, check_k_or_radius and neighbour_rows (rows left
// on the device; also icpgpu_boundary.cpp, icpgpu_iss.cpp and icpgpu_mls.cpp) and deliver (results to the caller; every unit over the cloud).
#include "icp_ctx.h"

namespace icpgpu_impl {
namespace {

int count_finite(const float* xyzw, size_t n) {
  int nf = 0;
  for (size_t i = 0; i < n; ++i) nf += std::isfinite(xyzw[4 * i]) && std::isfinite(xyzw[4 * i + 1]) && std::isfinite(xyzw[4 * i + 2]);
  return nf;
}

}  // namespace

SearchView view_of(const icpgpu_ctx* c) {
  const auto& S = c->search;
  SearchView v;
  v.cloud = S.cloud.data();
  v.n = (int)S.n;
  v.n_eval = S.n_finite > 0 ? v.n : 0;
  if (S.n && S.grid.usable) {
    v.sorted = S.grid.sorted.as<const float4>();
    v.cell_start = S.grid.cell_start.as<const int>();
    v.g = S.grid.g;
  }
  return v;
}

int check_k_or_radius(icpgpu_ctx* c, const char* what, int k, int min_k, double radius) {
  const bool by_k = k != 0, by_radius = radius != 0.0;
  if (by_k == by_radius) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: exactly one of k and radius must be set (k %d, radius %g)", what, k, radius);
  if (by_k && (k < min_k || k > ICPGPU_SEARCH_MAX_K)) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: k %d outside %d..%d", what, k, min_k, ICPGPU_SEARCH_MAX_K);
  if (by_radius && !(std::isfinite(radius) && radius > 0.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: radius must be finite and > 0", what);
  return ICPGPU_OK;
}

// the queries of a call in device memory: the caller's (uploaded into the call's scratch) or the search cloud's own points
int stage_queries(icpgpu_ctx* c, const char* what, const float* queries_xyzw, size_t n_q, const float4*& d_queries) {
  auto& S = c->search;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: no search cloud (icpgpu_search_set_input)", what);
  if (!queries_xyzw) {
    if (n_q != 0 && n_q != S.n) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: null queries mean the search cloud's %zu points, n_q = %zu", what, S.n, n_q);
    d_queries = S.cloud.data();
    return ICPGPU_OK;
  }
  if (n_q > (size_t)INT32_MAX - 4096) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: too many queries: %zu", what, n_q);
  if (n_q == 0) return ICPGPU_OK;
  int rc;
  if ((rc = ensure(c, S.queries, n_q * sizeof(float4)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(S.queries.ptr, queries_xyzw, n_q * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  d_queries = S.queries.as<const float4>();
  return ICPGPU_OK;
}

// what launch_search_radius_count writes for `rows` = n_q + 1 row starts (a buffer that grows is freed first, which waits for the
// device: a call that queues two searches reserves the larger one before the first)
int reserve_radius_rows(icpgpu_ctx* c, size_t rows) {
  auto& S = c->search;
  int rc;
  if ((rc = ensure(c, S.counts, rows * sizeof(int)))) return rc;
  if ((rc = ensure(c, S.longs, rows * sizeof(int)))) return rc;
  if ((rc = ensure(c, S.row_start, rows * sizeof(int)))) return rc;
  if ((rc = ensure(c, S.scratch_start, rows * sizeof(int)))) return rc;
  if ((rc = ensure(c, S.scan, exclusive_scan_scratch_ints((int)rows) * sizeof(int)))) return rc;
  if ((rc = ensure(c, S.totals, 2 * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(c, S.row_start64, rows * sizeof(long long)))) return rc;
  return ICPGPU_OK;
}

// Radius search, first half, queued: the rows' lengths, their scans and the totals (launch_search_radius_count) for n_q > 0 queries.
// shells / r2: what the second half (launch_search_radius_fill) must be given again.
int queue_radius_count(icpgpu_ctx* c, const float4* d_queries, size_t n_q, double radius, int max_nn, int& shells, float& r2) {
  auto& S = c->search;
  int rc;
  if ((rc = reserve_radius_rows(c, n_q + 1))) return rc;
  const SearchView v = view_of(c);
  r2 = (float)(radius * radius);
  shells = v.shells(radius);
  HIP_TRY(c, launch_search_radius_count(d_queries, (int)n_q, v.cloud, v.n_eval, v.sorted, v.cell_start, v.g, shells, r2, max_nn, S.counts.as<int>(),
                                        S.longs.as<int>(), S.row_start.as<int>(), S.scratch_start.as<int>(), S.scan.as<int>(),
                                        S.totals.as<unsigned long long>(), S.row_start64.as<long long>(), c->stream));
  return ICPGPU_OK;
}

// ... second half, queued: `total` (> 0) neighbours into S.idx / S.d2, `scratch_words` 64-bit words of scratch for the long rows
int queue_radius_fill(icpgpu_ctx* c, const float4* d_queries, size_t n_q, int shells, float r2, size_t total, size_t scratch_words) {
  auto& S = c->search;
  int rc;
  if ((rc = ensure(c, S.idx, total * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, S.d2, total * sizeof(float)))) return rc;
  if ((rc = ensure(c, S.scratch, std::max<size_t>(scratch_words, 1) * sizeof(unsigned long long)))) return rc;
  const SearchView v = view_of(c);
  HIP_TRY(c, launch_search_radius_fill(d_queries, (int)n_q, v.cloud, v.n, v.sorted, v.cell_start, v.g, shells, r2, S.row_start.as<int>(),
                                       S.scratch_start.as<int>(), S.scratch.as<unsigned long long>(), S.idx.as<int32_t>(), S.d2.as<float>(),
                                       c->stream));
  return ICPGPU_OK;
}

// what launch_search_knn writes for `rows` queries of k neighbours each
int reserve_knn_rows(icpgpu_ctx* c, size_t rows, int k) {
  auto& S = c->search;
  int rc;
  if ((rc = ensure(c, S.idx, rows * (size_t)k * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, S.d2, rows * (size_t)k * sizeof(float)))) return rc;
  if ((rc = ensure(c, S.n_found, rows * sizeof(int32_t)))) return rc;
  return ensure(c, S.far, (rows + 2) * sizeof(int));
}

// One k-nearest search, queued, its rows left on the device: S.idx / S.d2 with stride k, the lengths in S.n_found.  No host wait.
int knn_rows_on_device(icpgpu_ctx* c, const float4* d_points, size_t n_points, int k) {
  auto& S = c->search;
  int rc;
  if ((rc = reserve_knn_rows(c, n_points, k))) return rc;
  const SearchView v = view_of(c);
  HIP_TRY(c, launch_search_knn(d_points, (int)n_points, v.cloud, v.n, v.sorted, v.cell_start, v.g, k, S.idx.as<int32_t>(), S.d2.as<float>(),
                               S.n_found.as<int32_t>(), S.far.as<int>(), c->stream));
  return ICPGPU_OK;
}

// One radius search, queued, its rows left on the device: S.idx / S.d2 in CSR form by S.row_start, the lengths in S.counts.  One host
// wait, for the totals that size the rows.
int radius_rows_on_device(icpgpu_ctx* c, const char* what, const float4* d_points, size_t n_points, double radius) {
  auto& S = c->search;
  int shells, rc;
  float r2;
  if ((rc = queue_radius_count(c, d_points, n_points, radius, 0, shells, r2))) return rc;
  unsigned long long totals[2] = {0, 0};
  const Delivery first[1] = {{totals, S.totals.ptr, sizeof totals}};
  if ((rc = deliver(c, first, 1))) return rc;
  if (totals[0] > (unsigned long long)INT32_MAX || totals[1] > (unsigned long long)INT32_MAX)
    return fail(c, ICPGPU_ERR_UNSUPPORTED, "%s: %llu neighbours in all, more than the int32 scans carry", what, totals[0]);
  if (totals[0]) return queue_radius_fill(c, d_points, n_points, shells, r2, (size_t)totals[0], (size_t)totals[1]);
  if ((rc = ensure(c, S.idx, sizeof(int32_t)))) return rc;  // (every row is empty: nothing is read through the pointers)
  return ensure(c, S.d2, sizeof(float));
}

int neighbour_rows(icpgpu_ctx* c, const char* what, const float4* d_points, size_t n_points, int k, double radius, NeighbourRows& rows,
                   size_t reserve_points) {
  auto& S = c->search;
  int rc;
  if (k) {
    if (reserve_points > n_points && (rc = reserve_knn_rows(c, reserve_points, k))) return rc;
    if ((rc = knn_rows_on_device(c, d_points, n_points, k))) return rc;
    rows = {S.idx.as<int32_t>(), S.d2.as<float>(), S.n_found.as<int32_t>(), k, nullptr, S.n_found.ptr};
  } else {
    if (reserve_points > n_points && (rc = reserve_radius_rows(c, reserve_points + 1))) return rc;
    if ((rc = radius_rows_on_device(c, what, d_points, n_points, radius))) return rc;
    rows = {S.idx.as<int32_t>(), S.d2.as<float>(), nullptr, 0, S.row_start.as<int>(), S.counts.ptr};
  }
  return ICPGPU_OK;
}

// (Delivery: icp_ctx.h)  Results on their way to the caller's (pageable) arrays: up to three device arrays copied into consecutive slices of the pinned
// staging buffer -- copies the stream really queues -- ONE wait for the stream, then a memcpy each.  Results that do not fit the
// staging buffer (kStageMaxBytes) are copied straight into the caller's memory, where the runtime may wait inside every copy.
int deliver(icpgpu_ctx* c, const Delivery* parts, int n_parts) {
  size_t total = 0;
  for (int i = 0; i < n_parts; ++i) total += (parts[i].bytes + 15) & ~(size_t)15;
  if (total == 0) return ICPGPU_OK;
  if (total > kStageMaxBytes) {
    for (int i = 0; i < n_parts; ++i)
      if (parts[i].bytes) HIP_TRY(c, hipMemcpyAsync(parts[i].dst, parts[i].d_src, parts[i].bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ICPGPU_OK;
  }
  int rc;
  if ((rc = ensure_stage(c, total))) return rc;
  size_t at = 0;
  for (int i = 0; i < n_parts; ++i) {
    if (parts[i].bytes) HIP_TRY(c, hipMemcpyAsync(static_cast<char*>(c->h_stage) + at, parts[i].d_src, parts[i].bytes, hipMemcpyDeviceToHost, c->stream));
    at += (parts[i].bytes + 15) & ~(size_t)15;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  at = 0;
  for (int i = 0; i < n_parts; ++i) {
    if (parts[i].bytes) std::memcpy(parts[i].dst, static_cast<const char*>(c->h_stage) + at, parts[i].bytes);
    at += (parts[i].bytes + 15) & ~(size_t)15;
  }
  return ICPGPU_OK;
}

}  // namespace icpgpu_impl

extern "C" {

// Copies the cloud and builds its k-NN grid.  Nothing of the context's source, target, their grids, the covariances, the NDT cells
// or the filters' results is touched; the previous search cloud, and a clustering, region growing,
// plane segmentation, ground filter, sample-consensus alignment, ISS or moving least squares result over it, is gone whatever this call returns.
int icpgpu_search_set_input(icpgpu_ctx* c, const float* xyzw, size_t n) {
  ENTER(c);
  auto& S = c->search;
  S.set = false;
  S.n = 0;
  S.n_finite = 0;
  S.grid.built = S.grid.usable = false;  // (version 0: a build never stands for the next cloud)
  c->cluster.have = false;               // (a clustering result is a result over the cloud that goes)
  c->region.have = false;                // (and so is a region growing result)
  c->sac.have = false;                   // (and so is a plane segmentation)
  c->pmf.have = c->pmf.ran = false;      // (and a ground filter's)
  c->scp.have = false;                   // (and a sample-consensus alignment)
  c->iss.have = false;                   // (and the ISS keypoints)
  c->mls.have = false;                   // (and the moving least squares record)
  if (n && !xyzw) return fail(c, ICPGPU_ERR_INVALID_ARG, "null cloud pointer with n = %zu", n);
  if (n > (size_t)INT32_MAX - 4096) return fail(c, ICPGPU_ERR_INVALID_ARG, "cloud too large: %zu points", n);
  if (n) {
    int rc;
    if ((rc = ensure(c, S.cloud.buf, n * sizeof(float4)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(S.cloud.buf.ptr, xyzw, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    S.cloud.n = n;
    S.cloud.set = true;
    S.cloud.bbox_version = 0;
    S.cloud.finite_version = 0;
    if ((rc = build_knn_grid(c, S.cloud, S.grid))) return rc;
    if (!S.grid.usable && n > (size_t)kGicpCovFarMost)
      return fail(c, ICPGPU_ERR_UNSUPPORTED, "neighbour search: cannot index this cloud of %zu points", n);
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller's buffer is free from here on)
    S.n_finite = S.grid.n_finite >= 0 ? S.grid.n_finite : count_finite(xyzw, n);
  }
  S.n = n;
  S.set = true;
  return ICPGPU_OK;
}

int icpgpu_search_size(const icpgpu_ctx* c, size_t* n, size_t* n_finite) {
  if (!c) return ICPGPU_ERR_INVALID_ARG;
  if (n) *n = c->search.set ? c->search.n : 0;
  if (n_finite) *n_finite = c->search.set ? (size_t)c->search.n_finite : 0;
  return c->search.set ? ICPGPU_OK : ICPGPU_ERR_INVALID_ARG;
}

// One wait per call (deliver): the kernels, the rows into the staging buffer, the stream.
int icpgpu_search_knn(icpgpu_ctx* c, const float* queries_xyzw, size_t n_q, int k, int32_t* idx, float* d2, int32_t* n_found) {
  ENTER(c);
  const float4* d_queries = nullptr;
  int rc;
  if (k < 1 || k > ICPGPU_SEARCH_MAX_K) return fail(c, ICPGPU_ERR_INVALID_ARG, "search_knn: k %d outside 1..%d", k, ICPGPU_SEARCH_MAX_K);
  if ((rc = stage_queries(c, "search_knn", queries_xyzw, n_q, d_queries))) return rc;
  if (n_q == 0) return ICPGPU_OK;
  if (!idx || !d2) return fail(c, ICPGPU_ERR_INVALID_ARG, "search_knn: null result pointer");
  NeighbourRows rows;
  if ((rc = neighbour_rows(c, "search_knn", d_queries, n_q, k, 0.0, rows))) return rc;
  const size_t cells = n_q * (size_t)k;
  const Delivery out[3] = {{idx, rows.idx, cells * sizeof(int32_t)}, {d2, rows.d2, cells * sizeof(float)},
                           {n_found, rows.n_found, n_found ? n_q * sizeof(int32_t) : 0}};
  return deliver(c, out, 3);
}

// Two waits at most (deliver): the totals with row_start, then the rows.
int icpgpu_search_radius(icpgpu_ctx* c, const float* queries_xyzw, size_t n_q, double radius, int max_nn, size_t capacity, int64_t* row_start,
                         int32_t* idx, float* d2, size_t* n_total) {
  ENTER(c);
  auto& S = c->search;
  if (n_total) *n_total = 0;
  const float4* d_queries = nullptr;
  int rc;
  if (!std::isfinite(radius) || radius < 0.0) return fail(c, ICPGPU_ERR_INVALID_ARG, "search_radius: radius must be finite and >= 0");
  if (max_nn < 0) return fail(c, ICPGPU_ERR_INVALID_ARG, "search_radius: max_nn %d < 0", max_nn);
  if (!row_start || !n_total) return fail(c, ICPGPU_ERR_INVALID_ARG, "search_radius: null row_start or n_total");
  if ((rc = stage_queries(c, "search_radius", queries_xyzw, n_q, d_queries))) return rc;
  row_start[0] = 0;
  if (n_q == 0) return ICPGPU_OK;
  const size_t rows = n_q + 1;
  int shells;
  float r2;
  if ((rc = queue_radius_count(c, d_queries, n_q, radius, max_nn, shells, r2))) return rc;
  unsigned long long totals[2] = {0, 0};
  const Delivery first[2] = {{totals, S.totals.ptr, sizeof totals}, {row_start, S.row_start64.ptr, rows * sizeof(int64_t)}};
  if ((rc = deliver(c, first, 2))) return rc;
  if (totals[0] > (unsigned long long)INT32_MAX || totals[1] > (unsigned long long)INT32_MAX) {
    for (size_t i = 0; i < rows; ++i) row_start[i] = 0;  // (the int32 scan has wrapped)
    return fail(c, ICPGPU_ERR_UNSUPPORTED, "search_radius: %llu neighbours in all, more than the int32 scans carry", totals[0]);
  }
  const size_t total = (size_t)totals[0];
  *n_total = total;
  if (total == 0) return ICPGPU_OK;
  if (total > capacity || !idx || !d2) return fail(c, ICPGPU_ERR_INVALID_ARG, "search_radius: %zu neighbours, room for %zu", total, idx && d2 ? capacity : (size_t)0);
  if ((rc = queue_radius_fill(c, d_queries, n_q, shells, r2, total, (size_t)totals[1]))) return rc;
  const Delivery second[2] = {{idx, S.idx.ptr, total * sizeof(int32_t)}, {d2, S.d2.ptr, total * sizeof(float)}};
  return deliver(c, second, 2);
}

// pcl::NormalEstimation over the search cloud (rules: include/icpgpu.h "normal estimation").  The neighbour rows never leave the
// device: the search's launchers write them into the search state's buffers and normals_from_rows_kernel (icp_normals.hip) reads
// them there.  One wait per call with k (deliver), two at most with a radius: the totals that size the rows, then the results.
int icpgpu_normal_estimation(icpgpu_ctx* c, const float* queries_xyzw, size_t n_q, int k, double radius, const float* viewpoint3, float* out_nxyzc,
                             int32_t* n_neighbours, float* moments9) {
  ENTER(c);
  auto& S = c->search;
  const float4* d_queries = nullptr;
  int rc;
  if ((rc = check_k_or_radius(c, "normal_estimation", k, 1, radius))) return rc;
  float vp[3] = {0.f, 0.f, 0.f};
  if (viewpoint3) {
    for (int a = 0; a < 3; ++a) vp[a] = viewpoint3[a];
    if (!std::isfinite(vp[0]) || !std::isfinite(vp[1]) || !std::isfinite(vp[2])) return fail(c, ICPGPU_ERR_INVALID_ARG, "normal_estimation: non-finite viewpoint");
  }
  if ((rc = stage_queries(c, "normal_estimation", queries_xyzw, n_q, d_queries))) return rc;
  if (n_q == 0) return ICPGPU_OK;
  if (!out_nxyzc) return fail(c, ICPGPU_ERR_INVALID_ARG, "normal_estimation: null result pointer");
  if ((rc = ensure(c, S.normals, n_q * sizeof(float4)))) return rc;
  if (moments9 && (rc = ensure(c, S.moments, n_q * 9 * sizeof(float)))) return rc;
  float* d_moments = moments9 ? S.moments.as<float>() : nullptr;
  const SearchView v = view_of(c);
  NeighbourRows rows;
  if ((rc = neighbour_rows(c, "normal_estimation", d_queries, n_q, k, radius, rows))) return rc;
  HIP_TRY(c, launch_normals_from_rows(d_queries, (int)n_q, v.cloud, v.n, rows.idx, rows.n_found, rows.k, rows.row_start, vp, S.normals.as<float4>(),
                                      d_moments, c->stream));
  const Delivery out[3] = {{out_nxyzc, S.normals.ptr, n_q * sizeof(float4)},
                           {n_neighbours, rows.counts, n_neighbours ? n_q * sizeof(int32_t) : 0},
                           {moments9, d_moments, moments9 ? n_q * 9 * sizeof(float) : 0}};
  return deliver(c, out, 3);
}

// pcl::FPFHEstimation over the search cloud (rules: include/icpgpu.h "fast point feature histograms"; kernels: icp_fpfh.hip).  The
// cloud's own rows feed spfh_from_rows_kernel; the queries' rows -- the same rows when the queries are the cloud's points, a second
// search behind the first otherwise -- feed fpfh_from_rows_kernel.  The rows never leave the device.  Host waits: one with k (the
// results); with a radius one more per search for the totals that size its rows -- two without queries, three with.
int icpgpu_fpfh_estimation(icpgpu_ctx* c, const float* normals_nxyzc, const float* queries_xyzw, size_t n_q, int k, double radius, float* out_fpfh,
                           int32_t* n_neighbours, float* spfh) {
  ENTER(c);
  auto& S = c->search;
  const float4* d_queries = nullptr;
  int rc;
  if ((rc = check_k_or_radius(c, "fpfh_estimation", k, 2, radius))) return rc;
  if ((rc = stage_queries(c, "fpfh_estimation", queries_xyzw, n_q, d_queries))) return rc;
  const size_t n = S.n;
  if (n && !normals_nxyzc) return fail(c, ICPGPU_ERR_INVALID_ARG, "fpfh_estimation: null normals for a search cloud of %zu points", n);
  if (n_q && !out_fpfh) return fail(c, ICPGPU_ERR_INVALID_ARG, "fpfh_estimation: null result pointer");
  if (n_q == 0) return ICPGPU_OK;
  const bool own = !queries_xyzw;  // the queries' rows are the cloud's own rows
  if ((rc = ensure(c, S.fpfh_normals, std::max<size_t>(n, 1) * sizeof(float4)))) return rc;
  if ((rc = ensure(c, S.spfh, std::max<size_t>(n, 1) * ICPGPU_FPFH_BINS * sizeof(float)))) return rc;
  if ((rc = ensure(c, S.fpfh, std::max<size_t>(n_q, 1) * ICPGPU_FPFH_BINS * sizeof(float)))) return rc;
  if (n) HIP_TRY(c, hipMemcpyAsync(S.fpfh_normals.ptr, normals_nxyzc, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  const SearchView v = view_of(c);
  float* d_spfh = S.spfh.as<float>();
  float* d_fpfh = S.fpfh.as<float>();
  NeighbourRows rows;
  if (n) {  // (reserved for the longer of the two searches before the first: a buffer that grows is freed first, which waits)
    if ((rc = neighbour_rows(c, "fpfh_estimation", v.cloud, n, k, radius, rows, n_q))) return rc;
    HIP_TRY(c, launch_spfh_from_rows(v.cloud, v.n, S.fpfh_normals.as<const float4>(), rows.idx, rows.n_found, rows.k, rows.row_start, d_spfh, c->stream));
  }
  if (!own) {
    if ((rc = neighbour_rows(c, "fpfh_estimation", d_queries, n_q, k, radius, rows))) return rc;
  }
  HIP_TRY(c, launch_fpfh_from_rows(d_queries, (int)n_q, v.n, d_spfh, rows.idx, rows.d2, rows.n_found, rows.k, rows.row_start, d_fpfh, c->stream));
  const Delivery out[3] = {{out_fpfh, d_fpfh, n_q * ICPGPU_FPFH_BINS * sizeof(float)},
                           {n_neighbours, rows.counts, n_neighbours ? n_q * sizeof(int32_t) : 0},
                           {spfh, d_spfh, spfh ? n * ICPGPU_FPFH_BINS * sizeof(float) : 0}};
  return deliver(c, out, 3);
}

// pcl::EuclideanClusterExtraction over the search cloud (rules: include/icpgpu.h "euclidean clustering"; kernels: icp_cluster.hip).
// Everything the call writes is the cluster state's own: the search state's scratch, and so a later search or normal estimation,
// never meets it.  One wait (deliver): the two counts.
int icpgpu_euclidean_cluster_extraction(icpgpu_ctx* c, double tolerance, int min_size, int max_size, size_t* n_clusters, size_t* n_clustered) {
  ENTER(c);
  auto& S = c->search;
  auto& K = c->cluster;
  K.have = false;
  if (n_clusters) *n_clusters = 0;
  if (n_clustered) *n_clustered = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "euclidean_cluster_extraction: no search cloud (icpgpu_search_set_input)");
  if (!std::isfinite(tolerance) || tolerance < 0.0) return fail(c, ICPGPU_ERR_INVALID_ARG, "euclidean_cluster_extraction: tolerance must be finite and >= 0");
  if (!n_clusters || !n_clustered) return fail(c, ICPGPU_ERR_INVALID_ARG, "euclidean_cluster_extraction: null n_clusters or n_clustered");
  const size_t n = S.n, ints = std::max<size_t>(n, 1) * sizeof(int);
  int rc;
  for (DeviceBuf* b : {&K.parent, &K.sizes, &K.component, &K.labels, &K.rank_of})
    if ((rc = ensure(c, *b, ints))) return rc;
  for (DeviceBuf* b : {&K.csize, &K.cstart})
    if ((rc = ensure(c, *b, (n + 1) * sizeof(int)))) return rc;
  for (DeviceBuf* b : {&K.keys, &K.vals})
    if ((rc = ensure(c, *b, 2 * ints))) return rc;
  if ((rc = ensure(c, K.cstart64, (n + 1) * sizeof(long long)))) return rc;
  if ((rc = ensure(c, K.scratch, cluster_scratch_ints((int)n) * sizeof(int)))) return rc;
  if ((rc = ensure(c, K.counts, 2 * sizeof(int)))) return rc;
  const SearchView v = view_of(c);
  const float r2 = (float)(tolerance * tolerance);
  HIP_TRY(c, launch_cluster_extract(v.cloud, v.n, v.n_eval > 0, v.sorted, v.cell_start, v.g, v.shells(tolerance), r2, min_size, max_size,
                                    K.parent.as<int>(), K.sizes.as<int>(), K.component.as<int>(), K.labels.as<int>(), K.rank_of.as<int>(),
                                    K.csize.as<int>(), K.cstart.as<int>(), K.cstart64.as<long long>(), K.keys.as<int>(), K.vals.as<int>(),
                                    K.scratch.as<int>(), K.counts.as<int>(), c->stream));
  int counts[2] = {0, 0};
  const Delivery out[1] = {{counts, K.counts.ptr, sizeof counts}};
  if ((rc = deliver(c, out, 1))) return rc;
  K.n = n;
  K.n_clusters = (size_t)counts[0];
  K.n_clustered = (size_t)counts[1];
  K.have = true;
  *n_clusters = K.n_clusters;
  *n_clustered = K.n_clustered;
  return ICPGPU_OK;
}

int icpgpu_cluster_fetch(icpgpu_ctx* c, size_t capacity_clusters, size_t capacity_indices, int64_t* cluster_start, int32_t* indices, int32_t* labels,
                         int32_t* component) {
  ENTER(c);
  const auto& K = c->cluster;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "cluster_fetch: no result (icpgpu_euclidean_cluster_extraction)");
  if (!cluster_start) return fail(c, ICPGPU_ERR_INVALID_ARG, "cluster_fetch: null cluster_start");
  if (K.n_clusters > capacity_clusters || K.n_clustered > capacity_indices || (K.n_clustered && !indices))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "cluster_fetch: %zu clusters of %zu points, room for %zu and %zu", K.n_clusters, K.n_clustered,
                capacity_clusters, indices ? capacity_indices : (size_t)0);
  const Delivery out[4] = {{cluster_start, K.cstart64.ptr, (K.n_clusters + 1) * sizeof(int64_t)},
                           {indices, K.vals.as<const int>() + K.n, K.n_clustered * sizeof(int32_t)},
                           {labels, K.labels.ptr, labels ? K.n * sizeof(int32_t) : 0},
                           {component, K.component.ptr, component ? K.n * sizeof(int32_t) : 0}};
  return deliver(c, out, 4);
}

}  // extern "C"
