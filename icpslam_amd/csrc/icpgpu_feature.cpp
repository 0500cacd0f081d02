// icpgpu_feature.cpp -- host side of the feature-space k-nearest search (pcl::KdTreeFLANN<pcl::FPFHSignature33>::nearestKSearch and, with
// it, feature-space CorrespondenceEstimation; rules: include/icpgpu.h "feature-space k-nearest"; kernels: icp_feature.hip).
//
// Everything the call reads or writes on the device is the feature state's own (icpgpu_ctx::feature): the search cloud, its grid, the
// search calls' scratch and the results of clustering and plane segmentation never meet it.
//
// ... and of the sample-consensus alignment with pre-rejection (pcl::SampleConsensusPrerejective; rules: include/icpgpu.h
// "sample-consensus alignment").  The hypotheses are a pure function of (seed, t, sizes), so the loop runs a CHUNK at a time: the
// device samples and pre-rejects the chunk, the host solves the survivors (solve_umeyama) after one wait, the device scores them 64 at
// a time with every launch queued, and a second wait collects the chunk's counts and sums.  PCL's choice -- the lowest error among
// the hypotheses with enough inliers, the lowest t among equals -- is replayed over them HERE.  Everything the call writes on the device
// is the alignment state's own (icpgpu_ctx::scp).
#include "icp_ctx.h"

static_assert(ICPGPU_FPFH_BINS == kFeatureBins, "the kernels' row length is the header's");
static_assert(ICPGPU_SCP_CHUNK == kScpChunk && ICPGPU_SCP_MAX_SAMPLES == kScpMaxSamples && ICPGPU_SCP_INVALID == kScpInvalid &&
                  ICPGPU_SCP_PREREJECTED == kScpPrerejected && ICPGPU_SCP_NO_TRANSFORM == kScpNoTransform && ICPGPU_SCP_EVALUATED == kScpEvaluated,
              "the kernels' constants are the header's");

extern "C" {

// One wait per call (deliver): the two uploads, the kernels, the rows into the staging buffer, the stream.
int icpgpu_feature_knn(icpgpu_ctx* c, const float* target_feat, size_t n_t, const float* query_feat, size_t n_q, int k, int32_t* idx, float* d2,
                       int32_t* n_found) {
  ENTER(c);
  auto& F = c->feature;
  if (k < 1 || k > ICPGPU_SEARCH_MAX_K) return fail(c, ICPGPU_ERR_INVALID_ARG, "feature_knn: k %d outside 1..%d", k, ICPGPU_SEARCH_MAX_K);
  if (n_t > (size_t)INT32_MAX - 4096 || n_q > (size_t)INT32_MAX - 4096)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "feature_knn: too many rows: %zu targets, %zu queries", n_t, n_q);
  if ((n_t && !target_feat) || (n_q && !query_feat)) return fail(c, ICPGPU_ERR_INVALID_ARG, "feature_knn: null descriptors against a non-zero size");
  if (n_q && (!idx || !d2)) return fail(c, ICPGPU_ERR_INVALID_ARG, "feature_knn: null result pointer");
  if (n_q == 0) return ICPGPU_OK;
  const size_t row = ICPGPU_FPFH_BINS * sizeof(float), cells = n_q * (size_t)k;
  int rc;
  if ((rc = ensure(c, F.target, std::max<size_t>(n_t, 1) * row))) return rc;
  if ((rc = ensure(c, F.finite, std::max<size_t>(n_t, 1) * sizeof(int)))) return rc;
  if ((rc = ensure(c, F.query, n_q * row))) return rc;
  if ((rc = ensure(c, F.idx, cells * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, F.d2, cells * sizeof(float)))) return rc;
  if ((rc = ensure(c, F.n_found, n_q * sizeof(int32_t)))) return rc;
  if (n_t) HIP_TRY(c, hipMemcpyAsync(F.target.ptr, target_feat, n_t * row, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(F.query.ptr, query_feat, n_q * row, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_feature_knn(F.target.as<const float>(), (int)n_t, F.query.as<const float>(), (int)n_q, k, F.finite.as<int>(), F.idx.as<int32_t>(),
                                F.d2.as<float>(), F.n_found.as<int32_t>(), c->stream));
  const Delivery out[3] = {{idx, F.idx.ptr, cells * sizeof(int32_t)}, {d2, F.d2.ptr, cells * sizeof(float)},
                           {n_found, F.n_found.ptr, n_found ? n_q * sizeof(int32_t) : 0}};
  return deliver(c, out, 3);
}

// ---- sample-consensus alignment -------------------------------------------------------------------------------------------------
int icpgpu_scp_align(icpgpu_ctx* c, const float* source_xyzw, size_t n_s, const float* source_feat, const float* target_feat, int nr_samples,
                     int k_correspondences, double similarity_threshold, double max_correspondence_distance, double inlier_fraction,
                     int max_iterations, uint64_t seed, float T16[16], size_t* n_inliers, float* fitness, int32_t* converged, float* out_xyzw) {
  ENTER(c);
  auto& S = c->search;
  auto& K = c->scp;
  K.have = false;
  if (T16)
    for (int i = 0; i < 16; ++i) T16[i] = i % 5 == 0 ? 1.f : 0.f;
  if (n_inliers) *n_inliers = 0;
  if (fitness) *fitness = FLT_MAX;
  if (converged) *converged = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: no search cloud (icpgpu_search_set_input)");
  if (nr_samples < 3 || nr_samples > ICPGPU_SCP_MAX_SAMPLES)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: nr_samples %d outside 3..%d", nr_samples, ICPGPU_SCP_MAX_SAMPLES);
  if (k_correspondences < 1 || k_correspondences > ICPGPU_SEARCH_MAX_K)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: k_correspondences %d outside 1..%d", k_correspondences, ICPGPU_SEARCH_MAX_K);
  if (!(similarity_threshold >= 0.0 && similarity_threshold <= 1.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: similarity_threshold must be inside [0, 1]");
  if (!std::isfinite(max_correspondence_distance) || max_correspondence_distance < 0.0)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: max_correspondence_distance must be finite and >= 0");
  if (!(inlier_fraction >= 0.0 && inlier_fraction <= 1.0)) return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: inlier_fraction must be inside [0, 1]");
  if (max_iterations < 0 || max_iterations > ICPGPU_SCP_MAX_ITERATIONS)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: max_iterations %d outside 0..%d", max_iterations, ICPGPU_SCP_MAX_ITERATIONS);
  if (n_s > (size_t)INT32_MAX - 4096) return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: too many source points: %zu", n_s);
  const size_t n = S.n;
  if ((n_s && (!source_xyzw || !source_feat)) || (n && !target_feat)) return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: null cloud or descriptors against a non-zero size");
  if (!T16 || !n_inliers || !fitness || !converged) return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_align: null output pointer");

  const int nr = nr_samples, kc = k_correspondences, ns = (int)n_s, it = max_iterations;
  const float sim2 = (float)(similarity_threshold * similarity_threshold);
  const float r2 = (float)(max_correspondence_distance * max_correspondence_distance);
  const float frac = (float)inlier_fraction;
  K.n = n, K.n_s = n_s, K.nr = nr, K.max_iterations = it;
  K.converged = 0, K.best_t = -1, K.waits = 0, K.evaluated = 0, K.n_inliers = 0, K.solve_ms = 0.0;
  K.fitness = FLT_MAX;
  for (int i = 0; i < 16; ++i) K.T[i] = i % 5 == 0 ? 1.f : 0.f;
  K.status.assign((size_t)it, ICPGPU_SCP_INVALID);
  K.sidx.assign((size_t)it * nr, -1);
  K.tidx.assign((size_t)it * nr, -1);
  K.count.assign((size_t)it, 0);
  K.sum.assign((size_t)it, 0.0);
  K.error.assign((size_t)it, FLT_MAX);
  K.transforms.assign((size_t)it * 16, 0.f);

  // the search cloud as the evaluation sees it
  const SearchView v = view_of(c);
  const float4* d_cloud = v.cloud;
  const GridDesc& g = v.g;
  const int shells = v.shells(max_correspondence_distance);
  ScpBox box{};
  if (v.sorted) {
    // every finite target point lies in the grid's cells; an image farther outside them than the distance (and a margin far above the
    // binning's rounding) has every d2 above r2
    const double grow = max_correspondence_distance * 1.01 + 0.05 * (double)g.h;
    const double o[3] = {(double)g.ox, (double)g.oy, (double)g.oz}, e[3] = {(double)g.nx, (double)g.ny, (double)g.nz};
    for (int a = 0; a < 3; ++a) {
      box.lo[a] = std::nextafterf((float)(o[a] - grow), -INFINITY);
      box.hi[a] = std::nextafterf((float)(o[a] + e[a] * (double)g.h + grow), INFINITY);
    }
    box.use = 1;
  }

  int rc;
  const float4* d_source = nullptr;
  if (n_s > 0) {
    if ((rc = ensure(c, K.source, n_s * sizeof(float4)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(K.source.ptr, source_xyzw, n_s * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    d_source = K.source.as<const float4>();
  }
  if (it > 0 && n_s > 0) {
    const size_t row = ICPGPU_FPFH_BINS * sizeof(float);
    if ((rc = ensure(c, K.sfeat, n_s * row))) return rc;
    if ((rc = ensure(c, K.tfeat, std::max<size_t>(n, 1) * row))) return rc;
    if ((rc = ensure(c, K.finite, std::max<size_t>(n, 1) * sizeof(int)))) return rc;
    if ((rc = ensure(c, K.rows, n_s * (size_t)kc * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, K.rows_d2, n_s * (size_t)kc * sizeof(float)))) return rc;
    if ((rc = ensure(c, K.found, n_s * sizeof(int32_t)))) return rc;
    const size_t chunk = (size_t)std::min(it, kScpChunk);
    if ((rc = ensure(c, K.c_status, chunk * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, K.c_sidx, chunk * nr * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, K.c_tidx, chunk * nr * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, K.c_sums, chunk * kReduceTerms * sizeof(double)))) return rc;
    if ((rc = ensure(c, K.xforms, chunk * sizeof(Xform)))) return rc;
    if ((rc = ensure(c, K.results, chunk * sizeof(ScpResult)))) return rc;
    if ((rc = ensure(c, K.partials, (size_t)scp_eval_blocks(ns) * kScpBatch * sizeof(ScpPartial)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(K.sfeat.ptr, source_feat, n_s * row, hipMemcpyHostToDevice, c->stream));
    if (n) HIP_TRY(c, hipMemcpyAsync(K.tfeat.ptr, target_feat, n * row, hipMemcpyHostToDevice, c->stream));
    // the correspondence rows of every source point, up front: icpgpu_feature_knn's rows, which stay on the device
    HIP_TRY(c, launch_feature_knn(K.tfeat.as<const float>(), (int)n, K.sfeat.as<const float>(), ns, kc, K.finite.as<int>(), K.rows.as<int32_t>(),
                                  K.rows_d2.as<float>(), K.found.as<int32_t>(), c->stream));

    std::vector<double> sums;
    std::vector<Xform> xforms;
    std::vector<int> survivors;
    std::vector<ScpResult> results;
    float best_error = FLT_MAX;
    for (int t0 = 0; t0 < it; t0 += kScpChunk) {
      const int m = std::min(kScpChunk, it - t0);
      HIP_TRY(c, launch_scp_sample(d_source, ns, d_cloud, v.n, K.rows.as<const int32_t>(), K.found.as<const int32_t>(), kc, (unsigned long long)seed, t0, m,
                                   nr, sim2, K.c_status.as<int32_t>(), K.c_sidx.as<int32_t>(), K.c_tidx.as<int32_t>(), K.c_sums.as<double>(), c->stream));
      sums.resize((size_t)m * kReduceTerms);
      HIP_TRY(c, hipMemcpyAsync(K.status.data() + t0, K.c_status.ptr, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(K.sidx.data() + (size_t)t0 * nr, K.c_sidx.ptr, (size_t)m * nr * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(K.tidx.data() + (size_t)t0 * nr, K.c_tidx.ptr, (size_t)m * nr * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(sums.data(), K.c_sums.ptr, sums.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      ++K.waits;
      // the host's half: a small SVD per survivor
      const auto solve_start = std::chrono::steady_clock::now();
      xforms.clear();
      survivors.clear();
      for (int e = 0; e < m; ++e) {
        const int st = K.status[(size_t)t0 + e];
        if (st < ICPGPU_SCP_INVALID || st > ICPGPU_SCP_EVALUATED) return fail(c, ICPGPU_ERR_HIP, "scp_align: hypothesis %d has status %d (internal error)", t0 + e, st);
        if (st != ICPGPU_SCP_EVALUATED) continue;
        Mat4d Tk;
        if (!solve_umeyama(sums.data() + (size_t)e * kReduceTerms, Tk)) {
          K.status[(size_t)t0 + e] = ICPGPU_SCP_NO_TRANSFORM;
          continue;
        }
        float* Tf = K.transforms.data() + ((size_t)t0 + e) * 16;
        mat4_to_float(Tk, Tf);
        xforms.push_back(to_xform(Tf));
        survivors.push_back(e);
      }
      K.solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - solve_start).count();
      const int L = (int)survivors.size();
      K.evaluated += L;
      if (L == 0) continue;
      HIP_TRY(c, hipMemcpyAsync(K.xforms.ptr, xforms.data(), (size_t)L * sizeof(Xform), hipMemcpyHostToDevice, c->stream));
      for (int b = 0; b < L; b += kScpBatch)
        HIP_TRY(c, launch_scp_eval(d_source, ns, K.xforms.as<const Xform>() + b, std::min(kScpBatch, L - b), d_cloud, v.n_eval, v.sorted, v.cell_start, g,
                                   shells, box, r2, K.partials.as<ScpPartial>(), K.results.as<ScpResult>() + b, c->stream));
      results.resize((size_t)L);
      HIP_TRY(c, hipMemcpyAsync(results.data(), K.results.ptr, (size_t)L * sizeof(ScpResult), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      ++K.waits;
      for (int l = 0; l < L; ++l) {  // (survivors are in t order: the choice goes through t ascending)
        const size_t t = (size_t)t0 + survivors[l];
        const long long cnt = results[l].count;
        if (cnt < 0 || cnt > (long long)ns) return fail(c, ICPGPU_ERR_HIP, "scp_align: hypothesis %zu counts %lld of %d points (internal error)", t, cnt, ns);
        K.count[t] = (int32_t)cnt;
        K.sum[t] = results[l].sum;
        if (cnt > 0) {
          const float err = (float)(results[l].sum / (double)cnt);
          K.error[t] = err;
          if ((float)cnt / (float)ns >= frac && err < best_error) {
            best_error = err;
            K.best_t = (int)t;
          }
        }
      }
    }

  }

  if (n_s > 0) {  // the best hypothesis (or the identity): the inlier list and the aligned cloud
    if ((rc = ensure_compaction(c, K.sel, n_s))) return rc;
    if ((rc = ensure(c, K.ints, 4 * sizeof(int)))) return rc;
    if ((rc = ensure(c, K.aligned, n_s * sizeof(float4)))) return rc;
    Xform Tb = to_xform(static_cast<const float*>(nullptr));
    if (K.best_t >= 0) {
      K.converged = 1;
      K.fitness = K.error[(size_t)K.best_t];
      for (int i = 0; i < 16; ++i) K.T[i] = K.transforms[(size_t)K.best_t * 16 + i];
      Tb = to_xform(K.T);
      HIP_TRY(c, launch_scp_select(d_source, ns, Tb, d_cloud, v.n_eval, v.sorted, v.cell_start, g, shells, box, r2, K.sel.flags.as<int>(),
                                   K.sel.pos.as<int>(), K.sel.scan.as<int>(), K.sel.kept.as<int>(), K.ints.as<int>(), c->stream));
    } else {
      HIP_TRY(c, hipMemsetAsync(K.ints.ptr, 0, 4 * sizeof(int), c->stream));
    }
    HIP_TRY(c, launch_transform(d_source, ns, Tb, K.aligned.as<float4>(), c->stream));
    int m_in = 0;
    const Delivery out[2] = {{&m_in, K.ints.ptr, sizeof(int)}, {out_xyzw, K.aligned.ptr, out_xyzw ? n_s * sizeof(float4) : 0}};
    if ((rc = deliver(c, out, 2))) return rc;
    ++K.waits;
    if (K.best_t >= 0 && m_in != K.count[(size_t)K.best_t])
      return fail(c, ICPGPU_ERR_HIP, "scp_align: %d inliers selected, %d counted (internal error)", m_in, K.count[(size_t)K.best_t]);
    K.n_inliers = (size_t)m_in;
  }
  K.have = true;
  for (int i = 0; i < 16; ++i) T16[i] = K.T[i];
  *n_inliers = K.n_inliers;
  *fitness = K.fitness;
  *converged = K.converged;
  return ICPGPU_OK;
}

int icpgpu_scp_fetch(icpgpu_ctx* c, size_t capacity_hypotheses, size_t capacity_inliers, int32_t* status, int32_t* source_idx, int32_t* target_idx,
                     float* transforms, int32_t* counts, double* sums, float* errors, int32_t* best_t, int32_t* inliers) {
  ENTER(c);
  const auto& K = c->scp;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_fetch: no result (icpgpu_scp_align)");
  const size_t it = (size_t)K.max_iterations;
  const bool per_hypothesis = status || source_idx || target_idx || transforms || counts || sums || errors;
  if ((per_hypothesis && it > capacity_hypotheses) || (inliers && K.n_inliers > capacity_inliers))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "scp_fetch: %zu hypotheses and %zu inliers, room for %zu and %zu", it, K.n_inliers, capacity_hypotheses,
                capacity_inliers);
  if (inliers && K.n_inliers) {
    const int rc = copy_to_host(c, inliers, K.sel.kept.ptr, K.n_inliers * sizeof(int32_t));
    if (rc) return rc;
  }
  if (it) {
    if (status) std::memcpy(status, K.status.data(), it * sizeof(int32_t));
    if (source_idx) std::memcpy(source_idx, K.sidx.data(), it * K.nr * sizeof(int32_t));
    if (target_idx) std::memcpy(target_idx, K.tidx.data(), it * K.nr * sizeof(int32_t));
    if (transforms) std::memcpy(transforms, K.transforms.data(), it * 16 * sizeof(float));
    if (counts) std::memcpy(counts, K.count.data(), it * sizeof(int32_t));
    if (sums) std::memcpy(sums, K.sum.data(), it * sizeof(double));
    if (errors) std::memcpy(errors, K.error.data(), it * sizeof(float));
  }
  if (best_t) *best_t = K.best_t;
  return ICPGPU_OK;
}

int icpgpu_scp_stats(const icpgpu_ctx* c, int32_t* host_waits, int32_t* evaluated, double* host_solve_ms) {
  if (!c || !c->scp.have) return ICPGPU_ERR_INVALID_ARG;
  if (host_waits) *host_waits = c->scp.waits;
  if (evaluated) *evaluated = c->scp.evaluated;
  if (host_solve_ms) *host_solve_ms = c->scp.solve_ms;
  return ICPGPU_OK;
}

}  // extern "C"
