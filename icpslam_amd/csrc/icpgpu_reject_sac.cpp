// icpgpu_reject_sac.cpp -- host side of pcl::registration::CorrespondenceRejectorSampleConsensus (rules: include/icpgpu.h
// "sample-consensus rejector"; kernels: icp_reject_sac.hip): the core over m gathered pairs, the stage of the rejector chain that
// runs it on the keys the stages before it left, the call of its own over two host clouds and a pair list, and the fetch.
//
// The sequential RANSAC loop runs HERE, as the plane segmentation's does (icpgpu_sac.cpp), over counts the device takes 64
// hypotheses at a time.  Host waits of the core: ONE for m and the sample-distance moments, then TWO per batch the loop enters --
// the batch's 17-sum records come to the host, which solves them (solve_umeyama, the SCP section's arithmetic) and sends the float
// transforms back; the counts follow.  With m < 3 every hypothesis is INVALID by rule and no batch is launched.  Everything the
// core writes on the device is the rejector state's own (icpgpu_ctx::rsac).
#include "icp_ctx.h"
#include "icp_jacobi3.h"

namespace icpgpu_impl {
namespace {

// the smallest float32 that is not below t (t >= 0, finite): for every float32 f, f < it <=> (double)f < t
float image_not_below(double t) {
  float f = (float)t;
  if ((double)f < t) f = std::nextafterf(f, INFINITY);
  return f;
}

// SAMPLE DISTANCE's host half: the nine sums over n finite points -> sample_d2
double sample_distance2(const double S[9], double n) {
  const double mx = S[6] / n, my = S[7] / n, mz = S[8] / n;
  double a[3][3], V[3][3];
  a[0][0] = S[0] / n - mx * mx;
  a[0][1] = a[1][0] = S[1] / n - mx * my;
  a[0][2] = a[2][0] = S[2] / n - mx * mz;
  a[1][1] = S[3] / n - my * my;
  a[1][2] = a[2][1] = S[4] / n - my * mz;
  a[2][2] = S[5] / n - mz * mz;
  jacobi3(a, V);
  double e[3] = {a[0][0], a[1][1], a[2][2]};
  std::sort(e, e + 3);
  for (double& v : e)
    if (v < 0.0) v = 0.0;
  const double s = ((std::sqrt(e[0]) + std::sqrt(e[1])) + std::sqrt(e[2])) / 3.0;
  return s * s;
}

void reset(icpgpu_ctx::Rsac& K) {
  K.have = false;
  K.m = K.iterations = K.status = K.waits = 0;
  K.best_t = -1;
  K.n_kept = 0;
  K.sample_d2 = 0.0;
  for (double& v : K.moments) v = 0.0;
  for (int i = 0; i < 16; ++i) K.best_T[i] = i % 5 == 0 ? 1.f : 0.f;
  K.counts.clear();
  K.ranks.clear();
  K.transforms.clear();
}

int ensure_core(icpgpu_ctx* c, size_t m_cap) {
  auto& K = c->rsac;
  int rc;
  const size_t rows = std::max<size_t>(m_cap, 1);
  if ((rc = ensure(c, K.P, rows * sizeof(float4)))) return rc;
  if ((rc = ensure(c, K.Q, rows * sizeof(float4)))) return rc;
  if ((rc = ensure(c, K.rank, rows * sizeof(int)))) return rc;
  if ((rc = ensure_compaction(c, K.sel, rows))) return rc;
  if ((rc = ensure(c, K.ints, 4 * sizeof(int)))) return rc;
  if ((rc = ensure(c, K.sums, 14 * sizeof(double)))) return rc;
  if ((rc = ensure(c, K.models, sizeof(RsacModels)))) return rc;
  return ensure(c, K.batch, sizeof(RsacBatch));
}

// The core over the gathered pairs (K.P, K.Q): m, the sample distance, the loop.  m comes from the device (m_dev) or the caller.
// Leaves status, best_t, best_T, the per-hypothesis record and the waits; the flags are the caller's step.  *best_count: the
// best hypothesis' inliers (0 without one).
int rsac_core(icpgpu_ctx* c, int m_host, const int* m_dev, int m_cap, double inlier_threshold, int max_iterations, uint64_t seed, float* thr_out,
              int* best_count_out) {
  auto& K = c->rsac;
  int rc;
  double out[14];
  HIP_TRY(c, launch_rsac_moments(K.P.as<const float4>(), m_host, m_dev, m_cap, K.sums.as<double>(), c->stream));
  if ((rc = copy_to_host(c, out, K.sums.ptr, sizeof out))) return rc;
  ++K.waits;
  if (!(out[13] >= 0.0 && out[13] <= (double)m_cap && out[12] >= 0.0 && out[12] <= out[13]))
    return fail(c, ICPGPU_ERR_HIP, "sample-consensus rejector: %g pairs, %g finite, room for %d (internal error)", out[13], out[12], m_cap);
  const int m = (int)out[13];
  K.m = m;
  if (out[12] > 0.0) {
    for (int a = 0; a < 9; ++a) K.moments[a] = out[a];
    K.sample_d2 = sample_distance2(out, out[12]);
  }
  const float thr = image_not_below(inlier_threshold * inlier_threshold);
  *thr_out = thr;
  *best_count_out = 0;
  if (m == 0) {
    K.status = 0;
    return ICPGPU_OK;
  }
  int best_count = 0;
  if (m < 3) {  // no draw can be good: every hypothesis is INVALID and counts as an iteration
    K.iterations = max_iterations;
    K.counts.assign((size_t)max_iterations, -1);
    K.ranks.assign((size_t)max_iterations * 3, -1);
    K.transforms.assign((size_t)max_iterations * 16, 0.f);
  } else {
    RsacModels hm;
    RsacBatch hb;
    float Tf[kSacBatch][16];
    double k = INFINITY;
    int t = 0;
    for (;; ++t) {
      if (t >= max_iterations || (double)t >= k) break;
      const int h = t % kSacBatch;
      if (h == 0) {  // the loop goes on into the next batch: take it
        HIP_TRY(c, launch_rsac_models(K.P.as<const float4>(), K.Q.as<const float4>(), m, (unsigned long long)seed, t, max_iterations, K.sample_d2,
                                      K.models.as<RsacModels>(), c->stream));
        if ((rc = copy_to_host(c, &hm, K.models.ptr, sizeof hm))) return rc;
        ++K.waits;
        for (int l = 0; l < kSacBatch; ++l) {  // the host's half: a small SVD per good draw
          hb.count[l] = -1;
          for (float& v : hb.T[l].m) v = NAN;
          for (float& v : Tf[l]) v = 0.f;
          if (!hm.good[l]) continue;
          Mat4d Tk;
          if (!solve_umeyama(hm.sums[l], Tk)) continue;
          float f[16];
          mat4_to_float(Tk, f);
          bool finite = true;
          for (float v : f) finite = finite && std::isfinite(v);
          if (!finite) continue;
          std::memcpy(Tf[l], f, sizeof f);
          hb.T[l] = to_xform(f);
          hb.count[l] = 0;
        }
        HIP_TRY(c, hipMemcpyAsync(K.batch.ptr, &hb, sizeof hb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, launch_rsac_count(K.P.as<const float4>(), K.Q.as<const float4>(), m, thr, K.batch.as<RsacBatch>(), c->stream));
        if ((rc = copy_to_host(c, hb.count, K.batch.ptr, sizeof hb.count))) return rc;  // (count is the record's first member)
        ++K.waits;
      }
      const int cnt = hb.count[h];
      if (cnt < -1 || cnt > m) return fail(c, ICPGPU_ERR_HIP, "sample-consensus rejector: hypothesis %d counts %d of %d pairs (internal error)", t, cnt, m);
      K.counts.push_back(cnt);
      for (int a = 0; a < 3; ++a) K.ranks.push_back(hm.ranks[h][a]);
      K.transforms.insert(K.transforms.end(), Tf[h], Tf[h] + 16);
      if (cnt > 0 && cnt > best_count) {
        best_count = cnt;
        K.best_t = t;
        const double w = (double)cnt / (double)m;
        double p = 1.0 - w * w * w;
        p = std::max(p, DBL_EPSILON);
        p = std::min(p, 1.0 - DBL_EPSILON);
        k = std::log(1.0 - 0.99) / std::log(p);
      }
    }
    K.iterations = t;
  }
  if (K.best_t < 0) K.status = 1;
  else if (best_count < 3) K.status = 2;
  else {
    K.status = 3;
    std::memcpy(K.best_T, K.transforms.data() + (size_t)K.best_t * 16, 16 * sizeof(float));
  }
  *best_count_out = best_count;
  return ICPGPU_OK;
}

}  // namespace

int reject_sac_stage(icpgpu_ctx* c, unsigned long long* keys, float gate, const Xform& T, const icpgpu_rejector& r, unsigned int* stats) {
  auto& K = c->rsac;
  reset(K);
  const int n_s = (int)c->src.n, n_t = (int)c->tgt.n;
  HIP_TRY(c, hipMemsetAsync(stats, 0, (size_t)(kRejectStateInts - kRejectStats) * sizeof(unsigned int), c->stream));
  if (n_s <= 0 || n_t <= 0) {  // no pair: status 0, nothing launched, no wait
    K.have = true;
    return ICPGPU_OK;
  }
  int rc = ensure_core(c, (size_t)n_s);
  if (rc) return rc;
  HIP_TRY(c, launch_rsac_gather_keys(c->src.data(), n_s, c->tgt.data(), n_t, keys, gate, T, K.sel.flags.as<int>(), K.sel.pos.as<int>(),
                                     K.sel.scan.as<int>(), K.rank.as<int>(), K.ints.as<int>(), K.P.as<float4>(), K.Q.as<float4>(), c->stream));
  float thr = 0.f;
  int best_count = 0;
  if ((rc = rsac_core(c, 0, K.ints.as<const int>(), n_s, r.value, (int)r.min_correspondences, c->rsac_seed, &thr, &best_count))) return rc;
  if (K.m > 0)
    HIP_TRY(c, launch_rsac_flags(K.P.as<const float4>(), K.Q.as<const float4>(), K.rank.as<const int>(), K.m, to_xform(K.best_T), thr, K.status != 3,
                                 nullptr, keys, n_s, nullptr, stats, c->stream));
  K.n_kept = K.status == 3 ? (size_t)best_count : (size_t)K.m;
  K.have = true;
  return ICPGPU_OK;
}

}  // namespace icpgpu_impl

extern "C" {

int icpgpu_set_rejector_sac_seed(icpgpu_ctx* c, uint64_t seed) {
  if (!c) return fail(nullptr, ICPGPU_ERR_INVALID_ARG, "null context");
  c->rsac_seed = seed;
  return ICPGPU_OK;
}

int icpgpu_get_rejector_sac_seed(const icpgpu_ctx* c, uint64_t* seed) {
  if (!c || !seed) return ICPGPU_ERR_INVALID_ARG;
  *seed = c->rsac_seed;
  return ICPGPU_OK;
}

int icpgpu_correspondence_rejector_sample_consensus(icpgpu_ctx* c, const float* source_xyzw, size_t n_s, const float* target_xyzw, size_t n_t,
                                                    const int32_t* index_query, const int32_t* index_match, size_t n_pairs, double inlier_threshold,
                                                    int max_iterations, uint64_t seed, int32_t* kept, size_t* n_kept, float best_T16[16]) {
  ENTER(c);
  auto& K = c->rsac;
  reset(K);
  if (n_kept) *n_kept = 0;
  if (best_T16)
    for (int i = 0; i < 16; ++i) best_T16[i] = i % 5 == 0 ? 1.f : 0.f;
  const char* what = "correspondence_rejector_sample_consensus";
  if (!n_kept || !best_T16) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: null n_kept or best_T16", what);
  if ((n_s && !source_xyzw) || (n_t && !target_xyzw) || (n_pairs && (!index_query || !index_match)))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: null array against a non-zero size", what);
  if (!std::isfinite(inlier_threshold) || inlier_threshold < 0.0) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: inlier_threshold must be finite and >= 0", what);
  if (max_iterations < 0 || max_iterations > ICPGPU_RSAC_MAX_ITERATIONS)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: max_iterations %d outside 0..%d", what, max_iterations, ICPGPU_RSAC_MAX_ITERATIONS);
  const size_t most = (size_t)INT32_MAX - 4096;
  if (n_s > most || n_t > most || n_pairs > most) return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: too many points or pairs", what);
  for (size_t r = 0; r < n_pairs; ++r)
    if (index_query[r] < 0 || (size_t)index_query[r] >= n_s || index_match[r] < 0 || (size_t)index_match[r] >= n_t)
      return fail(c, ICPGPU_ERR_INVALID_ARG, "%s: pair %zu (%d, %d) names a point outside its cloud (%zu, %zu points)", what, r, (int)index_query[r],
                  (int)index_match[r], n_s, n_t);
  if (n_pairs == 0) {  // status 0: nothing launched, no wait
    K.have = true;
    return ICPGPU_OK;
  }
  const int m = (int)n_pairs;
  int rc = ensure_core(c, n_pairs);
  if (rc) return rc;
  if ((rc = ensure(c, K.source, n_s * sizeof(float4)))) return rc;
  if ((rc = ensure(c, K.target, n_t * sizeof(float4)))) return rc;
  if ((rc = ensure(c, K.iq, n_pairs * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, K.im, n_pairs * sizeof(int32_t)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(K.source.ptr, source_xyzw, n_s * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(K.target.ptr, target_xyzw, n_t * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(K.iq.ptr, index_query, n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(K.im.ptr, index_match, n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_rsac_gather_index(K.source.as<const float4>(), (int)n_s, K.target.as<const float4>(), (int)n_t, K.iq.as<const int32_t>(),
                                      K.im.as<const int32_t>(), m, K.P.as<float4>(), K.Q.as<float4>(), K.rank.as<int>(), c->stream));
  float thr = 0.f;
  int best_count = 0;
  if ((rc = rsac_core(c, m, nullptr, m, inlier_threshold, max_iterations, seed, &thr, &best_count))) return rc;
  const size_t expect = K.status == 3 ? (size_t)best_count : (size_t)m;
  if (kept) {  // the flags, and their number with them: one more wait
    int* d_kept = K.ints.as<int>() + 1;
    HIP_TRY(c, hipMemsetAsync(d_kept, 0, sizeof(int), c->stream));
    HIP_TRY(c, launch_rsac_flags(K.P.as<const float4>(), K.Q.as<const float4>(), K.rank.as<const int>(), m, to_xform(K.best_T), thr, K.status != 3,
                                 K.sel.flags.as<int>(), nullptr, 0, reinterpret_cast<unsigned int*>(d_kept), nullptr, c->stream));
    int got = -1;
    if ((rc = copy_to_host(c, kept, K.sel.flags.ptr, n_pairs * sizeof(int32_t), d_kept, 1, &got))) return rc;
    ++K.waits;
    if ((size_t)got != expect) return fail(c, ICPGPU_ERR_HIP, "%s: %d pairs flagged, %zu counted (internal error)", what, got, expect);
  }
  K.n_kept = expect;
  K.have = true;
  *n_kept = K.n_kept;
  std::memcpy(best_T16, K.best_T, sizeof K.best_T);
  return ICPGPU_OK;
}

int icpgpu_rejector_sac_fetch(icpgpu_ctx* c, size_t capacity_iterations, int32_t* m, double* sample_d2, double moments9[9], int32_t* iterations,
                              int32_t* status, int32_t* counts, int32_t* ranks, float* transforms, int32_t* best_t, float best_T16[16], size_t* n_kept,
                              int32_t* host_waits) {
  if (!c) return fail(nullptr, ICPGPU_ERR_INVALID_ARG, "null context");
  const auto& K = c->rsac;
  if (!K.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "rejector_sac_fetch: no result (a chain with a sample-consensus stage, or icpgpu_correspondence_rejector_sample_consensus)");
  const size_t it = (size_t)K.iterations;
  if ((counts || ranks || transforms) && it > capacity_iterations)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "rejector_sac_fetch: %zu iterations, room for %zu", it, capacity_iterations);
  if (m) *m = K.m;
  if (sample_d2) *sample_d2 = K.sample_d2;
  if (moments9)
    for (int a = 0; a < 9; ++a) moments9[a] = K.moments[a];
  if (iterations) *iterations = K.iterations;
  if (status) *status = K.status;
  if (it) {
    if (counts) std::memcpy(counts, K.counts.data(), it * sizeof(int32_t));
    if (ranks) std::memcpy(ranks, K.ranks.data(), it * 3 * sizeof(int32_t));
    if (transforms) std::memcpy(transforms, K.transforms.data(), it * 16 * sizeof(float));
  }
  if (best_t) *best_t = K.best_t;
  if (best_T16) std::memcpy(best_T16, K.best_T, sizeof K.best_T);
  if (n_kept) *n_kept = K.n_kept;
  if (host_waits) *host_waits = K.waits;
  return ICPGPU_OK;
}

}  // extern "C"
