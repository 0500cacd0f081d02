// icpgpu_reject.cpp -- the correspondence rejectors' host side (PCL: Registration::addCorrespondenceRejector and
// CorrespondenceRejectorMedianDistance / Trimmed / OneToOne) and that of reciprocal correspondences (setUseReciprocalCorrespondences):
// the context's chain and flag, the gated key-writing search they run behind, the reciprocal stage's launch (icp_reciprocal.hip), the
// chain's (icp_reject.hip), the point-to-point sweep with either, and the entry points that show what they keep
// (icpgpu_correspondences, icpgpu_rejector_stats, icpgpu_reciprocal_stats).  An iteration on the keys path is search -> reciprocal
// stage -> chain stages -> the method's keys reduction, queued back to back: nothing of the stages is read by the host until the
// alignment ends (reject_fetch_stats: one posted read-back of the last iteration's statistics through the result mailbox).  The one
// exception is a sample-consensus stage (kind 5; icpgpu_reject_sac.cpp), whose loop runs on the host and waits inside the iteration:
// reject_run_chain queues the device's stages run by run around it.
#include "icp_ctx.h"

namespace icpgpu_impl {

// keys of T * source (the caller's order) in the target, exact wherever d2 <= thr: the gated grid search, or the brute-force keys
int gated_keys(icpgpu_ctx* c, const Xform& T, float thr, unsigned long long* keys) {
  const int n_s = (int)c->src.n, n_t = (int)c->tgt.n;
  if (n_s <= 0) return ICPGPU_OK;
  if (grid_ready(c)) {
    unsigned int* prev = nullptr;  // each iteration's neighbours bound the next one's search
    bool use_prev = false;
    int rc = prev_neighbours(c, c->grid, c->src.data(), n_s, grid_flags(c->grid, false), prev, use_prev);
    if (rc) return rc;
    HIP_TRY(c, launch_nn_grid_search(c->src.data(), n_s, grid_flags(c->grid, false), T, static_cast<const float4*>(c->grid.sorted.ptr),
                                     static_cast<const int*>(c->grid.cell_start.ptr), c->grid.g, thr, keys, nullptr, nullptr, nullptr,
                                     c->stream, prev, use_prev));
    c->prof.grid_launches += 1;
    c->prof.grid_bytes += 16ull * ((uint64_t)n_s + (uint64_t)n_t) + 8ull * (uint64_t)n_s;
    return ICPGPU_OK;
  }
  c->prof.nn_launches += 1;
  c->prof.nn_pairs += (uint64_t)n_s * (uint64_t)n_t;
  c->prof.nn_bytes += 16ull * ((uint64_t)n_s + (uint64_t)n_t) + 8ull * (uint64_t)n_s;
  return nn_keys_brute(c, c->tgt.data(), n_t, T, keys);
}

// The reciprocal stage over the keys of T * source (flag off: nothing).  Where the forward search used the target's grid the
// transformed source is binned into that grid's lattice; otherwise every winner is tested against the whole source.  Everything
// is queued: the stage reads nothing back.
int reciprocal_run(icpgpu_ctx* c, const Xform& T, unsigned long long* keys, float thr) {
  if (!c->reciprocal) return ICPGPU_OK;
  const int n_s = (int)c->src.n, n_t = (int)c->tgt.n;
  if (n_s <= 0 || n_t <= 0) return ICPGPU_OK;  // (no pair: the statistics read as zeroes)
  int rc = ensure(c, c->rcp_state, kRecipStateInts * sizeof(unsigned int));
  if (rc) return rc;
  if ((rc = ensure(c, c->rej_winners, (size_t)n_t * sizeof(unsigned long long)))) return rc;  // (shared with one-to-one: stages run one after the other)
  auto* state = static_cast<unsigned int*>(c->rcp_state.ptr);
  auto* winners = static_cast<unsigned long long*>(c->rej_winners.ptr);
  if (grid_ready(c)) {
    const GridDesc& g = c->grid.g;
    const size_t table = reciprocal_cells(g) + 1;
    if ((rc = ensure(c, c->rcp_counts, table * sizeof(int)))) return rc;
    if ((rc = ensure(c, c->rcp_cell_start, table * sizeof(int)))) return rc;
    if ((rc = ensure(c, c->rcp_scan, exclusive_scan_scratch_ints((int)table) * sizeof(int)))) return rc;
    if ((rc = ensure(c, c->rcp_cell_of_point, (size_t)n_s * sizeof(int)))) return rc;
    if ((rc = ensure(c, c->rcp_rank, (size_t)n_s * sizeof(int)))) return rc;
    if ((rc = ensure(c, c->rcp_binned, (size_t)n_s * sizeof(float4)))) return rc;
    HIP_TRY(c, launch_reciprocal_grid(c->src.data(), n_s, c->tgt.data(), n_t, T, thr, keys, g, static_cast<int*>(c->rcp_counts.ptr),
                                      static_cast<int*>(c->rcp_cell_start.ptr), static_cast<int*>(c->rcp_scan.ptr),
                                      static_cast<int*>(c->rcp_cell_of_point.ptr), static_cast<int*>(c->rcp_rank.ptr),
                                      static_cast<float4*>(c->rcp_binned.ptr), winners, state, c->stream));
  } else {
    HIP_TRY(c, launch_reciprocal_brute(c->src.data(), n_s, c->tgt.data(), n_t, T, thr, keys, winners, state, c->stream));
  }
  c->rcp_ran = true;
  return ICPGPU_OK;
}

static bool chain_reads_normals(const icpgpu_ctx* c) {
  for (int s = 0; s < c->n_rejectors; ++s)
    if (c->rejectors[s].kind == ICPGPU_REJECT_SURFACE_NORMAL) return true;
  return false;
}

// both clouds' normals for a surface-normal stage: the caller's or the estimate (cached per cloud version: the first call pays).
// Without a pair (an empty cloud) the stage reads none.
static int chain_normals(icpgpu_ctx* c, const float4** src_normals, const float4** tgt_normals) {
  *src_normals = *tgt_normals = nullptr;
  if (!chain_reads_normals(c) || c->src.n == 0 || c->tgt.n == 0) return ICPGPU_OK;
  const int rc = ensure_normals(c, /*of_target=*/false, src_normals);
  return rc ? rc : ensure_normals(c, /*of_target=*/true, tgt_normals);
}

int reject_prepare(icpgpu_ctx* c) {
  const float4 *a, *b;
  return chain_normals(c, &a, &b);
}

int reject_run_chain(icpgpu_ctx* c, unsigned long long* keys, float thr, const Xform& T) {
  const int n = c->n_rejectors;
  if (n <= 0) return ICPGPU_OK;
  const int n_s = (int)c->src.n, n_t = (int)c->tgt.n;
  RejectStage stages[kRejectMaxStages];
  bool winners = false;
  const float4 *src_normals, *tgt_normals;
  int rc = chain_normals(c, &src_normals, &tgt_normals);  // (cached by reject_prepare: nothing is launched here)
  if (rc) return rc;
  for (int s = 0; s < n; ++s) {
    const icpgpu_rejector& r = c->rejectors[s];
    stages[s].kind = r.kind;
    stages[s].min_corr = (unsigned int)r.min_correspondences;
    stages[s].ratio = (float)r.value;
    stages[s].factor = r.value;
    winners = winners || r.kind == ICPGPU_REJECT_ONE_TO_ONE;
  }
  if ((rc = ensure(c, c->rej_state, (size_t)kRejectMaxStages * kRejectStateInts * sizeof(unsigned int)))) return rc;
  if (winners && (rc = ensure(c, c->rej_winners, (size_t)(n_t ? n_t : 1) * sizeof(unsigned long long)))) return rc;
  // The device's stages are queued run by run around the sample-consensus stages, which are the host's (icpgpu_reject_sac.cpp: they
  // wait); `state` is offset per stage.  Without such a stage this is one call over the whole chain, as before the stage existed.
  auto* state = static_cast<unsigned int*>(c->rej_state.ptr);
  int first = 0;
  for (int s = 0; s <= n; ++s) {
    if (s < n && stages[s].kind != kRejectSampleConsensus) continue;
    if (s > first)
      HIP_TRY(c, launch_reject_chain(keys, n_s, n_t, thr, stages + first, s - first, state + (size_t)first * kRejectStateInts,
                                     static_cast<unsigned long long*>(c->rej_winners.ptr), c->stream, src_normals, tgt_normals, &T));
    if (s < n && (rc = reject_sac_stage(c, keys, thr, T, c->rejectors[s], state + (size_t)s * kRejectStateInts + kRejectStats))) return rc;
    first = s + 1;
  }
  c->rej_ran = n;
  return ICPGPU_OK;
}

int correspondence_keys(icpgpu_ctx* c, const Xform& T, float thr, unsigned long long* keys) {
  int rc = gated_keys(c, T, thr, keys);
  if (rc) return rc;
  if ((rc = reciprocal_run(c, T, keys, thr))) return rc;
  return reject_run_chain(c, keys, thr, T);
}

// the statistics of the last run of the chain and of the reciprocal stage -> c->rej_stats, c->rcp_stats (zeroes for whichever has
// not run since they were last taken); one read-back for both
int reject_fetch_stats(icpgpu_ctx* c) {
  std::memset(c->rej_stats, 0, sizeof c->rej_stats);
  c->rej_stats_n = c->n_rejectors;
  c->rcp_stats[0] = c->rcp_stats[1] = 0;
  const int n = c->rej_ran > 0 ? c->rej_ran : 0;
  const bool rcp = c->rcp_ran;
  if (n <= 0 && !rcp) return ICPGPU_OK;
  c->rej_ran = 0;
  c->rcp_ran = false;
  if ((int)c->rej_stats_n < n) c->rej_stats_n = n;
  int rc = ensure(c, c->rej_post, ((size_t)kRejectMaxStages * 3 + 2) * sizeof(int));
  if (rc) return rc;
  for (int s = 0; s < n; ++s)
    HIP_TRY(c, hipMemcpyAsync(static_cast<int*>(c->rej_post.ptr) + 3 * s,
                              static_cast<const unsigned int*>(c->rej_state.ptr) + (size_t)s * kRejectStateInts + kRejectStats, 3 * sizeof(int),
                              hipMemcpyDeviceToDevice, c->stream));
  if (rcp)
    HIP_TRY(c, hipMemcpyAsync(static_cast<int*>(c->rej_post.ptr) + 3 * n, c->rcp_state.ptr, 2 * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  int h[kRejectMaxStages * 3 + 2];
  if ((rc = fetch_ints(c, static_cast<const int*>(c->rej_post.ptr), 3 * n + (rcp ? 2 : 0), h))) return rc;
  for (int s = 0; s < n; ++s) {
    c->rej_stats[s].pairs_in = (uint32_t)h[3 * s];
    c->rej_stats[s].pairs_out = (uint32_t)h[3 * s + 1];
    c->rej_stats[s].cut_bits = (uint32_t)h[3 * s + 2];
  }
  if (rcp) {
    c->rcp_stats[0] = (uint32_t)h[3 * n];
    c->rcp_stats[1] = (uint32_t)h[3 * n + 1];
  }
  return ICPGPU_OK;
}

// sweep_issue's counterpart for a context with a chain or the reciprocal flag (gated sweeps only): the key-writing search over the
// source in the caller's order (one-to-one and reciprocal break ties on the caller's source index), the reciprocal stage, the chain,
// reduce_kernel over the keys that are left
int sweep_issue_rejected(icpgpu_ctx* c, const Xform& T, float thr, SweepTicket& tk) {
  const int n_s = (int)c->src.n;
  int rc = ensure(c, c->keys, (size_t)(n_s ? n_s : 1) * sizeof(unsigned long long));
  if (rc) return rc;
  auto* keys = static_cast<unsigned long long*>(c->keys.ptr);
  if ((rc = reject_prepare(c))) return rc;
  if ((rc = correspondence_keys(c, T, thr, keys))) return rc;
  if ((rc = ensure(c, c->partials, (size_t)kMaxReduceBlocks * kReduceTerms * sizeof(double)))) return rc;
  const unsigned long long seq = ++c->sums_seq;
  HIP_TRY(c, launch_reduce(c->src.data(), n_s, c->tgt.data(), keys, T, thr, static_cast<double*>(c->partials.ptr), c->h_sums_dev,
                           c->h_flags_dev, wire_seq(c, seq), c->stream));
  c->call_sweeps += 1;
  c->prof.reduce_launches += 1;
  c->prof.reduce_bytes += 40ull * (uint64_t)n_s + 136;
  tk = SweepTicket{};
  tk.seq = seq;
  tk.red_src = c->src.data();
  tk.red_n = n_s;
  tk.T = T;
  tk.thr = thr;
  return ICPGPU_OK;
}

static bool rejector_valid(const icpgpu_rejector& r) {
  switch (r.kind) {
    case ICPGPU_REJECT_MEDIAN_DISTANCE: return std::isfinite(r.value) && r.value >= 0.0;
    case ICPGPU_REJECT_TRIMMED: return r.value >= 0.0 && r.value <= 1.0 && r.min_correspondences >= 0;
    case ICPGPU_REJECT_ONE_TO_ONE: return true;
    case ICPGPU_REJECT_SURFACE_NORMAL: return std::isfinite(r.value);
    case ICPGPU_REJECT_SAMPLE_CONSENSUS:
      return std::isfinite(r.value) && r.value >= 0.0 && r.min_correspondences >= 1 && r.min_correspondences <= ICPGPU_RSAC_MAX_ITERATIONS;
    default: return false;
  }
}

}  // namespace icpgpu_impl

extern "C" {

int icpgpu_set_correspondence_rejectors(icpgpu_ctx* c, const icpgpu_rejector* rejectors, size_t n) {
  if (!c) return fail(nullptr, ICPGPU_ERR_INVALID_ARG, "null context");
  if (n > (size_t)ICPGPU_MAX_REJECTORS) return fail(c, ICPGPU_ERR_INVALID_ARG, "set_correspondence_rejectors: %zu rejectors (at most %d)", n, ICPGPU_MAX_REJECTORS);
  if (n && !rejectors) return fail(c, ICPGPU_ERR_INVALID_ARG, "set_correspondence_rejectors: null rejectors");
  for (size_t s = 0; s < n; ++s)
    if (!rejector_valid(rejectors[s]))
      return fail(c, ICPGPU_ERR_INVALID_ARG, "set_correspondence_rejectors: rejector %zu (kind %d, value %g, min_correspondences %d) is not valid", s,
                  (int)rejectors[s].kind, rejectors[s].value, (int)rejectors[s].min_correspondences);
  for (size_t s = 0; s < n; ++s) c->rejectors[s] = rejectors[s];
  c->n_rejectors = (int)n;
  return ICPGPU_OK;
}

int icpgpu_get_correspondence_rejectors(const icpgpu_ctx* c, icpgpu_rejector* out, size_t* n) {
  if (!c || !n) return ICPGPU_ERR_INVALID_ARG;
  *n = (size_t)c->n_rejectors;
  if (out)
    for (int s = 0; s < c->n_rejectors; ++s) out[s] = c->rejectors[s];
  return ICPGPU_OK;
}

int icpgpu_set_reciprocal_correspondences(icpgpu_ctx* c, int on) {
  if (!c) return fail(nullptr, ICPGPU_ERR_INVALID_ARG, "null context");
  c->reciprocal = on != 0;
  return ICPGPU_OK;
}

int icpgpu_get_reciprocal_correspondences(const icpgpu_ctx* c, int* on) {
  if (!c || !on) return ICPGPU_ERR_INVALID_ARG;
  *on = c->reciprocal ? 1 : 0;
  return ICPGPU_OK;
}

int icpgpu_reciprocal_stats(const icpgpu_ctx* c, uint32_t* pairs_in, uint32_t* pairs_out) {
  if (!c) return ICPGPU_ERR_INVALID_ARG;
  if (pairs_in) *pairs_in = c->rcp_stats[0];
  if (pairs_out) *pairs_out = c->rcp_stats[1];
  return ICPGPU_OK;
}

int icpgpu_correspondences(icpgpu_ctx* c, const float* T, int32_t* idx, float* d2) {
  ENTER(c);
  if (!c->src.set || !c->tgt.set) return fail(c, ICPGPU_ERR_NO_INPUT, "correspondences: source and target must be set first");
  const int n_s = (int)c->src.n;
  if (n_s && (!idx || !d2)) return fail(c, ICPGPU_ERR_INVALID_ARG, "null output");
  int rc = ensure(c, c->keys, (size_t)(n_s ? n_s : 1) * sizeof(unsigned long long));
  if (rc) return rc;
  if ((rc = ensure(c, c->idx, (size_t)(n_s ? n_s : 1) * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c, c->d2, (size_t)(n_s ? n_s : 1) * sizeof(float)))) return rc;
  const float thr = gate_threshold(c);
  auto* keys = static_cast<unsigned long long*>(c->keys.ptr);
  c->prev.valid = false;  // (as an alignment's first iteration: nothing carried over)
  c->rcp_ran = false;
  const Xform X = T ? to_xform(T) : to_xform(mat4_identity());
  if (c->tgt.n == 0) {  // no search and no reciprocal stage: every key empty, and the chain over them
    HIP_TRY(c, launch_fill_keys(keys, n_s, c->stream));
    if ((rc = reject_run_chain(c, keys, thr, X))) return rc;
  } else {
    if ((rc = reject_prepare(c))) return rc;
    if ((rc = ensure_grid(c, thr))) return rc;
    if ((rc = correspondence_keys(c, X, thr, keys))) return rc;
  }
  HIP_TRY(c, launch_reject_unpack(keys, n_s, thr, static_cast<int32_t*>(c->idx.ptr), static_cast<float*>(c->d2.ptr), c->stream));
  if (n_s) {
    HIP_TRY(c, hipMemcpyAsync(idx, c->idx.ptr, (size_t)n_s * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d2, c->d2.ptr, (size_t)n_s * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return reject_fetch_stats(c);
}

int icpgpu_rejector_stats(const icpgpu_ctx* c, size_t capacity, uint32_t* pairs_in, uint32_t* pairs_out, float* cut, size_t* n_stages) {
  if (!c || !n_stages) return ICPGPU_ERR_INVALID_ARG;
  *n_stages = c->rej_stats_n;
  if (c->rej_stats_n > capacity) return ICPGPU_OK;
  for (size_t s = 0; s < c->rej_stats_n; ++s) {
    if (pairs_in) pairs_in[s] = c->rej_stats[s].pairs_in;
    if (pairs_out) pairs_out[s] = c->rej_stats[s].pairs_out;
    if (cut) std::memcpy(&cut[s], &c->rej_stats[s].cut_bits, sizeof(float));
  }
  return ICPGPU_OK;
}

}  // extern "C"
