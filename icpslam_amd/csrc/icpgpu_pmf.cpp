// icpgpu_pmf.cpp -- host side of the ground filter (pcl::applyMorphologicalOperator, pcl::ProgressiveMorphologicalFilter and
// pcl::ExtractIndices over its result; rules: include/icpgpu.h "ground filter"; kernels: icp_morph.hip).
//
// The schedule of windows and thresholds is worked out HERE before anything is launched; the passes are then queued back to back.  The
// ground set's size stays on the device between passes (every launch is sized by n, the kernels read the live count), so a call waits
// for the device once, whatever the number of passes.  Everything the calls write on the device is the filter state's own
// (icpgpu_ctx::pmf), so no other call's result meets it.
#include "icp_ctx.h"

namespace icpgpu_impl {
namespace {

// extract's loop: (window, threshold) per pass.  < 0: refused (the message is in place)
int pmf_schedule(icpgpu_ctx* c, float max_window, float slope, float initial_distance, float max_distance, float cell, float base, bool exponential,
                 std::vector<float>& windows, std::vector<float>& thresholds) {
  windows.clear();
  thresholds.clear();
  float window = 0.f, previous = 0.f;
  double B = 1.0;  // base^it
  for (int it = 0; window < max_window; ++it) {
    if (it >= ICPGPU_PMF_MAX_PASSES)
      return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: the schedule has more than %d passes", ICPGPU_PMF_MAX_PASSES);
    previous = window;
    if (exponential) {
      window = (float)((double)cell * (2.0 * B + 1.0));
      B *= (double)base;
    } else {
      window = cell * (2.0f * (float)(it + 1) * base + 1.0f);
    }
    if (!std::isfinite(window)) return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: pass %d has a window that is not finite", it);
    float thr = it == 0 ? initial_distance : slope * (window - previous) * cell + initial_distance;
    if (thr > max_distance) thr = max_distance;
    windows.push_back(window);
    thresholds.push_back(thr);
  }
  return ICPGPU_OK;
}

int ensure_binning(icpgpu_ctx* c, size_t n) {
  auto& P = c->pmf;
  int rc;
  if ((rc = ensure(c, P.ints, 8 * sizeof(int)))) return rc;
  if ((rc = ensure(c, P.grid, sizeof(MorphGrid)))) return rc;
  if ((rc = ensure(c, P.table, kMorphTableInts * sizeof(int)))) return rc;
  if ((rc = ensure(c, P.cell_start, ((size_t)kMorphMaxCells + 1) * sizeof(int)))) return rc;
  if ((rc = ensure(c, P.scan, exclusive_scan_scratch_ints(kMorphMaxCells + 1) * sizeof(int)))) return rc;
  if ((rc = ensure(c, P.sxy, n * sizeof(float2)))) return rc;
  for (DeviceBuf* b : {&P.cellid, &P.sval, &P.va, &P.vb, &P.sidx, &P.scell})
    if ((rc = ensure(c, *b, n * sizeof(int)))) return rc;
  return ICPGPU_OK;
}

// One operator over the active set act[0 .. *d_count) of the search cloud, queued: a binning for `window`, one box pass (ERODE, DILATE)
// or two (OPEN, CLOSE).  *result: the operator's output in the binning's sorted order (pmf.sval: the points' z, pmf.sidx: their indices).
int queue_operator(icpgpu_ctx* c, const int* act, const int* d_count, float window, int op, unsigned long long* tests, const float** result) {
  auto& P = c->pmf;
  const auto& S = c->search;
  const int ni = (int)S.n;
  const bool first_max = op == ICPGPU_MORPH_DILATE || op == ICPGPU_MORPH_CLOSE;
  const bool two = op == ICPGPU_MORPH_OPEN || op == ICPGPU_MORPH_CLOSE;
  const MorphGrid* grid = P.grid.as<MorphGrid>();
  HIP_TRY(c, launch_morph_bin(S.cloud.data(), ni, act, d_count, P.ints.as<unsigned int>(), window, P.grid.as<MorphGrid>(), P.table.as<int>(),
                              P.cell_start.as<int>(), P.scan.as<int>(), P.cellid.as<int>(), P.sxy.as<float2>(), P.sval.as<float>(), P.sidx.as<int>(),
                              P.scell.as<int>(), first_max, c->stream));
  HIP_TRY(c, launch_morph_box(ni, d_count, grid, window, P.sxy.as<float2>(), P.cell_start.as<int>(), P.scell.as<int>(), P.sval.as<float>(),
                              P.table.as<int>(), 0, first_max, two, P.va.as<float>(), tests, c->stream));
  *result = P.va.as<float>();
  if (two) {
    HIP_TRY(c, launch_morph_box(ni, d_count, grid, window, P.sxy.as<float2>(), P.cell_start.as<int>(), P.scell.as<int>(), P.va.as<float>(),
                                P.table.as<int>(), 1, !first_max, false, P.vb.as<float>(), tests, c->stream));
    *result = P.vb.as<float>();
  }
  return ICPGPU_OK;
}

constexpr int kPmfLiveCount = 4, kPmfExtractCount = 5;  // pmf.ints: [0, 4) the xy box
constexpr int kPmfMaxPasses = ICPGPU_PMF_MAX_PASSES;  // (by this name inside HIP_TRY, whose message quotes its expression)
constexpr int kPmfAfterInts = kPmfMaxPasses + 2;  // pmf.after: the ground's size after each pass, then the point tests (64 bits)

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_morphological_operator(icpgpu_ctx* c, double resolution, int op, float* out_z) {
  ENTER(c);
  auto& S = c->search;
  auto& P = c->pmf;
  P.ran = false;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "morphological_operator: no search cloud (icpgpu_search_set_input)");
  const float window = (float)resolution;
  if (!std::isfinite(window) || !(window > 0.f)) return fail(c, ICPGPU_ERR_INVALID_ARG, "morphological_operator: resolution must be finite and > 0");
  if (op < ICPGPU_MORPH_ERODE || op > ICPGPU_MORPH_CLOSE) return fail(c, ICPGPU_ERR_INVALID_ARG, "morphological_operator: operator %d outside 0..3", op);
  if (!out_z) return fail(c, ICPGPU_ERR_INVALID_ARG, "morphological_operator: null output pointer");
  const size_t n = S.n;
  const int ni = (int)n;
  P.waits = 0;
  if (n > 0) {
    int rc;
    if ((rc = ensure_binning(c, n))) return rc;
    if ((rc = ensure_compaction(c, P.op, n))) return rc;
    if ((rc = ensure(c, P.out_z, n * sizeof(float)))) return rc;
    const Compaction& A = P.op;
    int* d_count = P.ints.as<int>() + kPmfLiveCount;
    const float* result = nullptr;
    HIP_TRY(c, launch_morph_init(S.cloud.data(), ni, A.flags.as<int>(), nullptr, P.out_z.as<float>(), P.ints.as<unsigned int>(), c->stream));
    HIP_TRY(c, launch_compact(A.flags.as<int>(), ni, A.pos.as<int>(), A.scan.as<int>(), A.kept.as<int>(), d_count, nullptr, nullptr, c->stream));
    if ((rc = queue_operator(c, A.kept.as<int>(), d_count, window, op, nullptr, &result))) return rc;
    HIP_TRY(c, launch_morph_unsort(ni, d_count, result, P.sidx.as<int>(), P.out_z.as<float>(), c->stream));
    if ((rc = copy_to_host(c, out_z, P.out_z.ptr, n * sizeof(float)))) return rc;
    ++P.waits;
  }
  P.ran = true;
  return ICPGPU_OK;
}

int icpgpu_progressive_morphological_filter(icpgpu_ctx* c, int max_window_size, double slope, double initial_distance, double max_distance,
                                            double cell_size, double base, int exponential, size_t* n_ground, int32_t* n_passes) {
  ENTER(c);
  auto& S = c->search;
  auto& P = c->pmf;
  P.have = P.ran = false;
  if (n_ground) *n_ground = 0;
  if (n_passes) *n_passes = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: no search cloud (icpgpu_search_set_input)");
  // PCL's setters take floats: every parameter is rounded once
  const float slope_f = (float)slope, initial_f = (float)initial_distance, max_f = (float)max_distance, cell_f = (float)cell_size, base_f = (float)base;
  if (!std::isfinite(slope_f) || !std::isfinite(initial_f) || !std::isfinite(max_f) || !std::isfinite(cell_f) || !std::isfinite(base_f))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: every parameter must be finite as a float");
  if (!(cell_f > 0.f)) return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: cell_size must be > 0");
  if (slope_f < 0.f || initial_f < 0.f || max_f < 0.f)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: slope, initial_distance and max_distance must be >= 0");
  if (exponential ? !(base_f > 1.f) : !(base_f > 0.f))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: base must be > 1 (exponential) or > 0 (linear)");
  int rc;
  if ((rc = pmf_schedule(c, (float)max_window_size, slope_f, initial_f, max_f, cell_f, base_f, exponential != 0, P.windows, P.thresholds))) return rc;
  if (!n_ground || !n_passes) return fail(c, ICPGPU_ERR_INVALID_ARG, "progressive_morphological_filter: null output pointer");

  const size_t n = S.n;
  const int ni = (int)n, np = (int)P.windows.size();
  P.n = n;
  P.n_ground = 0;
  P.waits = 0;
  P.ground_after.assign((size_t)np, 0);
  P.tests_total = 0;
  if (n > 0) {
    if ((rc = ensure_binning(c, n))) return rc;
    if ((rc = ensure_compaction(c, P.sel, n))) return rc;
    if ((rc = ensure(c, P.removed_at, n * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, P.after, kPmfAfterInts * sizeof(int)))) return rc;
    if ((rc = ensure(c, P.tests, (size_t)kMorphTestSlots * kMorphTestStride * sizeof(unsigned long long)))) return rc;
    const Compaction& G = P.sel;
    int* d_count = P.ints.as<int>() + kPmfLiveCount;
    unsigned long long* tests = P.tests.as<unsigned long long>();
    // the ground starts as every finite point
    HIP_TRY(c, launch_morph_init(S.cloud.data(), ni, G.flags.as<int>(), P.removed_at.as<int32_t>(), nullptr, P.ints.as<unsigned int>(), c->stream));
    HIP_TRY(c, launch_compact(G.flags.as<int>(), ni, G.pos.as<int>(), G.scan.as<int>(), G.kept.as<int>(), d_count, nullptr, nullptr, c->stream));
    if (np > 0) HIP_TRY(c, hipMemsetAsync(tests, 0, (size_t)kMorphTestSlots * kMorphTestStride * sizeof(unsigned long long), c->stream));
    for (int pass = 0; pass < np; ++pass) {
      const float* opened = nullptr;
      if ((rc = queue_operator(c, G.kept.as<int>(), d_count, P.windows[(size_t)pass], ICPGPU_MORPH_OPEN, tests, &opened))) return rc;
      HIP_TRY(c, launch_morph_judge(ni, d_count, P.sval.as<float>(), opened, P.sidx.as<int>(), P.thresholds[(size_t)pass], pass, G.flags.as<int>(),
                                    P.removed_at.as<int32_t>(), c->stream));
      // (the judged flags of the points that left earlier are the zeros they left with)
      HIP_TRY(c, launch_compact(G.flags.as<int>(), ni, G.pos.as<int>(), G.scan.as<int>(), G.kept.as<int>(), d_count, nullptr, nullptr, c->stream));
      HIP_TRY(c, hipMemcpyAsync(P.after.as<int>() + pass, d_count, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    }
    if (np > 0) {
      int after[kPmfAfterInts];
      HIP_TRY(c, launch_morph_tests_total(tests, reinterpret_cast<unsigned long long*>(P.after.as<int>() + kPmfMaxPasses), c->stream));
      if ((rc = copy_to_host(c, after, P.after.ptr, sizeof after))) return rc;
      ++P.waits;
      int before = S.n_finite;
      for (int pass = 0; pass < np; ++pass) {
        if (after[pass] < 0 || after[pass] > before)
          return fail(c, ICPGPU_ERR_HIP, "progressive_morphological_filter: %d ground points after pass %d, %d before (internal error)", after[pass], pass,
                      before);
        P.ground_after[(size_t)pass] = before = after[pass];
      }
      std::memcpy(&P.tests_total, after + kPmfMaxPasses, sizeof P.tests_total);
      P.n_ground = (size_t)before;
    } else {
      P.n_ground = (size_t)S.n_finite;  // (no pass: the ground is every finite point, whose number the search cloud knows)
    }
  }
  P.have = P.ran = true;
  *n_ground = P.n_ground;
  *n_passes = np;
  return ICPGPU_OK;
}

int icpgpu_pmf_fetch(icpgpu_ctx* c, size_t capacity_ground, size_t capacity_passes, int32_t* ground, float* window_sizes, float* height_thresholds,
                     int32_t* ground_after, int32_t* removed_at) {
  ENTER(c);
  const auto& P = c->pmf;
  if (!P.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "pmf_fetch: no result (icpgpu_progressive_morphological_filter)");
  const size_t np = P.windows.size();
  if (P.n_ground > capacity_ground || np > capacity_passes)
    return fail(c, ICPGPU_ERR_INVALID_ARG, "pmf_fetch: %zu ground points and %zu passes, room for %zu and %zu", P.n_ground, np, capacity_ground,
                capacity_passes);
  const Delivery parts[2] = {{ground, P.sel.kept.ptr, ground ? P.n_ground * sizeof(int32_t) : 0},
                             {removed_at, P.removed_at.ptr, removed_at ? P.n * sizeof(int32_t) : 0}};
  const int rc = deliver(c, parts, 2);
  if (rc) return rc;
  if (window_sizes && np) std::memcpy(window_sizes, P.windows.data(), np * sizeof(float));
  if (height_thresholds && np) std::memcpy(height_thresholds, P.thresholds.data(), np * sizeof(float));
  if (ground_after && np) std::memcpy(ground_after, P.ground_after.data(), np * sizeof(int32_t));
  return ICPGPU_OK;
}

int icpgpu_pmf_stats(const icpgpu_ctx* c, int32_t* host_waits, uint64_t* point_tests) {
  if (!c || !c->pmf.ran) return ICPGPU_ERR_INVALID_ARG;
  if (host_waits) *host_waits = c->pmf.waits;
  if (point_tests) *point_tests = c->pmf.have ? c->pmf.tests_total : 0;
  return ICPGPU_OK;
}

}  // extern "C"

namespace icpgpu_impl {
namespace {

// pcl::ExtractIndices over the last filter result: the cloud's points in (negative = 0) or not in (1) the ground, in cloud order, written
// by the compaction's last kernel into the pinned staging buffer.  One wait: the count.
int pmf_extract(icpgpu_ctx* c, int negative, float* out_xyzw, const float** view_xyzw, bool view, size_t* n_out) {
  auto& S = c->search;
  auto& P = c->pmf;
  if (view && view_xyzw) *view_xyzw = nullptr;
  if (n_out) *n_out = 0;
  if (!n_out || (view && !view_xyzw)) return fail(c, ICPGPU_ERR_INVALID_ARG, "pmf_extract: null argument");
  if (!P.have || !S.set || P.n != S.n) return fail(c, ICPGPU_ERR_INVALID_ARG, "pmf_extract: no result (icpgpu_progressive_morphological_filter)");
  const size_t n = P.n, want = negative ? n - P.n_ground : P.n_ground;
  if (want == 0) return ICPGPU_OK;
  const int ni = (int)n;
  int rc;
  Compaction& C = P.ext;
  if ((rc = ensure_compaction(c, C, n))) return rc;
  if ((rc = ensure_stage(c, want * sizeof(float4), /*any_size=*/true))) return rc;
  int* d_count = P.ints.as<int>() + kPmfExtractCount;
  HIP_TRY(c, launch_pmf_flags(P.removed_at.as<int32_t>(), ni, negative != 0, C.flags.as<int>(), c->stream));
  HIP_TRY(c, launch_compact(C.flags.as<int>(), ni, C.pos.as<int>(), C.scan.as<int>(), C.kept.as<int>(), d_count, S.cloud.data(),
                            static_cast<float4*>(c->h_stage_dev), c->stream));
  int m = 0;
  if ((rc = fetch_ints(c, d_count, 1, &m))) return rc;
  if ((size_t)m != want) return fail(c, ICPGPU_ERR_HIP, "pmf_extract: %d points extracted, %zu expected (internal error)", m, want);
  if (view) *view_xyzw = static_cast<const float*>(c->h_stage);
  else if (out_xyzw) std::memcpy(out_xyzw, c->h_stage, want * sizeof(float4));
  *n_out = want;
  return ICPGPU_OK;
}

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_pmf_extract(icpgpu_ctx* c, int negative, float* out_xyzw, size_t* n_out) {
  ENTER(c);
  return pmf_extract(c, negative, out_xyzw, nullptr, false, n_out);
}

int icpgpu_pmf_extract_view(icpgpu_ctx* c, int negative, const float** view_xyzw, size_t* n_out) {
  ENTER(c);
  return pmf_extract(c, negative, nullptr, view_xyzw, true, n_out);
}

}  // extern "C"
