// icpgpu_outlier.cpp -- host side of the outlier filters (pcl::StatisticalOutlierRemoval, pcl::RadiusOutlierRemoval; rules:
// include/icpgpu.h; kernels: icp_outlier.hip).
#include "icp_ctx.h"


namespace icpgpu_impl {
namespace {

enum { kOutlierSor = 1, kOutlierRor = 2 };
struct OutlierCall {
  int kind = 0;
  int mean_k = 0;
  double stddev_mult = 0.0;
  double radius = 0.0;
  int min_pts = 0;
  int negative = 0;
};

// device ints of a call: [0] the kept points' count, [2..9] SOR's mean, stddev, threshold, n_valid as doubles
constexpr int kOutlierInts = 16;

int count_finite_host(const float* xyzw, size_t n) {
  int nf = 0;
  for (size_t i = 0; i < n; ++i) nf += std::isfinite(xyzw[4 * i]) && std::isfinite(xyzw[4 * i + 1]) && std::isfinite(xyzw[4 * i + 2]);
  return nf;
}

// The statistical filter's k-NN grid: the covariance pass's builder and its rule for the cells (a typical point shares its cell with
// ~32 others; the neighbours are exact whatever the cells), but the first cell size comes from the CLOUD -- its box filled evenly
// would put 32 points in a cell of that size -- and not from the registration's correspondence gate, which has nothing to do with
// a filter.  The count pass then corrects it once, as for every k-NN grid (down to a 16th for points on surfaces, up to 8 times).
// (Shared with the neighbour search, icpgpu_search.cpp: declared in icp_ctx.h.)
}  // namespace
int build_knn_grid(icpgpu_ctx* c, const Cloud& cloud, GridIndex& G) {
  constexpr double kKnnPopulation = 32.0;
  GridBuild b;
  b.post = true;  // (the read-backs go through fetch_ints, as in build_grid)
  int rc = gb_begin(c, b, cloud, 0, /*cut=*/1.0, /*adapt=*/false, G, nullptr, kKnnPopulation, 0.0);
  while (!rc && b.state != GridBuild::Done) {
    const int* d_ints = G.ints.as<const int>();
    if (b.state == GridBuild::WaitBbox) {
      if ((rc = fetch_ints(c, d_ints, 6, c->h_ints))) break;
      float lo[3], hi[3];
      decode_bbox(c->h_ints, lo, hi);
      double ext[3], widest = 0.0;
      for (int a = 0; a < 3; ++a) widest = std::max(widest, ext[a] = (double)hi[a] - (double)lo[a]);
      if (widest > 0.0 && std::isfinite(widest)) {  // (else: no finite point, or all of them in one place -- the builder's own start)
        double volume = 1.0;
        for (int a = 0; a < 3; ++a) volume *= std::max(ext[a], 1e-3 * widest);  // (a flat cloud: the count pass grows the cells)
        const double h = std::cbrt(volume * kKnnPopulation / (double)cloud.n);
        if (h > 0.0 && std::isfinite(h)) {
          b.h_start = h;
          b.cut = 4.0 * h;  // (the builder keeps the cells between cut / 64 and 8 times the first size)
        }
      }
    } else {
      rc = fetch_ints(c, d_ints + 6, kGridStatInts, c->h_ints + 6);
    }
    if (!rc) rc = gb_advance(c, b);
  }
  return rc;
}
namespace {

// One filter call: upload, the cloud's own grid, the measure, flags, compaction.  The kept points are written by the last kernel
// into the pinned staging buffer, in front of the count the host waits for -- one wait per call, as icpgpu_voxel_grid_view has it.
// Nothing of the context's source, target, their grids or the voxel filter's result is touched.
int outlier_filter(icpgpu_ctx* c, const float* xyzw, size_t n, const OutlierCall& q, size_t* n_out) {
  auto& O = c->outlier;
  O.kind = 0;
  O.n_in = O.n_kept = O.n_valid = 0;
  O.mean = O.stddev = O.threshold = 0.0;
  *n_out = 0;
  if (n && !xyzw) return fail(c, ICPGPU_ERR_INVALID_ARG, "null cloud pointer with n = %zu", n);
  if (n > (size_t)INT32_MAX - 4096) return fail(c, ICPGPU_ERR_INVALID_ARG, "cloud too large: %zu points", n);
  if (q.kind == kOutlierSor) {
    if (q.mean_k < 1 || q.mean_k > ICPGPU_SOR_MAX_K)
      return fail(c, ICPGPU_ERR_INVALID_ARG, "statistical outlier removal: mean_k %d outside 1..%d", q.mean_k, ICPGPU_SOR_MAX_K);
  } else {
    if (!std::isfinite(q.radius) || q.radius < 0.0) return fail(c, ICPGPU_ERR_INVALID_ARG, "radius outlier removal: radius must be finite and >= 0");
    if (q.min_pts < 0) return fail(c, ICPGPU_ERR_INVALID_ARG, "radius outlier removal: min_pts %d < 0", q.min_pts);
  }
  if (n == 0) {
    O.kind = q.kind;
    return ICPGPU_OK;
  }
  const int ni = (int)n;
  int rc;
  if ((rc = ensure(c, O.cloud.buf, n * sizeof(float4)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(O.cloud.buf.ptr, xyzw, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  O.cloud.n = n;
  O.cloud.set = true;
  O.cloud.bbox_version = 0;
  O.cloud.finite_version = 0;
  if ((rc = ensure(c, O.measure, n * sizeof(float)))) return rc;
  if ((rc = ensure_compaction(c, O.comp, n))) return rc;
  if ((rc = ensure(c, O.far, (n + 2) * sizeof(int)))) return rc;
  if ((rc = ensure(c, O.ints, kOutlierInts * sizeof(int)))) return rc;
  if ((rc = ensure_stage(c, n * sizeof(float4), /*any_size=*/true))) return rc;  // (a filter's result is never longer than its input)
  const float4* d_cloud = O.cloud.data();
  float* d_measure = O.measure.as<float>();
  int* d_flags = O.comp.flags.as<int>();
  int* d_ints = O.ints.as<int>();
  double* d_stats = reinterpret_cast<double*>(d_ints + 2);
  GridIndex& G = O.grid;
  G.built = G.usable = false;  // (version 0: a build never stands for the next call's cloud)
  if (q.kind == kOutlierSor) {
    if ((rc = build_knn_grid(c, O.cloud, G))) return rc;
    const int n_finite = G.n_finite >= 0 ? G.n_finite : count_finite_host(xyzw, n);
    if (n_finite < q.mean_k + 1)
      return fail(c, ICPGPU_ERR_INVALID_ARG, "statistical outlier removal: %d finite points, mean_k + 1 = %d needed", n_finite, q.mean_k + 1);
    if (!G.usable && n > (size_t)kGicpCovFarMost)
      return fail(c, ICPGPU_ERR_UNSUPPORTED, "statistical outlier removal: cannot index this cloud of %zu points", n);
    HIP_TRY(c, launch_sor_distances(d_cloud, ni, G.usable ? G.sorted.as<const float4>() : nullptr, G.cell_start.as<const int>(), G.g,
                                    G.usable ? G.n_binned : 0, q.mean_k, d_measure, O.far.as<int>(), c->stream));
    HIP_TRY(c, launch_sor_flags(d_cloud, d_measure, ni, q.stddev_mult, q.negative, d_stats, d_flags, c->stream));
  } else {
    const float r2 = (float)(q.radius * q.radius);
    bool brute = false, grid = false;
    if (r2 > 0.f) {  // (r2 == 0: no d2 is below it, k = 0 everywhere)
      if (q.radius <= 1e6) {
        // the radius is this grid's gate: cells and r_max by the NN grid's rule, so that the cube of r_max cells contains the ball
        if ((rc = build_grid(c, O.cloud, 0, q.radius, /*adapt=*/true, G))) return rc;
        grid = G.usable;
      }
      brute = !grid;
    }
    HIP_TRY(c, launch_ror_counts(d_cloud, ni, grid ? G.sorted.as<const float4>() : nullptr, G.cell_start.as<const int>(), G.g,
                                 grid ? G.n_binned : 0, r2, q.min_pts, q.negative, brute, d_measure, d_flags, c->stream));
  }
  HIP_TRY(c, launch_compact(d_flags, ni, O.comp.pos.as<int>(), O.comp.scan.as<int>(), O.comp.kept.as<int>(), d_ints, d_cloud,
                            static_cast<float4*>(c->h_stage_dev), c->stream));
  int hv[10] = {0};
  const int n_ints = q.kind == kOutlierSor ? 10 : 1;
  if ((rc = fetch_ints(c, d_ints, n_ints, hv))) return rc;
  if (hv[0] < 0 || hv[0] > ni) return fail(c, ICPGPU_ERR_HIP, "outlier removal: %d points kept of %d (internal error)", hv[0], ni);
  if (q.kind == kOutlierSor) {
    double st[4];
    std::memcpy(st, hv + 2, sizeof st);
    O.mean = st[0];
    O.stddev = st[1];
    O.threshold = st[2];
    O.n_valid = (size_t)st[3];
  }
  O.kind = q.kind;
  O.n_in = n;
  O.n_kept = (size_t)hv[0];
  *n_out = O.n_kept;
  return ICPGPU_OK;
}

int outlier_entry(icpgpu_ctx* c, const float* xyzw, size_t n, const OutlierCall& q, float* out_xyzw, const float** view_xyzw, bool view, size_t* n_out) {
  if (!n_out || (view && !view_xyzw)) return fail(c, ICPGPU_ERR_INVALID_ARG, "null argument");
  if (view) *view_xyzw = nullptr;
  size_t m = 0;
  *n_out = 0;
  const int rc = outlier_filter(c, xyzw, n, q, &m);
  if (rc) return rc;
  if (m) {
    if (view) *view_xyzw = static_cast<const float*>(c->h_stage);
    else if (out_xyzw) std::memcpy(out_xyzw, c->h_stage, m * sizeof(float4));
  }
  *n_out = m;
  return ICPGPU_OK;
}

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_statistical_outlier_removal(icpgpu_ctx* c, const float* xyzw, size_t n, int mean_k, double stddev_mult, int negative, float* out_xyzw,
                                       size_t* n_out) {
  ENTER(c);
  OutlierCall q;
  q.kind = kOutlierSor, q.mean_k = mean_k, q.stddev_mult = stddev_mult, q.negative = negative ? 1 : 0;
  return outlier_entry(c, xyzw, n, q, out_xyzw, nullptr, false, n_out);
}

int icpgpu_statistical_outlier_removal_view(icpgpu_ctx* c, const float* xyzw, size_t n, int mean_k, double stddev_mult, int negative,
                                            const float** view_xyzw, size_t* n_out) {
  ENTER(c);
  OutlierCall q;
  q.kind = kOutlierSor, q.mean_k = mean_k, q.stddev_mult = stddev_mult, q.negative = negative ? 1 : 0;
  return outlier_entry(c, xyzw, n, q, nullptr, view_xyzw, true, n_out);
}

int icpgpu_radius_outlier_removal(icpgpu_ctx* c, const float* xyzw, size_t n, double radius, int min_pts, int negative, float* out_xyzw,
                                  size_t* n_out) {
  ENTER(c);
  OutlierCall q;
  q.kind = kOutlierRor, q.radius = radius, q.min_pts = min_pts, q.negative = negative ? 1 : 0;
  return outlier_entry(c, xyzw, n, q, out_xyzw, nullptr, false, n_out);
}

int icpgpu_radius_outlier_removal_view(icpgpu_ctx* c, const float* xyzw, size_t n, double radius, int min_pts, int negative,
                                       const float** view_xyzw, size_t* n_out) {
  ENTER(c);
  OutlierCall q;
  q.kind = kOutlierRor, q.radius = radius, q.min_pts = min_pts, q.negative = negative ? 1 : 0;
  return outlier_entry(c, xyzw, n, q, nullptr, view_xyzw, true, n_out);
}

int icpgpu_outlier_stats(const icpgpu_ctx* c, double* mean, double* stddev, double* threshold, size_t* n_valid) {
  if (!c) return ICPGPU_ERR_INVALID_ARG;
  if (c->outlier.kind != kOutlierSor) return ICPGPU_ERR_INVALID_ARG;  // (no statistical filter call to report on)
  if (mean) *mean = c->outlier.mean;
  if (stddev) *stddev = c->outlier.stddev;
  if (threshold) *threshold = c->outlier.threshold;
  if (n_valid) *n_valid = c->outlier.n_valid;
  return ICPGPU_OK;
}

int icpgpu_outlier_fetch(icpgpu_ctx* c, size_t capacity, float* measure, int32_t* kept_index, size_t* n_in, size_t* n_kept) {
  ENTER(c);
  const auto& O = c->outlier;
  if (n_in) *n_in = O.kind ? O.n_in : 0;
  if (n_kept) *n_kept = O.kind ? O.n_kept : 0;
  if (!O.kind) return fail(c, ICPGPU_ERR_INVALID_ARG, "outlier_fetch: no outlier filter call to report on");
  if (!measure && !kept_index) return ICPGPU_OK;  // (the sizes alone: what a caller asks first, to make room)
  if (O.n_in > capacity) return fail(c, ICPGPU_ERR_INVALID_ARG, "outlier_fetch: %zu points, room for %zu", O.n_in, capacity);
  if (measure && O.n_in) HIP_TRY(c, hipMemcpyAsync(measure, O.measure.ptr, O.n_in * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (kept_index && O.n_kept) HIP_TRY(c, hipMemcpyAsync(kept_index, O.comp.kept.ptr, O.n_kept * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ICPGPU_OK;
}

}  // extern "C"
