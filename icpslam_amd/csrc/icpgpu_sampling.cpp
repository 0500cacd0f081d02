// icpgpu_sampling.cpp -- host side of the cropping and sampling filters (pcl::PassThrough, pcl::CropBox, pcl::UniformSampling,
// pcl::FarthestPointSampling; rules: include/icpgpu.h; kernels: icp_sampling.hip; arithmetic: icp_sampling.h).
#include "icp_ctx.h"
#include "icp_sampling.h"
#include "icp_voxel_plan.h"

namespace icpgpu_impl {
namespace {

struct SubsetCall {
  int kind = 0;
  CropRule crop{};
  float leaf = 0.f;
  size_t n_samples = 0;
  int64_t first_index = -1;
};

static_assert(kFpsOneMax == ICPGPU_FPS_ONE_WORKGROUP_MAX && kSubsetPassThrough == ICPGPU_SUBSET_PASS_THROUGH && kSubsetCropBox == ICPGPU_SUBSET_CROP_BOX &&
                  kSubsetUniform == ICPGPU_SUBSET_UNIFORM_SAMPLING && kSubsetFarthest == ICPGPU_SUBSET_FARTHEST_POINT_SAMPLING &&
                  kFpsPathOne == ICPGPU_FPS_PATH_ONE && kFpsPathMany == ICPGPU_FPS_PATH_MANY,
              "include/icpgpu.h states these constants");
constexpr int kSubsetInts = 4;  // device ints of a call: [0] the kept rows' count, [1] icpgpu_subset_removed's count

// what the host learns of the caller's cloud in one pass: the finite rows' number, the lowest of them and their box
struct HostScan {
  size_t n_finite = 0, first_finite = 0;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
};
HostScan scan_host(const float* xyzw, size_t n) {
  HostScan s;
  for (size_t i = 0; i < n; ++i) {
    const float* p = xyzw + 4 * i;
    if (!sampling_finite3(p[0], p[1], p[2])) continue;
    if (!s.n_finite++) s.first_finite = i;
    for (int a = 0; a < 3; ++a) s.lo[a] = std::min(s.lo[a], p[a]), s.hi[a] = std::max(s.hi[a], p[a]);
  }
  return s;
}

// One call: the checks, the upload into the section's own buffer, the filter's kernels, the kept rows into the pinned staging buffer
// in front of the count the host waits for -- one wait per call.  Nothing of the context's other state is read or written.
int subset_filter(icpgpu_ctx* c, const float* xyzw, size_t n, const SubsetCall& q, size_t* n_out) {
  auto& S = c->subset;
  S.kind = 0;
  S.n_in = S.n_kept = 0;
  S.waits = S.launches = S.path = 0;
  *n_out = 0;
  if (n && !xyzw) return fail(c, ICPGPU_ERR_INVALID_ARG, "null cloud pointer with n = %zu", n);
  if (n > (size_t)INT32_MAX - 4096) return fail(c, ICPGPU_ERR_INVALID_ARG, "cloud too large: %zu points", n);
  const int ni = (int)n;
  UniformLattice L{};
  int first = 0;
  bool empty = n == 0;
  if (q.kind == kSubsetPassThrough) {
    if (q.crop.field < -1 || q.crop.field > 2) return fail(c, ICPGPU_ERR_INVALID_ARG, "pass through: field %d outside -1 .. 2", q.crop.field);
    if (std::isnan(q.crop.lo[0]) || std::isnan(q.crop.hi[0])) return fail(c, ICPGPU_ERR_INVALID_ARG, "pass through: a limit is NaN");
  } else if (q.kind == kSubsetCropBox) {
    for (int a = 0; a < 3; ++a)
      if (std::isnan(q.crop.lo[a]) || std::isnan(q.crop.hi[a])) return fail(c, ICPGPU_ERR_INVALID_ARG, "crop box: a corner is NaN");
  } else if (q.kind == kSubsetUniform) {
    if (!(q.leaf > 0.f) || !std::isfinite(q.leaf)) return fail(c, ICPGPU_ERR_INVALID_ARG, "uniform sampling: leaf must be positive and finite");
    if (n > (size_t)kUniformMaxRows) return fail(c, ICPGPU_ERR_UNSUPPORTED, "uniform sampling: %zu rows, %d at most", n, kUniformMaxRows);
    if (n) {
      const HostScan s = scan_host(xyzw, n);
      L.leaf = q.leaf;
      L.inv = 1.0f / q.leaf;
      long long ncells = 0;
      const int verdict = voxel_grid_plan(s.lo, s.hi, L.inv, L.minb, L.divb, &ncells);
      if (verdict == kVoxelPlanPassThrough)
        return fail(c, ICPGPU_ERR_UNSUPPORTED, "uniform sampling: the leaf is too small for this cloud (the cell index would overflow)");
      if (verdict == kVoxelPlanWrap) return fail(c, ICPGPU_ERR_UNSUPPORTED, "uniform sampling: the cell index of this cloud would wrap");
      empty = verdict == kVoxelPlanNoFinite;
    }
  } else {
    const HostScan s = n ? scan_host(xyzw, n) : HostScan{};
    if (q.first_index < -1 || (q.first_index >= 0 && (uint64_t)q.first_index >= n))
      return fail(c, ICPGPU_ERR_INVALID_ARG, "farthest point sampling: first_index %lld outside the cloud of %zu rows", (long long)q.first_index, n);
    if (q.first_index >= 0) {
      const float* p = xyzw + 4 * (size_t)q.first_index;
      if (!sampling_finite3(p[0], p[1], p[2]))
        return fail(c, ICPGPU_ERR_INVALID_ARG, "farthest point sampling: row %lld, the first point, is not finite", (long long)q.first_index);
    }
    if (q.n_samples > s.n_finite)
      return fail(c, ICPGPU_ERR_INVALID_ARG, "farthest point sampling: %zu samples asked of %zu finite rows", q.n_samples, s.n_finite);
    first = q.first_index >= 0 ? (int)q.first_index : (int)s.first_finite;
    empty = q.n_samples == 0;
  }
  if (empty) {
    S.kind = q.kind;
    S.n_in = n;
    return ICPGPU_OK;
  }
  int rc;
  if ((rc = ensure(c, S.cloud.buf, n * sizeof(float4)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(S.cloud.buf.ptr, xyzw, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  S.cloud.n = n;
  S.cloud.set = true;
  S.cloud.bbox_version = 0;
  S.cloud.finite_version = 0;
  if ((rc = ensure_compaction(c, S.comp, n))) return rc;
  if ((rc = ensure(c, S.ints, kSubsetInts * sizeof(int)))) return rc;
  const size_t n_most = q.kind == kSubsetFarthest ? q.n_samples : n;  // (a filter's result is never longer than its input)
  if ((rc = ensure_stage(c, n_most * sizeof(float4), /*any_size=*/true))) return rc;
  const float4* d_cloud = S.cloud.data();
  int* d_flags = S.comp.flags.as<int>();
  int* d_kept = S.comp.kept.as<int>();
  int* d_ints = S.ints.as<int>();
  float4* d_stage = static_cast<float4*>(c->h_stage_dev);
  if (q.kind == kSubsetPassThrough || q.kind == kSubsetCropBox) {
    HIP_TRY(c, launch_crop_flags(d_cloud, ni, q.crop, d_flags, c->stream));
    HIP_TRY(c, launch_compact(d_flags, ni, S.comp.pos.as<int>(), S.comp.scan.as<int>(), d_kept, d_ints, d_cloud, d_stage, c->stream));
    S.launches = 1 + 4;
  } else if (q.kind == kSubsetUniform) {
    const size_t slots = uniform_table_slots(ni);
    if ((rc = ensure(c, S.cells, slots * sizeof(int)))) return rc;
    if ((rc = ensure(c, S.best, slots * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure(c, S.slot_of, n * sizeof(unsigned int)))) return rc;
    if ((rc = ensure(c, S.d2_of, n * sizeof(float)))) return rc;
    if ((rc = ensure(c, S.measure, n * sizeof(float)))) return rc;
    HIP_TRY(c, launch_uniform_flags(d_cloud, ni, L, S.cells.as<int>(), S.best.as<unsigned long long>(), S.slot_of.as<unsigned int>(), S.d2_of.as<float>(),
                                    d_flags, c->stream));
    HIP_TRY(c, launch_compact(d_flags, ni, S.comp.pos.as<int>(), S.comp.scan.as<int>(), d_kept, d_ints, d_cloud, d_stage, c->stream));
    HIP_TRY(c, launch_subset_gather(d_kept, d_ints, ni, nullptr, nullptr, S.d2_of.as<float>(), S.measure.as<float>(), nullptr, c->stream));
    S.launches = 3 + 4 + 1;
  } else {
    const int ns = (int)q.n_samples;
    if ((rc = ensure(c, S.measure, n * sizeof(float)))) return rc;
    if (ni <= kFpsOneMax) {
      HIP_TRY(c, launch_fps_one(d_cloud, ni, ns, first, d_kept, S.measure.as<float>(), c->stream));
      S.path = kFpsPathOne;
      S.launches = 1;
    } else {
      if ((rc = ensure(c, S.m, n * sizeof(float)))) return rc;
      if ((rc = ensure(c, S.slots, 2 * (size_t)kFpsManyBlocksMax * sizeof(unsigned long long)))) return rc;
      HIP_TRY(c, launch_fps_many(d_cloud, ni, ns, first, S.m.as<float>(), S.slots.as<unsigned long long>(), d_kept, S.measure.as<float>(), &S.launches,
                                 c->stream));
      S.path = kFpsPathMany;
    }
    HIP_TRY(c, launch_subset_gather(d_kept, nullptr, ns, d_cloud, d_stage, nullptr, nullptr, d_ints, c->stream));
    S.launches += 1;
  }
  int kept = 0;
  if ((rc = fetch_ints(c, d_ints, 1, &kept))) return rc;
  S.waits = 1;
  if (kept < 0 || (size_t)kept > n_most) return fail(c, ICPGPU_ERR_HIP, "subset filter: %d rows kept of %zu (internal error)", kept, n_most);
  S.kind = q.kind;
  S.n_in = n;
  S.n_kept = (size_t)kept;
  *n_out = S.n_kept;
  return ICPGPU_OK;
}

int subset_entry(icpgpu_ctx* c, const float* xyzw, size_t n, const SubsetCall& q, float* out_xyzw, const float** view_xyzw, bool view, size_t* n_out) {
  c->subset.kind = 0;  // (a refused call leaves nothing to fetch)
  if (!n_out || (view && !view_xyzw)) return fail(c, ICPGPU_ERR_INVALID_ARG, "null argument");
  if (view) *view_xyzw = nullptr;
  size_t m = 0;
  *n_out = 0;
  const int rc = subset_filter(c, xyzw, n, q, &m);
  if (rc) return rc;
  if (m) {
    if (view) *view_xyzw = static_cast<const float*>(c->h_stage);
    else if (out_xyzw) std::memcpy(out_xyzw, c->h_stage, m * sizeof(float4));
  }
  *n_out = m;
  return ICPGPU_OK;
}

SubsetCall pass_through_call(int field, float lo, float hi, int negative) {
  SubsetCall q;
  q.kind = kSubsetPassThrough;
  q.crop.box = 0, q.crop.field = field, q.crop.negative = negative ? 1 : 0, q.crop.has_T = 0;
  q.crop.lo[0] = lo, q.crop.hi[0] = hi;
  return q;
}

int crop_box_call(icpgpu_ctx* c, const float* min3, const float* max3, const float* T, int negative, SubsetCall& q) {
  c->subset.kind = 0;
  if (!min3 || !max3) return fail(c, ICPGPU_ERR_INVALID_ARG, "crop box: null corner");
  q.kind = kSubsetCropBox;
  q.crop.box = 1, q.crop.field = -1, q.crop.negative = negative ? 1 : 0, q.crop.has_T = T ? 1 : 0;
  for (int a = 0; a < 3; ++a) q.crop.lo[a] = min3[a], q.crop.hi[a] = max3[a];
  q.crop.T = to_xform(T);
  return ICPGPU_OK;
}

SubsetCall uniform_call(float leaf) {
  SubsetCall q;
  q.kind = kSubsetUniform;
  q.leaf = leaf;
  return q;
}

SubsetCall farthest_call(size_t n_samples, int64_t first_index) {
  SubsetCall q;
  q.kind = kSubsetFarthest;
  q.n_samples = n_samples, q.first_index = first_index;
  return q;
}

// c = a * b, 4 x 4 row-major doubles, every entry a[i][0] b[0][j] + ... + a[i][3] b[3][j] added from the left
void mul4(const double a[16], const double b[16], double out[16]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = a[4 * i] * b[j];
      for (int k = 1; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
      out[4 * i + j] = s;
    }
}

}  // namespace
}  // namespace icpgpu_impl

extern "C" {

int icpgpu_pass_through(icpgpu_ctx* c, const float* xyzw, size_t n, int field, float lo, float hi, int negative, float* out_xyzw, size_t* n_out) {
  ENTER(c);
  return subset_entry(c, xyzw, n, pass_through_call(field, lo, hi, negative), out_xyzw, nullptr, false, n_out);
}

int icpgpu_pass_through_view(icpgpu_ctx* c, const float* xyzw, size_t n, int field, float lo, float hi, int negative, const float** view_xyzw,
                             size_t* n_out) {
  ENTER(c);
  return subset_entry(c, xyzw, n, pass_through_call(field, lo, hi, negative), nullptr, view_xyzw, true, n_out);
}

int icpgpu_crop_box(icpgpu_ctx* c, const float* xyzw, size_t n, const float* min3, const float* max3, const float* T, int negative, float* out_xyzw,
                    size_t* n_out) {
  ENTER(c);
  SubsetCall q;
  if (n_out) *n_out = 0;
  const int rc = crop_box_call(c, min3, max3, T, negative, q);
  return rc ? rc : subset_entry(c, xyzw, n, q, out_xyzw, nullptr, false, n_out);
}

int icpgpu_crop_box_view(icpgpu_ctx* c, const float* xyzw, size_t n, const float* min3, const float* max3, const float* T, int negative,
                         const float** view_xyzw, size_t* n_out) {
  ENTER(c);
  SubsetCall q;
  if (n_out) *n_out = 0;
  if (view_xyzw) *view_xyzw = nullptr;
  const int rc = crop_box_call(c, min3, max3, T, negative, q);
  return rc ? rc : subset_entry(c, xyzw, n, q, nullptr, view_xyzw, true, n_out);
}

int icpgpu_crop_box_matrix(const float* transform16, const float* translation3, const float* rotation3, float* out16) {
  if (!translation3 || !rotation3 || !out16) return ICPGPU_ERR_INVALID_ARG;
  // row-major doubles from the column-major floats
  double tf[16], tr[16], rx[16], ry[16], rz[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const double e = i == j ? 1.0 : 0.0;
      tf[4 * i + j] = transform16 ? (double)transform16[4 * j + i] : e;
      tr[4 * i + j] = rx[4 * i + j] = ry[4 * i + j] = rz[4 * i + j] = e;
    }
  for (int a = 0; a < 3; ++a) tr[4 * a + 3] = -(double)translation3[a];
  const double ca = std::cos((double)rotation3[0]), sa = std::sin((double)rotation3[0]);
  const double cb = std::cos((double)rotation3[1]), sb = std::sin((double)rotation3[1]);
  const double cc = std::cos((double)rotation3[2]), sc = std::sin((double)rotation3[2]);
  rx[5] = ca, rx[6] = -sa, rx[9] = sa, rx[10] = ca;
  ry[0] = cb, ry[2] = sb, ry[8] = -sb, ry[10] = cb;
  rz[0] = cc, rz[1] = -sc, rz[4] = sc, rz[5] = cc;
  double zy[16], r[16], rinv[16], a[16], m[16];
  mul4(rz, ry, zy);
  mul4(zy, rx, r);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) rinv[4 * i + j] = r[4 * j + i];  // (a rotation's inverse: its transpose)
  mul4(tr, tf, a);
  mul4(rinv, a, m);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out16[4 * j + i] = (float)m[4 * i + j];
  return ICPGPU_OK;
}

int icpgpu_uniform_sampling(icpgpu_ctx* c, const float* xyzw, size_t n, float leaf, float* out_xyzw, size_t* n_out) {
  ENTER(c);
  return subset_entry(c, xyzw, n, uniform_call(leaf), out_xyzw, nullptr, false, n_out);
}

int icpgpu_uniform_sampling_view(icpgpu_ctx* c, const float* xyzw, size_t n, float leaf, const float** view_xyzw, size_t* n_out) {
  ENTER(c);
  return subset_entry(c, xyzw, n, uniform_call(leaf), nullptr, view_xyzw, true, n_out);
}

int icpgpu_farthest_point_sampling(icpgpu_ctx* c, const float* xyzw, size_t n, size_t n_samples, int64_t first_index, float* out_xyzw, size_t* n_out) {
  ENTER(c);
  return subset_entry(c, xyzw, n, farthest_call(n_samples, first_index), out_xyzw, nullptr, false, n_out);
}

int icpgpu_farthest_point_sampling_view(icpgpu_ctx* c, const float* xyzw, size_t n, size_t n_samples, int64_t first_index, const float** view_xyzw,
                                        size_t* n_out) {
  ENTER(c);
  return subset_entry(c, xyzw, n, farthest_call(n_samples, first_index), nullptr, view_xyzw, true, n_out);
}

int icpgpu_subset_fetch(icpgpu_ctx* c, size_t capacity, int32_t* kept_index, float* measure, size_t* n_in, size_t* n_kept) {
  ENTER(c);
  const auto& S = c->subset;
  if (n_in) *n_in = S.kind ? S.n_in : 0;
  if (n_kept) *n_kept = S.kind ? S.n_kept : 0;
  if (!S.kind) return fail(c, ICPGPU_ERR_INVALID_ARG, "subset_fetch: no cropping or sampling call to report on");
  if (!kept_index && !measure) return ICPGPU_OK;  // (the sizes alone: what a caller asks first, to make room)
  if (S.n_kept > capacity) return fail(c, ICPGPU_ERR_INVALID_ARG, "subset_fetch: %zu rows kept, room for %zu", S.n_kept, capacity);
  if (!S.n_kept) return ICPGPU_OK;
  const bool device_measure = S.kind == kSubsetUniform || S.kind == kSubsetFarthest;
  if (kept_index) HIP_TRY(c, hipMemcpyAsync(kept_index, S.comp.kept.ptr, S.n_kept * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (measure && device_measure) HIP_TRY(c, hipMemcpyAsync(measure, S.measure.ptr, S.n_kept * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (measure && !device_measure) std::fill(measure, measure + S.n_kept, 0.f);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ICPGPU_OK;
}

int icpgpu_subset_removed(icpgpu_ctx* c, size_t capacity, int32_t* removed_index, size_t* n_removed) {
  ENTER(c);
  auto& S = c->subset;
  const size_t n_rem = S.kind ? S.n_in - S.n_kept : 0;
  if (n_removed) *n_removed = n_rem;
  if (!S.kind) return fail(c, ICPGPU_ERR_INVALID_ARG, "subset_removed: no cropping or sampling call to report on");
  if (!removed_index) return ICPGPU_OK;
  if (n_rem > capacity) return fail(c, ICPGPU_ERR_INVALID_ARG, "subset_removed: %zu rows removed, room for %zu", n_rem, capacity);
  if (!n_rem) return ICPGPU_OK;
  if (!S.n_kept) {  // (nothing was kept, perhaps nothing was uploaded: every row)
    for (size_t i = 0; i < n_rem; ++i) removed_index[i] = (int32_t)i;
    return ICPGPU_OK;
  }
  const int ni = (int)S.n_in;
  int rc;
  if ((rc = ensure_compaction(c, S.rem, S.n_in))) return rc;
  int* d_ints = S.ints.as<int>();
  HIP_TRY(c, launch_subset_removed_flags(S.comp.kept.as<const int>(), (int)S.n_kept, ni, S.rem.flags.as<int>(), c->stream));
  HIP_TRY(c, launch_compact(S.rem.flags.as<int>(), ni, S.rem.pos.as<int>(), S.rem.scan.as<int>(), S.rem.kept.as<int>(), d_ints + 1, nullptr, nullptr,
                            c->stream));
  HIP_TRY(c, hipMemcpyAsync(removed_index, S.rem.kept.ptr, n_rem * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return ICPGPU_OK;
}

int icpgpu_subset_stats(const icpgpu_ctx* c, int32_t* kind, int32_t* host_waits, int32_t* launches, int32_t* path) {
  if (!c) return ICPGPU_ERR_INVALID_ARG;
  if (!c->subset.kind) return ICPGPU_ERR_INVALID_ARG;  // (no call to report on)
  if (kind) *kind = c->subset.kind;
  if (host_waits) *host_waits = c->subset.waits;
  if (launches) *launches = c->subset.launches;
  if (path) *path = c->subset.path;
  return ICPGPU_OK;
}

}  // extern "C"
