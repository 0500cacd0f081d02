// icpgpu_p2plane.cpp -- point-to-plane ICP behind icpgpu_align (method ICPGPU_P2PLANE): pcl::IterativeClosestPointWithNormals with
// pcl::registration::TransformationEstimationPointToPlaneLLS (PCL 1.8), the alternative the reference names at
// icp_odometer.cpp:187 of the reference.  Per iteration: the exact key-writing correspondence search (the gated grid
// search GICP uses, or the brute-force keys) -> p2plane_reduce_kernel + p2plane_final_kernel (icp_p2plane.hip) store the 29 sums as
// result pairs into the pinned host mailbox -> the host polls them, solves the 6 x 6 system (partial-pivot LU, float64), builds
// the incremental transform and runs the point-to-point loop's convergence test (icp_solver.cpp) -> next search.  The target's
// normals are the caller's or GICP's plane, estimated once per target cloud by the covariance kernels (icp_gicp_cov.hip).
#include "icp_ctx.h"
#include "icp_trig.h"

namespace icpgpu_impl {

int ensure_normals(icpgpu_ctx* c, bool of_target, const float4** out) {
  *out = nullptr;
  if (of_target && c->nrm_supplied) {
    *out = static_cast<const float4*>(c->nrm_user.ptr);
    return ICPGPU_OK;
  }
  if (!of_target && source_normals_supplied(c)) {
    *out = static_cast<const float4*>(c->nrm_src_user.ptr);
    return ICPGPU_OK;
  }
  const Cloud& cl = of_target ? c->tgt : c->src;
  const uint64_t version = of_target ? c->tgt_version : c->src_version;
  DeviceBuf& buf = of_target ? c->nrm_tgt : c->nrm_src;
  uint64_t& have = of_target ? c->nrm_tgt_version : c->nrm_src_version;
  if (cl.n < (size_t)kGicpK)
    return fail(c, ICPGPU_ERR_INVALID_ARG,
                "point-to-plane: estimated normals need at least %d points per cloud (or icpgpu_set_target_normals / icpgpu_set_source_normals)", kGicpK);
  if (!(have == version && buf.ptr)) {
    have = 0;
    int rc = ensure(c, buf, cl.n * sizeof(float4));
    if (rc) return rc;
    // (the normals' grid serves both clouds, whose version counters are distinct sequences: never taken for another cloud's)
    c->nrm_grid.built = c->nrm_grid.usable = false;
    uint64_t raw_version = 0;  // (the raw covariances are scratch: never cached)
    if ((rc = ensure_covariances(c, cl, version, c->nrm_grid, c->nrm_raw, raw_version, /*allow_unchecked=*/false, static_cast<float4*>(buf.ptr))))
      return rc;
    have = version;
  }
  *out = static_cast<const float4*>(buf.ptr);
  return ICPGPU_OK;
}

// x = (A^T A)^-1 A^T r; false when a pivot is zero (or NaN) or x is not finite
static bool solve_normal_equations(const double sums[kP2planeTerms], double x[6]) {
  // ATA.coeffRef(6) = ATA.coeff(1), ...: the symmetric matrix from its upper triangle
  double A[6][6], b[6];
  for (int i = 0, k = 2; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) A[i][j] = A[j][i] = sums[k];
  for (int i = 0; i < 6; ++i) b[i] = sums[23 + i];
  // ATA.inverse(): Eigen's PartialPivLU -- row k swapped with the row of the largest |A(i, k)|, i >= k (the first of equals), the
  // column below the pivot divided by it, the trailing block updated; then LU x = P I, column by column
  int perm[6] = {0, 1, 2, 3, 4, 5};
  for (int k = 0; k < 6; ++k) {
    int p = k;
    double best = std::fabs(A[k][k]);
    for (int i = k + 1; i < 6; ++i)
      if (std::fabs(A[i][k]) > best) {
        best = std::fabs(A[i][k]);
        p = i;
      }
    if (!(best > 0.0)) return false;  // singular -- PCL leaves this case undefined (include/icpgpu.h)
    if (p != k) {
      for (int j = 0; j < 6; ++j) std::swap(A[k][j], A[p][j]);
      std::swap(perm[k], perm[p]);
    }
    for (int i = k + 1; i < 6; ++i) {
      A[i][k] /= A[k][k];
      for (int j = k + 1; j < 6; ++j) A[i][j] -= A[i][k] * A[k][j];
    }
  }
  double inv[6][6];
  for (int col = 0; col < 6; ++col) {
    double y[6];
    for (int i = 0; i < 6; ++i) y[i] = perm[i] == col ? 1.0 : 0.0;
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < i; ++j) y[i] -= A[i][j] * y[j];
    for (int i = 5; i >= 0; --i) {
      for (int j = i + 1; j < 6; ++j) y[i] -= A[i][j] * y[j];
      y[i] /= A[i][i];
    }
    for (int i = 0; i < 6; ++i) inv[i][col] = y[i];
  }
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
    for (int j = 0; j < 6; ++j) s += inv[i][j] * b[j];
    x[i] = s;
    if (!std::isfinite(s)) return false;
  }
  return true;
}

// constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz): R = Rz(gamma) Ry(beta) Rx(alpha), as PCL writes it term by term
static Mat4d construct_transformation(double alpha, double beta, double gamma, double tx, double ty, double tz) {
  double sa, ca, sb, cb, sg, cg;
  trig::sincos_cr(alpha, &sa, &ca);
  trig::sincos_cr(beta, &sb, &cb);
  trig::sincos_cr(gamma, &sg, &cg);
  Mat4d M{};
  auto at = [&M](int r, int col) -> double& { return M[col * 4 + r]; };
  at(0, 0) = cg * cb;
  at(0, 1) = -sg * ca + cg * sb * sa;
  at(0, 2) = sg * sa + cg * sb * ca;
  at(1, 0) = sg * cb;
  at(1, 1) = cg * ca + sg * sb * sa;
  at(1, 2) = -cg * sa + sg * sb * ca;
  at(2, 0) = -sb;
  at(2, 1) = cb * sa;
  at(2, 2) = cb * ca;
  at(0, 3) = tx;
  at(1, 3) = ty;
  at(2, 3) = tz;
  at(3, 3) = 1.0;
  return M;
}

bool solve_point_to_plane(const double sums[kP2planeTerms], Mat4d& Tk) {
  Tk = mat4_identity();
  double x[6];
  if (!solve_normal_equations(sums, x)) return false;
  Tk = construct_transformation(x[0], x[1], x[2], x[3], x[4], x[5]);
  return true;
}

// PCL: rotation_z * rotation_y * rotation_x * translation * rotation_z * rotation_y * rotation_x, evaluated as (R * Tr) * R
bool solve_symmetric_point_to_plane(const double sums[kP2planeTerms], Mat4d& Tk) {
  Tk = mat4_identity();
  double x[6];
  if (!solve_normal_equations(sums, x)) return false;
  const Mat4d R = construct_transformation(x[0], x[1], x[2], 0.0, 0.0, 0.0);
  Mat4d Tr = mat4_identity();
  Tr[12] = x[3];
  Tr[13] = x[4];
  Tr[14] = x[5];
  Tk = mat4_mul(mat4_mul(R, Tr), R);
  return true;
}

// the 29 sums of mailbox sweep `seq` (the pairs at h_flags words 2k, 2k + 1; p2plane_final_kernel)
static int wait_p2plane_sums(icpgpu_ctx* c, unsigned long long seq, double* sums) {
  const int rc = wait_flags(c, c->h_flags, kP2planeTerms, seq);
  if (!rc) take_pairs(c, kP2planeTerms, sums);
  return rc;
}

int align_p2plane(icpgpu_ctx* c, const float* guess, float* out_xyzw, int want_fitness, icpgpu_result* res) {
  const auto t_start = std::chrono::steady_clock::now();
  int rc = call_begin(c, res);
  if (rc) return rc;
  start_cold(c);  // every alignment starts cold
  Mat4d final_T = mat4_identity();
  if (guess)
    for (int i = 0; i < 16; ++i) final_T[i] = (double)guess[i];
  const int n_s = (int)c->src.n, n_t = (int)c->tgt.n;
  bool converged = false;
  int nr = 0, state = ICPGPU_NOT_CONVERGED;
  unsigned n_corr = 0;
  double mse = 0.0;
  if (n_t == 0) {  // PCL: setInputTarget refuses an empty target, align() leaves converged_ = false and T = identity
    final_T = mat4_identity();
  } else {
    const float4* normals = nullptr;
    if ((rc = ensure_normals(c, /*of_target=*/true, &normals))) return rc;
    const bool symmetric = c->p2plane_symmetric;  // (icpgpu_set_p2plane_symmetric: only the reduction and the solve differ)
    const float4* src_normals = nullptr;
    if (symmetric && n_s > 0 && (rc = ensure_normals(c, /*of_target=*/false, &src_normals))) return rc;
    if ((rc = reject_prepare(c))) return rc;
    const icpgpu_params& P = c->params;
    ConvergenceCriteria crit(P.max_iterations, P.transformation_epsilon, P.euclidean_fitness_epsilon, P.force_iterations != 0);
    const float thr = gate_threshold(c);
    if ((rc = ensure_grid(c, thr))) return rc;
    if ((rc = ensure(c, c->keys, (size_t)(n_s ? n_s : 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure(c, c->p2plane_partials, (size_t)p2plane_blocks(n_s) * kP2planeTerms * sizeof(double)))) return rc;
    auto* keys = static_cast<unsigned long long*>(c->keys.ptr);
    double sums[kP2planeTerms];
    for (;;) {
      const Xform T = to_xform(final_T);
      if ((rc = correspondence_keys(c, T, thr, keys))) return rc;
      const unsigned long long seq = ++c->sums_seq;
      if (symmetric)
        HIP_TRY(c, launch_p2plane_sym_reduce(c->src.data(), src_normals, n_s, c->tgt.data(), normals, keys, T, thr, c->p2plane_enforce_same_direction,
                                             static_cast<double*>(c->p2plane_partials.ptr), nullptr, c->h_flags_dev, wire_seq(c, seq), c->stream));
      else
        HIP_TRY(c, launch_p2plane_reduce(c->src.data(), n_s, c->tgt.data(), normals, keys, T, thr, static_cast<double*>(c->p2plane_partials.ptr),
                                         nullptr, c->h_flags_dev, wire_seq(c, seq), c->stream));
      c->prof.reduce_launches += 1;
      c->prof.reduce_bytes += (symmetric ? 72ull : 56ull) * (uint64_t)n_s + 232ull * (uint64_t)p2plane_blocks(n_s);
      if ((rc = wait_p2plane_sums(c, seq, sums))) return rc;
      n_corr = (unsigned)sums[0];
      if ((int)n_corr < P.min_correspondences) {
        state = ICPGPU_CONV_NO_CORRESPONDENCES;
        converged = false;
        break;
      }
      Mat4d Tk;
      if (!(symmetric ? solve_symmetric_point_to_plane(sums, Tk) : solve_point_to_plane(sums, Tk))) {  // singular system: stop where the last finite transform left the source
        state = ICPGPU_NOT_CONVERGED;
        converged = false;
        break;
      }
      final_T = mat4_mul(Tk, final_T);
      mse = sums[1] / sums[0];
      ++nr;
      c->prof.iterations += 1;
      if (crit.has_converged(nr, Tk, mse)) {
        converged = true;
        state = crit.state();
        break;
      }
    }
  }
  if ((rc = reject_fetch_stats(c))) return rc;  // the chain's statistics of the last iteration (none, and nothing fetched, without a chain)
  record_result(c, res, final_T, converged, nr, state, n_corr, mse);
  return cloud_then_fitness(c, to_xform(final_T), out_xyzw, want_fitness && n_t > 0, res, t_start);
}

}  // namespace icpgpu_impl

extern "C" {

int icpgpu_set_target_normals(icpgpu_ctx* c, const float* nxyzw, size_t n) {
  ENTER(c);
  if (!c->tgt.set) return fail(c, ICPGPU_ERR_NO_INPUT, "set_target_normals: no target set");
  if (n != c->tgt.n) return fail(c, ICPGPU_ERR_INVALID_ARG, "set_target_normals: %zu normals for a target of %zu points", n, c->tgt.n);
  if (n && !nxyzw) return fail(c, ICPGPU_ERR_INVALID_ARG, "set_target_normals: null normals");
  c->nrm_supplied = false;
  int rc = ensure(c, c->nrm_user, (n ? n : 1) * sizeof(float4));
  if (rc) return rc;
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(c->nrm_user.ptr, nxyzw, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller may reuse its buffer on return)
  }
  c->nrm_supplied = true;
  return ICPGPU_OK;
}

int icpgpu_set_source_normals(icpgpu_ctx* c, const float* nxyzw, size_t n) {
  ENTER(c);
  if (!c->src.set) return fail(c, ICPGPU_ERR_NO_INPUT, "set_source_normals: no source set");
  if (n != c->src.n) return fail(c, ICPGPU_ERR_INVALID_ARG, "set_source_normals: %zu normals for a source of %zu points", n, c->src.n);
  if (n && !nxyzw) return fail(c, ICPGPU_ERR_INVALID_ARG, "set_source_normals: null normals");
  c->nrm_src_user_version = 0;
  int rc = ensure(c, c->nrm_src_user, (n ? n : 1) * sizeof(float4));
  if (rc) return rc;
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(c->nrm_src_user.ptr, nxyzw, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller may reuse its buffer on return)
  }
  c->nrm_src_user_version = c->src_version;
  return ICPGPU_OK;
}

int icpgpu_set_p2plane_symmetric(icpgpu_ctx* c, int on, int enforce_same_direction) {
  if (!c) return fail(nullptr, ICPGPU_ERR_INVALID_ARG, "null context");
  c->p2plane_symmetric = on != 0;
  c->p2plane_enforce_same_direction = enforce_same_direction != 0;
  return ICPGPU_OK;
}

int icpgpu_get_p2plane_symmetric(const icpgpu_ctx* c, int* on, int* enforce_same_direction) {
  if (!c || (!on && !enforce_same_direction)) return ICPGPU_ERR_INVALID_ARG;
  if (on) *on = c->p2plane_symmetric ? 1 : 0;
  if (enforce_same_direction) *enforce_same_direction = c->p2plane_enforce_same_direction ? 1 : 0;
  return ICPGPU_OK;
}

int icpgpu_normals(icpgpu_ctx* c, int of_target, float* out_nxyzw) {
  ENTER(c);
  const Cloud& cl = of_target ? c->tgt : c->src;
  if (!cl.set) return fail(c, ICPGPU_ERR_NO_INPUT, "normals: cloud not set");
  if (cl.n && !out_nxyzw) return fail(c, ICPGPU_ERR_INVALID_ARG, "null output");
  const float4* nrm = nullptr;
  int rc = ensure_normals(c, of_target != 0, &nrm);
  if (rc) return rc;
  if (cl.n) HIP_TRY(c, hipMemcpyAsync(out_nxyzw, nrm, cl.n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return resolve_cov_timing(c);
}

// icpgpu_reduce_point_to_plane and its symmetric counterpart: the 29 sums of the last icpgpu_nn sweep
static int reduce_p2plane_entry(icpgpu_ctx* c, const float* T, double max_dist, bool symmetric, bool enforce, double* sums, const char* what) {
  ENTER(c);
  if (!sums || !T) return fail(c, ICPGPU_ERR_INVALID_ARG, "null argument");
  if (!c->src.set || !c->tgt.set) return fail(c, ICPGPU_ERR_NO_INPUT, "%s: source and target must be set first", what);
  if (!c->keys.ptr || c->keys.cap < c->src.n * sizeof(unsigned long long))
    return fail(c, ICPGPU_ERR_NO_INPUT, "%s: no nearest-neighbour sweep to reduce (call icpgpu_nn first)", what);
  if (c->tgt.n == 0) {  // (no pair: nothing to read)
    for (int k = 0; k < kP2planeTerms; ++k) sums[k] = 0.0;
    return ICPGPU_OK;
  }
  const float4 *normals = nullptr, *src_normals = nullptr;
  int rc = ensure_normals(c, /*of_target=*/true, &normals);
  if (rc) return rc;
  const int n_s = (int)c->src.n;
  if (symmetric && n_s > 0 && (rc = ensure_normals(c, /*of_target=*/false, &src_normals))) return rc;
  if ((rc = ensure(c, c->p2plane_partials, (size_t)p2plane_blocks(n_s) * kP2planeTerms * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, kP2planeTerms * sizeof(double)))) return rc;
  const auto* keys = static_cast<const unsigned long long*>(c->keys.ptr);
  const float thr = threshold_from(max_dist * max_dist);
  auto* partials = static_cast<double*>(c->p2plane_partials.ptr);
  auto* d_sums = static_cast<double*>(c->sums.ptr);
  if (symmetric)
    HIP_TRY(c, launch_p2plane_sym_reduce(c->src.data(), src_normals, n_s, c->tgt.data(), normals, keys, to_xform(T), thr, enforce, partials, d_sums,
                                         nullptr, 0, c->stream));
  else
    HIP_TRY(c, launch_p2plane_reduce(c->src.data(), n_s, c->tgt.data(), normals, keys, to_xform(T), thr, partials, d_sums, nullptr, 0, c->stream));
  HIP_TRY(c, hipMemcpyAsync(sums, c->sums.ptr, kP2planeTerms * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return resolve_cov_timing(c);
}

int icpgpu_reduce_point_to_plane(icpgpu_ctx* c, const float* T, double max_dist, double sums[29]) {
  return reduce_p2plane_entry(c, T, max_dist, false, false, sums, "reduce_point_to_plane");
}

int icpgpu_reduce_symmetric_point_to_plane(icpgpu_ctx* c, const float* T, double max_dist, int enforce_same_direction, double sums[29]) {
  return reduce_p2plane_entry(c, T, max_dist, true, enforce_same_direction != 0, sums, "reduce_symmetric_point_to_plane");
}

int icpgpu_solve_symmetric_point_to_plane(const double sums[29], double Tk[16]) {
  if (!sums || !Tk) return ICPGPU_ERR_INVALID_ARG;
  Mat4d M;
  const bool ok = solve_symmetric_point_to_plane(sums, M);
  for (int i = 0; i < 16; ++i) Tk[i] = M[i];
  return ok ? ICPGPU_OK : ICPGPU_ERR_INVALID_ARG;
}

int icpgpu_solve_point_to_plane(const double sums[29], double Tk[16]) {
  if (!sums || !Tk) return ICPGPU_ERR_INVALID_ARG;
  Mat4d M;
  const bool ok = solve_point_to_plane(sums, M);
  for (int i = 0; i < 16; ++i) Tk[i] = M[i];
  return ok ? ICPGPU_OK : ICPGPU_ERR_INVALID_ARG;
}

}  // extern "C"
