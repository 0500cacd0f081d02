"""Second, independent restatement of PCL point-to-point ICP in NumPy/SciPy (float64 solve, cKDTree NN).

TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED: exists to cross-check
oracle/icp_oracle.c.  Restates SURVEY.md Appendix A.1 for the call sites at
/root/reference/src/icpslam/icp_odometer.cpp:188-201 and src/icpslam/octree_mapper.cpp:104-117.
Deliberately written differently from the C oracle (library SVD, two-pass demeaned covariance,
library kd-tree with float64 distances) so a shared bug is unlikely.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)


def transform_cloud_f32(T32: np.ndarray, xyz: np.ndarray) -> np.ndarray:
    """p = R s + t evaluated in float32 (rounding differs from the fmaf chain by <= 2 ulp)."""
    R, t = T32[:3, :3].astype(np.float32), T32[:3, 3].astype(np.float32)
    return (xyz.astype(np.float32) @ R.T + t).astype(np.float32)


def umeyama(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Eigen::umeyama(src=p, dst=q, with_scaling=false), float64."""
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    sigma = (q - mq).T @ (p - mp) / p.shape[0]
    U, d, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = U @ np.diag(S) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T


def icp_align(src, tgt, max_iterations=10, transformation_epsilon=1e-6, max_correspondence_distance=1.0,
              euclidean_fitness_epsilon=-np.finfo(np.float64).max, min_correspondences=3, guess=None,
              force_iterations=False, want_fitness=False):
    src = np.asarray(src, np.float32)[:, :3]
    tgt = np.asarray(tgt, np.float32)[:, :3]
    out = dict(T=np.eye(4, dtype=np.float32), converged=False, iterations=0, state=NOT_CONVERGED, n_corr=0,
               mse=0.0, fitness=float("nan"), trace=[])
    if tgt.shape[0] == 0:
        return out
    tree = cKDTree(tgt.astype(np.float64), leafsize=15)
    final = np.eye(4) if guess is None else np.asarray(guess, np.float64).copy()
    r2 = max_correspondence_distance ** 2
    mse_prev = np.finfo(np.float64).max
    nr, converged, state, n_c, mse = 0, False, NOT_CONVERGED, 0, 0.0
    while True:
        X = transform_cloud_f32(final.astype(np.float32), src)
        if X.shape[0]:
            d, j = tree.query(X.astype(np.float64), k=1)
            d2 = (d * d)
        else:
            d2, j = np.zeros(0), np.zeros(0, np.int64)
        keep = d2.astype(np.float32) <= r2
        n_c = int(keep.sum())
        if n_c < min_correspondences:
            state, converged = NO_CORRESPONDENCES, False
            break
        p = X[keep].astype(np.float64)
        q = tgt[j[keep]].astype(np.float64)
        Tk = umeyama(p, q)
        final = Tk @ final
        mse = float(d2[keep].mean())
        out["trace"].append(dict(Tk=Tk.copy(), final=final.copy(), n_corr=n_c, mse=mse))
        nr += 1
        if nr >= max_iterations:
            converged, state = True, ITERATIONS
        elif not force_iterations:
            cos_angle = 0.5 * (np.trace(Tk[:3, :3]) - 1.0)
            tsq = float(Tk[:3, 3] @ Tk[:3, 3])
            if cos_angle >= 1.0 - transformation_epsilon and tsq <= transformation_epsilon:
                converged, state = True, TRANSFORM
            elif abs(mse - mse_prev) < 1e-12:
                converged, state = True, ABS_MSE
            elif abs(mse - mse_prev) / mse_prev < euclidean_fitness_epsilon:
                converged, state = True, REL_MSE
            mse_prev = mse
        if converged:
            break
    out.update(T=final.astype(np.float32), converged=converged, iterations=nr, state=state, n_corr=n_c, mse=mse)
    if want_fitness and src.shape[0]:
        X = transform_cloud_f32(final.astype(np.float32), src)
        d, _ = tree.query(X.astype(np.float64), k=1)
        out["fitness"] = float((d * d).mean())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the 17 point-to-point sums, the second restatement of oracle/icp_oracle.c's orc_reduce_ex: the fma chain of p = T s rounded
# once per step (no double rounding), the terms widened, math.fsum for the exact sums
# ---------------------------------------------------------------------------------------------------------------------
def fma_f32(a, b, c):
    """fmaf(a, b, c) for float32 arrays of finite values, correctly rounded: a b is exact in float64, TwoSum gives a b + c as a
    rounded float64 s and its exact error e, and where s is the midpoint of two neighbouring floats e decides the side."""
    f = np.float32
    ab = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = ab + c
    bb = s - ab
    e = (ab - (s - bb)) + (c - bb)
    r = s.astype(f)
    d = r.astype(np.float64)
    other = np.where(s > d, np.nextafter(r, f(np.inf)), np.nextafter(r, f(-np.inf))).astype(f)
    tie = (d != s) & ((other.astype(np.float64) + d) * 0.5 == s) & (e != 0.0)
    return np.where(tie, np.where(e > 0.0, np.maximum(r, other), np.minimum(r, other)), r).astype(f)


def transform_cloud_fma(T32, xyz):
    """p.x = fma(m02, s.z, fma(m01, s.y, fma(m00, s.x, m03))) ... in float32, rows of finite points"""
    T = np.asarray(T32, np.float32)
    xyz = np.asarray(xyz, np.float32)
    out = np.empty((xyz.shape[0], 3), np.float32)
    for r in range(3):
        acc = np.full(xyz.shape[0], T[r, 3], np.float32)
        for k in range(3):
            acc = fma_f32(np.full(xyz.shape[0], T[r, k], np.float32), xyz[:, k], acc)
        out[:, r] = acc
    return out


def reduce_sums(src, tgt, T32, idx, d2, max_dist, absolute=False):
    """(17,) float64: the exact sums (of the magnitudes with absolute) of 1, p, q, q p^T row by row and d2 over the pairs with
    idx >= 0 and (double)d2 <= max_dist^2, each rounded once (math.fsum)."""
    import math
    idx = np.asarray(idx)
    d2 = np.asarray(d2, np.float32)
    keep = (idx >= 0) & (d2.astype(np.float64) <= max_dist * max_dist)
    p = transform_cloud_fma(T32, np.asarray(src, np.float32)[keep, :3]).astype(np.float64)
    q = np.asarray(tgt, np.float32)[idx[keep], :3].astype(np.float64)
    cols = [np.ones(p.shape[0])] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)]
    cols += [q[:, a] * p[:, b] for a in range(3) for b in range(3)] + [d2[keep].astype(np.float64)]
    return np.array([math.fsum(np.abs(c) if absolute else c) for c in cols])


# ---------------------------------------------------------------------------------------------------------------------
# point-to-plane (pcl::IterativeClosestPointWithNormals + TransformationEstimationPointToPlaneLLS), the second restatement
# of oracle/p2plane_oracle.c: float32 terms from NumPy casts, math.fsum for the exact sums, the LU in plain Python floats,
# sin / cos from mpmath at 120 bits rounded once.  Correspondences from the library kd-tree, re-ranked by the float32 key.
# ---------------------------------------------------------------------------------------------------------------------
def _d2_f32(q, p):
    """fma(dz, dz, fma(dy, dy, dx dx)) in float32 (a float product is exact in float64; the cast is the fma's rounding, which
    only an exact float32 midpoint could double-round)"""
    f = np.float32
    dx, dy, dz = ((q[:, k] - p[:, k]).astype(f).astype(np.float64) for k in range(3))
    a = (dx * dx).astype(f).astype(np.float64)
    a = (dy * dy + a).astype(f).astype(np.float64)
    return (dz * dz + a).astype(f)


def nn_f32(X, tgt, tree=None, fin=None, k=8):
    """(idx, d2): the lowest (float32 d2, index) among the k nearest in float64; -1 for non-finite queries or no target"""
    n = X.shape[0]
    idx = np.full(n, -1, np.int64)
    d2 = np.full(n, np.inf, np.float32)
    if fin is None:
        fin = np.flatnonzero(np.isfinite(tgt).all(axis=1))
    if n == 0 or fin.size == 0:
        return idx, d2
    if tree is None:
        tree = cKDTree(tgt[fin].astype(np.float64), leafsize=15)
    ok = np.isfinite(X).all(axis=1)
    kk = min(k, fin.size)
    _, jj = tree.query(X[ok].astype(np.float64), k=kk)
    jj = fin[np.asarray(jj).reshape(-1, kk)]
    cand = np.stack([_d2_f32(tgt[jj[:, c]], X[ok]) for c in range(kk)], axis=1)
    best = cand.min(axis=1)
    jbest = np.where(cand == best[:, None], jj, np.iinfo(np.int64).max).min(axis=1)
    idx[ok], d2[ok] = jbest, best
    return idx, d2


def p2plane_terms(s, d, n):
    """The float32 terms of estimateRigidTransformation for pairs (s = T source, d = target, n = normal): (m, 29) float64
    columns 2.. (columns 0, 1 left to the caller)"""
    f = np.float32
    sx, sy, sz = (s[:, k].astype(f) for k in range(3))
    nx, ny, nz = (n[:, k].astype(f) for k in range(3))
    dx, dy, dz = (d[:, k].astype(f) for k in range(3))
    a = (nz * sy) - (ny * sz)
    b = (nx * sz) - (nz * sx)
    c = (ny * sx) - (nx * sy)
    r = ((nx * dx) + (ny * dy)) + (nz * dz)
    r = ((r - (nx * sx)) - (ny * sy)) - (nz * sz)
    W = np.stack([a, b, c, nx, ny, nz], axis=1).astype(np.float64)
    iu = np.triu_indices(6)
    return np.concatenate([(W[:, :, None] * W[:, None, :])[:, iu[0], iu[1]], W * r.astype(np.float64)[:, None]], axis=1)


def p2plane_sums(X, tgt, nrm, idx, d2, max_dist):
    import math
    keep = (idx >= 0) & (d2.astype(np.float64) <= max_dist * max_dist)
    j = idx[keep]
    n = nrm[j, :3]
    fin = np.isfinite(n).all(axis=1)
    terms = p2plane_terms(X[keep][fin], tgt[j][fin], n[fin])
    sums = [float(keep.sum()), math.fsum(d2[keep].astype(np.float64))]
    sums += [math.fsum(terms[:, k]) for k in range(27)]
    return np.array(sums)


def p2plane_solve(sums):
    """symmetrise, Eigen's PartialPivLU (first of equal pivots), inverse column by column, x = inv b, PCL's
    constructTransformationMatrix with correctly rounded sin / cos; None when singular"""
    import mpmath
    A = [[0.0] * 6 for _ in range(6)]
    it = iter(sums[2:23])
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(next(it))
    b = [float(v) for v in sums[23:29]]
    perm = list(range(6))
    for k in range(6):
        p, m = k, abs(A[k][k])
        for i in range(k + 1, 6):
            if abs(A[i][k]) > m:
                p, m = i, abs(A[i][k])
        if not m > 0.0:
            return None
        A[k], A[p] = A[p], A[k]
        perm[k], perm[p] = perm[p], perm[k]
        for i in range(k + 1, 6):
            A[i][k] = A[i][k] / A[k][k]
            for j in range(k + 1, 6):
                A[i][j] = A[i][j] - A[i][k] * A[k][j]
    inv = [[0.0] * 6 for _ in range(6)]
    for col in range(6):
        y = [1.0 if perm[i] == col else 0.0 for i in range(6)]
        for i in range(6):
            for j in range(i):
                y[i] = y[i] - A[i][j] * y[j]
        for i in reversed(range(6)):
            for j in range(i + 1, 6):
                y[i] = y[i] - A[i][j] * y[j]
            y[i] = y[i] / A[i][i]
        for i in range(6):
            inv[i][col] = y[i]
    x = []
    for i in range(6):
        acc = 0.0
        for j in range(6):
            acc = acc + inv[i][j] * b[j]
        if not np.isfinite(acc):
            return None
        x.append(acc)
    with mpmath.workprec(120):
        sc = [(float(mpmath.sin(mpmath.mpf(v))), float(mpmath.cos(mpmath.mpf(v)))) if abs(v) <= 524288.0
              else (float(np.sin(v)), float(np.cos(v))) for v in x[:3]]
    (sa, ca), (sb, cb), (sg, cg) = sc
    return np.array([[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca, x[3]],
                     [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def p2plane_align(src, tgt, nrm, max_iterations=10, transformation_epsilon=1e-6, max_correspondence_distance=1.0,
                  euclidean_fitness_epsilon=-np.finfo(np.float64).max, min_correspondences=3, guess=None,
                  force_iterations=False, want_fitness=False):
    """The second restatement of orc_p2plane_align; nrm (n_t, >= 3) the target's normals.  trace entries: final (before the
    step), Tk, sums, n_corr, mse"""
    from oracle.gicp_oracle_np import transform_f32
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32)[:, :3]
    nrm = np.asarray(nrm, np.float32)[:, :3]
    out = dict(T=np.eye(4, dtype=np.float32), converged=False, iterations=0, state=NOT_CONVERGED, n_corr=0, mse=0.0,
               fitness=float("nan"), trace=[])
    if tgt.shape[0] == 0:
        return out
    fin = np.flatnonzero(np.isfinite(tgt).all(axis=1))
    tree = cKDTree(tgt[fin].astype(np.float64), leafsize=15) if fin.size else None
    final = np.eye(4) if guess is None else np.asarray(guess, np.float32).astype(np.float64)
    mse_prev = np.finfo(np.float64).max
    nr, converged, state, n_c, mse = 0, False, NOT_CONVERGED, 0, 0.0
    while True:
        X = transform_f32(src, final.astype(np.float32))
        idx, d2 = nn_f32(X, tgt, tree, fin)
        sums = p2plane_sums(X, tgt, nrm, idx, d2, max_correspondence_distance)
        n_c = int(sums[0])
        if n_c < min_correspondences:
            state, converged = NO_CORRESPONDENCES, False
            break
        Tk = p2plane_solve(sums)
        if Tk is None:
            state, converged = NOT_CONVERGED, False
            break
        mse = sums[1] / sums[0]
        out["trace"].append(dict(final=final.copy(), Tk=Tk, sums=sums, n_corr=n_c, mse=mse))
        final = Tk @ final
        nr += 1
        if nr >= max_iterations:
            converged, state = True, ITERATIONS
        elif not force_iterations:
            cos_angle = 0.5 * (np.trace(Tk[:3, :3]) - 1.0)
            tsq = float(Tk[:3, 3] @ Tk[:3, 3])
            if cos_angle >= 1.0 - transformation_epsilon and tsq <= transformation_epsilon:
                converged, state = True, TRANSFORM
            elif abs(mse - mse_prev) < 1e-12:
                converged, state = True, ABS_MSE
            elif abs(mse - mse_prev) / mse_prev < euclidean_fitness_epsilon:
                converged, state = True, REL_MSE
            mse_prev = mse
        if converged:
            break
    out.update(T=final.astype(np.float32), converged=converged, iterations=nr, state=state, n_corr=n_c, mse=mse)
    if want_fitness:
        X = transform_f32(src, final.astype(np.float32))
        _, d2 = nn_f32(X, tgt, tree, fin)
        ok = np.isfinite(d2)
        out["fitness"] = float(d2[ok].astype(np.float64).mean()) if ok.any() else float(np.finfo(np.float64).max)
    return out


# ---- pcl::VoxelGrid<PointXYZ>::filter, third statement (oracle/icp_oracle.c: orc_voxel_grid; the library: icp_voxel_plan.h) ----
INT32_MAX = 2**31 - 1
VOXEL_FILTER, VOXEL_NO_FINITE_POINT, VOXEL_PASS_THROUGH = "filter", "no finite point", "pass-through"


def voxel_plan_np(lo, hi, leaf):
    """What the filter does with a cloud whose finite points have the bounding box [lo, hi]: (verdict, min_b, div_b), the last two
    as Python integers (None unless the verdict is VOXEL_FILTER).  float32 where PCL computes in float, Python integers -- which
    cannot wrap -- everywhere else.  The input comes back unchanged (PCL: "leaf size is too small ... integer indices would
    overflow") exactly when, on some axis, (hi - lo) * inv is not finite or reaches 2^63, or floor(lo * inv) / floor(hi * inv) is
    no int32, or when the product of the extents int((hi - lo) * inv) + 1 exceeds INT32_MAX (PCL's rule where
    PCL's int64 / int32 arithmetic is defined, its stated intent where it is not)."""
    f32 = np.float32
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    if not bool((lo <= hi).all()):
        return VOXEL_NO_FINITE_POINT, None, None
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(leaf)
        span = (hi - lo) * inv
        first, last = np.floor(lo * inv), np.floor(hi * inv)
    assert span.dtype == first.dtype == last.dtype == f32
    if not np.isfinite(span).all() or not np.isfinite(first).all() or not np.isfinite(last).all():
        return VOXEL_PASS_THROUGH, None, None
    d = [int(v) + 1 for v in span]                        # a finite float32 is an integer-valued fraction: int() is exact
    first, last = [int(v) for v in first], [int(v) for v in last]
    if max(d) - 1 >= 2**63 or min(first) < -2**31 or max(last) > INT32_MAX or max(first) > INT32_MAX or min(last) < -2**31:
        return VOXEL_PASS_THROUGH, None, None
    if d[0] * d[1] * d[2] > INT32_MAX:
        return VOXEL_PASS_THROUGH, None, None
    return VOXEL_FILTER, first, [b - a + 1 for a, b in zip(first, last)]


def voxel_grid_np(cloud, leaf):
    """The filter itself for small clouds: one float32 mean per occupied cell, members added in input order, cells ascending by
    PCL's int32 index (reduced from the exact integer index: it wraps when the integer extents exceed the float ones)."""
    f32 = np.float32
    cloud = np.ascontiguousarray(cloud, f32)
    fin = np.isfinite(cloud[:, :3]).all(axis=1)
    pts = cloud[fin, :3]
    if not len(pts):
        return np.empty((0, 4), f32)
    verdict, minb, divb = voxel_plan_np(pts.min(axis=0), pts.max(axis=0), leaf)
    if verdict == VOXEL_PASS_THROUGH:
        return cloud.copy()
    inv = f32(1.0) / f32(leaf)
    cells = {}
    for p in pts:
        ijk = [int(v) - m for v, m in zip(np.floor(p * inv), minb)]
        idx = (ijk[0] + ijk[1] * divb[0] + ijk[2] * divb[0] * divb[1]) % 2**32
        cells.setdefault(idx - 2**32 if idx >= 2**31 else idx, []).append(p)
    out = np.ones((len(cells), 4), f32)
    for row, key in enumerate(sorted(cells)):
        acc = np.zeros(3, f32)
        for p in cells[key]:
            acc = acc + p
        out[row, :3] = acc / f32(len(cells[key]))
    return out
