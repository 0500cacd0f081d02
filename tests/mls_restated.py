"""An independent NumPy restatement of the moving least squares projection (include/icpgpu.h, "moving least squares"):
pcl::MovingLeastSquares with UpsamplingMethod NONE over a search surface.  It never calls the library.  The radius rows come from
tests/search_restated.py, the Jacobi sweeps from tests/normals_restated.py; every other step is restated here in Python floats
(float64, one IEEE operation at a time -- NumPy fuses nothing), so the device's answers can be compared bit for bit.

    row      search_restated.radius(radius, 0)'s: d2 < float32(radius * radius), ascending by (d2, index); m entries, the first is j_0
    wsum     entry t into partial t mod 64 (from +0.0, ascending t); then for mask = 32 .. 1 partial[l] += partial[l ^ mask], all at
             once; the sum is partial 0
    plane    m >= 3.  d = q - K, K = cloud[j_0]; nine wsums dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz, each / m; covariance
             a_ij - a_i a_j; centroid a_i + K; 8 cyclic Jacobi sweeps; N = the column of the smallest diagonal entry (lowest index
             among equals); curvature = |float32(lambda / tr)|, tr = (xx + yy) + zz, 0 when tr == 0; dist = (P - c) . N; Q = P - dist N
    frame    Eigen's unitOrthogonal of N -> V; U = N x V
    fit      order >= 2 and m >= nc.  de = q - Q; w = exp_neg(-(de . de) / s); u, v, f = de . U, de . V, de . N; monomials in PCL's
             order; A_ab = wsum(P_a w P_b), b_a = wsum(P_a w f); Cholesky, forward and backward substitution
    result   status 0 (m < 3), 1 (plane only), 2 (polynomial: c_0 finite), 3 (fit refused); point Q + c_0 N, normal
             (N - c_(order+1) U) - c_1 V; else Q and N

project_exact is the same projection as a literal loop per query and per neighbour in fractions.Fraction -- exact sums, an exact
solve, numpy.linalg.eigh for the plane -- which shares no arithmetic with the rule: what project is held against.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import normals_restated as NR
import search_restated as S

F32, F64 = np.float32, np.float64
MAX_ORDER = 3
Refused = S.Refused
FIELDS = ("points", "normals", "index", "status", "n_neighbours", "plane7", "coeff10")

LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42feep-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
EXP_C = [float(Fraction(1, math.factorial(n))) for n in range(14)]        # the doubles nearest 1 / n!


def exp_neg(a):
    """exp(a) for a <= 0, elementwise, by the rule's steps."""
    a = np.asarray(a, F64)
    with np.errstate(all="ignore"):
        k = np.rint(a * LOG2E)
        r = (a - k * LN2_HI) - k * LN2_LO
        p = np.full(a.shape, EXP_C[13])
        for n in range(12, -1, -1):
            p = p * r + EXP_C[n]
        safe = np.where(np.isfinite(k), k, 0.0).astype(np.int64)
        w = np.ldexp(p, safe)
    return np.where(np.isnan(a), a, np.where(a < -708.0, 0.0, w))


def wsum(terms):
    """The rule's sum of a row's terms: (m,) -> a float, or (m, S) -> S sums at once."""
    terms = np.asarray(terms, F64)
    t2 = terms.reshape(terms.shape[0], int(np.prod(terms.shape[1:])))
    part = np.zeros((64, t2.shape[1]))
    with np.errstate(all="ignore"):
        for at in range(0, t2.shape[0], 64):
            block = t2[at:at + 64]
            part[:block.shape[0]] = part[:block.shape[0]] + block
        lanes = np.arange(64)
        for mask in (32, 16, 8, 4, 2, 1):
            part = part + part[lanes ^ mask]
    return float(part[0, 0]) if terms.ndim == 1 else part[0].copy()


def n_coefficients(order: int) -> int:
    return (order + 1) * (order + 2) // 2


def monomials(u, v, order: int):
    """PCL's order and PCL's powers: u_pow and v_pow by repeated multiplication from 1.0."""
    out = []
    u_pow = np.ones_like(u)
    for ui in range(order + 1):
        v_pow = np.ones_like(v)
        for _vi in range(order - ui + 1):
            out.append(u_pow * v_pow)
            v_pow = v_pow * v
        u_pow = u_pow * u
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def frame_of(N):
    """(U, V) of (k, 3) normals."""
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    with np.errstate(all="ignore"):
        first = (np.abs(nx) > 1e-12 * np.abs(nz)) | (np.abs(ny) > 1e-12 * np.abs(nz))
        inv1 = 1.0 / np.sqrt(nx * nx + ny * ny)
        inv2 = 1.0 / np.sqrt(ny * ny + nz * nz)
        zero = np.zeros_like(nx)
        V = np.where(first[:, None], np.stack([-ny * inv1, nx * inv1, zero], 1), np.stack([zero, -nz * inv2, ny * inv2], 1))
        U = np.stack([ny * V[:, 2] - nz * V[:, 1], nz * V[:, 0] - nx * V[:, 2], nx * V[:, 1] - ny * V[:, 0]], 1)
    return U, V


def cholesky_solve(A, b):
    """A (k, nc, nc; the lower triangle is read), b (k, nc) -> c (k, nc), the rule's order of operations, every system at once."""
    nc = b.shape[1]
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(nc):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            L[:, j, j] = np.sqrt(s)
            for i in range(j + 1, nc):
                s = A[:, i, j].copy()
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                L[:, i, j] = s / L[:, j, j]
        y = np.zeros_like(b)
        for i in range(nc):
            s = b[:, i].copy()
            for k in range(i):
                s = s - L[:, i, k] * y[:, k]
            y[:, i] = s / L[:, i, i]
        c = np.zeros_like(b)
        for i in range(nc - 1, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, nc):
                s = s - L[:, k, i] * c[:, k]
            c[:, i] = s / L[:, i, i]
    return c


def check_arguments(radius, order, sqr_gauss_param):
    if not (math.isfinite(radius) and radius > 0):
        raise Refused("radius")
    if not (isinstance(order, (int, np.integer)) and 0 <= order <= MAX_ORDER):
        raise Refused("order")
    if not (sqr_gauss_param == 0 or (math.isfinite(sqr_gauss_param) and sqr_gauss_param > 0)):
        raise Refused("sqr_gauss_param")


def project(cloud, queries, radius: float, order: int = 2, sqr_gauss_param: float = 0.0) -> dict:
    """dict(n_out, points (n_out, 4) f32, normals (n_out, 4) f32, index (n_out,) i32, and per query status i32, n_neighbours i32,
    plane7 (n_q, 7) f64, coeff10 (n_q, 10) f64)."""
    check_arguments(radius, order, sqr_gauss_param)
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    q = cloud if queries is None else np.asarray(queries, F32).reshape(-1, 4)
    n_q = q.shape[0]
    s = float(radius) * float(radius) if sqr_gauss_param == 0 else float(sqr_gauss_param)
    start, idx, _ = S.radius(cloud, queries, radius, 0)
    m = np.diff(start).astype(np.int64)
    xyz = cloud[:, :3].astype(F64)
    P = q[:, :3].astype(F64)
    status = np.zeros(n_q, np.int32)
    plane7 = np.full((n_q, 7), np.nan)
    coeff10 = np.full((n_q, 10), np.nan)
    pts = np.full((n_q, 4), np.nan, F32)
    nrm = np.full((n_q, 4), np.nan, F32)
    kept = np.flatnonzero(m >= 3)
    if kept.size:
        with np.errstate(all="ignore"):
            sums = np.empty((kept.size, 9))
            K = xyz[idx[start[kept]]]
            for r, i in enumerate(kept):
                d = xyz[idx[start[i]:start[i + 1]]] - K[r]
                dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
                sums[r] = wsum(np.stack([dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz, dx, dy, dz], 1))
            a = sums / m[kept].astype(F64)[:, None]
            xx, xy, xz = a[:, 0] - a[:, 6] * a[:, 6], a[:, 1] - a[:, 6] * a[:, 7], a[:, 2] - a[:, 6] * a[:, 8]
            yy, yz, zz = a[:, 3] - a[:, 7] * a[:, 7], a[:, 4] - a[:, 7] * a[:, 8], a[:, 5] - a[:, 8] * a[:, 8]
            c = a[:, 6:9] + K
            cov = np.stack([np.stack([xx, xy, xz], 1), np.stack([xy, yy, yz], 1), np.stack([xz, yz, zz], 1)], 1)
            d_, E = NR.jacobi3(cov)
            lam = d_[:, 0, 0].copy()
            col = np.zeros(kept.size, np.int64)
            for j in (1, 2):
                less = d_[:, j, j] < lam
                lam = np.where(less, d_[:, j, j], lam)
                col = np.where(less, j, col)
            N = np.take_along_axis(E, col[:, None, None], axis=2)[:, :, 0]
            tr = (xx + yy) + zz
            curv = np.where(tr != 0, np.abs((lam / tr).astype(F32)), F32(0)).astype(F32)
            e = P[kept] - c
            dist = _dot(e, N)
            Q = P[kept] - dist[:, None] * N
            U, V = frame_of(N)
        plane7[kept, 0:3], plane7[kept, 3:6], plane7[kept, 6] = N, c, lam
        status[kept] = 1
        pts[kept, :3], pts[kept, 3] = Q.astype(F32), 1
        nrm[kept, :3], nrm[kept, 3] = N.astype(F32), curv
        nc = n_coefficients(order)
        fit = np.flatnonzero(m[kept] >= nc) if order >= 2 else np.zeros(0, np.int64)
        if fit.size:
            with np.errstate(all="ignore"):
                A = np.zeros((fit.size, nc, nc))
                b = np.zeros((fit.size, nc))
                for r, k in enumerate(fit):
                    i = kept[k]
                    de = xyz[idx[start[i]:start[i + 1]]] - Q[k]
                    dd = (de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]) + de[:, 2] * de[:, 2]
                    w = exp_neg(-dd / s)
                    u, v, f = _dot(de, U[k][None]), _dot(de, V[k][None]), _dot(de, N[k][None])
                    mono = monomials(u, v, order)
                    pw = [p * w for p in mono]
                    terms = [pw[a_] * mono[b_] for a_ in range(nc) for b_ in range(a_ + 1)] + [pw[a_] * f for a_ in range(nc)]
                    sums_ = wsum(np.stack(terms, 1))
                    at = 0
                    for a_ in range(nc):
                        for b_ in range(a_ + 1):
                            A[r, a_, b_] = sums_[at]
                            at += 1
                    b[r] = sums_[at:]
                cf = cholesky_solve(A, b)
                rows = kept[fit]
                coeff10[rows, :nc] = cf
                good = np.isfinite(cf[:, 0])
                status[rows] = np.where(good, 2, 3)
                Qf, Nf, Uf, Vf = Q[fit], N[fit], U[fit], V[fit]
                point = Qf + cf[:, 0:1] * Nf
                normal = (Nf - cf[:, order + 1:order + 2] * Uf) - cf[:, 1:2] * Vf
                g = rows[good]
                pts[g, :3] = point[good].astype(F32)
                nrm[g, :3] = normal[good].astype(F32)
    out_rows = np.flatnonzero(status != 0)
    return {"n_out": int(out_rows.size), "points": pts[out_rows], "normals": nrm[out_rows], "index": out_rows.astype(np.int32), "status": status,
            "n_neighbours": m.astype(np.int32), "plane7": plane7, "coeff10": coeff10}


# ---- the literal loop in exact rationals ---------------------------------------------------------------------------------------
def _fr(x):
    return Fraction(float(x))


def project_exact(cloud, queries, radius: float, order: int = 2, sqr_gauss_param: float = 0.0, align_with=None, only=None) -> dict:
    """The projection per query and per neighbour with exact sums: the moments and the covariance as rationals rounded once, the
    plane by numpy.linalg.eigh, the weights math.exp's float64 values taken as rationals, A and b exact sums of exact products, the
    solve by Gaussian elimination in rationals.  align_with: (n_q, 3) normals whose sign the plane's normal takes (an eigenvector's
    sign is free).  only: the queries to do (the others stay NaN / status -1).  Returns status, n_neighbours, normal (n_q, 3), centroid,
    point (n_q, 3) float64, coeff (n_q, 10), singular (the elimination met a zero pivot), rcond (the reciprocal 2-norm condition number
    of A rounded to float64)."""
    check_arguments(radius, order, sqr_gauss_param)
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    q = cloud if queries is None else np.asarray(queries, F32).reshape(-1, 4)
    n_q = q.shape[0]
    s = float(radius) * float(radius) if sqr_gauss_param == 0 else float(sqr_gauss_param)
    start, idx, _ = S.radius_literal(cloud, queries, radius, 0) if n_q * cloud.shape[0] <= 1 << 20 else S.radius(cloud, queries, radius, 0)
    nc = n_coefficients(order)
    out = {"status": np.full(n_q, -1, np.int32), "n_neighbours": np.diff(start).astype(np.int32), "normal": np.full((n_q, 3), np.nan),
           "centroid": np.full((n_q, 3), np.nan), "point": np.full((n_q, 3), np.nan), "coeff": np.full((n_q, 10), np.nan),
           "singular": np.zeros(n_q, bool), "rcond": np.full(n_q, np.nan)}
    for i in (range(n_q) if only is None else only):
        row = idx[start[i]:start[i + 1]]
        m = len(row)
        if m < 3:
            out["status"][i] = 0
            continue
        pts = [[_fr(cloud[j, e]) for e in range(3)] for j in row]
        mean = [sum(p[e] for p in pts) / m for e in range(3)]
        cov = np.array([[float(sum((p[a] - mean[a]) * (p[b] - mean[b]) for p in pts) / m) for b in range(3)] for a in range(3)])
        lam, vec = np.linalg.eigh(cov)
        N = vec[:, 0]
        if align_with is not None and float(np.dot(N, align_with[i])) < 0:
            N = -N
        P = np.array([float(q[i, e]) for e in range(3)])
        c = np.array([float(x) for x in mean])
        Q = P - float(np.dot(P - c, N)) * N
        U, V = frame_of(N[None])
        U, V = U[0], V[0]
        out["normal"][i], out["centroid"][i], out["point"][i], out["status"][i] = N, c, Q, 1
        if order < 2 or m < nc:
            continue
        Qf, Uf, Vf, Nf = ([_fr(x) for x in vec_] for vec_ in (Q, U, V, N))
        A = [[Fraction(0)] * nc for _ in range(nc)]
        b = [Fraction(0)] * nc
        for p in pts:
            de = [p[e] - Qf[e] for e in range(3)]
            dd = sum(x * x for x in de)
            w = _fr(math.exp(-float(dd) / s))
            u, v, f = (sum(de[e] * axis[e] for e in range(3)) for axis in (Uf, Vf, Nf))
            mono = [u ** ui * v ** vi for ui in range(order + 1) for vi in range(order - ui + 1)]
            for a_ in range(nc):
                for b_ in range(nc):
                    A[a_][b_] += w * mono[a_] * mono[b_]
                b[a_] += w * mono[a_] * f
        Af = np.array([[float(x) for x in r_] for r_ in A])
        sv = np.linalg.svd(Af, compute_uv=False)
        out["rcond"][i] = sv[-1] / sv[0] if sv[0] > 0 else 0.0
        coeff = _solve_exact(A, b)
        if coeff is None:
            out["singular"][i], out["status"][i] = True, 3
            continue
        out["coeff"][i, :nc] = [float(x) for x in coeff]
        out["status"][i] = 2
        out["point"][i] = Q + out["coeff"][i, 0] * N
    return out


def _solve_exact(A, b):
    n = len(b)
    M = [row[:] + [b[i]] for i, row in enumerate(A)]
    for j in range(n):
        piv = next((r for r in range(j, n) if M[r][j] != 0), None)
        if piv is None:
            return None
        M[j], M[piv] = M[piv], M[j]
        for r in range(j + 1, n):
            if M[r][j] != 0:
                fct = M[r][j] / M[j][j]
                M[r] = [x - fct * y for x, y in zip(M[r], M[j])]
    x = [Fraction(0)] * n
    for i in range(n - 1, -1, -1):
        x[i] = (M[i][n] - sum(M[i][k] * x[k] for k in range(i + 1, n))) / M[i][i]
    return x
