"""The rules of the segmentation from normals (include/icpgpu.h, "segmentation from normals") restated in NumPy / Python, operation
for operation, on top of sac_restated.py's generator, loop and plane refinement:

    samples   NORMAL_PLANE: the plane's triples (counter 3 t + c + 1); CYLINDER: two indices with the counter 2 t + c + 1
    models    the plane's model; the cylinder from two points and their normals (closest approach of the two normal lines), float32
    angle     folded_angle(y, x): one division, a degree-8 polynomial in t^2 by Horner's rule with emulated fmaf
    distance  val = w theta + (1 - w) d_e in float32, an inlier iff (double)val < distance_threshold
    loop      the plane's, with p = 1 - w w for the cylinder
    refine    NORMAL_PLANE: the plane's; CYLINDER: Gauss-Newton over 21 sums per pass (math.fsum of float64 terms), Cholesky in
              Python floats

segment() is the vectorised form the device is compared with; segment_literal() beside it is a per-hypothesis, per-point Python
loop with Python integers for the generator and, for the cylinder's refinement, fractions.Fraction sums of the float64 terms --
tests/test_sac_normals_host.py holds the two against each other bit for bit."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import sac_restated as SR
from sac_restated import Refused
from symmetric_restated import fma_f32

F32, F64 = np.float32, np.float64
NORMAL_PLANE, CYLINDER = 11, 5
CYLINDER_ITERATIONS = 10
STOP_PASSES, STOP_CHOLESKY, STOP_NOT_FINITE, STOP_SMALL_STEP, STOP_NO_DECREASE = 1, 2, 3, 4, 5
HALF_PI = F32(1.57079637050628662109375)
ANGLE_C = tuple(F32(float.fromhex(h)) for h in ("-0x1.55551ep-2", "0x1.998bbcp-3", "-0x1.23e71cp-3", "0x1.be6df6p-4", "-0x1.525702p-4",
                                                "0x1.c7f87cp-5", "-0x1.db5118p-6", "0x1.414704p-7", "-0x1.97ba58p-10"))
ANGLE_BOUND = 2.0 ** -22   # 2 ulp of pi / 2 (include/icpgpu.h, THE ANGLE)


# ---- the angle ---------------------------------------------------------------------------------------------------------------
def angle_poly(t):
    t = np.asarray(t, F32)
    with np.errstate(all="ignore"):
        s = (t * t).astype(F32)
        r = np.full(t.shape, ANGLE_C[8], F32)
        for k in range(7, -1, -1):
            r = fma_f32(r, s, np.full(t.shape, ANGLE_C[k], F32))
        return fma_f32((t * s).astype(F32), r, t)


def folded_angle(y, x):
    """A(y, x) for float32 arrays y = |m x g| >= 0, x = |m . g| >= 0."""
    y, x = np.broadcast_arrays(np.asarray(y, F32), np.asarray(x, F32))
    with np.errstate(all="ignore"):
        low = angle_poly((y / x).astype(F32))
        high = (HALF_PI - angle_poly((x / y).astype(F32))).astype(F32)
        out = np.where(y <= x, low, np.where(y > x, high, F32(np.nan))).astype(F32)
        return np.where(y == 0, F32(0), out).astype(F32)


def pair_angle(m, g):
    """theta of normals m (k, 3) against directions g (k, 3) or (3,), float32."""
    m = np.asarray(m, F32)
    g = np.broadcast_to(np.asarray(g, F32), m.shape)
    with np.errstate(all="ignore"):
        cx = m[:, 1] * g[:, 2] - m[:, 2] * g[:, 1]
        cy = m[:, 2] * g[:, 0] - m[:, 0] * g[:, 2]
        cz = m[:, 0] * g[:, 1] - m[:, 1] * g[:, 0]
        y = np.sqrt((cx * cx + cy * cy) + cz * cz).astype(F32)
        x = np.abs((m[:, 0] * g[:, 0] + m[:, 1] * g[:, 1]) + m[:, 2] * g[:, 2]).astype(F32)
    return folded_angle(y, x)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def check(model, normals, threshold, weight, radius_min, radius_max, max_iterations, probability, axis, eps_angle):
    if model not in (NORMAL_PLANE, CYLINDER):
        raise Refused("model")
    if normals is None:
        raise Refused("normals")
    if not (math.isfinite(threshold) and threshold >= 0.0):
        raise Refused("distance_threshold")
    if not 0.0 <= weight <= 1.0:
        raise Refused("normal_distance_weight")
    if not (math.isfinite(radius_min) and math.isfinite(radius_max) and radius_min >= 0.0 and radius_max >= 0.0):
        raise Refused("radius limits")
    if radius_max < radius_min and not (radius_min == 0.0 and radius_max == 0.0):
        raise Refused("radius limits")
    if not 0 <= max_iterations <= SR.MAX_ITERATIONS:
        raise Refused("max_iterations")
    if not 0.0 < probability < 1.0:
        raise Refused("probability")
    if axis is None:
        return None, 0.0
    if model == NORMAL_PLANE:
        raise Refused("an axis with NORMAL_PLANE")
    a = SR.unit_axis(axis)
    if not (math.isfinite(eps_angle) and eps_angle >= 0.0):
        raise Refused("eps_angle")
    return a, math.cos(eps_angle)


# ---- models ------------------------------------------------------------------------------------------------------------------
def samples2(seed: int, t0: int, m: int, n: int) -> np.ndarray:
    """(m, 2) int64: the cylinder's samples of hypotheses t0 .. t0 + m - 1, in uint64 arithmetic."""
    with np.errstate(over="ignore"):
        t = np.arange(t0, t0 + m, dtype=np.uint64)[:, None]
        c = np.arange(2, dtype=np.uint64)[None, :]
        z = np.uint64(seed & SR.MASK) + (np.uint64(2) * t + c + np.uint64(1)) * np.uint64(SR.GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(SR.MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(SR.MIX2)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def sample2_int(seed: int, t: int, c: int, n: int) -> int:
    z = (seed + (2 * t + c + 1) * SR.GOLDEN) & SR.MASK
    z = ((z ^ (z >> 30)) * SR.MIX1) & SR.MASK
    z = ((z ^ (z >> 27)) * SR.MIX2) & SR.MASK
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)


def cylinder_models(cloud, normals, S, radius_min=0.0, radius_max=0.0, axis=None, cos_eps: float = 0.0):
    """(coefficients (m, 7) float32 -- NaN where INVALID --, valid (m,) bool) of the sample rows S (m, 2)."""
    xyz = np.asarray(cloud, F32).reshape(-1, 4)[:, :3]
    nrm = np.asarray(normals, F32).reshape(-1, 4)[:, :3]
    m = S.shape[0]
    out = np.full((m, 7), np.nan, F32)
    valid = S[:, 0] != S[:, 1]
    if m == 0:
        return out, valid
    p1, p2, n1, n2 = xyz[S[:, 0]], xyz[S[:, 1]], nrm[S[:, 0]], nrm[S[:, 1]]
    for v in (p1, p2, n1, n2):
        valid = valid & np.isfinite(v).all(axis=1)
    with np.errstate(all="ignore"):
        w = p1 - p2
        a, b, c, d, e = _dot(n1, n1), _dot(n1, n2), _dot(n2, n2), _dot(n1, w), _dot(n2, w)
        den = a * c - b * b
        valid &= (den > 0) & np.isfinite(den)
        sc, tc = (b * e - c * d) / den, (a * e - b * d) / den
        A = p1 + sc[:, None] * n1
        B = p2 + tc[:, None] * n2
        u = B - A
        l2 = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        valid &= (l2 != 0) & np.isfinite(l2)
        direction = u / np.sqrt(l2)[:, None]
        x = _cross(p1 - A, direction)
        r = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        valid &= np.isfinite(A).all(axis=1) & np.isfinite(r)
        if radius_min != 0.0 or radius_max != 0.0:
            valid &= (r.astype(F64) >= radius_min) & (r.astype(F64) <= radius_max)
        if axis is not None:
            dd = direction.astype(F64)
            valid &= np.abs((F64(axis[0]) * dd[:, 0] + F64(axis[1]) * dd[:, 1]) + F64(axis[2]) * dd[:, 2]) >= cos_eps
    full = np.concatenate((A, direction, r[:, None]), axis=1).astype(F32)
    out[valid] = full[valid]
    return out, valid


# ---- distance ----------------------------------------------------------------------------------------------------------------
def values(model, cloud, normals, coeff, weight: float) -> np.ndarray:
    """(n,) float32: val of every point under the model; NaN for a point that can never be an inlier."""
    c = np.asarray(cloud, F32).reshape(-1, 4)
    nr = np.asarray(normals, F32).reshape(-1, 4)
    co = np.asarray(coeff, F32)
    W = F32(weight)
    ok = np.isfinite(c[:, :3]).all(axis=1) & np.isfinite(nr).all(axis=1)
    with np.errstate(all="ignore"):
        if model == NORMAL_PLANE:
            s = fma_f32(co[2], c[:, 2], fma_f32(co[1], c[:, 1], (co[0] * c[:, 0]).astype(F32))) + co[3]
            de = np.abs(s.astype(F32))
            w = (W * (F32(1) - nr[:, 3])).astype(F32)
            theta = pair_angle(nr[:, :3], co[:3])
        else:
            v = (c[:, :3] - co[:3]).astype(F32)
            d = np.broadcast_to(co[3:6], v.shape)
            x = _cross(v, d)
            dist = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).astype(F32)
            de = np.abs(dist - co[6]).astype(F32)
            t = _dot(v, d).astype(F32)
            g = (v - (t[:, None] * d).astype(F32)).astype(F32)
            ok &= ~((g == 0).all(axis=1))
            w = np.full(c.shape[0], W, F32)
            theta = pair_angle(nr[:, :3], g)
        val = ((w * theta).astype(F32) + ((F32(1) - w).astype(F32) * de).astype(F32)).astype(F32)
    return np.where(ok, val, F32(np.nan)).astype(F32)


def inlier_mask(model, cloud, normals, coeff, threshold: float, weight: float) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return values(model, cloud, normals, coeff, weight).astype(F64) < threshold


def next_k(count: int, n: int, probability: float, size: int) -> float:
    if size == 3:
        return SR.next_k(count, n, probability)
    w = count / float(n)
    p = 1.0 - w * w
    p = max(p, SR.DBL_EPSILON)
    p = min(p, 1.0 - SR.DBL_EPSILON)
    return math.log(1.0 - probability) / math.log(p)


# ---- the cylinder's refinement -------------------------------------------------------------------------------------------------
def cyl_terms(P, D, ia: int, ib: int, r: float, q) -> np.ndarray:
    """(k, 21) float64: the terms of the inliers q (k, 3) float32 for the axis P + s D."""
    q = np.asarray(q, F32).astype(F64)
    P, D = np.asarray(P, F64), np.asarray(D, F64)
    k = q.shape[0]
    with np.errstate(all="ignore"):
        v = q - P[None, :]
        Db = np.broadcast_to(D, v.shape)
        c = _cross(v, Db)
        cn = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        L2 = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
        L = np.sqrt(L2)
        dist, den = cn / L, cn * L
        u = _cross(Db, c)
        w = _cross(c, v)
        J = np.zeros((k, 5), F64)
        J[:, 0], J[:, 1] = -u[:, ia] / den, -u[:, ib] / den
        J[:, 2] = w[:, ia] / den - (dist * D[ia]) / L2
        J[:, 3] = w[:, ib] / den - (dist * D[ib]) / L2
        J[:, 4] = -1.0
        rho = dist - F64(r)
        on = cn == 0
        J[on, :4] = 0.0
        rho = np.where(on, -F64(r), rho)
    cols = [J[:, i] * J[:, j] for i in range(5) for j in range(i, 5)] + [J[:, i] * rho for i in range(5)] + [rho * rho]
    return np.stack(cols, axis=1)


def cyl_step(S):
    """delta (5 floats) of (J^T J) delta = -J^T rho by Cholesky in Python floats, or None where a pivot is not > 0."""
    S = [float(v) for v in S]
    A = [[0.0] * 5 for _ in range(5)]
    k = 0
    for i in range(5):
        for j in range(i, 5):
            A[i][j] = A[j][i] = S[k]
            k += 1
    L = [[0.0] * 5 for _ in range(5)]
    for j in range(5):
        s = A[j][j]
        for q in range(j):
            s -= L[j][q] * L[j][q]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 5):
            u = A[i][j]
            for q in range(j):
                u -= L[i][q] * L[j][q]
            L[i][j] = u / L[j][j]
    y = [0.0] * 5
    for i in range(5):
        u = -S[15 + i]
        for q in range(i):
            u -= L[i][q] * y[q]
        y[i] = u / L[i][i]
    delta = [0.0] * 5
    for i in range(4, -1, -1):
        u = y[i]
        for q in range(i + 1, 5):
            u -= L[q][i] * delta[q]
        delta[i] = u / L[i][i]
    return delta


def chart_of(unrefined, K):
    """(e, ia, ib, Ke, p0): the chart of the unrefined coefficients (7 float32) and the best sample's first point K."""
    u = [float(v) for v in np.asarray(unrefined, F32)]
    e = 0
    if abs(u[4]) > abs(u[3 + e]):
        e = 1
    if abs(u[5]) > abs(u[3 + e]):
        e = 2
    ia = 1 if e == 0 else 0
    ib = 1 if e == 2 else 2
    Ke = float(F32(K[e]))
    de, s = u[3 + e], Ke - u[e]
    p = [u[ia] + (s / de) * u[3 + ia], u[ib] + (s / de) * u[3 + ib], u[3 + ia] / de, u[3 + ib] / de, u[6]]
    return e, ia, ib, Ke, p


def chart_axis(e, ia, ib, Ke, p):
    P, D = [0.0] * 3, [0.0] * 3
    P[ia], P[ib], P[e] = p[0], p[1], Ke
    D[ia], D[ib], D[e] = p[2], p[3], 1.0
    return P, D


def cyl_refine(unrefined, K, pass_sums):
    """The Gauss-Newton loop: pass_sums(P, D, ia, ib, r) -> the 21 sums of a pass.  (coeff (7,) float32, sums (passes, 21), stop)"""
    e, ia, ib, Ke, p = chart_of(unrefined, K)
    record = []

    def take(q):
        P, D = chart_axis(e, ia, ib, Ke, q)
        S = [float(v) for v in pass_sums(P, D, ia, ib, q[4])]
        record.append(S)
        return S

    cur = take(p)
    while True:
        if len(record) >= CYLINDER_ITERATIONS:
            stop = STOP_PASSES
            break
        delta = cyl_step(cur)
        if delta is None:
            stop = STOP_CHOLESKY
            break
        trial = [p[a] + delta[a] for a in range(5)]
        if not all(math.isfinite(v) for v in trial):
            stop = STOP_NOT_FINITE
            break
        if max(abs(v) for v in delta) <= 1e-12 * (1.0 + max(abs(v) for v in p)):
            stop = STOP_SMALL_STEP
            break
        nxt = take(trial)
        if not nxt[20] < cur[20]:
            stop = STOP_NO_DECREASE
            break
        p, cur = trial, nxt
    P, D = chart_axis(e, ia, ib, Ke, p)
    length = math.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
    sign = -1.0 if float(np.asarray(unrefined, F32)[3 + e]) < 0 else 1.0
    coeff = np.array(P + [sign * (D[a] / length) for a in range(3)] + [abs(p[4])], F64).astype(F32)
    return coeff, np.array(record, F64).reshape(-1, 21), stop


def fsum_pass(cloud, inliers):
    xyz = np.asarray(cloud, F32).reshape(-1, 4)[:, :3]
    q = xyz[np.asarray(inliers, np.int64)]

    def sums(P, D, ia, ib, r):
        T = cyl_terms(P, D, ia, ib, r, q)
        return [math.fsum(T[:, e].tolist()) for e in range(21)]
    return sums


def fraction_pass(cloud, inliers):
    """The same sums by the letter: one inlier at a time, exact rational sums of the float64 terms, rounded once."""
    xyz = np.asarray(cloud, F32).reshape(-1, 4)[:, :3]
    idx = [int(i) for i in inliers]

    def sums(P, D, ia, ib, r):
        acc = [Fraction(0)] * 21
        for i in idx:
            T = cyl_terms(P, D, ia, ib, r, xyz[i:i + 1])[0]
            acc = [a + Fraction(float(t)) for a, t in zip(acc, T)]
        return [float(a) for a in acc]
    return sums


# ---- the call ----------------------------------------------------------------------------------------------------------------
def _finish(model, cloud, out, optimize, inliers_of, pass_of):
    nc = 4 if model == NORMAL_PLANE else 7
    out["found"] = int(out["best_t"] >= 0)
    out["moments"] = np.zeros(9, F64)
    out["cylinder_sums"] = np.zeros((0, 21), F64)
    out["cylinder_stop"] = 0
    out["coeff"] = np.zeros(nc, F32)
    out["inliers"] = np.zeros(0, np.int32)
    out["n_unrefined"] = 0
    if not out["found"]:
        out["coeff_unrefined"] = np.zeros(nc, F32)
        return out
    inliers = inliers_of(out["coeff_unrefined"])
    out["n_unrefined"] = int(inliers.size)
    out["coeff"] = out["coeff_unrefined"].copy()
    k_index = int(out["sample"][0])
    K = np.asarray(cloud, F32).reshape(-1, 4)[k_index, :3]
    if optimize and model == NORMAL_PLANE and inliers.size >= 3:
        out["moments"] = SR.moments_of(cloud, inliers, k_index)
        out["coeff"] = SR.refine(out["moments"], K, inliers.size, out["coeff_unrefined"])
        inliers = inliers_of(out["coeff"])
    elif optimize and model == CYLINDER and inliers.size >= 5:
        out["coeff"], out["cylinder_sums"], out["cylinder_stop"] = cyl_refine(out["coeff_unrefined"], K, pass_of(cloud, inliers))
        inliers = inliers_of(out["coeff"])
    out["inliers"] = inliers.astype(np.int32)
    return out


def expected_waits(out, optimize: bool, model: int) -> int:
    """The host-wait formula of the header's OUTPUT paragraph."""
    waits = (out["iterations"] + 63) // 64
    if optimize and model == NORMAL_PLANE and out["n_unrefined"] >= 3:
        waits += 2
    if optimize and model == CYLINDER and out["n_unrefined"] >= 5:
        waits += out["cylinder_sums"].shape[0] + 1
    return waits


def segment(model, cloud, normals, threshold: float, weight: float = 0.1, radius_min: float = 0.0, radius_max: float = 0.0,
            max_iterations: int = 50, probability: float = 0.99, seed: int = 0, optimize: bool = True, axis=None, eps_angle: float = 0.0) -> dict:
    """counts, iterations, best_t, sample (3,) int32 (the third -1 for a cylinder), coeff_unrefined, n_unrefined, moments,
    cylinder_sums (passes, 21), cylinder_stop, coeff, inliers int32 ascending, found."""
    a, cos_eps = check(model, normals, threshold, weight, radius_min, radius_max, max_iterations, probability, axis, eps_angle)
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    normals = np.asarray(normals, F32).reshape(-1, 4)
    n = cloud.shape[0]
    size = 3 if model == NORMAL_PLANE else 2
    counts, k, best, best_count, t = [], math.inf, -1, 0, 0
    sample, co = np.full(3, -1, np.int32), np.zeros(4 if model == NORMAL_PLANE else 7, F32)
    chunk_S = chunk_co = chunk_valid = None
    while n > 0 and t < max_iterations and float(t) < k:
        if t % 64 == 0:
            m = min(64, max_iterations - t)
            if model == NORMAL_PLANE:
                chunk_S = SR.samples(seed, t, m, n)
                chunk_co, chunk_valid = SR.models(cloud, chunk_S)
            else:
                chunk_S = samples2(seed, t, m, n)
                chunk_co, chunk_valid = cylinder_models(cloud, normals, chunk_S, radius_min, radius_max, a, cos_eps)
        h = t % 64
        count = int(inlier_mask(model, cloud, normals, chunk_co[h], threshold, weight).sum()) if chunk_valid[h] else -1
        counts.append(count)
        if count > 0 and count > best_count:
            best, best_count = t, count
            sample = np.full(3, -1, np.int32)
            sample[:size] = chunk_S[h]
            co = chunk_co[h].copy()
            k = next_k(count, n, probability, size)
        t += 1
    out = {"counts": np.array(counts, np.int32), "iterations": t, "best_t": best, "sample": sample, "coeff_unrefined": co}
    return _finish(model, cloud, out, optimize, lambda p: np.flatnonzero(inlier_mask(model, cloud, normals, p, threshold, weight)), fsum_pass)


# ---- the literal form ----------------------------------------------------------------------------------------------------------
def _f(v):
    return F32(v)


def angle_literal(y, x):
    y, x = F32(y), F32(x)
    with np.errstate(all="ignore"):
        def poly(t):
            s = F32(t * t)
            r = ANGLE_C[8]
            for k in range(7, -1, -1):
                r = F32(fma_f32(r, s, ANGLE_C[k]))
            return F32(fma_f32(F32(t * s), r, t))
        if y == 0:
            return F32(0)
        if y <= x:
            return poly(F32(y / x))
        if y > x:
            return F32(HALF_PI - poly(F32(x / y)))
        return F32(np.nan)


def _dot_l(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _cross_l(a, b):
    return [F32(F32(a[1] * b[2]) - F32(a[2] * b[1])), F32(F32(a[2] * b[0]) - F32(a[0] * b[2])), F32(F32(a[0] * b[1]) - F32(a[1] * b[0]))]


def _norm_l(x):
    return F32(np.sqrt(F32(F32(F32(x[0] * x[0]) + F32(x[1] * x[1])) + F32(x[2] * x[2]))))


def pair_angle_literal(m, g):
    with np.errstate(all="ignore"):
        return angle_literal(_norm_l(_cross_l(m, g)), F32(abs(_dot_l(m, g))))


def is_inlier_literal(model, co, q, nrow, threshold: float, weight: float) -> bool:
    if not all(math.isfinite(float(v)) for v in q[:3]) or not all(math.isfinite(float(v)) for v in nrow[:4]):
        return False
    W = F32(weight)
    m = [F32(v) for v in nrow[:3]]
    with np.errstate(all="ignore"):
        if model == NORMAL_PLANE:
            s = F32(F32(fma_f32(co[2], q[2], fma_f32(co[1], q[1], F32(co[0] * q[0])))) + co[3])
            de = F32(abs(s))
            w = F32(W * F32(F32(1) - F32(nrow[3])))
            theta = pair_angle_literal(m, co[:3])
        else:
            v = [F32(q[e] - co[e]) for e in range(3)]
            d = [co[3], co[4], co[5]]
            de = F32(abs(F32(_norm_l(_cross_l(v, d)) - co[6])))
            t = _dot_l(v, d)
            g = [F32(v[e] - F32(t * d[e])) for e in range(3)]
            if g[0] == 0 and g[1] == 0 and g[2] == 0:
                return False
            w = W
            theta = pair_angle_literal(m, g)
        val = F32(F32(w * theta) + F32(F32(F32(1) - w) * de))
    return float(val) < threshold


def cylinder_model_literal(p1, n1, p2, n2):
    """The seven coefficients of one pair of samples, or None."""
    with np.errstate(all="ignore"):
        w = [F32(p1[e] - p2[e]) for e in range(3)]
        a, b, c, d, e_ = _dot_l(n1, n1), _dot_l(n1, n2), _dot_l(n2, n2), _dot_l(n1, w), _dot_l(n2, w)
        den = F32(F32(a * c) - F32(b * b))
        if not den > 0 or not math.isfinite(float(den)):
            return None
        sc = F32(F32(F32(b * e_) - F32(c * d)) / den)
        tc = F32(F32(F32(a * e_) - F32(b * d)) / den)
        A = [F32(p1[e] + F32(sc * n1[e])) for e in range(3)]
        B = [F32(p2[e] + F32(tc * n2[e])) for e in range(3)]
        u = [F32(B[e] - A[e]) for e in range(3)]
        l2 = F32(F32(F32(u[0] * u[0]) + F32(u[1] * u[1])) + F32(u[2] * u[2]))
        if l2 == 0 or not math.isfinite(float(l2)):
            return None
        l = F32(np.sqrt(l2))
        direction = [F32(u[e] / l) for e in range(3)]
        r = _norm_l(_cross_l([F32(p1[e] - A[e]) for e in range(3)], direction))
        if not all(math.isfinite(float(v)) for v in A) or not math.isfinite(float(r)):
            return None
    return np.array(A + direction + [r], F32)


def segment_literal(model, cloud, normals, threshold: float, weight: float = 0.1, radius_min: float = 0.0, radius_max: float = 0.0,
                    max_iterations: int = 50, probability: float = 0.99, seed: int = 0, optimize: bool = True, axis=None,
                    eps_angle: float = 0.0) -> dict:
    """The same answer by the rules' letter: one hypothesis and one point at a time, scalars only."""
    a, cos_eps = check(model, normals, threshold, weight, radius_min, radius_max, max_iterations, probability, axis, eps_angle)
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    normals = np.asarray(normals, F32).reshape(-1, 4)
    n = cloud.shape[0]
    size = 3 if model == NORMAL_PLANE else 2

    def inliers_of(co):
        return np.array([i for i in range(n) if is_inlier_literal(model, co, cloud[i], normals[i], threshold, weight)], np.int64)

    def hypothesis(t):
        if model == NORMAL_PLANE:
            s = [SR.sample_int(seed, t, c, n) for c in range(3)]
            planes, valid = SR.models(cloud, np.array([s], np.int64))   # (the plane's model is test_sac_host.py's to hold to its letter)
            return s, (planes[0] if valid[0] else None)
        s = [sample2_int(seed, t, c, n) for c in range(2)]
        if s[0] == s[1]:
            return s, None
        p1, p2, n1, n2 = cloud[s[0], :3], cloud[s[1], :3], normals[s[0], :3], normals[s[1], :3]
        if not all(math.isfinite(float(v)) for x in (p1, p2, n1, n2) for v in x):
            return s, None
        co = cylinder_model_literal(p1, n1, p2, n2)
        if co is None:
            return s, None
        if (radius_min != 0.0 or radius_max != 0.0) and not radius_min <= float(co[6]) <= radius_max:
            return s, None
        if a is not None and not abs((a[0] * float(co[3]) + a[1] * float(co[4])) + a[2] * float(co[5])) >= cos_eps:
            return s, None
        return s, co

    counts, k, best, best_count, t = [], math.inf, -1, 0, 0
    sample, best_co = np.full(3, -1, np.int32), np.zeros(4 if model == NORMAL_PLANE else 7, F32)
    while n > 0 and t < max_iterations and float(t) < k:
        s, co = hypothesis(t)
        count = -1 if co is None else sum(is_inlier_literal(model, co, cloud[i], normals[i], threshold, weight) for i in range(n))
        counts.append(count)
        if count > 0 and count > best_count:
            best, best_count, best_co = t, count, co
            sample = np.full(3, -1, np.int32)
            sample[:size] = s
            k = next_k(count, n, probability, size)
        t += 1
    out = {"counts": np.array(counts, np.int32), "iterations": t, "best_t": best, "sample": sample, "coeff_unrefined": best_co}
    return _finish(model, cloud, out, optimize, inliers_of, fraction_pass)
