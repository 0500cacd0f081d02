"""An independent NumPy restatement of the outlier filters (include/icpgpu.h, "outlier removal"): PCL 1.8's
StatisticalOutlierRemoval and RadiusOutlierRemoval, rule by rule, brute force in row chunks.  It never calls the library.
(sor_distances_literal / ror_counts_literal: the same with the exact expression on every pair, for small clouds -- what the chunked
forms, whose plain-float32 pass only narrows the pairs that get the exact expression, are tested against.)

    d2            float32, dx = q.x - p.x, ...; fma(dz, dz, fma(dy, dy, dx * dx)) with the fused operations emulated exactly
    SOR dist      the mean_k + 1 smallest d2 over the finite points (the point itself included), the smallest dropped, np.sqrt on
                  float32, added in ascending order into a Python float, divided by mean_k, rounded to float32
    SOR stats     math.fsum for sum and sq_sum (exact, rounded once), then IEEE float64 operation by operation
    ROR k         the finite points with d2 < (float32)(radius * radius), strict
"""
from __future__ import annotations

import math

import numpy as np

F32, F64 = np.float32, np.float64
SOR_MAX_K = 63


class Refused(ValueError):
    """The library answers ICPGPU_ERR_INVALID_ARG."""


def fma32(a, b, c):
    """fmaf(a, b, c) exactly: the float64 product of two floats is exact; the one double rounding of the sum is undone where it
    lands on a float32 midpoint."""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    p = a.astype(F64) * b.astype(F64)
    c64 = c.astype(F64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    r = s.astype(F32)
    r64 = r.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        other = np.nextafter(r, np.where(s > r64, F32(np.inf), F32(-np.inf)).astype(F32))
        mid = (r64 + other.astype(F64)) * 0.5
        tie = (s == mid) & (e != 0) & (s != r64)
    return np.where(tie, np.where(e > 0, np.maximum(r, other), np.minimum(r, other)), r).astype(F32)


def finite_mask(cloud) -> np.ndarray:
    return np.isfinite(np.asarray(cloud, F32)[:, :3]).all(axis=1)


def d2_rows(p, q) -> np.ndarray:
    """d2 of every point of p (rows) against every point of q (columns), float32."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    dx = q[None, :, 0] - p[:, None, 0]
    dy = q[None, :, 1] - p[:, None, 1]
    dz = q[None, :, 2] - p[:, None, 2]
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def _chunks(n, m):
    rows = max(1, min(n, (1 << 21) // max(m, 1)))
    for a in range(0, n, rows):
        yield a, min(n, a + rows)


# A plain float32 expression (no fused operation) is within a few ulp of d2: it only NARROWS which pairs get the exact expression.
# Every pair within _SLACK (relative) of a decision -- the K-th smallest, the radius -- is decided by the exact expression.
_SLACK = F32(1e-5)


def _plain_rows(p, q) -> np.ndarray:
    dx = q[None, :, 0] - p[:, None, 0]
    dy = q[None, :, 1] - p[:, None, 1]
    dz = q[None, :, 2] - p[:, None, 2]
    return dx * dx + dy * dy + dz * dz


def _d2_pairs(p, q) -> np.ndarray:
    """d2 of p[..., :] against q[..., :] element by element (same leading shape)."""
    dx, dy, dz = (q[..., k] - p[..., k] for k in range(3))
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def k_smallest_d2(p, q, K: int) -> np.ndarray:
    """The K smallest d2 of every row point against all of q, ascending (float32)."""
    m = q.shape[0]
    E = min(m, K + 8)
    if E == m:
        return np.sort(d2_rows(p, q), axis=1)[:, :K]
    with np.errstate(over="ignore", invalid="ignore"):
        plain = _plain_rows(p, q)
        idx = np.argpartition(plain, E - 1, axis=1)[:, :E]
        sel = np.sort(np.take_along_axis(plain, idx, axis=1), axis=1)
        sure = sel[:, E - 1] > sel[:, K - 1] * (F32(1) + _SLACK)  # nothing outside the E candidates can reach the K smallest
    near = np.sort(_d2_pairs(np.broadcast_to(p[:, None, :], (p.shape[0], E, 3)), q[idx]), axis=1)[:, :K]
    for i in np.flatnonzero(~sure):
        near[i] = np.sort(d2_rows(p[i:i + 1], q), axis=1)[0, :K]
    return near


def sor_distances(cloud, mean_k: int) -> np.ndarray:
    cloud = np.asarray(cloud, F32)
    fin = finite_mask(cloud)
    pts = cloud[fin, :3]
    m = pts.shape[0]
    if not 1 <= mean_k <= SOR_MAX_K or m < mean_k + 1:
        raise Refused(f"mean_k {mean_k}, {m} finite points")
    K = mean_k + 1
    near = np.empty((m, K), F32)
    for a, b in _chunks(m, m):
        near[a:b] = k_smallest_d2(pts[a:b], pts, K)
    roots = np.sqrt(near[:, 1:])  # (float32 in, float32 out: correctly rounded)
    dist_f = np.empty(m, F32)
    for i in range(m):
        s = 0.0
        for v in roots[i].tolist():
            s += v
        dist_f[i] = F32(s / float(mean_k))
    dist = np.zeros(cloud.shape[0], F32)
    dist[fin] = dist_f
    return dist


def sor_stats(dist, n_valid: int, stddev_mult: float) -> dict:
    d = [float(v) for v in np.asarray(dist, F32)]
    total = math.fsum(d)
    sq_total = math.fsum(v * v for v in d)  # (v * v is exact in float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = F64(n_valid)
        mean = F64(total) / nv
        var = (F64(sq_total) - F64(total) * F64(total) / nv) / (nv - F64(1.0))
        stddev = np.sqrt(var)
        threshold = mean + F64(stddev_mult) * stddev
    return {"mean": float(mean), "stddev": float(stddev), "threshold": float(threshold), "n_valid": int(n_valid)}


def _result(cloud, measure, removed_mask, extra=None) -> dict:
    idx = np.arange(cloud.shape[0], dtype=np.int32)
    out = {"measure": measure, "kept": idx[~removed_mask], "removed": idx[removed_mask], "cloud": cloud[~removed_mask].copy()}
    out.update(extra or {})
    return out


def statistical_outlier_removal(cloud, mean_k: int, stddev_mult: float, negative: bool = False) -> dict:
    cloud = np.ascontiguousarray(cloud, F32)
    if cloud.shape[0] == 0:
        if not 1 <= mean_k <= SOR_MAX_K:
            raise Refused("mean_k")
        return _result(cloud, np.zeros(0, F32), np.zeros(0, bool), {"mean": 0.0, "stddev": 0.0, "threshold": 0.0, "n_valid": 0})
    dist = sor_distances(cloud, mean_k)
    st = sor_stats(dist, int(finite_mask(cloud).sum()), stddev_mult)
    d64, thr = dist.astype(F64), F64(st["threshold"])
    with np.errstate(invalid="ignore"):
        removed = (d64 <= thr) if negative else (d64 > thr)
    return _result(cloud, dist, removed, st)


def ror_counts(cloud, radius: float) -> np.ndarray:
    cloud = np.asarray(cloud, F32)
    fin = finite_mask(cloud)
    pts = cloud[fin, :3]
    m = pts.shape[0]
    r2 = F32(float(radius) * float(radius))
    k_f = np.zeros(m, np.int64)
    if r2 > 0:
        for a, b in _chunks(m, m):
            with np.errstate(over="ignore", invalid="ignore"):
                plain = _plain_rows(pts[a:b], pts)
                inside = plain < r2 * (F32(1) - _SLACK)
                close = ~inside & ~(plain > r2 * (F32(1) + _SLACK))
            k_f[a:b] = inside.sum(axis=1)
            rows, cols = np.nonzero(close)
            if rows.size:
                np.add.at(k_f, a + rows, (_d2_pairs(pts[a + rows], pts[cols]) < r2).astype(np.int64))
    k = np.zeros(cloud.shape[0], np.int64)
    k[fin] = k_f
    return k


def radius_outlier_removal(cloud, radius: float, min_pts: int, negative: bool = False) -> dict:
    cloud = np.ascontiguousarray(cloud, F32)
    if not math.isfinite(radius) or radius < 0 or min_pts < 0:
        raise Refused("radius / min_pts")
    k = ror_counts(cloud, radius)
    removed = (k > min_pts) if negative else (k <= min_pts)
    return _result(cloud, k.astype(F32), removed, {"k": k})


def sor_distances_literal(cloud, mean_k: int) -> np.ndarray:
    """sor_distances without the narrowing pass: the exact d2 of every pair."""
    cloud = np.asarray(cloud, F32)
    fin = finite_mask(cloud)
    pts = cloud[fin, :3]
    near = np.sort(d2_rows(pts, pts), axis=1)[:, 1:mean_k + 1]
    roots = np.sqrt(near)
    dist = np.zeros(cloud.shape[0], F32)
    out = []
    for row in roots.tolist():
        s = 0.0
        for v in row:
            s += v
        out.append(F32(s / float(mean_k)))
    dist[fin] = np.array(out, F32)
    return dist


def ror_counts_literal(cloud, radius: float) -> np.ndarray:
    cloud = np.asarray(cloud, F32)
    fin = finite_mask(cloud)
    pts = cloud[fin, :3]
    k = np.zeros(cloud.shape[0], np.int64)
    k[fin] = (d2_rows(pts, pts) < F32(float(radius) * float(radius))).sum(axis=1)
    return k
