"""An independent NumPy restatement of the normal estimation (include/icpgpu.h, "normal estimation"):
pcl::NormalEstimation over a search surface.  It never calls the library.  Neighbour rows come from tests/search_restated.py; the
Jacobi sweeps are restated here.

    neighbours  row i of search_restated.knn(k) (its first n_found entries) or of search_restated.radius(radius, 0): ascending by key
    moments     float32, sequential in row order, about the row's first point K: nine accumulators a0..a8 over
                d = q - K (dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz, dx, dy, dz), each /= float32(m); cov = a_ij - a_i a_j;
                centroid = (a6, a7, a8) + K
    plane       the six entries in float64 through 8 cyclic Jacobi sweeps; the column of the smallest diagonal entry (lowest index
                among equals) rounded to float32; curvature = |float32(lambda) / tr| with tr = (xx + yy) + zz, 0 when tr == 0
    orientation v = viewpoint - query; cos = (vx*nx + vy*ny) + vz*nz in float32; negated when cos < 0
    NaN         m < 3 (a non-finite query has m = 0), or a non-finite covariance entry
"""
from __future__ import annotations

import math

import numpy as np

import search_restated as S

F32, F64 = np.float32, np.float64
JACOBI_SWEEPS = 8
Refused = S.Refused


def jacobi3(a):
    """Cyclic Jacobi on (m, 3, 3) symmetric float64 matrices: (the matrices after the sweeps -- eigenvalues on the diagonal --, V)."""
    a = np.array(a, F64)
    m = a.shape[0]
    v = np.zeros((m, 3, 3))
    v[:, [0, 1, 2], [0, 1, 2]] = 1.0
    with np.errstate(all="ignore"):
        for _sweep in range(JACOBI_SWEEPS):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = a[:, p, q].copy()
                on = apq != 0.0                      # a rotation whose entry is exactly zero is skipped
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                sign = np.where(theta >= 0.0, 1.0, -1.0)
                t = sign / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                new = {(p, p): a[:, p, p] - t * apq, (q, q): a[:, q, q] + t * apq, (p, q): np.zeros(m),
                       (r, p): c * arp - s * arq, (r, q): s * arp + c * arq}
                for (i, j), val in new.items():
                    a[:, i, j] = np.where(on, val, a[:, i, j])
                    a[:, j, i] = a[:, i, j]
                vp_, vq_ = v[:, :, p].copy(), v[:, :, q].copy()
                v[:, :, p] = np.where(on[:, None], c[:, None] * vp_ - s[:, None] * vq_, vp_)
                v[:, :, q] = np.where(on[:, None], s[:, None] * vp_ + c[:, None] * vq_, vq_)
    return a, v


def rows(cloud, queries, k: int = 0, radius: float = 0.0):
    """The neighbour rows in CSR form (start (n_q + 1,) int64, idx int32) for either mode."""
    if (k != 0) == (radius != 0.0):
        raise Refused("exactly one of k and radius")
    if k != 0:
        idx, _, n_found = S.knn(cloud, queries, k)              # (refuses k outside 1..64)
        keep = np.arange(idx.shape[1])[None, :] < n_found[:, None]
        return np.concatenate([[0], np.cumsum(n_found, dtype=np.int64)]).astype(np.int64), idx[keep].astype(np.int32)
    if not (math.isfinite(radius) and radius > 0):
        raise Refused("radius")
    start, idx, _ = S.radius(cloud, queries, radius, 0)
    return start, idx


def moments_of_rows(cloud, start, idx, about_origin: bool = False):
    """(counts int32, moments (n_q, 9) float32 = xx, xy, xz, yy, yz, zz, cx, cy, cz; NaN where m < 3).  about_origin: PCL 1.8's
    letter -- K = (0, 0, 0) instead of the row's first point -- for the accuracy comparison only."""
    xyz = np.asarray(cloud, F32).reshape(-1, 4)[:, :3]
    m = np.diff(start).astype(np.int64)
    n_q = len(m)
    out = np.full((n_q, 9), np.nan, F32)
    big = np.flatnonzero(m >= 3)
    if big.size:
        st, mb = start[:-1][big], m[big]
        K = np.zeros((big.size, 3), F32) if about_origin else xyz[idx[st]]
        acc = np.zeros((big.size, 9), F32)
        with np.errstate(all="ignore"):
            for t in range(int(mb.max())):
                sel = np.flatnonzero(mb > t)
                d = xyz[idx[st[sel] + t]] - K[sel]
                dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
                terms = (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz, dx, dy, dz)
                for e, term in enumerate(terms):
                    acc[sel, e] = acc[sel, e] + term
            acc = acc / mb.astype(F32)[:, None]
            mx, my, mz = acc[:, 6], acc[:, 7], acc[:, 8]
            res = np.stack([acc[:, 0] - mx * mx, acc[:, 1] - mx * my, acc[:, 2] - mx * mz, acc[:, 3] - my * my, acc[:, 4] - my * mz,
                            acc[:, 5] - mz * mz, mx + K[:, 0], my + K[:, 1], mz + K[:, 2]], axis=1)
        out[big] = res.astype(F32)
    return m.astype(np.int32), out


def plane_of_moments(moments, queries, viewpoint):
    """(n_q, 4) float32 {nx, ny, nz, curvature} from the moments, oriented towards the viewpoint as seen from the queries."""
    n_q = moments.shape[0]
    out = np.full((n_q, 4), np.nan, F32)
    ok = np.flatnonzero(np.isfinite(moments[:, :6]).all(axis=1))
    if ok.size == 0:
        return out
    c = moments[ok].astype(F32)
    a = np.zeros((ok.size, 3, 3))
    for e, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        a[:, i, j] = a[:, j, i] = c[:, e].astype(F64)
    d, V = jacobi3(a)
    lam = d[:, 0, 0].copy()
    col = np.zeros(ok.size, np.int64)
    for j in (1, 2):
        less = d[:, j, j] < lam
        lam = np.where(less, d[:, j, j], lam)
        col = np.where(less, j, col)
    with np.errstate(all="ignore"):
        nrm = np.take_along_axis(V, col[:, None, None], axis=2)[:, :, 0].astype(F32)
        tr = (c[:, 0] + c[:, 3]) + c[:, 5]
        curv = np.where(tr != 0, np.abs(lam.astype(F32) / tr), F32(0)).astype(F32)
        vp = np.asarray(viewpoint, F32).reshape(3)
        p = np.asarray(queries, F32).reshape(-1, 4)[ok, :3]
        v = vp[None, :] - p
        cos = (v[:, 0] * nrm[:, 0] + v[:, 1] * nrm[:, 1]) + v[:, 2] * nrm[:, 2]
        nrm = np.where((cos < 0)[:, None], -nrm, nrm)
    out[ok, :3] = nrm
    out[ok, 3] = curv
    return out


def estimate(cloud, queries, k: int = 0, radius: float = 0.0, viewpoint=(0.0, 0.0, 0.0)):
    """(normals (n_q, 4) float32, n_neighbours (n_q,) int32, moments (n_q, 9) float32)."""
    if not np.isfinite(np.asarray(viewpoint, F32)).all():
        raise Refused("viewpoint")
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    q = cloud if queries is None else np.asarray(queries, F32).reshape(-1, 4)
    start, idx = rows(cloud, queries, k, radius)
    counts, moments = moments_of_rows(cloud, start, idx)
    return plane_of_moments(moments, q, viewpoint), counts, moments


def estimate_literal(cloud, queries, k: int = 0, radius: float = 0.0, viewpoint=(0.0, 0.0, 0.0), about_origin: bool = False):
    """The rule point by point with float32 scalars (small clouds).  about_origin: PCL 1.8's letter -- the moments about (0, 0, 0)
    instead of the first neighbour -- for the accuracy comparison only."""
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    q = cloud if queries is None else np.asarray(queries, F32).reshape(-1, 4)
    start, idx = rows(cloud, queries, k, radius)
    vp = [F32(x) for x in viewpoint]
    n_q = q.shape[0]
    normals, counts, moments = np.full((n_q, 4), np.nan, F32), np.zeros(n_q, np.int32), np.full((n_q, 9), np.nan, F32)
    with np.errstate(all="ignore"):
        for i in range(n_q):
            row = idx[start[i]:start[i + 1]]
            m = len(row)
            counts[i] = m
            if m < 3:
                continue
            K = [F32(0)] * 3 if about_origin else [F32(x) for x in cloud[row[0], :3]]
            a = [F32(0)] * 9
            for j in row:
                dx, dy, dz = (F32(cloud[j, e]) - K[e] for e in range(3))
                for e, term in enumerate((dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz, dx, dy, dz)):
                    a[e] = F32(a[e] + F32(term))
            a = [F32(v / F32(m)) for v in a]
            cov = [F32(a[0] - F32(a[6] * a[6])), F32(a[1] - F32(a[6] * a[7])), F32(a[2] - F32(a[6] * a[8])), F32(a[3] - F32(a[7] * a[7])),
                   F32(a[4] - F32(a[7] * a[8])), F32(a[5] - F32(a[8] * a[8]))]
            moments[i] = cov + [F32(a[6] + K[0]), F32(a[7] + K[1]), F32(a[8] + K[2])]
            if not all(np.isfinite(v) for v in cov):
                continue
            A = np.array([[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]], F64)
            d, V = jacobi3(A[None])
            lam, col = d[0, 0, 0], 0
            for j in (1, 2):
                if d[0, j, j] < lam:
                    lam, col = d[0, j, j], j
            n = [F32(V[0, e, col]) for e in range(3)]
            tr = F32(F32(cov[0] + cov[3]) + cov[5])
            curv = F32(abs(F32(F32(lam) / tr))) if tr != 0 else F32(0)
            v = [F32(vp[e] - F32(q[i, e])) for e in range(3)]
            cos = F32(F32(F32(v[0] * n[0]) + F32(v[1] * n[1])) + F32(v[2] * n[2]))
            if cos < 0:
                n = [-x for x in n]
            normals[i] = n + [curv]
    return normals, counts, moments
