"""An independent NumPy restatement of the fast point feature histograms (include/icpgpu.h, "fast point feature histograms";
DESIGN.md section 3): pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33> over a search surface.  It never calls the library.
Neighbour rows come from tests/search_restated.py; the ten edge directions of the angle bins are read from the header, the one
place they are written down.

    rows      row i of search_restated.knn(k) (its first n_found entries) or of search_restated.radius(radius, 0), with their d2
    pair      (p, j), j an entry of p's row with j != p; float32, every operation rounded on its own:
              d = P_j - P_p; f4 = sqrt((dx dx + dy dy) + dz dz); skipped when f4 == 0 or a normal component is not finite;
              a1 = (n_p . d) / f4, a2 = (n_j . d) / f4; swap iff |a1| < |a2| (n1 = n_j, n2 = n_p, d = -d, f3 = -a2; else f3 = a1);
              v = d x n1; vn = sqrt(|v|^2); skipped when vn == 0; v /= vn; w = n1 x v; f2 = v . n2; y = w . n2; x = n1 . n2
    bins      b2, b3 = clamp(floor(11.0 * ((f + 1.0) * 0.5)), 0, 10) in float64, NaN -> 0; b1 = the number of edges k with
              c_k * b - s_k * a >= 0 for (a, b) = (-x, -y): edges 1..5 when b >= 0, else 5 + those among edges 6..10
    spfh      integer counts c[b] of b1, 11 + b2, 22 + b3; incr = 100 / float32(m - 1); c == 0 ? 0 : float32(c) * incr; zeros for m < 2
    fpfh      over the query's row in order: d2 == 0 skipped; w = 1 / d2; h[b] += spfh[j][b] * w in float32; per sub-histogram
              s = ((h0 + h1) + ..) + h10 in float64; s != 0: h[b] *= float32(100.0 / s); NaN for a non-finite query
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

import search_restated as S

F32, F64 = np.float32, np.float64
BINS = 33
MIN_K = 2
Refused = S.Refused

_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "icpgpu.h")


def _edges():
    text = open(_HEADER).read()
    out = []
    for name in ("ICPGPU_FPFH_EDGE_COS", "ICPGPU_FPFH_EDGE_SIN"):
        body = re.search(r"#define\s+" + name + r"\s*\\?\s*\{(.*?)\}", text, flags=re.S).group(1)
        vals = [float.fromhex(tok.strip().rstrip("f")) for tok in body.replace("\\", " ").split(",")]
        arr = np.array(vals, F32)
        assert len(vals) == 10 and (arr.astype(F64) == np.array(vals)).all()  # (ten float32 constants, exactly)
        out.append(arr)
    return out


EDGE_COS, EDGE_SIN = _edges()


def rows(cloud, queries, k: int = 0, radius: float = 0.0):
    """The neighbour rows in CSR form (start (n_q + 1,) int64, idx int32, d2 float32) for either mode."""
    if (k != 0) == (radius != 0.0):
        raise Refused("exactly one of k and radius")
    if k != 0:
        if not MIN_K <= k <= S.SEARCH_MAX_K:
            raise Refused(f"k {k}")
        idx, d2, n_found = S.knn(cloud, queries, k)
        keep = np.arange(idx.shape[1])[None, :] < n_found[:, None]
        return np.concatenate([[0], np.cumsum(n_found, dtype=np.int64)]).astype(np.int64), idx[keep].astype(np.int32), d2[keep].astype(F32)
    if not (math.isfinite(radius) and radius > 0):
        raise Refused("radius")
    return S.radius(cloud, queries, radius, 0)


def angle_bin(y, x) -> np.ndarray:
    """b1 of arrays y, x (float32): the sector rule."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    a, b = -x, -y
    upper = b >= 0
    passed = np.where(upper, 0, 5).astype(np.int64)
    with np.errstate(all="ignore"):
        for e in range(5):
            c = np.where(upper, EDGE_COS[e], EDGE_COS[5 + e]).astype(F32)
            s = np.where(upper, EDGE_SIN[e], EDGE_SIN[5 + e]).astype(F32)
            passed = passed + ((c * b - s * a) >= 0)
    return passed


def unit_bin(f) -> np.ndarray:
    """b2 / b3 of an array f (float32)."""
    with np.errstate(all="ignore"):
        t = np.floor(11.0 * ((np.asarray(f, F32).astype(F64) + 1.0) * 0.5))
        t = np.where(t >= 0, np.minimum(t, 10.0), 0.0)   # (NaN: bin 0)
    return t.astype(np.int64)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def pair_bins(Pp, Np, Pj, Nj):
    """(ok, b1, b2, b3) of pairs given as (m, 3) float32 arrays."""
    Pp, Np, Pj, Nj = (np.asarray(v, F32).reshape(-1, 3) for v in (Pp, Np, Pj, Nj))
    with np.errstate(all="ignore"):
        d = Pj - Pp
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        f4 = np.sqrt((dx * dx + dy * dy) + dz * dz)
        ok = (f4 != 0) & np.isfinite(Np).all(axis=1) & np.isfinite(Nj).all(axis=1)
        a1 = _dot(Np[:, 0], Np[:, 1], Np[:, 2], dx, dy, dz) / f4
        a2 = _dot(Nj[:, 0], Nj[:, 1], Nj[:, 2], dx, dy, dz) / f4
        swap = np.abs(a1) < np.abs(a2)
        n1 = np.where(swap[:, None], Nj, Np)
        n2 = np.where(swap[:, None], Np, Nj)
        d = np.where(swap[:, None], -d, d)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        f3 = np.where(swap, -a2, a1)
        n1x, n1y, n1z = n1[:, 0], n1[:, 1], n1[:, 2]
        n2x, n2y, n2z = n2[:, 0], n2[:, 1], n2[:, 2]
        vx, vy, vz = dy * n1z - dz * n1y, dz * n1x - dx * n1z, dx * n1y - dy * n1x
        vn = np.sqrt((vx * vx + vy * vy) + vz * vz)
        ok &= vn != 0
        vx, vy, vz = vx / vn, vy / vn, vz / vn
        wx, wy, wz = n1y * vz - n1z * vy, n1z * vx - n1x * vz, n1x * vy - n1y * vx
        f2 = _dot(vx, vy, vz, n2x, n2y, n2z)
        y = _dot(wx, wy, wz, n2x, n2y, n2z)
        x = _dot(n1x, n1y, n1z, n2x, n2y, n2z)
    return ok, angle_bin(y, x), unit_bin(f2), unit_bin(f3)


def spfh_of_rows(cloud, normals, start, idx):
    """(n, 33) float32: every cloud point's SPFH from the cloud's own rows."""
    xyz = np.asarray(cloud, F32).reshape(-1, 4)[:, :3]
    nrm = np.asarray(normals, F32).reshape(-1, 4)[:, :3]
    n = xyz.shape[0]
    m = np.diff(start).astype(np.int64)
    p = np.repeat(np.arange(n, dtype=np.int64), m)
    j = idx.astype(np.int64)
    sel = (j != p) & (m[p] >= 2)
    p, j = p[sel], j[sel]
    counts = np.zeros((n, BINS), np.int64)
    if p.size:
        ok, b1, b2, b3 = pair_bins(xyz[p], nrm[p], xyz[j], nrm[j])
        for off, b in ((0, b1), (11, b2), (22, b3)):
            np.add.at(counts, (p[ok], off + b[ok]), 1)
    with np.errstate(all="ignore"):
        incr = F32(100.0) / (m - 1).astype(F32)
        out = counts.astype(F32) * incr[:, None]
    return np.where(counts == 0, F32(0), out).astype(F32)


def fpfh_of_rows(queries, spfh, start, idx, d2):
    """(n_q, 33) float32: the queries' rows weighted over the SPFH."""
    q = np.asarray(queries, F32).reshape(-1, 4)
    n_q = q.shape[0]
    m = np.diff(start).astype(np.int64)
    st = start[:-1]
    h = np.zeros((n_q, BINS), F32)
    with np.errstate(all="ignore"):
        for t in range(int(m.max()) if n_q else 0):
            sel = np.flatnonzero(m > t)
            j, d = idx[st[sel] + t].astype(np.int64), d2[st[sel] + t].astype(F32)
            use = d != 0
            w = F32(1.0) / d[use]
            h[sel[use]] = h[sel[use]] + spfh[j[use]] * w[:, None]
        for a in (0, 11, 22):
            s = h[:, a].astype(F64)
            for e in range(1, 11):
                s = s + h[:, a + e].astype(F64)
            factor = (100.0 / s).astype(F32)
            h[:, a:a + 11] = np.where((s != 0)[:, None], h[:, a:a + 11] * factor[:, None], h[:, a:a + 11])
    h[~S.finite_mask(q)] = np.nan
    return h


def _check_normals(cloud, normals):
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    if cloud.shape[0] and normals is None:
        raise Refused("null normals")
    normals = np.zeros((0, 4), F32) if normals is None else np.asarray(normals, F32).reshape(-1, 4)
    assert normals.shape[0] == cloud.shape[0]
    return cloud, normals


def estimate(cloud, normals, queries, k: int = 0, radius: float = 0.0):
    """(fpfh (n_q, 33) float32, n_neighbours (n_q,) int32, spfh (n, 33) float32)."""
    start_c, idx_c, d2_c = rows(cloud, None, k, radius)
    cloud, normals = _check_normals(cloud, normals)
    spfh = spfh_of_rows(cloud, normals, start_c, idx_c)
    if queries is None:
        q, start_q, idx_q, d2_q = cloud, start_c, idx_c, d2_c
    else:
        q = np.asarray(queries, F32).reshape(-1, 4)
        start_q, idx_q, d2_q = rows(cloud, q, k, radius)
    return fpfh_of_rows(q, spfh, start_q, idx_q, d2_q), np.diff(start_q).astype(np.int32), spfh


def _f(v):
    return F32(v)


def pair_bins_literal(Pp, Np, Pj, Nj):
    """One pair with float32 scalars: None when the pair is skipped, else (b1, b2, b3)."""
    Pp, Np, Pj, Nj = ([_f(v) for v in a[:3]] for a in (Pp, Np, Pj, Nj))
    with np.errstate(all="ignore"):
        d = [_f(Pj[e] - Pp[e]) for e in range(3)]
        f4 = np.sqrt(_f(_f(_f(d[0] * d[0]) + _f(d[1] * d[1])) + _f(d[2] * d[2])))
        if f4 == 0 or not all(np.isfinite(v) for v in Np + Nj):
            return None
        dot = lambda a, b: _f(_f(_f(a[0] * b[0]) + _f(a[1] * b[1])) + _f(a[2] * b[2]))  # noqa: E731
        cross = lambda a, b: [_f(_f(a[1] * b[2]) - _f(a[2] * b[1])), _f(_f(a[2] * b[0]) - _f(a[0] * b[2])), _f(_f(a[0] * b[1]) - _f(a[1] * b[0]))]  # noqa: E731
        a1, a2 = _f(dot(Np, d) / f4), _f(dot(Nj, d) / f4)
        if abs(a1) < abs(a2):
            n1, n2, d, f3 = Nj, Np, [-v for v in d], -a2
        else:
            n1, n2, f3 = Np, Nj, a1
        v = cross(d, n1)
        vn = np.sqrt(dot(v, v))
        if vn == 0:
            return None
        v = [_f(c / vn) for c in v]
        w = cross(n1, v)
        f2, y, x = dot(v, n2), dot(w, n2), dot(n1, n2)
        a, b = -x, -y
        if b >= 0:
            b1, first = 0, 0
        else:
            b1, first = 5, 5
        for e in range(first, first + 5):
            if _f(_f(EDGE_COS[e] * b) - _f(EDGE_SIN[e] * a)) >= 0:
                b1 += 1
        out = [b1]
        for f in (f2, f3):
            t = float(np.floor(F64(11.0) * ((F64(f) + F64(1.0)) * F64(0.5))))
            out.append(0 if not t >= 0 else (10 if t > 10 else int(t)))
    return tuple(out)


def estimate_literal(cloud, normals, queries, k: int = 0, radius: float = 0.0):
    """The rule point by point and pair by pair with float32 scalars (small clouds)."""
    start_c, idx_c, d2_c = rows(cloud, None, k, radius)
    cloud, normals = _check_normals(cloud, normals)
    n = cloud.shape[0]
    spfh = np.zeros((n, BINS), F32)
    with np.errstate(all="ignore"):
        for p in range(n):
            row = idx_c[start_c[p]:start_c[p + 1]]
            m = len(row)
            if m < 2:
                continue
            c = [0] * BINS
            for j in row:
                if j == p:
                    continue
                got = pair_bins_literal(cloud[p], normals[p], cloud[j], normals[j])
                if got is not None:
                    c[got[0]] += 1
                    c[11 + got[1]] += 1
                    c[22 + got[2]] += 1
            incr = _f(_f(100.0) / _f(m - 1))
            spfh[p] = [_f(0) if cb == 0 else _f(_f(cb) * incr) for cb in c]
        if queries is None:
            q, start_q, idx_q, d2_q = cloud, start_c, idx_c, d2_c
        else:
            q = np.asarray(queries, F32).reshape(-1, 4)
            start_q, idx_q, d2_q = rows(cloud, q, k, radius)
        n_q = q.shape[0]
        fpfh = np.zeros((n_q, BINS), F32)
        for i in range(n_q):
            if not np.isfinite(q[i, :3]).all():
                fpfh[i] = np.nan
                continue
            h = [_f(0)] * BINS
            for t in range(start_q[i], start_q[i + 1]):
                d = _f(d2_q[t])
                if d == 0:
                    continue
                w = _f(_f(1.0) / d)
                h = [_f(h[b] + _f(spfh[idx_q[t], b] * w)) for b in range(BINS)]
            for a in (0, 11, 22):
                s = F64(h[a])
                for e in range(1, 11):
                    s = F64(s + F64(h[a + e]))
                if s != 0:
                    factor = _f(F64(100.0) / s)
                    for e in range(11):
                        h[a + e] = _f(h[a + e] * factor)
            fpfh[i] = h
    return fpfh, np.diff(start_q).astype(np.int32), spfh
