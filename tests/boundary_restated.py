"""An independent NumPy restatement of the boundary estimation (include/icpgpu.h, "boundary estimation"):
pcl::BoundaryEstimation over the neighbour rows of tests/search_restated.py.  It never calls the library.

    rows        normals_restated.rows: row q of knn(k) or of radius(radius, max_nn = 0), in CSR form
    frame       float32: near = |nx| <= 1e-5f |nz| and |ny| <= 1e-5f |nz|; v = (-ny, nx, 0) / sqrtf(nx nx + ny ny) unless near, else
                (0, -nz, ny) / sqrtf(ny ny + nz nz), as a product with inv = 1 / sqrtf(..); u = n x v component by component
    directions  d = P_j - P_q in float32; x = (u.x d.x + u.y d.y) + u.z d.z, y likewise with v; an entry is skipped when d == 0, when
                x or y is not finite, or when x == y == 0
    sector      float64 on exact products: cr = xa yb - ya xb, dt = xa xb + ya yb, na, nb; b is in a's sector iff cr >= 0, not
                (cr == 0 and dt > 0), and for c = cos(threshold) >= 0: dt >= 0 and dt dt >= (c2 na) nb; for c < 0: dt >= 0 or
                dt dt <= (c2 na) nb
    boundary    the query is finite, its row has >= 3 entries and >= 1 direction, and some direction has an empty sector; witness =
                the lowest cloud index among those, else -1.  n_directions is 0 where the row has fewer than 3 entries.
(estimate_literal: the same query by query and pair by pair, cr / dt / na / nb as fractions.Fraction rounded once -- for small clouds.
pcl_rule: PCL's own atan2 / sort / largest-gap rule in float64 on the same directions, for the comparison within 1e-6 rad.)
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import normals_restated as N
import search_restated as S

F32, F64 = np.float32, np.float64
Refused = S.Refused
FIELDS = ("boundary", "n_neighbours", "n_directions", "witness")


def check_threshold(angle_threshold: float):
    if not (math.isfinite(angle_threshold) and 0.0 < angle_threshold <= math.pi):
        raise Refused("angle_threshold")


def frame(normals):
    """(u (m, 3), v (m, 3)) float32 from normals (m, >= 3)."""
    nrm = np.asarray(normals, F32)
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    zero = np.zeros_like(nx)
    with np.errstate(all="ignore"):
        lim = F32(1e-5) * np.abs(nz)
        near = (np.abs(nx) <= lim) & (np.abs(ny) <= lim)
        inv_a = F32(1) / np.sqrt(nx * nx + ny * ny)
        inv_b = F32(1) / np.sqrt(ny * ny + nz * nz)
        va = np.stack([-ny * inv_a, nx * inv_a, zero], 1)
        vb = np.stack([zero, -nz * inv_b, ny * inv_b], 1)
        v = np.where(near[:, None], vb, va).astype(F32)
        u = np.stack([ny * v[:, 2] - nz * v[:, 1], nz * v[:, 0] - nx * v[:, 2], nx * v[:, 1] - ny * v[:, 0]], 1).astype(F32)
    return u, v


def directions_of_row(p, u, v, pts):
    """(x, y float32, keep bool) of the row's points pts (m, 3) about the query p (3,)."""
    with np.errstate(all="ignore"):
        d = (pts - p[None, :]).astype(F32)
        x = (u[0] * d[:, 0] + u[1] * d[:, 1]) + u[2] * d[:, 2]
        y = (v[0] * d[:, 0] + v[1] * d[:, 1]) + v[2] * d[:, 2]
    keep = (d != 0).any(axis=1) & np.isfinite(x) & np.isfinite(y) & ~((x == 0) & (y == 0))
    return x.astype(F32), y.astype(F32), keep


def in_sector(xa, ya, xb, yb, c: float):
    """b in a's sector, elementwise on float64 arrays holding float32 values."""
    c2 = F64(c) * F64(c)
    with np.errstate(all="ignore"):
        cr = xa * yb - ya * xb
        dt = xa * xb + ya * yb
        na = xa * xa + ya * ya
        nb = xb * xb + yb * yb
        lhs, rhs = dt * dt, (c2 * na) * nb
        cone = ((dt >= 0) & (lhs >= rhs)) if c >= 0 else ((dt >= 0) | (lhs <= rhs))
    return (cr >= 0) & ~((cr == 0) & (dt > 0)) & cone


def survivors(x, y, c: float):
    """Which of the directions (x, y float32 arrays) have an empty sector."""
    xd, yd = x.astype(F64), y.astype(F64)
    hit = in_sector(xd[:, None], yd[:, None], xd[None, :], yd[None, :], c)
    return ~hit.any(axis=1)


def from_rows(cloud, queries, normals, start, idx, angle_threshold: float, min_row: int = 3):
    check_threshold(angle_threshold)
    cloud = np.ascontiguousarray(cloud, F32).reshape(-1, 4)
    queries = cloud if queries is None else np.ascontiguousarray(queries, F32).reshape(-1, 4)
    n_q = queries.shape[0]
    c = math.cos(angle_threshold)
    u, v = frame(np.asarray(normals, F32).reshape(n_q, -1) if n_q else np.zeros((0, 4), F32))
    counts = np.diff(start).astype(np.int32)
    finite = S.finite_mask(queries)
    out = {"boundary": np.zeros(n_q, np.uint8), "n_neighbours": counts, "n_directions": np.zeros(n_q, np.int32),
           "witness": np.full(n_q, -1, np.int32)}
    for q in np.flatnonzero(finite & (counts >= max(min_row, 3))):
        row = idx[start[q]:start[q + 1]]
        x, y, keep = directions_of_row(queries[q, :3], u[q], v[q], cloud[row, :3])
        out["n_directions"][q] = keep.sum()
        if keep.any():
            alive = survivors(x[keep], y[keep], c)
            if alive.any():
                out["boundary"][q] = 1
                out["witness"][q] = row[keep][alive].min()
    return out


def estimate(cloud, queries, normals, k: int = 0, radius: float = 0.0, angle_threshold: float = math.pi / 2):
    """dict(boundary uint8, n_neighbours, n_directions, witness int32), n_q entries each."""
    check_threshold(angle_threshold)
    start, idx = N.rows(cloud, queries, k, radius)
    return from_rows(cloud, queries, normals, start, idx, angle_threshold)


def _round(fr: Fraction) -> float:
    return fr.numerator / fr.denominator   # int / int is correctly rounded


def in_sector_literal(xa, ya, xb, yb, c: float) -> bool:
    """One pair, scalars: the four sums as exact fractions rounded once, the rest in Python floats."""
    fxa, fya, fxb, fyb = (Fraction(float(t)) for t in (xa, ya, xb, yb))
    cr, dt = _round(fxa * fyb - fya * fxb), _round(fxa * fxb + fya * fyb)
    na, nb = _round(fxa * fxa + fya * fya), _round(fxb * fxb + fyb * fyb)
    c2 = c * c
    if not cr >= 0.0 or (cr == 0.0 and dt > 0.0):
        return False
    if c >= 0:
        return dt >= 0.0 and dt * dt >= (c2 * na) * nb
    return dt >= 0.0 or dt * dt <= (c2 * na) * nb


def estimate_literal(cloud, queries, normals, k: int = 0, radius: float = 0.0, angle_threshold: float = math.pi / 2):
    """The rule query by query: the literal rows, scalar float32 arithmetic, every pair on its own."""
    check_threshold(angle_threshold)
    cloud = np.ascontiguousarray(cloud, F32).reshape(-1, 4)
    qs = cloud if queries is None else np.ascontiguousarray(queries, F32).reshape(-1, 4)
    normals = np.asarray(normals, F32).reshape(qs.shape[0], -1)
    if (k != 0) == (radius != 0.0):
        raise Refused("exactly one of k and radius")
    if k:
        ki, _, kf = S.knn_literal(cloud, queries, k)
        rows = [ki[q, :kf[q]] for q in range(qs.shape[0])]
    else:
        st, ri, _ = S.radius_literal(cloud, queries, radius, 0)
        rows = [ri[st[q]:st[q + 1]] for q in range(qs.shape[0])]
    c = math.cos(angle_threshold)
    n_q = qs.shape[0]
    out = {"boundary": np.zeros(n_q, np.uint8), "n_neighbours": np.array([len(r) for r in rows], np.int32),
           "n_directions": np.zeros(n_q, np.int32), "witness": np.full(n_q, -1, np.int32)}
    one = F32(1)
    with np.errstate(all="ignore"):
        for q in range(n_q):
            p = qs[q]
            if not all(math.isfinite(float(t)) for t in p[:3]) or len(rows[q]) < 3:
                continue
            nx, ny, nz = (F32(t) for t in normals[q, :3])
            lim = F32(1e-5) * abs(nz)
            if not (abs(nx) <= lim and abs(ny) <= lim):
                inv = one / np.sqrt(F32(F32(nx * nx) + F32(ny * ny)))
                v = (F32(-ny * inv), F32(nx * inv), F32(0))
            else:
                inv = one / np.sqrt(F32(F32(ny * ny) + F32(nz * nz)))
                v = (F32(0), F32(-nz * inv), F32(ny * inv))
            u = (F32(F32(ny * v[2]) - F32(nz * v[1])), F32(F32(nz * v[0]) - F32(nx * v[2])), F32(F32(nx * v[1]) - F32(ny * v[0])))
            dirs = []
            for j in rows[q]:
                d = [F32(cloud[j, a] - p[a]) for a in range(3)]
                if d[0] == 0 and d[1] == 0 and d[2] == 0:
                    continue
                x = F32(F32(F32(u[0] * d[0]) + F32(u[1] * d[1])) + F32(u[2] * d[2]))
                y = F32(F32(F32(v[0] * d[0]) + F32(v[1] * d[1])) + F32(v[2] * d[2]))
                if not (math.isfinite(float(x)) and math.isfinite(float(y))) or (x == 0 and y == 0):
                    continue
                dirs.append((float(x), float(y), int(j)))
            out["n_directions"][q] = len(dirs)
            alive = [ja for xa, ya, ja in dirs if not any(in_sector_literal(xa, ya, xb, yb, c) for xb, yb, _ in dirs)]
            if alive:
                out["boundary"][q], out["witness"][q] = 1, min(alive)
    return out


def pcl_rule(x, y, angle_threshold: float):
    """PCL's isBoundaryPoint on directions (x, y): (largest angular gap in float64, gap > threshold).  A single direction: 2 pi."""
    ang = np.sort(np.arctan2(np.asarray(y, F64), np.asarray(x, F64)))
    if ang.size == 0:
        return 0.0, False
    gaps = np.diff(ang)
    wrap = 2 * math.pi - (ang[-1] - ang[0])
    largest = float(max(gaps.max(), wrap)) if gaps.size else 2 * math.pi
    return largest, largest > angle_threshold


def same_bits(a: dict, b: dict) -> list:
    """The names of the fields whose bits differ."""
    bad = []
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(f)
    return bad
