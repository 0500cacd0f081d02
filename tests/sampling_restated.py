"""The cropping and sampling filters' rules (include/icpgpu.h, "cropping and sampling filters") restated in NumPy, float32 step by step:

    pass through   a finite row is removed when (!negative && (v < lo || v > hi)) || (negative && v >= lo && v <= hi); no field:
                   every finite row stays
    crop box       q = p, or the three fma chains of T * p (fused operations emulated exactly: symmetric_restated.fma_f32); outside
                   iff a comparison q.a < min.a or q.a > max.a holds, so a NaN q is inside
    crop matrix    M = R^-1 Tr(-translation) transform in Python floats, every 4 x 4 product added from the left, rounded once
    uniform        the voxel filter's plan (voxel_edge_cases.plan_exact) over the finite rows' box; cell = floor(p * inv), centre =
                   (cell + 0.5) * leaf, d2 = fma(dz, dz, fma(dy, dy, dx * dx)); the smallest (d2 bits, index) key of every cell
    farthest       m = +inf; per sample m = min(m, d2(i, last)) over the unselected finite rows and the largest m, lowest index

Every rule returns the kept rows' indices (and its measure).  Beside each vectorised rule stands a literal per-point (and per-sample)
Python loop with exact rational arithmetic for the fused operations; tests/test_sampling_host.py holds the two against each other."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import voxel_edge_cases as vx
from symmetric_restated import fma_f32

F32 = np.float32
INT32_MAX = 2**31 - 1
FPS_ONE_WORKGROUP_MAX = 16384
FLT_MIN, FLT_MAX = float(np.finfo(F32).tiny), float(np.finfo(F32).max)
MASK = (1 << 64) - 1


class Refused(Exception):
    """What the library answers with ICPGPU_ERR_INVALID_ARG."""


class Unsupported(Exception):
    """What the library answers with ICPGPU_ERR_UNSUPPORTED."""


def finite_rows(cloud) -> np.ndarray:
    return np.isfinite(np.asarray(cloud, F32)[:, :3]).all(axis=1)


def removed_of(n: int, kept) -> np.ndarray:
    mask = np.ones(n, bool)
    mask[np.asarray(kept, np.int64)] = False
    return np.flatnonzero(mask).astype(np.int32)


# ---- exact scalar arithmetic for the literal loops ------------------------------------------------------------------------------
def round_f32(value: Fraction) -> np.float32:
    """The float32 nearest to an exact rational, ties to even."""
    r = F32(float(value))  # (within one float32 step of the answer)
    best = None
    for cand in (np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - value)
        even = (int(np.array([cand], F32).view(np.uint32)[0]) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    if best is None or abs(value) >= Fraction(FLT_MAX) + Fraction(2.0**103):  # (beyond the last finite float32's half step)
        return F32(math.copysign(math.inf, float(value)))
    return F32(best[1])


def fma_scalar(a, b, c) -> np.float32:
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))  # (a NaN or an infinity either way: no rounding to get wrong)
    return round_f32(Fraction(a) * Fraction(b) + Fraction(c))


# ---- pass through ----------------------------------------------------------------------------------------------------------------
def check_pass_through(field, lo, hi):
    if field not in (-1, 0, 1, 2):
        raise Refused("field")
    if math.isnan(lo) or math.isnan(hi):
        raise Refused("NaN limit")


def pass_through(cloud, field=-1, lo=FLT_MIN, hi=FLT_MAX, negative=False) -> np.ndarray:
    check_pass_through(field, lo, hi)
    cloud = np.asarray(cloud, F32)
    keep = finite_rows(cloud)
    if field >= 0:
        v = cloud[:, field]
        lo, hi = F32(lo), F32(hi)
        with np.errstate(invalid="ignore"):
            removed = ((v >= lo) & (v <= hi)) if negative else ((v < lo) | (v > hi))
        keep &= ~removed
    return np.flatnonzero(keep).astype(np.int32)


def pass_through_literal(cloud, field=-1, lo=FLT_MIN, hi=FLT_MAX, negative=False) -> np.ndarray:
    check_pass_through(field, lo, hi)
    lo, hi = float(F32(lo)), float(F32(hi))
    kept = []
    for i, p in enumerate(np.asarray(cloud, F32).tolist()):
        if not all(math.isfinite(c) for c in p[:3]):
            continue
        if field >= 0:
            v = p[field]
            if (not negative and (v < lo or v > hi)) or (negative and lo <= v <= hi):
                continue
        kept.append(i)
    return np.array(kept, np.int32)


# ---- crop box ----------------------------------------------------------------------------------------------------------------------
def xform(T, cloud) -> np.ndarray:
    """T * p for every row: px = fma(m02, z, fma(m01, y, fma(m00, x, m03))), likewise y and z."""
    T = np.asarray(T, F32).reshape(4, 4)
    x, y, z = (np.asarray(cloud, F32)[:, a] for a in range(3))
    return np.stack([fma_f32(T[r, 2], z, fma_f32(T[r, 1], y, fma_f32(T[r, 0], x, np.full_like(x, T[r, 3])))) for r in range(3)], axis=1)


def check_crop_box(mn, mx):
    if np.isnan(np.asarray(mn, F32)).any() or np.isnan(np.asarray(mx, F32)).any():
        raise Refused("NaN corner")


def crop_box(cloud, mn, mx, T=None, negative=False) -> np.ndarray:
    check_crop_box(mn, mx)
    cloud = np.asarray(cloud, F32)
    mn, mx = np.asarray(mn, F32).reshape(3), np.asarray(mx, F32).reshape(3)
    q = cloud[:, :3] if T is None else xform(T, cloud)
    with np.errstate(invalid="ignore"):
        outside = ((q < mn) | (q > mx)).any(axis=1)
    return np.flatnonzero(finite_rows(cloud) & (outside if negative else ~outside)).astype(np.int32)


def crop_box_literal(cloud, mn, mx, T=None, negative=False) -> np.ndarray:
    check_crop_box(mn, mx)
    mn, mx = np.asarray(mn, F32).reshape(3).tolist(), np.asarray(mx, F32).reshape(3).tolist()
    Tm = None if T is None else np.asarray(T, F32).reshape(4, 4).tolist()
    kept = []
    for i, p in enumerate(np.asarray(cloud, F32).tolist()):
        if not all(math.isfinite(c) for c in p[:3]):
            continue
        q = p[:3]
        if Tm is not None:
            q = [float(fma_scalar(Tm[r][2], p[2], fma_scalar(Tm[r][1], p[1], fma_scalar(Tm[r][0], p[0], Tm[r][3])))) for r in range(3)]
        outside = any(q[a] < mn[a] or q[a] > mx[a] for a in range(3))
        if outside == bool(negative):
            kept.append(i)
    return np.array(kept, np.int32)


def _mul4(a, b):
    out = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            s = a[i][0] * b[0][j]
            for k in range(1, 4):
                s += a[i][k] * b[k][j]
            out[i][j] = s
    return out


def crop_box_matrix(transform=None, translation=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """M = R^-1 Tr(-translation) transform, R = (Rz Ry) Rx, in Python floats (float64; math.sin / cos: the host's libm); float32 once."""
    eye = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    tf = eye if transform is None else [[float(v) for v in row] for row in np.asarray(transform, F32).reshape(4, 4).tolist()]
    tr = [row[:] for row in eye]
    for a in range(3):
        tr[a][3] = -float(F32(translation[a]))
    rx, ry, rz = ([row[:] for row in eye] for _ in range(3))
    a, b, c = (float(F32(v)) for v in rotation)
    rx[1][1], rx[1][2], rx[2][1], rx[2][2] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    ry[0][0], ry[0][2], ry[2][0], ry[2][2] = math.cos(b), math.sin(b), -math.sin(b), math.cos(b)
    rz[0][0], rz[0][1], rz[1][0], rz[1][1] = math.cos(c), -math.sin(c), math.sin(c), math.cos(c)
    r = _mul4(_mul4(rz, ry), rx)
    rinv = [[r[j][i] for j in range(4)] for i in range(4)]
    return np.array(_mul4(rinv, _mul4(tr, tf)), np.float64).astype(F32)


# ---- uniform sampling --------------------------------------------------------------------------------------------------------------
def check_uniform(leaf):
    if not (math.isfinite(leaf) and F32(leaf) > 0):
        raise Refused("leaf")


def uniform_plan(cloud, leaf):
    """(minb, divb) of the plan over the finite rows' box, None without a finite row; Unsupported for the two refused verdicts."""
    cloud = np.asarray(cloud, F32)
    if not finite_rows(cloud).any():
        return None
    lo, hi = vx.bbox(cloud)
    verdict, minb, divb = vx.plan_exact(lo, hi, leaf)
    if verdict == vx.NO_FINITE:
        return None
    if verdict in (vx.PASS_THROUGH, vx.WRAP):
        raise Unsupported(verdict)
    return [int(v) for v in minb], [int(v) for v in divb]


def uniform_cells(cloud, leaf):
    """Per row: the cell (int64 x 3) and d2 (float32) -- rows that are not finite get garbage the callers mask."""
    p = np.asarray(cloud, F32)[:, :3]
    leaf32 = F32(leaf)
    inv = F32(1.0) / leaf32
    with np.errstate(invalid="ignore", over="ignore"):
        cell = np.floor(p * inv)
        c = (cell.astype(F32) + F32(0.5)) * leaf32
        d = (p - c).astype(F32)
        d2 = fma_f32(d[:, 2], d[:, 2], fma_f32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
        cell = np.where(np.isfinite(cell), cell, 0).astype(np.int64)
    return cell, d2


def uniform_sampling(cloud, leaf):
    """(kept ascending, measure): the row with the smallest (d2 bits, index) key of every occupied cell."""
    check_uniform(leaf)
    cloud = np.asarray(cloud, F32)
    plan = uniform_plan(cloud, leaf)
    if plan is None:
        return np.empty(0, np.int32), np.empty(0, F32)
    minb, divb = plan
    rows = np.flatnonzero(finite_rows(cloud))
    cell, d2 = uniform_cells(cloud, leaf)
    cell, d2 = cell[rows], d2[rows]
    index = (cell[:, 0] - minb[0]) + divb[0] * ((cell[:, 1] - minb[1]) + divb[1] * (cell[:, 2] - minb[2]))
    assert (index >= 0).all() and (index <= INT32_MAX).all()
    bits = d2.view(np.uint32).astype(np.int64)
    order = np.lexsort((rows, bits, index))
    first = np.ones(len(order), bool)
    first[1:] = index[order][1:] != index[order][:-1]
    win = np.sort(order[first])
    return rows[win].astype(np.int32), d2[win]


def uniform_sampling_literal(cloud, leaf):
    check_uniform(leaf)
    cloud = np.asarray(cloud, F32)
    plan = uniform_plan(cloud, leaf)
    if plan is None:
        return np.empty(0, np.int32), np.empty(0, F32)
    leaf32 = F32(leaf)
    inv = F32(1.0) / leaf32
    best = {}
    for i, p in enumerate(cloud[:, :3]):
        if not np.isfinite(p).all():
            continue
        cell, d = [], []
        for a in range(3):
            ia = int(math.floor(float(F32(p[a] * inv))))
            cell.append(ia)
            d.append(F32(p[a] - F32(F32(F32(ia) + F32(0.5)) * leaf32)))
        d2 = fma_scalar(d[2], d[2], fma_scalar(d[1], d[1], F32(d[0] * d[0])))
        key = (int(np.array([d2], F32).view(np.uint32)[0]), i)
        if tuple(cell) not in best or key < best[tuple(cell)][0]:
            best[tuple(cell)] = (key, d2)
    won = sorted((key[1], d2) for key, d2 in best.values())
    return np.array([w[0] for w in won], np.int32), np.array([w[1] for w in won], F32)


# ---- farthest point sampling -------------------------------------------------------------------------------------------------------
def d2_rows(cloud, j) -> np.ndarray:
    """d2(i, j) of the outlier section for every row i: dx = p_i.x - p_j.x, ...; fma(dz, dz, fma(dy, dy, dx * dx))."""
    p = np.asarray(cloud, F32)[:, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - p[j]).astype(F32)
        return fma_f32(d[:, 2], d[:, 2], fma_f32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))


def check_farthest(cloud, n_samples, first_index):
    cloud = np.asarray(cloud, F32)
    n, fin = cloud.shape[0], finite_rows(cloud)
    if first_index < -1 or first_index >= n:
        raise Refused("first_index outside the cloud")
    if first_index >= 0 and not fin[first_index]:
        raise Refused("first_index names a non-finite row")
    if n_samples < 0 or n_samples > int(fin.sum()):
        raise Refused("n_samples above the finite rows")


def farthest_point_sampling(cloud, n_samples, first_index=-1):
    """(kept in selection order, measure): measure[j] = m of s_j when it was chosen, +inf for the first."""
    check_farthest(cloud, n_samples, first_index)
    cloud = np.asarray(cloud, F32)
    if n_samples == 0:
        return np.empty(0, np.int32), np.empty(0, F32)
    fin = finite_rows(cloud)
    m = np.where(fin, F32(np.inf), F32(-1.0)).astype(F32)  # (-1: not a candidate)
    s = int(first_index) if first_index >= 0 else int(np.flatnonzero(fin)[0])
    kept, measure = [s], [F32(np.inf)]
    for _ in range(1, n_samples):
        live = m >= 0
        m = np.where(live, np.minimum(m, d2_rows(cloud, s)), m).astype(F32)
        m[s] = F32(-1.0)
        s = int(np.argmax(m))  # (the first of the largest: ties go to the lowest index)
        kept.append(s)
        measure.append(m[s])
    return np.array(kept, np.int32), np.array(measure, F32)


def farthest_point_sampling_literal(cloud, n_samples, first_index=-1):
    check_farthest(cloud, n_samples, first_index)
    cloud = np.asarray(cloud, F32)
    if n_samples == 0:
        return np.empty(0, np.int32), np.empty(0, F32)
    rows = [i for i, p in enumerate(cloud[:, :3]) if np.isfinite(p).all()]
    m = {i: F32(np.inf) for i in rows}
    s = int(first_index) if first_index >= 0 else rows[0]
    kept, measure = [s], [F32(np.inf)]
    del m[s]
    for _ in range(1, n_samples):
        ps = cloud[s, :3]
        best = None
        for i in sorted(m):
            d = [F32(cloud[i, a] - ps[a]) for a in range(3)]
            with np.errstate(over="ignore"):
                d2 = fma_scalar(d[2], d[2], fma_scalar(d[1], d[1], F32(d[0] * d[0])))
            if d2 < m[i]:
                m[i] = d2
            if best is None or m[i] > m[best]:
                best = i
        s = best
        kept.append(s)
        measure.append(m.pop(s))
    return np.array(kept, np.int32), np.array(measure, F32)


def seeded_first_row(cloud, seed: int) -> int:
    """setSeed's first row: the plane segmentation's generator (sac_restated.sample_int at t = 0, c = 0) over n, advanced cyclically
    to the next finite row; -1 without one."""
    import sac_restated as SR
    cloud = np.asarray(cloud, F32)
    n = cloud.shape[0]
    fin = finite_rows(cloud)
    if n == 0 or not fin.any():
        return -1
    start = SR.sample_int(seed & MASK, 0, 0, n)
    for step in range(n):
        if fin[(start + step) % n]:
            return (start + step) % n
    return -1


def cover_radius(cloud, sample) -> float:
    """r(S): the largest distance of a finite cloud point to its nearest sample (float64)."""
    p = np.asarray(cloud, np.float64)[finite_rows(cloud), :3]
    s = np.asarray(cloud, np.float64)[np.asarray(sample, np.int64), :3]
    nearest = np.full(len(p), np.inf)
    for q in s:
        nearest = np.minimum(nearest, ((p - q) ** 2).sum(axis=1))
    return float(np.sqrt(nearest.max()))
