"""The ground filter's rule (include/icpgpu.h, "ground filter") restated in NumPy float32: what the kernels are compared with, bit for
bit.  Two forms that share no code: the vectorised one (operator, run) and a literal loop (operator_literal, run_literal) -- per pass,
per point, per candidate, plain Python comparisons on np.float32 scalars."""
import math

import numpy as np

F32 = np.float32
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
MAX_PASSES = 32
DEFAULTS = dict(max_window_size=33, slope=0.7, initial_distance=0.15, max_distance=10.0, cell_size=1.0, base=2.0, exponential=True)


class Refused(ValueError):
    pass


# ---- the schedule --------------------------------------------------------------------------------------------------------------
def validate(max_window_size=33, slope=0.7, initial_distance=0.15, max_distance=10.0, cell_size=1.0, base=2.0, exponential=True):
    """The arguments as the float32 values the rule works with; Refused where the entry point refuses them."""
    with np.errstate(over="ignore"):
        slope, initial_distance, max_distance, cell_size, base = (F32(v) for v in (slope, initial_distance, max_distance, cell_size, base))
    if not all(np.isfinite(v) for v in (slope, initial_distance, max_distance, cell_size, base)):
        raise Refused("a parameter is not finite")
    if not cell_size > 0:
        raise Refused("cell_size")
    if slope < 0 or initial_distance < 0 or max_distance < 0:
        raise Refused("a negative parameter")
    if not (base > 1 if exponential else base > 0):
        raise Refused("base")
    return F32(int(max_window_size)), slope, initial_distance, max_distance, cell_size, base, bool(exponential)


def schedule(**kw):
    """(windows, thresholds) float32 of extract's loop."""
    max_window, slope, initial, max_distance, cell, base, exponential = validate(**kw)
    windows, thresholds = [], []
    window, power, it = F32(0), 1.0, 0
    with np.errstate(over="ignore"):
        while window < max_window:
            if it >= MAX_PASSES:
                raise Refused("more than MAX_PASSES passes")
            previous = window
            if exponential:
                window = F32(float(cell) * (2.0 * power + 1.0))
                power *= float(base)
            else:
                window = cell * (F32(2) * F32(it + 1) * base + F32(1))
            if not np.isfinite(window):
                raise Refused("a window that is not finite")
            thr = initial if it == 0 else slope * (window - previous) * cell + initial
            if thr > max_distance:
                thr = max_distance
            assert type(window) is F32 and type(thr) is F32
            windows.append(window)
            thresholds.append(thr)
            it += 1
    return np.array(windows, F32), np.array(thresholds, F32)


# ---- the vectorised form -------------------------------------------------------------------------------------------------------
def finite_rows(cloud) -> np.ndarray:
    return np.isfinite(cloud[:, :3]).all(axis=1)


def keys(v: np.ndarray) -> np.ndarray:
    """The integer keys whose order is the rule's total order of floats (-0.0 below +0.0)."""
    bits = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(bits >> 31 != 0, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k: np.ndarray) -> np.ndarray:
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def boxes(cloud, active: np.ndarray, window, rows=None) -> np.ndarray:
    """M[a, b]: active point b is in active point a's box (rows: only these positions a of the active list)."""
    h = F32(window) / F32(2)
    x, y = cloud[active, 0].astype(F32), cloud[active, 1].astype(F32)
    cx, cy = (x, y) if rows is None else (x[rows], y[rows])
    with np.errstate(over="ignore"):
        lox, hix, loy, hiy = cx - h, cx + h, cy - h, cy + h
    return (lox[:, None] <= x[None, :]) & (x[None, :] <= hix[:, None]) & (loy[:, None] <= y[None, :]) & (y[None, :] <= hiy[:, None])


def extremum(M: np.ndarray, values: np.ndarray, take_max: bool) -> np.ndarray:
    k = keys(values)
    if take_max:
        return unkeys(np.where(M, k[None, :], np.uint32(0)).max(axis=1))
    return unkeys(np.where(M, k[None, :], np.uint32(0xFFFFFFFF)).min(axis=1))


def operator(cloud, window, op: int, active=None) -> np.ndarray:
    """pcl::applyMorphologicalOperator over the active set (default: every finite point): z of every point, float32."""
    if not (np.isfinite(F32(window)) and F32(window) > 0) or op not in (ERODE, DILATE, OPEN, CLOSE):
        raise Refused("operator")
    out = cloud[:, 2].astype(F32).copy()
    active = np.flatnonzero(finite_rows(cloud)) if active is None else np.asarray(active)
    if active.size == 0:
        return out
    M = boxes(cloud, active, window)
    first_max = op in (DILATE, CLOSE)
    v = extremum(M, out[active], first_max)
    if op in (OPEN, CLOSE):
        v = extremum(M, v, not first_max)
    out[active] = v
    return out


def run(cloud, **kw) -> dict:
    """pcl::ProgressiveMorphologicalFilter::extract: ground, windows, thresholds, ground_after, removed_at."""
    windows, thresholds = schedule(**kw)
    finite = finite_rows(cloud)
    removed_at = np.where(finite, -1, -2).astype(np.int32)
    ground = np.flatnonzero(finite)
    z = cloud[:, 2].astype(F32)
    after = []
    for p, (w, thr) in enumerate(zip(windows, thresholds)):
        if ground.size:
            o = operator(cloud, w, OPEN, ground)
            with np.errstate(over="ignore", invalid="ignore"):
                stays = (z[ground] - o[ground]) < thr
            removed_at[ground[~stays]] = p
            ground = ground[stays]
        after.append(ground.size)
    return {"ground": ground.astype(np.int32), "windows": windows, "thresholds": thresholds, "ground_after": np.array(after, np.int32),
            "removed_at": removed_at}


def extract(cloud, ground, negative: bool) -> np.ndarray:
    mask = np.zeros(len(cloud), bool)
    mask[np.asarray(ground, np.int64)] = True
    return cloud[~mask if negative else mask]


# ---- the literal loop ----------------------------------------------------------------------------------------------------------
def _below(a, b) -> bool:
    """a before b in the rule's total order."""
    return bool(a < b) or (bool(a == b) and bool(np.signbit(a)) and not bool(np.signbit(b)))


def _members(cloud, active, window):
    h = F32(window) / F32(2.0)
    rows = []
    for i in active:
        px, py = F32(cloud[i, 0]), F32(cloud[i, 1])
        with np.errstate(over="ignore"):
            lox, hix, loy, hiy = px - h, px + h, py - h, py + h
        row = []
        for j in active:
            qx, qy = F32(cloud[j, 0]), F32(cloud[j, 1])
            if lox <= qx and qx <= hix and loy <= qy and qy <= hiy:
                row.append(j)
        rows.append(row)
    return rows


def _sweep(active, rows, values: dict, take_max: bool) -> dict:
    out = {}
    for i, row in zip(active, rows):
        best = None
        for j in row:
            v = values[j]
            if best is None or (_below(best, v) if take_max else _below(v, best)):
                best = v
        out[i] = best
    return out


def operator_literal(cloud, window, op: int, active=None) -> np.ndarray:
    n = len(cloud)
    if active is None:
        active = [i for i in range(n) if all(math.isfinite(float(cloud[i, a])) for a in range(3))]
    out = [F32(cloud[i, 2]) for i in range(n)]
    rows = _members(cloud, active, window)
    values = {i: out[i] for i in active}
    first_max = op in (DILATE, CLOSE)
    values = _sweep(active, rows, values, first_max)
    if op in (OPEN, CLOSE):
        values = _sweep(active, rows, values, not first_max)
    for i in active:
        out[i] = values[i]
    return np.array(out, F32)


def run_literal(cloud, **kw) -> dict:
    windows, thresholds = schedule(**kw)
    n = len(cloud)
    removed_at = [-1 if all(math.isfinite(float(cloud[i, a])) for a in range(3)) else -2 for i in range(n)]
    ground = [i for i in range(n) if removed_at[i] == -1]
    after = []
    for p in range(len(windows)):
        opened = operator_literal(cloud, windows[p], OPEN, ground)
        keep = []
        for i in ground:
            with np.errstate(over="ignore", invalid="ignore"):
                diff = F32(cloud[i, 2]) - opened[i]
            if diff < thresholds[p]:
                keep.append(i)
            else:
                removed_at[i] = p
        ground = keep
        after.append(len(ground))
    return {"ground": np.array(ground, np.int32), "windows": windows, "thresholds": thresholds, "ground_after": np.array(after, np.int32),
            "removed_at": np.array(removed_at, np.int32)}
