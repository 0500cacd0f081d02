"""The correspondence rejectors restated in NumPy (include/icpgpu.h, "correspondence rejectors"): the three rules from sorted
arrays and np.unique, and an ICP loop with a chain for P2P_SVD and P2PLANE built from the oracle's pinned primitives (oracle.nn,
oracle.reduce, oracle.umeyama, oracle.p2plane_sums, oracle.p2plane_solve; the convergence rule of oracle/icp_oracle_np.py:
icp_align).  A rejected pair reaches the oracle's reductions as a distance beyond the gate.

A chain is a list of (kind, value, min_correspondences) tuples, kind one of MEDIAN, TRIMMED, ONE_TO_ONE.  Every stage also reports
its CUT MARGIN: the relative gap between the cut and the nearest d2 on the other side of it (one-to-one: between a target's
winner and its runner-up) -- how far a d2 may move before the kept set changes -- and the d2 it was measured at (margin_at)."""
from __future__ import annotations

import numpy as np

MEDIAN, TRIMMED, ONE_TO_ONE = 1, 2, 3
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = 0, 1, 2, 3, 4, 5
_INF = float("inf")


def _rel_gap(a, b):
    """|a - b| relative to the larger magnitude (inf when one side does not exist)"""
    if a is None or b is None:
        return _INF
    a, b = float(a), float(b)
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0.0 else 0.0


def median_distance(d2, alive, factor):
    """-> kept mask, stats dict.  median = sorted[n // 2]; keep (double)d2 <= (double)median * factor."""
    d2 = np.asarray(d2, np.float32)
    n = int(alive.sum())
    if n == 0:
        return np.zeros_like(alive), dict(pairs_in=0, pairs_out=0, cut=np.float32(0.0), margin=_INF, margin_at=0.0)
    s = np.sort(d2[alive])
    med = s[n // 2]
    limit = float(med) * float(factor)
    kept = alive & (d2.astype(np.float64) <= limit)
    # the kept set changes when a d2 crosses the limit (which itself moves with the median, by as little as a d2 does)
    d = d2[alive].astype(np.float64)
    above, below = d[d > limit], d[d < limit]
    margin = min(_rel_gap(above.min(), limit) if above.size else _INF, _rel_gap(below.max(), limit) if below.size else _INF)
    return kept, dict(pairs_in=n, pairs_out=int(kept.sum()), cut=np.float32(med), margin=margin, margin_at=limit)


def trimmed_count(n, ratio, min_corr):
    """m = min(n, max(min_correspondences, (unsigned)(overlap_ratio * (float)n))), ratio and product in float32"""
    m = int(np.float32(ratio) * np.float32(n))
    return min(n, max(int(min_corr), m))


def trimmed(d2, alive, ratio, min_corr=0):
    """-> kept mask, stats.  Keep d2 <= the m-th smallest (ties at the cut all stay)."""
    d2 = np.asarray(d2, np.float32)
    n = int(alive.sum())
    m = trimmed_count(n, ratio, min_corr)
    if m == 0:
        return np.zeros_like(alive), dict(pairs_in=n, pairs_out=0, cut=np.float32(0.0), margin=_INF, margin_at=0.0)
    s = np.sort(d2[alive])
    t = s[m - 1]
    kept = alive & (d2 <= t)
    above = s[s > t]
    margin = _rel_gap(above.min(), t) if above.size else _INF
    return kept, dict(pairs_in=n, pairs_out=int(kept.sum()), cut=np.float32(t), margin=margin, margin_at=float(t))


def one_to_one(idx, d2, alive):
    """-> kept mask, stats.  Per target index the pair with the smallest d2, the lowest source index among equals."""
    d2 = np.asarray(d2, np.float32)
    kept = np.zeros_like(alive)
    src = np.flatnonzero(alive)
    margin, at = _INF, 0.0
    if src.size:
        order = np.lexsort((src, d2[src], idx[src]))          # by target, then d2, then source index
        t_sorted = idx[src][order]
        _, first = np.unique(t_sorted, return_index=True)
        kept[src[order][first]] = True
        d_sorted = d2[src][order].astype(np.float64)
        second = first + 1
        ok = (second < t_sorted.size)
        ok[ok] = t_sorted[second[ok]] == t_sorted[first[ok]]
        if ok.any():
            a, b = d_sorted[first[ok]], d_sorted[second[ok]]
            mx = np.maximum(np.abs(a), np.abs(b))
            gap = np.where(mx > 0, np.abs(b - a) / np.where(mx > 0, mx, 1.0), 0.0)
            margin, at = float(gap.min()), float(a[int(gap.argmin())])
    return kept, dict(pairs_in=int(alive.sum()), pairs_out=int(kept.sum()), cut=np.float32(0.0), margin=margin, margin_at=at)


def apply_chain(idx, d2, max_dist, chain):
    """The gate, then the chain.  -> kept mask (per source point), [stats per stage]."""
    idx = np.asarray(idx)
    d2 = np.asarray(d2, np.float32)
    with np.errstate(invalid="ignore"):
        alive = (idx >= 0) & (d2.astype(np.float64) <= float(max_dist) * float(max_dist))
    stats = []
    for stage in chain:
        kind, value = int(stage[0]), float(stage[1]) if len(stage) > 1 else 0.0
        minc = int(stage[2]) if len(stage) > 2 else 0
        if kind == MEDIAN:
            alive, st = median_distance(d2, alive, value)
        elif kind == TRIMMED:
            alive, st = trimmed(d2, alive, value, minc)
        elif kind == ONE_TO_ONE:
            alive, st = one_to_one(idx, d2, alive)
        else:
            raise ValueError(kind)
        stats.append(st)
    return alive, stats


def correspondences(src, tgt, T, max_dist, chain):
    """What one iteration at T hands to the solve: idx (-1 = removed), d2 (+inf = removed), stats."""
    import oracle
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32)
    if src.shape[0] == 0 or tgt.shape[0] == 0:
        idx = np.full(src.shape[0], -1, np.int32)
        d2 = np.full(src.shape[0], np.inf, np.float32)
    else:
        idx, d2 = oracle.nn(src, tgt, T)
    kept, stats = apply_chain(idx, d2, max_dist, chain)
    return np.where(kept, idx, -1).astype(np.int32), np.where(kept, d2, np.float32(np.inf)).astype(np.float32), stats


def align(src, tgt, chain, method="p2p", max_iterations=10, transformation_epsilon=1e-6, max_correspondence_distance=1.0,
          euclidean_fitness_epsilon=-np.finfo(np.float64).max, min_correspondences=3, guess=None, normals=None):
    """pcl::IterativeClosestPoint(WithNormals)::align with a rejector chain.  Returns dict(T, converged, iterations, state, n_corr,
    mse, stats (the last iteration's), margins (per iteration, per stage: the cut margin and the d2 it was measured at))."""
    import oracle
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32)
    out = dict(T=np.eye(4, dtype=np.float32), converged=False, iterations=0, state=NOT_CONVERGED, n_corr=0, mse=0.0, stats=[],
               margins=[])
    if tgt.shape[0] == 0:
        return out
    if method == "p2plane" and normals is None:
        normals = oracle.gicp_normals(tgt)
    final = np.eye(4) if guess is None else np.asarray(guess, np.float32).astype(np.float64)
    mse_prev = np.finfo(np.float64).max
    nr, converged, state, n_c, mse, stats = 0, False, NOT_CONVERGED, 0, 0.0, []
    while True:
        idx, d2, stats = correspondences(src, tgt, final, max_correspondence_distance, chain)
        out["margins"].append([(s["margin"], s["margin_at"]) for s in stats])
        if method == "p2plane":
            sums = oracle.p2plane_sums(src, tgt, normals, final, idx, d2, max_correspondence_distance)
            n_c, sum_d2 = int(sums[0]), sums[1]
        else:
            sums = oracle.reduce(src, tgt, final, idx, d2, max_correspondence_distance)
            n_c, sum_d2 = int(sums[0]), sums[16]
        if n_c < min_correspondences:
            state, converged = NO_CORRESPONDENCES, False
            break
        Tk = oracle.p2plane_solve(sums) if method == "p2plane" else oracle.umeyama(sums)
        if Tk is None:
            state, converged = NOT_CONVERGED, False
            break
        final = Tk @ final
        mse = sum_d2 / sums[0]
        nr += 1
        if nr >= max_iterations:
            converged, state = True, ITERATIONS
        else:
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
    out.update(T=final.astype(np.float32), converged=converged, iterations=nr, state=state, n_corr=n_c, mse=float(mse), stats=stats)
    return out
