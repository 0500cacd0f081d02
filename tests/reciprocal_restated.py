"""Reciprocal correspondences restated in NumPy (include/icpgpu.h, "reciprocal correspondences") from the oracle's pinned primitives
only: X = oracle.transform_cloud(src, T); forward oracle.nn(src, tgt, T); reverse oracle.nn(tgt, X, I) -- the nearest of ALL
transformed source points to every target point, the lowest source index among equals (the oracle's tie rule, here applied to the
source's order: the deviation from PCL the header records); a gated pair (i, j) stays iff reverse[j] == i.  The rejector chain of
tests/rejectors_restated.py then runs on the survivors, and align() is that module's ICP loop with this estimation step in it."""
from __future__ import annotations

import numpy as np

import rejectors_restated as R

_I4 = np.eye(4, dtype=np.float32)
_chain_correspondences = R.correspondences      # (align() below replaces the module's name while it runs)


def gate(idx, d2, max_dist):
    """the pairs past the distance gate: (double)d2 <= max_dist^2"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(idx) >= 0) & (np.asarray(d2, np.float32).astype(np.float64) <= float(max_dist) * float(max_dist))


def reverse_nn(src, tgt, T):
    """-> (k, d2) per target point: its nearest neighbour among the transformed source points (non-finite ones are nobody's
    neighbour: the oracle never returns them)"""
    import oracle
    X = oracle.transform_cloud(np.asarray(src, np.float32), T)
    return oracle.nn(np.asarray(tgt, np.float32), X, _I4)


def reciprocal(src, tgt, T, max_dist):
    """-> idx, d2 of the forward search, kept mask, stats dict(pairs_in, pairs_out)"""
    import oracle
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32)
    n = src.shape[0]
    if n == 0 or tgt.shape[0] == 0:
        return np.full(n, -1, np.int32), np.full(n, np.inf, np.float32), np.zeros(n, bool), dict(pairs_in=0, pairs_out=0)
    idx, d2 = oracle.nn(src, tgt, T)
    alive = gate(idx, d2, max_dist)
    k, _ = reverse_nn(src, tgt, T)
    kept = alive.copy()
    who = np.flatnonzero(alive)
    kept[who] = k[idx[who]] == who
    return idx, d2, kept, dict(pairs_in=int(alive.sum()), pairs_out=int(kept.sum()))


def correspondences(src, tgt, T, max_dist, chain=(), use_reciprocal=True):
    """What one iteration at T hands to the solve: gate, reciprocal test, chain.  -> idx (-1 = removed), d2 (+inf = removed),
    the chain's stats, the reciprocal stage's stats (zeroes with the flag off)"""
    if not use_reciprocal:
        idx, d2, stats = _chain_correspondences(src, tgt, T, max_dist, list(chain))
        return idx, d2, stats, dict(pairs_in=0, pairs_out=0)
    idx, d2, kept, rstats = reciprocal(src, tgt, T, max_dist)
    kept, stats = R.apply_chain(np.where(kept, idx, -1), d2, max_dist, list(chain))
    return np.where(kept, idx, -1).astype(np.int32), np.where(kept, d2, np.float32(np.inf)).astype(np.float32), stats, rstats


def align(src, tgt, chain=(), use_reciprocal=True, **kw):
    """rejectors_restated.align with the reciprocal estimation step in its loop (that module's loop calls its own module-level
    `correspondences` once per iteration: it is replaced for the duration of the call, not copied).  The result carries
    `reciprocal`: the stage's statistics of the last iteration."""
    last = dict(pairs_in=0, pairs_out=0)

    def step(s, t, T, max_dist, ch):
        idx, d2, stats, rstats = correspondences(s, t, T, max_dist, ch, use_reciprocal)
        last.update(rstats)
        return idx, d2, stats

    saved = R.correspondences
    R.correspondences = step
    try:
        out = R.align(src, tgt, list(chain), **kw)
    finally:
        R.correspondences = saved
    out["reciprocal"] = dict(last)
    return out
