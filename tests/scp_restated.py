"""The feature-space k-nearest search and the sample-consensus alignment with pre-rejection (include/icpgpu.h, "feature-space k-nearest"
and "sample-consensus alignment") restated in NumPy / Python, operation for operation.  It never calls the library.

    feature d2   d_b = q[b] - t[b] in float32; d2 = d_0 * d_0, then fmaf(d_b, d_b, d2) for b = 1 .. 32 (search_restated.fma32 emulates the
                 fused operation exactly)
    rows         by key = (bits of d2) << 32 | target row: np.lexsort((index, d2_bits)); the min(k, finite target rows) smallest; a row
                 with a non-finite component is never a neighbour (target) or finds nothing (query)
    hypotheses   sac_restated's splitmix64 over the counter (2 nr) t + c + 1: nr source draws, then nr target picks out of the sampled
                 source points' rows
    prerejection per polygon edge the search's d2 on the source and on the target side, min / max in float32 against
                 float32(similarity^2)
    transform    the 17 sums of the nr pairs in double, in sample order -> oracle.umeyama -> float32
    fitness      symmetric_restated.xform32 / xform_point's fma chain, the nearest target point by key (search_restated.knn with k = 1),
                 d2 < float32(d * d) strictly, the inliers' d2 summed by math.fsum (exact, rounded once)
    choice       t ascending; count > 0, float32(count) / float32(n_s) >= float32(inlier_fraction), error strictly below the best

feature_knn() / align() are the vectorised forms the device is compared with; feature_knn_literal() / align_literal() beside them are
per-pair, per-hypothesis, per-point Python loops with Python integers for the generator and exact rational arithmetic for the fused
operations -- tests/test_scp_host.py holds the two against each other."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import search_restated as SR
from sac_restated import GOLDEN, MASK, MIX1, MIX2
from search_restated import fma32
from symmetric_restated import xform32

F32, F64 = np.float32, np.float64
BINS = 33
SEARCH_MAX_K = SR.SEARCH_MAX_K
MAX_ITERATIONS = 1 << 20
MAX_SAMPLES = 8
CHUNK = 65536
FLT_MAX = float(np.finfo(F32).max)
INVALID, PREREJECTED, NO_TRANSFORM, EVALUATED = 0, 1, 2, 3


class Refused(Exception):
    """What the library answers with ICPGPU_ERR_INVALID_ARG."""


# ---- feature-space k-nearest --------------------------------------------------------------------------------------------------
def _feat(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).reshape(-1, BINS)


def feature_d2(query, target) -> np.ndarray:
    """(n_q, n_t) float32: the 33-term chain of every query row against every target row."""
    q, t = _feat(query), _feat(target)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, None, 0] - t[None, :, 0]
        acc = (d * d).astype(F32)
        for b in range(1, BINS):
            d = q[:, None, b] - t[None, :, b]
            acc = fma32(d, d, acc)
    return acc


def feature_knn(target, query, k: int):
    """(idx (n_q, k) int32, d2 (n_q, k) float32, n_found (n_q,) int32)."""
    if not 1 <= k <= SEARCH_MAX_K:
        raise Refused(f"k {k}")
    t, q = _feat(target), _feat(query)
    n_q = q.shape[0]
    idx = np.full((n_q, k), -1, np.int32)
    d2 = np.full((n_q, k), np.inf, F32)
    n_found = np.zeros(n_q, np.int32)
    tfin = np.flatnonzero(np.isfinite(t).all(axis=1))
    rows = np.flatnonzero(np.isfinite(q).all(axis=1))
    kk = min(k, tfin.size)
    if kk == 0 or rows.size == 0:
        return idx, d2, n_found
    tt = t[tfin]
    E = min(tfin.size, kk + 8)
    step = max(1, (1 << 21) // tfin.size)
    for a in range(0, rows.size, step):
        r = rows[a:a + step]
        if E == tfin.size or not (np.abs(q[r]).max() < 1e15 and np.abs(tt).max() < 1e15):
            for i, row in zip(r, feature_d2(q[r], tt)):
                order = np.lexsort((tfin, SR._bits(row)))[:kk]
                idx[i, :kk], d2[i, :kk] = tfin[order], row[order]
            continue
        # A float64 expansion is within 1e-9 (relative to the rows' norms) of the chain: it only NARROWS which pairs get the chain.  Rows
        # whose E-th candidate is not clearly beyond the kk-th get the chain against every target row.
        q64, t64 = q[r].astype(F64), tt.astype(F64)
        nq, nt = (q64 * q64).sum(axis=1), (t64 * t64).sum(axis=1)
        plain = nq[:, None] + nt[None, :] - 2.0 * (q64 @ t64.T)
        cand = np.argpartition(plain, E - 1, axis=1)[:, :E]
        sel = np.sort(np.take_along_axis(plain, cand, axis=1), axis=1)
        slack = 1e-5 * sel[:, kk - 1] + 1e-9 * (nq + nt.max())
        sure = sel[:, E - 1] > sel[:, kk - 1] + slack
        for n_row, i in enumerate(r):
            if sure[n_row]:
                c = np.sort(cand[n_row])
                row, index = feature_d2(q[i:i + 1], tt[c])[0], tfin[c]
            else:
                row, index = feature_d2(q[i:i + 1], tt)[0], tfin
            order = np.lexsort((index, SR._bits(row)))[:kk]
            idx[i, :kk], d2[i, :kk] = index[order], row[order]
    n_found[rows] = kk
    return idx, d2, n_found


def round_f32(x: Fraction) -> float:
    """The float32 nearest to the rational x, ties to even; +-inf beyond the format's range."""
    if x == 0:
        return 0.0
    with np.errstate(over="ignore"):
        r = F32(float(x))                    # correctly rounded to double, then to float32: at most one step off
    if not np.isfinite(r):
        top = Fraction(FLT_MAX) + Fraction(2) ** 103     # half an ulp above FLT_MAX: from here on the format rounds to infinity
        if abs(x) >= top:
            return float(r)
        r = F32(math.copysign(FLT_MAX, x))
    best = None
    with np.errstate(over="ignore"):
        around = (np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf)))
    for c in around:
        if not np.isfinite(c):
            continue
        err = abs(x - Fraction(float(c)))
        even = (int(np.asarray(c, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, float(c))
    return best[1]


def fma_exact(a: float, b: float, c: float) -> float:
    """fmaf(a, b, c) of three float32 values through exact rational arithmetic."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(F32(F64(a) * F64(b) + F64(c)))      # (an infinity or a NaN: no rounding is in question)
    return round_f32(Fraction(a) * Fraction(b) + Fraction(c))


def feature_d2_literal(q_row, t_row) -> float:
    """One pair's chain, the fused operations in exact rational arithmetic."""
    q_row, t_row = np.asarray(q_row, F32), np.asarray(t_row, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = F32(q_row[0] - t_row[0])
        acc = float(F32(d * d))
        for b in range(1, BINS):
            d = float(F32(q_row[b] - t_row[b]))
            acc = fma_exact(d, d, acc)
    return acc


def feature_knn_literal(target, query, k: int):
    """feature_knn as a per-pair Python loop: Python's sort over (bits(d2) << 32 | index)."""
    t, q = _feat(target), _feat(query)
    n_q = q.shape[0]
    idx = np.full((n_q, k), -1, np.int32)
    d2 = np.full((n_q, k), np.inf, F32)
    n_found = np.zeros(n_q, np.int32)
    for i in range(n_q):
        if not all(math.isfinite(float(v)) for v in q[i]):
            continue
        keys = []
        for j in range(t.shape[0]):
            if all(math.isfinite(float(v)) for v in t[j]):
                v = F32(feature_d2_literal(q[i], t[j]))
                keys.append((int(np.asarray(v, F32).view(np.uint32)) << 32) | j)
        keys.sort()
        for s, key in enumerate(keys[:k]):
            idx[i, s] = key & 0xFFFFFFFF
            d2[i, s] = np.uint32(key >> 32).view(F32)
        n_found[i] = min(k, len(keys))
    return idx, d2, n_found


# ---- the generator --------------------------------------------------------------------------------------------------------------
def draw_int(seed: int, t: int, c: int, nr: int) -> int:
    """u_c of hypothesis t in Python integers: the upper 32 bits of splitmix64 over the counter (2 nr) t + c + 1."""
    z = (seed + (2 * nr * t + c + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * MIX1) & MASK
    z = ((z ^ (z >> 27)) * MIX2) & MASK
    z ^= z >> 31
    return z >> 32


def scale_int(u: int, n: int) -> int:
    return (u * n) >> 32


def draws(seed: int, t0: int, m: int, nr: int) -> np.ndarray:
    """(m, 2 nr) uint64: u_c of hypotheses t0 .. t0 + m - 1, in uint64 arithmetic (NumPy's wraps modulo 2^64)."""
    with np.errstate(over="ignore"):
        t = np.arange(t0, t0 + m, dtype=np.uint64)[:, None]
        c = np.arange(2 * nr, dtype=np.uint64)[None, :]
        z = np.uint64(seed & MASK) + (np.uint64(2 * nr) * t + c + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
        return z >> np.uint64(32)


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def check(nr, kc, similarity, distance, fraction, max_iterations):
    if not 3 <= nr <= MAX_SAMPLES or not 1 <= kc <= SEARCH_MAX_K:
        raise Refused("nr_samples / k_correspondences")
    if not (0.0 <= similarity <= 1.0) or not (0.0 <= fraction <= 1.0):
        raise Refused("similarity_threshold / inlier_fraction")
    if not math.isfinite(distance) or distance < 0 or not 0 <= max_iterations <= MAX_ITERATIONS:
        raise Refused("max_correspondence_distance / max_iterations")


def _cloud(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).reshape(-1, 4)


def d2_points(p, q) -> np.ndarray:
    """The search section's d2 of p[...] against q[...] (xyz in the last axis), element by element."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (q[..., k] - p[..., k] for k in range(3))
        return fma32(dz, dz, fma32(dy, dy, (dx * dx).astype(F32)))


# ---- hypotheses: samples, validity, pre-rejection, sums -------------------------------------------------------------------------
def hypotheses(source, target, rows, found, nr: int, similarity: float, seed: int, t0: int, m: int):
    """(status (m,) int32 -- EVALUATED = survived the pre-rejection --, source_idx (m, nr), target_idx (m, nr) int32, sums (m, 17) float64)"""
    source, target = _cloud(source), _cloud(target)
    n_s = source.shape[0]
    status = np.full(m, INVALID, np.int32)
    sidx = np.full((m, nr), -1, np.int32)
    tidx = np.full((m, nr), -1, np.int32)
    sums = np.zeros((m, 17), F64)
    if n_s == 0 or m == 0:
        return status, sidx, tidx, sums
    u = draws(seed, t0, m, nr)
    s = ((u[:, :nr] * np.uint64(n_s)) >> np.uint64(32)).astype(np.int64)
    mm = np.asarray(found, np.int64)[s]
    j = ((u[:, nr:] * mm.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    g = np.where(mm > 0, np.asarray(rows, np.int64)[s, np.minimum(j, np.asarray(rows).shape[1] - 1)], -1)
    sidx[:], tidx[:] = s, g
    valid = (mm > 0).all(axis=1)
    for a in range(nr):
        for b in range(a + 1, nr):
            valid &= s[:, a] != s[:, b]
    P = source[s][..., :3]
    Q = (target[np.maximum(g, 0)][..., :3] if target.shape[0] else np.full((m, nr, 3), np.nan, F32))
    valid &= np.isfinite(P).all(axis=(1, 2)) & np.isfinite(Q).all(axis=(1, 2))
    sim2 = F32(float(similarity) * float(similarity))
    nxt = (np.arange(nr) + 1) % nr
    ds, dt = d2_points(P, P[:, nxt]), d2_points(Q, Q[:, nxt])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = (np.minimum(ds, dt) / np.maximum(ds, dt)).astype(F32)
        passed = (ratio >= sim2).all(axis=1)
    status[valid & ~passed] = PREREJECTED
    status[valid & passed] = EVALUATED
    P64, Q64 = P.astype(F64), Q.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(nr):                                           # in sample order, every sum from 0
            sums[:, 0] += 1.0
            sums[:, 1:4] += P64[:, c]
            sums[:, 4:7] += Q64[:, c]
            sums[:, 7:16] += (Q64[:, c, :, None] * P64[:, c, None, :]).reshape(m, 9)
    sums[status != EVALUATED] = 0.0
    return status, sidx, tidx, sums


def solve(status, sums):
    """oracle.umeyama per survivor, rounded to float32 column-major: (transforms (m, 16) float32, status with NO_TRANSFORM)."""
    import oracle
    status = np.array(status, np.int32)
    T = np.zeros((status.size, 16), F32)
    for e in np.flatnonzero(status == EVALUATED):
        Tk = oracle.umeyama(sums[e])
        if np.isfinite(Tk).all():
            T[e] = Tk.T.reshape(16).astype(F32)
        else:
            status[e] = NO_TRANSFORM
    return T, status


# ---- fitness --------------------------------------------------------------------------------------------------------------------
def transform(T16, cloud) -> np.ndarray:
    """xform_point over a cloud: p_r = fma(T[r, 2], z, fma(T[r, 1], y, fma(T[r, 0], x, T[r, 3]))) in float32; w = 1."""
    T = xform32(np.asarray(T16, F32).reshape(4, 4).T)
    cloud = _cloud(cloud)
    out = np.ones((cloud.shape[0], 4), F32)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out[:, r] = fma32(T[r, 2], z, fma32(T[r, 1], y, fma32(T[r, 0], x, T[r, 3])))
    return out


def inlier_d2(T16, source, target, distance: float):
    """(mask (n_s,) bool, d2 (n_s,) float32): the inliers of T16 and their nearest squared distances (+inf elsewhere)."""
    source, target = _cloud(source), _cloud(target)
    r2 = F32(float(distance) * float(distance))
    img = transform(T16, source)
    ok = np.isfinite(source[:, :3]).all(axis=1) & np.isfinite(img[:, :3]).all(axis=1)
    tfin = target[np.isfinite(target[:, :3]).all(axis=1)]
    d2 = np.full(source.shape[0], np.inf, F32)
    if tfin.shape[0] and ok.any() and r2 > 0:
        # an image farther than 1.01 d outside the target's box on an axis has d2 > r2: only the others are searched
        grow = float(distance) * 1.01 + 1e-30
        lo, hi = tfin[:, :3].astype(F64).min(axis=0) - grow, tfin[:, :3].astype(F64).max(axis=0) + grow
        near = ok & ((img[:, :3] >= lo) & (img[:, :3] <= hi)).all(axis=1)
        if near.any():
            d2[near] = SR.knn(tfin, img[near], 1)[1][:, 0]
    mask = ok & (d2 < r2)
    return mask, np.where(mask, d2, F32(np.inf)).astype(F32)


def score(transforms, status, source, target, distance: float):
    """(count (m,) int32, S (m,) float64, error (m,) float32) of the EVALUATED hypotheses' transforms; 0, 0, FLT_MAX elsewhere."""
    m = len(status)
    count, S, error = np.zeros(m, np.int32), np.zeros(m, F64), np.full(m, FLT_MAX, F32)
    for e in np.flatnonzero(np.asarray(status) == EVALUATED):
        mask, d2 = inlier_d2(transforms[e], source, target, distance)
        count[e] = mask.sum()
        S[e] = math.fsum(float(v) for v in d2[mask])
        if count[e] > 0:
            error[e] = F32(S[e] / float(count[e]))
    return count, S, error


def choose(count, error, n_s: int, fraction: float) -> int:
    """best_t: t ascending; count > 0, float32(count) / float32(n_s) >= float32(fraction), error strictly below the best."""
    best_t, best = -1, F32(FLT_MAX)
    for t in range(len(count)):
        if count[t] > 0 and F32(count[t]) / F32(n_s) >= F32(fraction) and error[t] < best:
            best_t, best = t, error[t]
    return best_t


def align(source, source_feat, target, target_feat, nr: int = 3, kc: int = 2, similarity: float = 0.9, distance: float = 1.0, fraction: float = 0.25,
          max_iterations: int = 1000, seed: int = 0, transforms=None, rows=None) -> dict:
    """The whole call.  transforms (max_iterations, 16): the device's own, to score with (the status then takes NO_TRANSFORM from the
    restated solve all the same); None: the restated solve's.  rows: feature_knn(target_feat, source_feat, kc), when the caller has it."""
    check(nr, kc, similarity, distance, fraction, max_iterations)
    source, target = _cloud(source), _cloud(target)
    n_s = source.shape[0]
    if rows is None:
        rows = feature_knn(target_feat, source_feat, kc) if n_s else (np.zeros((0, kc), np.int32), None, np.zeros(0, np.int32))
    rows, _, found = rows
    status, sidx, tidx, sums = hypotheses(source, target, rows, found, nr, similarity, seed, 0, max_iterations)
    solved, status = solve(status, sums)
    T = solved if transforms is None else np.where((status == EVALUATED)[:, None], np.asarray(transforms, F32).reshape(-1, 16), F32(0))
    count, S, error = score(T, status, source, target, distance)
    best_t = choose(count, error, n_s, fraction) if n_s else -1
    out = {"status": status, "source_idx": sidx, "target_idx": tidx, "sums17": sums, "solved": solved, "transforms": T, "count": count, "sum": S,
           "error": error, "best_t": best_t, "converged": int(best_t >= 0), "rows": rows, "found": found}
    Tb = T[best_t] if best_t >= 0 else np.eye(4, dtype=F32).reshape(16)
    out["T"] = np.asarray(Tb, F32).reshape(4, 4).T.copy()
    out["fitness"] = error[best_t] if best_t >= 0 else F32(FLT_MAX)
    out["inliers"] = np.flatnonzero(inlier_d2(Tb, source, target, distance)[0]).astype(np.int32) if best_t >= 0 else np.zeros(0, np.int32)
    out["cloud"] = transform(Tb, source)
    return out


# ---- the literal loop -----------------------------------------------------------------------------------------------------------
def _d2_literal(p, q) -> float:
    dx, dy, dz = (float(F32(F32(q[k]) - F32(p[k]))) for k in range(3))
    return fma_exact(dz, dz, fma_exact(dy, dy, float(F32(F32(dx) * F32(dx)))))


def _xform_literal(T, p):
    return [fma_exact(float(T[r, 2]), float(p[2]), fma_exact(float(T[r, 1]), float(p[1]), fma_exact(float(T[r, 0]), float(p[0]), float(T[r, 3]))))
            for r in range(3)]


def align_literal(source, source_feat, target, target_feat, nr: int = 3, kc: int = 2, similarity: float = 0.9, distance: float = 1.0,
                  fraction: float = 0.25, max_iterations: int = 1000, seed: int = 0) -> dict:
    """align() as a per-hypothesis, per-point Python loop: Python integers for the generator, exact rational arithmetic for every
    fused operation, math.fsum for the sums.  For small clouds."""
    import oracle
    check(nr, kc, similarity, distance, fraction, max_iterations)
    source, target = _cloud(source), _cloud(target)
    n_s, n = source.shape[0], target.shape[0]
    rows, _, found = feature_knn_literal(target_feat, source_feat, kc) if n_s else (np.zeros((0, kc), np.int32), None, np.zeros(0, np.int32))
    sim2 = F32(float(similarity) * float(similarity))
    r2 = float(F32(float(distance) * float(distance)))
    finite = lambda p: all(math.isfinite(float(v)) for v in p[:3])
    tfin = [j for j in range(n) if finite(target[j])]

    def inliers_of(T16):
        T = np.asarray(T16, F32).reshape(4, 4).T
        out = []
        for i in range(n_s):
            if not finite(source[i]):
                continue
            img = _xform_literal(T, source[i])
            if not all(math.isfinite(v) for v in img):
                continue
            best = min((_d2_literal(img, target[j]) for j in tfin), default=math.inf)
            if best < r2:
                out.append((i, best))
        return out

    it = max_iterations
    status, count = np.full(it, INVALID, np.int32), np.zeros(it, np.int32)
    sidx, tidx = np.full((it, nr), -1, np.int32), np.full((it, nr), -1, np.int32)
    T, S, error = np.zeros((it, 16), F32), np.zeros(it, F64), np.full(it, FLT_MAX, F32)
    best_t, best = -1, F32(FLT_MAX)
    for t in range(it if n_s else 0):
        s = [scale_int(draw_int(seed, t, c, nr), n_s) for c in range(nr)]
        g = [int(rows[s[c], scale_int(draw_int(seed, t, nr + c, nr), int(found[s[c]]))]) if found[s[c]] > 0 else -1 for c in range(nr)]
        sidx[t], tidx[t] = s, g
        if len(set(s)) < nr or min(g) < 0 or not all(finite(source[i]) for i in s) or not all(finite(target[j]) for j in g):
            continue
        status[t] = PREREJECTED
        passed = True
        for c in range(nr):
            c1 = (c + 1) % nr
            ds, dt = F32(_d2_literal(source[s[c]], source[s[c1]])), F32(_d2_literal(target[g[c]], target[g[c1]]))
            with np.errstate(invalid="ignore", divide="ignore"):
                passed = passed and bool(F32(min(ds, dt)) / F32(max(ds, dt)) >= sim2)
        if not passed:
            continue
        sums = [0.0] * 17
        for c in range(nr):
            p, q = [float(v) for v in source[s[c]][:3]], [float(v) for v in target[g[c]][:3]]
            sums[0] += 1.0
            for a in range(3):
                sums[1 + a] += p[a]
                sums[4 + a] += q[a]
                for b in range(3):
                    sums[7 + 3 * a + b] += q[a] * p[b]
        Tk = oracle.umeyama(np.array(sums))
        if not np.isfinite(Tk).all():
            status[t] = NO_TRANSFORM
            continue
        status[t] = EVALUATED
        T[t] = Tk.T.reshape(16).astype(F32)
        found_in = inliers_of(T[t])
        count[t] = len(found_in)
        S[t] = math.fsum(d for _, d in found_in)
        if count[t] > 0:
            error[t] = F32(S[t] / float(count[t]))
            if F32(count[t]) / F32(n_s) >= F32(fraction) and error[t] < best:
                best_t, best = t, error[t]
    Tb = T[best_t] if best_t >= 0 else np.eye(4, dtype=F32).reshape(16)
    Tm = np.asarray(Tb, F32).reshape(4, 4).T
    cloud = np.ones((n_s, 4), F32)
    for i in range(n_s):
        with np.errstate(invalid="ignore", over="ignore"):
            cloud[i, :3] = _xform_literal(Tm, source[i]) if finite(source[i]) else transform(Tb, source[i:i + 1])[0, :3]
    return {"status": status, "source_idx": sidx, "target_idx": tidx, "transforms": T, "count": count, "sum": S, "error": error, "best_t": best_t,
            "converged": int(best_t >= 0), "T": Tm.copy(), "fitness": error[best_t] if best_t >= 0 else F32(FLT_MAX),
            "inliers": np.array([i for i, _ in inliers_of(Tb)] if best_t >= 0 else [], np.int32), "cloud": cloud, "rows": rows, "found": found}
