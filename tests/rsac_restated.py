"""The sample-consensus rejector (include/icpgpu.h, "sample-consensus rejector") restated in NumPy / Python, operation for operation.
It never calls the library.

    ranks        splitmix64 over the counter 48 t + 3 d + c + 1 (sac_restated's constants), rank = ((z >> 32) * m) >> 32; up to 16
                 redraws, the first GOOD one is the sample
    spacing      the search's d2 = fma(dz, dz, fma(dy, dy, dx * dx)) in float32 (search_restated.fma32 emulates the fused operation
                 exactly) among the three sampled P, each (double)d2 > sample_d2
    sample_d2    the nine sums about the first finite P by math.fsum (exact, rounded once), means and covariances in double,
                 normals_restated.jacobi3, eigenvalues below 0 as 0, s = ((sqrt e0 + sqrt e1) + sqrt e2) / 3, s * s
    transform    the 17 sums of the three pairs in double, in sample order -> oracle.umeyama -> float32
    inlier       scp_restated.transform's fma chain, the search's d2, (double)d2 < threshold * threshold
    loop         sac_restated.next_k with n = m and probability 0.99

run() is the vectorised form the device is compared with (transforms=: the device's own, to score with); run_literal() beside it
is a per-hypothesis, per-pair Python loop with Python integers for the generator, exact rational arithmetic for the fused operations
and fractions.Fraction sums -- tests/test_rsac_host.py holds the two against each other.  stage() / correspondences() / align() put
run() where the chain puts the stage."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import normals_restated as NR
import scp_restated as SCP
from sac_restated import GOLDEN, MASK, MIX1, MIX2, next_k
from scp_restated import d2_points, fma_exact

F32, F64 = np.float32, np.float64
DRAWS = 16
BATCH = 64
MAX_ITERATIONS = 65536
PROBABILITY = 0.99
DEFAULT_SEED = 12345
KIND = 5   # ICPGPU_REJECT_SAMPLE_CONSENSUS


class Refused(Exception):
    """What the library answers with ICPGPU_ERR_INVALID_ARG."""


def check(threshold, max_iterations):
    if not (math.isfinite(threshold) and threshold >= 0.0):
        raise Refused("inlier_threshold")
    if not 0 <= max_iterations <= MAX_ITERATIONS:
        raise Refused("max_iterations")


def _cloud(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).reshape(-1, 4)


# ---- the generator ---------------------------------------------------------------------------------------------------------
def rank_int(seed: int, t: int, d: int, c: int, m: int) -> int:
    """rank_c of redraw d of hypothesis t in Python integers."""
    z = (seed + (48 * t + 3 * d + c + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * MIX1) & MASK
    z = ((z ^ (z >> 27)) * MIX2) & MASK
    z ^= z >> 31
    return ((z >> 32) * m) >> 32


def ranks_of(seed: int, t0: int, count: int, m: int) -> np.ndarray:
    """(count, 16, 3) int64: every redraw of hypotheses t0 .. t0 + count - 1, in uint64 arithmetic (NumPy's wraps modulo 2^64)."""
    with np.errstate(over="ignore"):
        t = np.arange(t0, t0 + count, dtype=np.uint64)[:, None, None]
        d = np.arange(DRAWS, dtype=np.uint64)[None, :, None]
        c = np.arange(3, dtype=np.uint64)[None, None, :]
        z = np.uint64(seed & MASK) + (np.uint64(48) * t + np.uint64(3) * d + c + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


# ---- the sample distance ---------------------------------------------------------------------------------------------------
def moments_of(P):
    """(moments9 float64, the number of finite P): the nine sums about the first finite P; zeros without one."""
    xyz = _cloud(P)[:, :3]
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    if fin.size == 0:
        return np.zeros(9, F64), 0
    d = (xyz[fin] - xyz[fin[0]]).astype(F64)      # (the subtraction in float32, then widened)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    terms = (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz, dx, dy, dz)
    return np.array([math.fsum(t.tolist()) for t in terms], F64), int(fin.size)


def eigenvalues_of(moments, n: int) -> np.ndarray:
    """The Jacobi's diagonal, ascending, BEFORE the clamp (float64)."""
    S, dn = np.asarray(moments, F64), F64(n)
    with np.errstate(all="ignore"):
        mean = S[6:9] / dn
        a = np.zeros((1, 3, 3))
        for e, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            a[0, i, j] = a[0, j, i] = S[e] / dn - mean[i] * mean[j]
        d, _ = NR.jacobi3(a)
    return np.sort(np.array([d[0, 0, 0], d[0, 1, 1], d[0, 2, 2]], F64))


def sample_d2_of(moments, n: int) -> float:
    if n == 0:
        return 0.0
    e = [0.0 if v < 0.0 else float(v) for v in eigenvalues_of(moments, n)]
    s = ((math.sqrt(e[0]) + math.sqrt(e[1])) + math.sqrt(e[2])) / 3.0
    return s * s


# ---- hypotheses ------------------------------------------------------------------------------------------------------------
def hypotheses(P, Q, seed: int, t0: int, count: int, sample_d2: float):
    """(ranks (count, 3) int32 -- -1 without a good draw --, good (count,) bool, sums17 (count, 17) float64, draw (count,) the
    redraw taken, -1 without one)."""
    P, Q = _cloud(P)[:, :3], _cloud(Q)[:, :3]
    m = P.shape[0]
    ranks = np.full((count, 3), -1, np.int32)
    good = np.zeros(count, bool)
    draw = np.full(count, -1, np.int32)
    sums = np.zeros((count, 17), F64)
    if m < 3 or count == 0:
        return ranks, good, sums, draw
    R = ranks_of(seed, t0, count, m)
    ok = (R[..., 0] != R[..., 1]) & (R[..., 0] != R[..., 2]) & (R[..., 1] != R[..., 2])
    p, q = P[R], Q[R]                                   # (count, 16, 3, 3)
    ok &= np.isfinite(p).all(axis=(2, 3)) & np.isfinite(q).all(axis=(2, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ok &= d2_points(p[:, :, a], p[:, :, b]).astype(F64) > sample_d2
    good = ok.any(axis=1)
    first = ok.argmax(axis=1)
    draw[good] = first[good]
    rows = np.arange(count)
    ranks[good] = R[rows, first][good]
    p64, q64 = p[rows, first].astype(F64), q[rows, first].astype(F64)     # (count, 3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):                               # in sample order, every sum from 0
            sums[:, 0] += 1.0
            sums[:, 1:4] += p64[:, c]
            sums[:, 4:7] += q64[:, c]
            sums[:, 7:16] += (q64[:, c, :, None] * p64[:, c, None, :]).reshape(count, 9)
    sums[~good] = 0.0
    return ranks, good, sums, draw


def solve(good, sums):
    """oracle.umeyama per good draw, rounded to float32: (transforms (count, 4, 4) float32 -- zeros where INVALID --, valid)."""
    import oracle
    T = np.zeros((len(good), 4, 4), F32)
    valid = np.zeros(len(good), bool)
    for e in np.flatnonzero(good):
        Tk = oracle.umeyama(sums[e])
        with np.errstate(over="ignore"):
            Tf = None if Tk is None else np.asarray(Tk, F64).astype(F32)
        if Tf is not None and np.isfinite(Tf).all():
            T[e], valid[e] = Tf, True
    return T, valid


def inlier_mask(T, P, Q, threshold: float) -> np.ndarray:
    """(m,) bool: the pairs that are inliers of the 4x4 float32 transform T."""
    P, Q = _cloud(P), _cloud(Q)
    img = SCP.transform(np.asarray(T, F32).T.reshape(16), P)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = d2_points(img[:, :3], Q[:, :3]).astype(F64)
        return np.isfinite(P[:, :3]).all(axis=1) & np.isfinite(Q[:, :3]).all(axis=1) & (d2 < float(threshold) * float(threshold))


# ---- the core --------------------------------------------------------------------------------------------------------------
def run(P, Q, threshold: float = 0.05, max_iterations: int = 1000, seed: int = DEFAULT_SEED, transforms=None) -> dict:
    """The core over the pairs (P_r, Q_r).  transforms (>= iterations, 4, 4): the device's own, to score with (validity is the restated
    solve's all the same); None: the restated solve's."""
    check(threshold, max_iterations)
    P, Q = _cloud(P), _cloud(Q)
    m = P.shape[0]
    mom, n_fin = moments_of(P)
    s_d2 = sample_d2_of(mom, n_fin)
    out = dict(m=m, moments9=mom, n_finite=n_fin, sample_d2=s_d2, iterations=0, status=0, best_t=-1, best_T=np.eye(4, dtype=F32),
               counts=np.zeros(0, np.int32), ranks=np.zeros((0, 3), np.int32), transforms=np.zeros((0, 4, 4), F32),
               solved=np.zeros((0, 4, 4), F32), sums17=np.zeros((0, 17), F64), valid=np.zeros(0, bool), draw=np.zeros(0, np.int32),
               kept=np.zeros(m, bool), n_kept=0, batches=0, host_waits=0)
    if m == 0:
        return out
    counts, ranks, T_used, T_solved, sums17, valid_all, draws = [], [], [], [], [], [], []
    best_count, best_t, k, t, batches = 0, -1, math.inf, 0, 0
    if m < 3:                                             # every hypothesis INVALID by rule; no batch
        it = max_iterations
        counts = [-1] * it
        ranks = [[-1, -1, -1]] * it
        T_used = T_solved = [np.zeros((4, 4), F32)] * it
        sums17 = [np.zeros(17)] * it
        valid_all, draws = [False] * it, [-1] * it
        t = it
    else:
        batch = None
        while True:
            if t >= max_iterations or float(t) >= k:
                break
            h = t % BATCH
            if h == 0:
                n_b = min(BATCH, max_iterations - t)
                b_ranks, b_good, b_sums, b_draw = hypotheses(P, Q, seed, t, n_b, s_d2)
                b_solved, b_valid = solve(b_good, b_sums)
                if transforms is None:
                    b_T = b_solved
                else:     # (the device hands out what its loop reached: the rest of the batch is never looked at, zeros will do)
                    given = np.zeros((n_b, 4, 4), F32)
                    have = np.asarray(transforms, F32).reshape(-1, 4, 4)[t:t + n_b]
                    given[:len(have)] = have
                    b_T = np.where(b_valid[:, None, None], given, F32(0))
                b_counts = np.array([int(inlier_mask(b_T[e], P, Q, threshold).sum()) if b_valid[e] else -1 for e in range(n_b)], np.int32)
                batch = (b_ranks, b_sums, b_draw, b_solved, b_valid, b_T, b_counts)
                batches += 1
            b_ranks, b_sums, b_draw, b_solved, b_valid, b_T, b_counts = batch
            cnt = int(b_counts[h])
            counts.append(cnt)
            ranks.append(b_ranks[h])
            T_used.append(b_T[h])
            T_solved.append(b_solved[h])
            sums17.append(b_sums[h])
            valid_all.append(bool(b_valid[h]))
            draws.append(int(b_draw[h]))
            if cnt > 0 and cnt > best_count:
                best_count, best_t = cnt, t
                k = next_k(cnt, m, PROBABILITY)
            t += 1
    it = t
    out.update(iterations=it, best_t=best_t, batches=batches, host_waits=1 + 2 * batches,
               counts=np.array(counts, np.int32).reshape(it), ranks=np.array(ranks, np.int32).reshape(it, 3),
               transforms=np.array(T_used, F32).reshape(it, 4, 4), solved=np.array(T_solved, F32).reshape(it, 4, 4),
               sums17=np.array(sums17, F64).reshape(it, 17), valid=np.array(valid_all, bool).reshape(it),
               draw=np.array(draws, np.int32).reshape(it))
    if best_t < 0:
        out["status"] = 1
    elif best_count < 3:
        out["status"] = 2
    else:
        out["status"] = 3
        out["best_T"] = out["transforms"][best_t].copy()
    out["kept"] = inlier_mask(out["best_T"], P, Q, threshold) if out["status"] == 3 else np.ones(m, bool)
    out["n_kept"] = int(out["kept"].sum())
    return out


def reject(source, target, index_query, index_match, threshold: float = 0.05, max_iterations: int = 1000, seed: int = DEFAULT_SEED,
           transforms=None) -> dict:
    """The call of its own: P_r = source[index_query[r]], Q_r = target[index_match[r]]; an index outside its cloud is Refused."""
    source, target = _cloud(source), _cloud(target)
    iq, im = np.asarray(index_query, np.int64).reshape(-1), np.asarray(index_match, np.int64).reshape(-1)
    check(threshold, max_iterations)
    if iq.size != im.size or (iq.size and (iq.min() < 0 or iq.max() >= len(source) or im.min() < 0 or im.max() >= len(target))):
        raise Refused("an index outside its cloud")
    return run(source[iq], target[im], threshold, max_iterations, seed, transforms)


# ---- the literal loop ------------------------------------------------------------------------------------------------------
def _d2_literal(p, q) -> float:
    dx, dy, dz = (float(F32(F32(q[k]) - F32(p[k]))) for k in range(3))
    return fma_exact(dz, dz, fma_exact(dy, dy, float(F32(F32(dx) * F32(dx)))))


def _xform_literal(T, p):
    return [fma_exact(float(T[r, 2]), float(p[2]), fma_exact(float(T[r, 1]), float(p[1]), fma_exact(float(T[r, 0]), float(p[0]), float(T[r, 3]))))
            for r in range(3)]


def run_literal(P, Q, threshold: float = 0.05, max_iterations: int = 1000, seed: int = DEFAULT_SEED) -> dict:
    """run() as a per-hypothesis, per-pair Python loop: Python integers for the generator, exact rational arithmetic for every fused
    operation, fractions.Fraction for the nine sums.  For small inputs."""
    import oracle
    check(threshold, max_iterations)
    P, Q = _cloud(P), _cloud(Q)
    m = P.shape[0]
    finite = lambda p: all(math.isfinite(float(v)) for v in p[:3])
    fin = [r for r in range(m) if finite(P[r])]
    mom = [0.0] * 9
    if fin:
        K = P[fin[0]]
        acc = [Fraction(0)] * 9
        for r in fin:
            dx, dy, dz = (Fraction(float(F32(P[r][a] - K[a]))) for a in range(3))
            for e, term in enumerate((dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz, dx, dy, dz)):
                acc[e] += term
        mom = [float(v) for v in acc]                      # (Fraction -> float rounds correctly: the exact sum rounded once)
    s_d2 = sample_d2_of(mom, len(fin))
    thr2 = float(threshold) * float(threshold)

    def inliers_of(T):
        out = []
        for r in range(m):
            if finite(P[r]) and finite(Q[r]) and _d2_literal(_xform_literal(T, P[r]), Q[r]) < thr2:
                out.append(r)
        return out

    counts, ranks, Ts = [], [], []
    best_count, best_t, k, t = 0, -1, math.inf, 0
    while m > 0:
        if t >= max_iterations or float(t) >= k:
            break
        s, T = [-1, -1, -1], np.zeros((4, 4), F32)
        cnt = -1
        for d in range(DRAWS if m >= 3 else 0):
            r = [rank_int(seed, t, d, c, m) for c in range(3)]
            if len(set(r)) < 3 or not all(finite(P[i]) and finite(Q[i]) for i in r):
                continue
            if not all(_d2_literal(P[r[a]], P[r[b]]) > s_d2 for a, b in ((0, 1), (0, 2), (1, 2))):
                continue
            s = r
            sums = [0.0] * 17
            for c in range(3):
                p, q = [float(v) for v in P[r[c]][:3]], [float(v) for v in Q[r[c]][:3]]
                sums[0] += 1.0
                for a in range(3):
                    sums[1 + a] += p[a]
                    sums[4 + a] += q[a]
                    for b in range(3):
                        sums[7 + 3 * a + b] += q[a] * p[b]
            Tk = oracle.umeyama(np.array(sums))
            with np.errstate(over="ignore"):
                Tf = None if Tk is None else np.asarray(Tk, F64).astype(F32)
            if Tf is not None and np.isfinite(Tf).all():
                T = Tf
                cnt = len(inliers_of(T))
            break
        counts.append(cnt)
        ranks.append(s)
        Ts.append(T)
        if cnt > 0 and cnt > best_count:
            best_count, best_t = cnt, t
            k = next_k(cnt, m, PROBABILITY)
        t += 1
    status = 0 if m == 0 else 1 if best_t < 0 else 2 if best_count < 3 else 3
    best_T = Ts[best_t] if status == 3 else np.eye(4, dtype=F32)
    kept = np.zeros(m, bool)
    kept[inliers_of(best_T) if status == 3 else list(range(m))] = True
    return dict(m=m, moments9=np.array(mom, F64), sample_d2=s_d2, iterations=t, status=status, best_t=best_t, best_T=best_T,
                counts=np.array(counts, np.int32), ranks=np.array(ranks, np.int32).reshape(t, 3), transforms=np.array(Ts, F32).reshape(t, 4, 4),
                kept=kept, n_kept=int(kept.sum()))


# ---- where the chain puts the stage ----------------------------------------------------------------------------------------
def stage(src, tgt, T, idx, alive, threshold: float, max_iterations: int, seed: int = DEFAULT_SEED, transforms=None):
    """The stage over the pairs `alive` marks: P_r = T * src[i] (the search's rounding), Q_r = tgt[idx[i]], ascending i.
    -> (alive afterwards, the core's record with `source_ranks`)."""
    src, tgt = _cloud(src), _cloud(tgt)
    ranks = np.flatnonzero(alive)
    img = SCP.transform(np.asarray(T, F64).astype(F32).T.reshape(16), src)
    r = run(img[ranks], tgt[np.asarray(idx)[ranks]] if len(tgt) else np.zeros((0, 4), F32), threshold, max_iterations, seed, transforms)
    r["source_ranks"] = ranks
    if ranks.size == 0:
        r["host_waits"] = 1 if (len(src) and len(tgt)) else 0
    out = np.zeros(len(src), bool)
    out[ranks[r["kept"]]] = True
    return out, r


def correspondences(src, tgt, T, max_dist, chain, seed: int = DEFAULT_SEED, nn=None, transforms=None):
    """rejectors_restated.correspondences for a chain that may hold (KIND, threshold, max_iterations) stages: idx (-1 = removed),
    d2 (+inf = removed), stats per stage, the record of the last sample-consensus stage (or None).  nn: (idx, d2) of every source
    point when the caller has them (e.g. past a reciprocal test: idx = -1 where it removed the pair)."""
    import oracle
    import rejectors_restated as RR
    src, tgt = _cloud(src), _cloud(tgt)
    if nn is not None:
        idx, d2 = np.asarray(nn[0]), np.asarray(nn[1], F32)
    elif len(src) == 0 or len(tgt) == 0:
        idx, d2 = np.full(len(src), -1, np.int32), np.full(len(src), np.inf, F32)
    else:
        idx, d2 = oracle.nn(src, tgt, T)
    alive, stats = RR.apply_chain(idx, d2, max_dist, [])
    rec = None
    last = max([i for i, st in enumerate(chain) if int(st[0]) == KIND], default=-1)
    for i, st in enumerate(chain):
        if int(st[0]) == KIND:
            n_in = int(alive.sum())
            alive, rec = stage(src, tgt, T, idx, alive, float(st[1]), int(st[2]), seed, transforms if i == last else None)
            stats.append(dict(pairs_in=n_in, pairs_out=int(alive.sum()), cut=F32(0.0)))
        else:
            masked = np.where(alive, idx, -1)
            alive, s1 = RR.apply_chain(masked, d2, max_dist, [st])
            stats += s1
    return np.where(alive, idx, -1).astype(np.int32), np.where(alive, d2, F32(np.inf)).astype(F32), stats, rec


def align(src, tgt, chain, max_iterations: int = 10, transformation_epsilon: float = 1e-6, max_correspondence_distance: float = 1.0,
          guess=None, seed: int = DEFAULT_SEED) -> dict:
    """Point-to-point pcl::IterativeClosestPoint::align with such a chain (rejectors_restated.align's loop): dict(T, iterations, n_corr)."""
    import oracle
    src, tgt = _cloud(src), _cloud(tgt)
    final = np.eye(4) if guess is None else np.asarray(guess, F32).astype(F64)
    nr, n_c = 0, 0
    mse_prev = np.finfo(F64).max
    while True:
        idx, d2, _, _ = correspondences(src, tgt, final, max_correspondence_distance, chain, seed)
        sums = oracle.reduce(src, tgt, final, idx, d2, max_correspondence_distance)
        n_c = int(sums[0])
        if n_c < 3:
            break
        Tk = oracle.umeyama(sums)
        if Tk is None:
            break
        final = Tk @ final
        mse = sums[16] / sums[0]
        nr += 1
        if nr >= max_iterations:
            break
        if 0.5 * (np.trace(Tk[:3, :3]) - 1.0) >= 1.0 - transformation_epsilon and float(Tk[:3, 3] @ Tk[:3, 3]) <= transformation_epsilon:
            break
        if abs(mse - mse_prev) < 1e-12:
            break
        mse_prev = mse
    return dict(T=final.astype(F32), iterations=nr, n_corr=n_c)
