"""An independent NumPy restatement of the neighbour search (include/icpgpu.h, "neighbour search"): exact
k-nearest and radius search over a cloud, brute force in row chunks.  It never calls the library.
(knn_literal / radius_literal: the same with the exact expression on every pair, for small clouds -- what the chunked forms, whose
plain-float32 pass only narrows the pairs that get the exact expression, are tested against.  knn_tree / radius_tree: the same
answers where brute force is too slow -- a k-d tree narrows instead, the exact expression still decides every kept pair; knn /
radius pick by size.)

    d2        float32, dx = q.x - p.x, ... (p the query, q the cloud point); fma(dz, dz, fma(dy, dy, dx * dx)) with the fused
              operations emulated exactly
    order     by key = (bits of d2) << 32 | index of the cloud point: np.lexsort((index, d2_bits))
    k-nearest the min(k, n_finite) smallest keys over the finite cloud points; the other slots -1 / +inf; a non-finite query: none
    radius    the finite cloud points with d2 < (float32)(radius * radius), strict, ascending by key; max_nn > 0 keeps the first
              max_nn of them; rows in CSR form
"""
from __future__ import annotations

import math

import numpy as np

F32, F64 = np.float32, np.float64
SEARCH_MAX_K = 64


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
    """d2 of every point of p (rows, the queries) against every point of q (columns), float32."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    dx = q[None, :, 0] - p[:, None, 0]
    dy = q[None, :, 1] - p[:, None, 1]
    dz = q[None, :, 2] - p[:, None, 2]
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def _d2_pairs(p, q) -> np.ndarray:
    """d2 of p[..., :] against q[..., :] element by element (same leading shape)."""
    dx, dy, dz = (q[..., k] - p[..., k] for k in range(3))
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def _plain_rows(p, q) -> np.ndarray:
    dx = q[None, :, 0] - p[:, None, 0]
    dy = q[None, :, 1] - p[:, None, 1]
    dz = q[None, :, 2] - p[:, None, 2]
    return dx * dx + dy * dy + dz * dz


def _chunks(n, m):
    rows = max(1, min(n, (1 << 21) // max(m, 1)))
    for a in range(0, n, rows):
        yield a, min(n, a + rows)


# A plain float32 expression (no fused operation) is within a few ulp of d2: it only NARROWS which pairs get the exact expression.
# Every pair within _SLACK (relative) of a decision -- the k-th smallest, the radius -- is decided by the exact expression.
_SLACK = F32(1e-5)


def _bits(d2) -> np.ndarray:
    return np.ascontiguousarray(d2, F32).view(np.uint32)


def _split(cloud, queries):
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    queries = cloud if queries is None else np.asarray(queries, F32).reshape(-1, 4)
    fin = finite_mask(cloud)
    return cloud[fin, :3], np.flatnonzero(fin).astype(np.int64), queries, finite_mask(queries)


def _ordered_rows(d2, index, k):
    """Rows of candidates (d2, index: same shape) -> their k smallest keys."""
    out_i, out_d = np.empty((d2.shape[0], k), np.int64), np.empty((d2.shape[0], k), F32)
    for r in range(d2.shape[0]):
        order = np.lexsort((index[r], _bits(d2[r])))[:k]
        out_i[r], out_d[r] = index[r][order], d2[r][order]
    return out_i, out_d


def knn_brute(cloud, queries, k: int):
    """(idx (n_q, k) int32, d2 (n_q, k) float32, n_found (n_q,) int32)."""
    if not 1 <= k <= SEARCH_MAX_K:
        raise Refused(f"k {k}")
    pts, orig, queries, qfin = _split(cloud, queries)
    n_q, m = queries.shape[0], pts.shape[0]
    idx = np.full((n_q, k), -1, np.int32)
    d2 = np.full((n_q, k), np.inf, F32)
    n_found = np.zeros(n_q, np.int32)
    kk = min(k, m)
    rows = np.flatnonzero(qfin)
    if kk == 0 or rows.size == 0:
        return idx, d2, n_found
    qp = queries[rows, :3]
    E = min(m, kk + 8)
    for a, b in _chunks(len(rows), m):
        p = qp[a:b]
        if E == m:
            got_i, got_d = _ordered_rows(d2_rows(p, pts), np.broadcast_to(orig, (b - a, m)), kk)
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                plain = _plain_rows(p, pts)
                cand = np.argpartition(plain, E - 1, axis=1)[:, :E]
                sel = np.sort(np.take_along_axis(plain, cand, axis=1), axis=1)
                sure = sel[:, E - 1] > sel[:, kk - 1] * (F32(1) + _SLACK)  # nothing outside the E candidates can reach the kk smallest
            got_i, got_d = _ordered_rows(_d2_pairs(np.broadcast_to(p[:, None, :], (b - a, E, 3)), pts[cand]), orig[cand], kk)
            for r in np.flatnonzero(~sure):
                got_i[r:r + 1], got_d[r:r + 1] = _ordered_rows(d2_rows(p[r:r + 1], pts), orig[None, :], kk)
        idx[rows[a:b], :kk] = got_i
        d2[rows[a:b], :kk] = got_d
    n_found[rows] = kk
    return idx, d2, n_found


def _csr(n_q, rows, cols_orig, d2v, max_nn):
    order = np.lexsort((cols_orig, _bits(d2v), rows))
    rows, cols_orig, d2v = rows[order], cols_orig[order], d2v[order]
    counts = np.bincount(rows, minlength=n_q).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)])
    if max_nn > 0:
        keep = (np.arange(rows.size) - start[rows]) < max_nn
        rows, cols_orig, d2v = rows[keep], cols_orig[keep], d2v[keep]
        start = np.concatenate([[0], np.cumsum(np.minimum(counts, max_nn))])
    return start.astype(np.int64), cols_orig.astype(np.int32), d2v.astype(F32)


def radius_brute(cloud, queries, radius_: float, max_nn: int = 0):
    """(row_start (n_q + 1,) int64, idx int32, d2 float32)."""
    if not math.isfinite(radius_) or radius_ < 0 or max_nn < 0:
        raise Refused("radius / max_nn")
    pts, orig, queries, qfin = _split(cloud, queries)
    n_q, m = queries.shape[0], pts.shape[0]
    r2 = F32(float(radius_) * float(radius_))
    qrows = np.flatnonzero(qfin)
    R, Cc, D = [], [], []
    if r2 > 0 and m and qrows.size:
        qp = queries[qrows, :3]
        for a, b in _chunks(len(qrows), m):
            with np.errstate(over="ignore", invalid="ignore"):
                plain = _plain_rows(qp[a:b], pts)
                maybe = ~(plain > r2 * (F32(1) + _SLACK))
            rows, cols = np.nonzero(maybe)
            exact = _d2_pairs(qp[a + rows], pts[cols])
            ok = exact < r2
            R.append(qrows[a + rows[ok]])
            Cc.append(orig[cols[ok]])
            D.append(exact[ok])
    if not R:
        return np.zeros(n_q + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, F32)
    return _csr(n_q, np.concatenate(R), np.concatenate(Cc), np.concatenate(D), max_nn)


# ---- the same answers for scan-size clouds: a k-d tree narrows, the exact expression decides ------------------------------------
# A cKDTree over the finite points (float64: float32 coordinates convert exactly) only PROPOSES pairs, as the plain float32 pass of
# the brute forms does.  float32 d2 is within a few 2^-24 (relative) of the true squared distance unless it under- or overflows, the
# tree's float64 distance within a few 2^-53: a pair the tree does not propose is more than _SLACK beyond the decision, so the exact
# expression cannot bring it back.  Every proposed pair gets _d2_pairs; order and cuts are the brute forms' lexsort.  A row for which
# that argument does not hold -- the last proposal not beyond the kk-th by the slack (ties), a non-finite or overflowing d2 among the
# proposals, distances so small that d2 may underflow -- is UNCERTAIN and is decided by d2_rows over the whole cloud: never by the
# tree's order among equals.
# n_q * n above which knn / radius take the tree forms.  The callers from before the tree forms stay below it -- the largest: 6 000 x
# 6 000 (test_cluster_host.py) and cluster_restated's windows of 1 024 x 22 000 -- and keep the brute form as their reference; the one
# above it, test_gpu_fpfh.py's refused cloud (22 000 x 22 000), keeps it by raising TREE_ABOVE for itself.
TREE_ABOVE = 1 << 26
_TINY, _HUGE = 1e-30, 1e37     # squared distances outside [_TINY, _HUGE] leave float32's relative accuracy: uncertain
tree_stats = {"rows": 0, "swept": 0}  # finite query rows the tree forms answered / of them, rows left to the whole-cloud sweep


def _tree(pts):
    from scipy.spatial import cKDTree
    return cKDTree(pts.astype(F64))


def knn_tree(cloud, queries, k: int):
    """knn_brute's answer, bit for bit."""
    if not 1 <= k <= SEARCH_MAX_K:
        raise Refused(f"k {k}")
    pts, orig, queries, qfin = _split(cloud, queries)
    n_q, m = queries.shape[0], pts.shape[0]
    kk = min(k, m)
    E = kk + 8
    rows = np.flatnonzero(qfin)
    if kk == 0 or rows.size == 0 or E >= m:  # (every point would be proposed: that is the brute form)
        return knn_brute(cloud, queries, k)
    idx = np.full((n_q, k), -1, np.int32)
    d2 = np.full((n_q, k), np.inf, F32)
    n_found = np.zeros(n_q, np.int32)
    qp = queries[rows, :3]
    dist, cand = _tree(pts).query(qp.astype(F64), E)
    with np.errstate(over="ignore", invalid="ignore"):
        t_k, t_e = dist[:, kk - 1] ** 2, dist[:, E - 1] ** 2
        exact = _d2_pairs(np.broadcast_to(qp[:, None, :], (len(rows), E, 3)), pts[cand])
        sure = (t_e > t_k * (1.0 + float(_SLACK))) & (t_e >= _TINY) & (t_e <= _HUGE) & np.isfinite(exact).all(axis=1)
    got_i, got_d = _ordered_rows(exact, orig[cand], kk)
    for r in np.flatnonzero(~sure):
        got_i[r:r + 1], got_d[r:r + 1] = _ordered_rows(d2_rows(qp[r:r + 1], pts), orig[None, :], kk)
    tree_stats["rows"] += len(rows)
    tree_stats["swept"] += int((~sure).sum())
    idx[rows, :kk] = got_i
    d2[rows, :kk] = got_d
    n_found[rows] = kk
    return idx, d2, n_found


def radius_tree(cloud, queries, radius_: float, max_nn: int = 0):
    """radius_brute's answer, bit for bit."""
    if not math.isfinite(radius_) or radius_ < 0 or max_nn < 0:
        raise Refused("radius / max_nn")
    pts, orig, queries, qfin = _split(cloud, queries)
    n_q, m = queries.shape[0], pts.shape[0]
    r2 = F32(float(radius_) * float(radius_))
    qrows = np.flatnonzero(qfin)
    if not (r2 > 0 and m and qrows.size):
        return np.zeros(n_q + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, F32)
    if not _TINY <= float(r2) <= _HUGE:  # (no relative accuracy at the decision itself)
        return radius_brute(cloud, queries, radius_, max_nn)
    qp = queries[qrows, :3]
    balls = _tree(pts).query_ball_point(qp.astype(F64), math.sqrt(float(r2) * (1.0 + float(_SLACK))), return_sorted=False)
    lens = np.fromiter((len(b) for b in balls), np.int64, len(balls))
    rows = np.repeat(np.arange(len(qrows)), lens)
    cols = np.concatenate([np.asarray(b, np.int64) for b in balls]) if lens.sum() else np.zeros(0, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        exact = _d2_pairs(qp[rows], pts[cols])
    unsure = np.zeros(len(qrows), bool)
    unsure[rows[~np.isfinite(exact)]] = True
    ok = (exact < r2) & ~unsure[rows]
    R, Cc, D = [qrows[rows[ok]]], [orig[cols[ok]]], [exact[ok]]
    for r in np.flatnonzero(unsure):
        row = d2_rows(qp[r:r + 1], pts)[0]
        sel = np.flatnonzero(row < r2)
        R.append(np.full(sel.size, qrows[r]))
        Cc.append(orig[sel])
        D.append(row[sel])
    tree_stats["rows"] += len(qrows)
    tree_stats["swept"] += int(unsure.sum())
    R = np.concatenate(R)
    if not R.size:
        return np.zeros(n_q + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, F32)
    return _csr(n_q, R, np.concatenate(Cc), np.concatenate(D), max_nn)


def _form(form, cloud, queries):
    if form not in (None, "brute", "tree"):
        raise ValueError(f"form {form!r}")
    if form is None:
        n = np.asarray(cloud).reshape(-1, 4).shape[0]
        n_q = n if queries is None else np.asarray(queries).reshape(-1, 4).shape[0]
        form = "tree" if n_q * n > TREE_ABOVE else "brute"
    return form


def knn(cloud, queries, k: int, form=None):
    """knn_brute, or above TREE_ABOVE pairs knn_tree: one answer.  form = "brute" / "tree" forces either."""
    return (knn_tree if _form(form, cloud, queries) == "tree" else knn_brute)(cloud, queries, k)


def radius(cloud, queries, radius_: float, max_nn: int = 0, form=None):
    """radius_brute, or above TREE_ABOVE pairs radius_tree: one answer.  form = "brute" / "tree" forces either."""
    return (radius_tree if _form(form, cloud, queries) == "tree" else radius_brute)(cloud, queries, radius_, max_nn)


def knn_literal(cloud, queries, k: int):
    """knn without the narrowing pass: the exact d2 of every pair."""
    pts, orig, queries, qfin = _split(cloud, queries)
    n_q, m = queries.shape[0], pts.shape[0]
    idx = np.full((n_q, k), -1, np.int32)
    d2 = np.full((n_q, k), np.inf, F32)
    n_found = np.zeros(n_q, np.int32)
    kk = min(k, m)
    for i in np.flatnonzero(qfin):
        if kk:
            row = d2_rows(queries[i:i + 1, :3], pts)[0]
            order = np.lexsort((orig, _bits(row)))[:kk]
            idx[i, :kk], d2[i, :kk], n_found[i] = orig[order], row[order], kk
    return idx, d2, n_found


def radius_literal(cloud, queries, radius_: float, max_nn: int = 0):
    pts, orig, queries, qfin = _split(cloud, queries)
    r2 = F32(float(radius_) * float(radius_))
    start, I, D = [0], [], []
    for i in range(queries.shape[0]):
        found = 0
        if qfin[i] and pts.shape[0]:
            row = d2_rows(queries[i:i + 1, :3], pts)[0]
            sel = np.flatnonzero(row < r2)
            order = sel[np.lexsort((orig[sel], _bits(row[sel])))]
            if max_nn > 0:
                order = order[:max_nn]
            I.append(orig[order])
            D.append(row[order])
            found = len(order)
        start.append(start[-1] + found)
    idx = np.concatenate(I).astype(np.int32) if I else np.zeros(0, np.int32)
    d2 = np.concatenate(D).astype(F32) if D else np.zeros(0, F32)
    return np.array(start, np.int64), idx, d2
