"""An independent NumPy restatement of the segment moments (include/icpgpu.h, "segment moments"): per-segment counts, sums, centroid,
covariance, principal axes, axis-aligned and oriented boxes over CSR segments of a cloud.  It never calls the library.

    points      a listed point with a non-finite x, y or z is skipped; count = the finite listed entries; K = the first of them in
                list order, first = its cloud index; none: status EMPTY, everything else zero
    sums        d = q - K in float32; the nine sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz over float64 terms (exact
                products), each the exact sum rounded once: math.fsum here, fractions.Fraction in the literal loop
    finish      float64, every operation rounded: mean = S / m, cov_ab = S_ab / m - m_a m_b, centroid = K + mean; normals_restated's
                Jacobi; columns (0, 1), (1, 2), (0, 1) change places iff the later eigenvalue is strictly larger; the major and the
                middle axis negated when their component of largest magnitude (lowest index among equals) is negative; minor = major x
                middle
    boxes       aabb: min / max of the float32 coordinates, -0 below +0.  obb: u_a = (dx e_ax + dy e_ay) + dz e_az in float64, lo / hi
                its min / max (-0 below +0), dims = hi - lo, position = K + ((c_0 e_0 + c_1 e_1) + c_2 e_2), c = (hi + lo) / 2

records(): vectorised inside a segment, the Jacobi over all segments at once.  records_literal(): a per-segment, per-point loop of
Python floats with Fraction sums and a scalar Jacobi of its own.  tests/test_segment_host.py holds the two to each other bit for bit.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import normals_restated as N

F32, F64 = np.float32, np.float64
OK, EMPTY = 0, 1
CHUNK = 64  # ICPGPU_SEGMENT_CHUNK: where the device cuts the list (no part of the answer inside the header's RANGE)
RECORD = np.dtype([("count", np.int64), ("status", np.int32), ("first", np.int32), ("K", F64, 3), ("moments", F64, 9), ("centroid", F64, 3),
                   ("cov", F64, 6), ("eigenvalues", F64, 3), ("axes", F64, 9), ("aabb_min", F32, 3), ("aabb_max", F32, 3), ("obb_lo", F64, 3),
                   ("obb_hi", F64, 3), ("obb_position", F64, 3), ("obb_dims", F64, 3)], align=True)
FIELDS = RECORD.names


def same_records(got, want) -> list:
    """The (field, segment) pairs whose bits differ, a NaN matching any NaN (a computed NaN's sign and payload are the processor's)."""
    bad = []
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    for f in FIELDS if len(got) else ():
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if g.dtype.kind == "f":
            u = np.uint32 if g.itemsize == 4 else np.uint64
            same = (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))
        else:
            same = g == w
        rows = np.flatnonzero(~same.reshape(len(g), -1).all(axis=1))
        bad += [(f, int(r)) for r in rows[:4]]
    return bad


def ordered_extremes(values):
    """(min, max) of a 1-D float array with -0 ordered below +0: on the sign-flipped integer keys."""
    values = np.ascontiguousarray(values)
    u = np.uint32 if values.itemsize == 4 else np.uint64
    bits = values.view(u)
    top = u(1) << u(8 * values.itemsize - 1)
    keys = np.where(bits & top, ~bits, bits ^ top)
    return values[int(np.argmin(keys))], values[int(np.argmax(keys))]


def listed(cloud, start, indices, r):
    """(the finite listed points of segment r as (m, 3) float32 in list order, their cloud indices)."""
    idx = np.asarray(indices, np.int64)[int(start[r]):int(start[r + 1])]
    pts = np.asarray(cloud, F32)[idx, :3]
    fin = np.isfinite(pts).all(axis=1)
    return pts[fin], idx[fin]


def records(cloud, start, indices) -> np.ndarray:
    cloud, start = np.asarray(cloud, F32), np.asarray(start, np.int64)
    n_seg = len(start) - 1
    out = np.zeros(n_seg, RECORD)
    live = []
    for r in range(n_seg):
        pts, idx = listed(cloud, start, indices, r)
        if len(pts) == 0:
            out[r]["status"] = EMPTY
            continue
        live.append(r)
        K = pts[0]
        d = (pts - K).astype(F64)                                   # (the float32 difference, widened)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        terms = (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz, dx, dy, dz)   # (24 x 24 bits: exact in float64)
        out[r]["count"], out[r]["first"], out[r]["K"] = len(pts), idx[0], K.astype(F64)
        out[r]["moments"] = [math.fsum(t.tolist()) for t in terms]
        for a in range(3):
            out[r]["aabb_min"][a], out[r]["aabb_max"][a] = ordered_extremes(pts[:, a])
    if not live:
        return out
    live = np.asarray(live)
    with np.errstate(all="ignore"):
        m = out["count"][live].astype(F64)
        S = out["moments"][live]
        mean = S[:, 6:9] / m[:, None]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        cov = np.stack([S[:, e] / m - mean[:, a] * mean[:, b] for e, (a, b) in enumerate(pairs)], axis=1)
        mat = np.empty((len(live), 3, 3))
        for e, (a, b) in enumerate(pairs):
            mat[:, a, b] = mat[:, b, a] = cov[:, e]
        diag, v = N.jacobi3(mat)
        lam = diag[:, [0, 1, 2], [0, 1, 2]].copy()
        for i, j in ((0, 1), (1, 2), (0, 1)):
            swap = lam[:, j] > lam[:, i]
            lam[swap, i], lam[swap, j] = lam[swap, j], lam[swap, i]
            v[swap, :, i], v[swap, :, j] = v[swap, :, j].copy(), v[swap, :, i].copy()
        axes = np.empty((len(live), 3, 3))
        for w in range(2):
            e = v[:, :, w].copy()
            big = e[:, 0].copy()
            for k in (1, 2):
                take = np.abs(e[:, k]) > np.abs(big)
                big[take] = e[take, k]
            e[big < 0.0] = -e[big < 0.0]
            axes[:, w] = e
        a, b = axes[:, 0], axes[:, 1]
        axes[:, 2, 0] = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        axes[:, 2, 1] = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        axes[:, 2, 2] = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        out["centroid"][live] = out["K"][live] + mean
        out["cov"][live], out["eigenvalues"][live], out["axes"][live] = cov, lam, axes.reshape(-1, 9)
        for at, r in enumerate(live):
            pts, _ = listed(cloud, start, indices, r)
            d = (pts - pts[0]).astype(F64)
            lo, hi = np.empty(3), np.empty(3)
            for w in range(3):
                e = axes[at, w]
                u = (d[:, 0] * e[0] + d[:, 1] * e[1]) + d[:, 2] * e[2]
                lo[w], hi[w] = ordered_extremes(u)
            c = (hi + lo) / 2.0
            out[r]["obb_lo"], out[r]["obb_hi"], out[r]["obb_dims"] = lo, hi, hi - lo
            out[r]["obb_position"] = out[r]["K"] + ((c[0] * axes[at, 0] + c[1] * axes[at, 1]) + c[2] * axes[at, 2])
    return out


# ---- the literal loop ---------------------------------------------------------------------------------------------------------
def _below(a: float, b: float) -> bool:
    """a orders below b, -0 below +0."""
    return a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))


def _jacobi3_scalar(a):
    """icp_jacobi3.h, line for line, on a list-of-lists symmetric 3 x 3 of Python floats: (a after 8 sweeps, v)."""
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _sweep in range(N.JACOBI_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = _div(a[q][q] - a[p][p], 2.0 * apq)
            t = _div(1.0 if theta >= 0.0 else -1.0, abs(theta) + _sqrt(theta * theta + 1.0))
            c = _div(1.0, _sqrt(t * t + 1.0))
            s = t * c
            r = 3 - p - q
            arp, arq = a[r][p], a[r][q]
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = 0.0
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = c * vkp - s * vkq
                v[k][q] = s * vkp + c * vkq
    return a, v


def _div(a: float, b: float) -> float:
    return float(F64(a) / F64(b))     # (IEEE division: inf and NaN instead of Python's ZeroDivisionError)


def _sqrt(a: float) -> float:
    return float(np.sqrt(F64(a)))


def _exact(terms) -> float:
    """The exact sum of float64 terms rounded once: through Fractions (Fraction -> float rounds to nearest even)."""
    return float(sum((Fraction(t) for t in terms), Fraction(0)))


def records_literal(cloud, start, indices) -> np.ndarray:
    cloud = np.asarray(cloud, F32)
    n_seg = len(start) - 1
    out = np.zeros(n_seg, RECORD)
    with np.errstate(all="ignore"):
        for r in range(n_seg):
            K, first, m = None, -1, 0
            terms = [[] for _ in range(9)]
            lo3, hi3 = [None] * 3, [None] * 3
            kept = []
            for e in range(int(start[r]), int(start[r + 1])):
                q = cloud[int(indices[e]), :3]
                if not (math.isfinite(q[0]) and math.isfinite(q[1]) and math.isfinite(q[2])):
                    continue
                if K is None:
                    K, first = q.copy(), int(indices[e])
                m += 1
                d = [float(F32(q[a]) - F32(K[a])) for a in range(3)]
                kept.append(d)
                for slot, t in enumerate((d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2], d[0], d[1], d[2])):
                    terms[slot].append(t)
                for a in range(3):
                    x = float(q[a])
                    if lo3[a] is None or _below(x, lo3[a]):
                        lo3[a] = x
                    if hi3[a] is None or _below(hi3[a], x):
                        hi3[a] = x
            rec = out[r]
            if K is None:
                rec["status"] = EMPTY
                continue
            S = [_exact(t) for t in terms]
            fm = float(m)
            mean = [_div(S[6 + a], fm) for a in range(3)]
            pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
            cov = [_div(S[e], fm) - mean[a] * mean[b] for e, (a, b) in enumerate(pairs)]
            mat = [[0.0] * 3 for _ in range(3)]
            for e, (a, b) in enumerate(pairs):
                mat[a][b] = mat[b][a] = cov[e]
            mat, v = _jacobi3_scalar(mat)
            lam = [mat[0][0], mat[1][1], mat[2][2]]
            for i, j in ((0, 1), (1, 2), (0, 1)):
                if lam[j] > lam[i]:
                    lam[i], lam[j] = lam[j], lam[i]
                    for k in range(3):
                        v[k][i], v[k][j] = v[k][j], v[k][i]
            axes = []
            for w in range(2):
                e = [v[k][w] for k in range(3)]
                big = e[0]
                for k in (1, 2):
                    if abs(e[k]) > abs(big):
                        big = e[k]
                if big < 0.0:
                    e = [-x for x in e]
                axes.append(e)
            a, b = axes
            axes.append([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
            lo, hi = [None] * 3, [None] * 3
            for d in kept:
                for w in range(3):
                    u = (d[0] * axes[w][0] + d[1] * axes[w][1]) + d[2] * axes[w][2]
                    if lo[w] is None or _below(u, lo[w]):
                        lo[w] = u
                    if hi[w] is None or _below(hi[w], u):
                        hi[w] = u
            c = [(hi[w] + lo[w]) / 2.0 for w in range(3)]
            rec["count"], rec["status"], rec["first"] = m, OK, first
            rec["K"] = [float(K[a]) for a in range(3)]
            rec["moments"], rec["cov"], rec["eigenvalues"] = S, cov, lam
            rec["centroid"] = [float(K[a]) + mean[a] for a in range(3)]
            rec["axes"] = axes[0] + axes[1] + axes[2]
            rec["aabb_min"], rec["aabb_max"] = lo3, hi3
            rec["obb_lo"], rec["obb_hi"] = lo, hi
            rec["obb_dims"] = [hi[w] - lo[w] for w in range(3)]
            rec["obb_position"] = [float(K[k]) + ((c[0] * axes[0][k] + c[1] * axes[1][k]) + c[2] * axes[2][k]) for k in range(3)]
    return out


def csr(segments) -> tuple:
    """(segment_start int64, indices int32) of a list of index lists."""
    start = np.zeros(len(segments) + 1, np.int64)
    np.cumsum([len(s) for s in segments], out=start[1:])
    flat = np.concatenate([np.asarray(s, np.int32).reshape(-1) for s in segments]) if segments else np.empty(0, np.int32)
    return start, flat.astype(np.int32)


def validate(n: int, source: int, n_segments: int, segment_start, indices, have_clusters=None, have_regions=None, sizeof_record=RECORD.itemsize,
             null_out=False, search_set=True) -> bool:
    """True where the header says the call is refused with ICPGPU_ERR_INVALID_ARG.  have_clusters / have_regions: the count of the
    context's clustering / region growing result over this search cloud, or None."""
    if not search_set or sizeof_record != RECORD.itemsize or (n_segments > 0 and null_out):
        return True
    if source == 0:
        if segment_start is None:
            return True
        s = [int(x) for x in segment_start]
        if s[0] != 0 or any(b < a for a, b in zip(s, s[1:n_segments + 1])):
            return True
        total = s[n_segments]
        if total and indices is None:
            return True
        return any(not 0 <= int(i) < n for i in list(indices)[:total]) if total else False
    if source in (1, 2):
        have = have_clusters if source == 1 else have_regions
        return have is None or segment_start is not None or indices is not None or have != n_segments
    return True
