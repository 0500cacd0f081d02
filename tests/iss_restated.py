"""An independent NumPy restatement of the ISS keypoints (include/icpgpu.h, "ISS keypoints"):
pcl::ISSKeypoint3D without border estimation over one cloud.  It never calls the library.  Neighbour rows come from
tests/search_restated.py, the Jacobi sweeps from tests/normals_restated.py.

    balls        row i of search_restated.radius(cloud, None, radius, 0), as a set, for the salient and the non-max radius
    scatter      d = P_j - P_i in float32; the six products dx dx, dx dy, dx dz, dy dy, dy dz, dz dz in float64 (exact); each sum
                 is math.fsum of its terms; six zeros when the ball holds fewer than min_neighbors points
    eigenvalues  8 cyclic Jacobi sweeps; the diagonal sorted descending by the network (0,1) (1,2) (0,1), a swap when a < b
    saliency     e3 iff the three are finite, e3 >= 0, n_salient >= min_neighbors, e2 / e1 < gamma_21 and e3 / e2 < gamma_32; else 0
    keypoint     saliency > 0, the non-max ball holds >= min_neighbors points, and no point of it has a larger saliency
(keypoints_literal: the same point by point and neighbour by neighbour, the sums as fractions.Fraction -- for small clouds.)
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import search_restated as S
from normals_restated import jacobi3

F32, F64 = np.float32, np.float64
Refused = S.Refused


def check_arguments(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors):
    for r in (salient_radius, non_max_radius):
        if not (math.isfinite(r) and r > 0):
            raise Refused("radius")
    if not (math.isfinite(gamma_21) and math.isfinite(gamma_32)):
        raise Refused("gamma")
    if min_neighbors < 0:
        raise Refused("min_neighbors")


def sort3(d):
    """(m, 3) -> descending by the rule's network."""
    e = np.array(d, F64).reshape(-1, 3)
    for a, b in ((0, 1), (1, 2), (0, 1)):
        swap = e[:, a] < e[:, b]
        e[swap, a], e[swap, b] = e[swap, b], e[swap, a]
    return e


def select(eig, n_salient, gamma_21: float, gamma_32: float, min_neighbors: int):
    """saliency (m,) from sorted eigenvalues (m, 3) and ball sizes: the selection rule alone."""
    eig = np.asarray(eig, F64).reshape(-1, 3)
    e1, e2, e3 = eig[:, 0], eig[:, 1], eig[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(eig).all(axis=1) & (e3 >= 0.0) & (np.asarray(n_salient) >= min_neighbors)
        ok &= (e2 / e1 < F64(gamma_21)) & (e3 / e2 < F64(gamma_32))
    return np.where(ok, e3, 0.0)


def scatter(cloud, start, idx, min_neighbors: int):
    """(n_salient (n,) int32, scatter6 (n, 6) float64) from the salient rows."""
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    xyz = cloud[:, :3]
    n = cloud.shape[0]
    counts = np.diff(start).astype(np.int32)
    out = np.zeros((n, 6), F64)
    for i in np.flatnonzero(counts >= max(min_neighbors, 1)):
        d = (xyz[idx[start[i]:start[i + 1]]] - xyz[i]).astype(F64)  # the float32 differences, then exact products
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        for e, t in enumerate((dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)):
            out[i, e] = math.fsum(t.tolist())
    return counts, out


def eigenvalues(scatter6, n_salient, min_neighbors: int, finite):
    s = np.asarray(scatter6, F64).reshape(-1, 6)
    a = np.empty((s.shape[0], 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2], a[:, 1, 1], a[:, 1, 2], a[:, 2, 2] = (s[:, e] for e in range(6))
    a[:, 1, 0], a[:, 2, 0], a[:, 2, 1] = a[:, 0, 1], a[:, 0, 2], a[:, 1, 2]
    d, _ = jacobi3(a)
    eig = sort3(d[:, [0, 1, 2], [0, 1, 2]])
    eig[~(np.asarray(finite) & (np.asarray(n_salient) >= min_neighbors))] = 0.0   # a skipped point
    return eig


def suppress(saliency, start, idx, min_neighbors: int):
    """The keypoint flags from the non-max rows."""
    n = saliency.shape[0]
    flags = np.zeros(n, bool)
    for i in np.flatnonzero(saliency > 0.0):
        row = idx[start[i]:start[i + 1]]
        flags[i] = row.size >= min_neighbors and not (saliency[row] > saliency[i]).any()
    return flags


def keypoints(cloud, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975, min_neighbors: int = 5):
    """dict(n_keypoints, keypoint_index int32, keypoints (m, 4) float32, n_salient int32, scatter6, eigenvalues3, saliency)."""
    check_arguments(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
    cloud = np.ascontiguousarray(cloud, F32).reshape(-1, 4)
    finite = S.finite_mask(cloud)
    start, idx, _ = S.radius(cloud, None, salient_radius, 0)
    n_salient, scatter6 = scatter(cloud, start, idx, min_neighbors)
    eig = eigenvalues(scatter6, n_salient, min_neighbors, finite)
    saliency = select(eig, n_salient, gamma_21, gamma_32, min_neighbors)
    saliency[~finite] = 0.0
    start2, idx2, _ = S.radius(cloud, None, non_max_radius, 0)
    index = np.flatnonzero(suppress(saliency, start2, idx2, min_neighbors)).astype(np.int32)
    return {"n_keypoints": int(index.size), "keypoint_index": index, "keypoints": cloud[index].copy(), "n_salient": n_salient,
            "scatter6": scatter6, "eigenvalues3": eig, "saliency": saliency}


def _round_fraction(fr: Fraction) -> float:
    return fr.numerator / fr.denominator   # int / int is correctly rounded


def keypoints_literal(cloud, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                      min_neighbors: int = 5):
    """The rule point by point: every pair's d2, every term a Fraction, every comparison a scalar one."""
    check_arguments(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
    cloud = np.ascontiguousarray(cloud, F32).reshape(-1, 4)
    n = cloud.shape[0]
    finite = S.finite_mask(cloud)
    r2s, r2n = F32(float(salient_radius) * float(salient_radius)), F32(float(non_max_radius) * float(non_max_radius))
    pts, orig = cloud[finite, :3], np.flatnonzero(finite)
    n_salient = np.zeros(n, np.int32)
    scatter6, eig, saliency = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n)
    balls = [np.zeros(0, np.int64)] * n
    for i in orig:
        row = S.d2_rows(cloud[i:i + 1, :3], pts)[0]
        ball = orig[row < r2s]
        balls[i] = orig[row < r2n]
        n_salient[i] = ball.size
        if ball.size < min_neighbors:
            continue
        sums = [Fraction(0)] * 6
        for j in ball:
            dx, dy, dz = (Fraction(float(F32(cloud[j, a] - cloud[i, a]))) for a in range(3))
            for e, t in enumerate((dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)):
                sums[e] += t
        scatter6[i] = [_round_fraction(s) for s in sums]
        s = scatter6[i]
        d, _ = jacobi3(np.array([[[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]]]))
        e = [float(d[0, k, k]) for k in range(3)]
        for a, b in ((0, 1), (1, 2), (0, 1)):
            if e[a] < e[b]:
                e[a], e[b] = e[b], e[a]
        eig[i] = e
        with np.errstate(all="ignore"):
            q21, q32 = F64(e[1]) / F64(e[0]), F64(e[2]) / F64(e[1])
        if all(math.isfinite(x) for x in e) and e[2] >= 0.0 and q21 < gamma_21 and q32 < gamma_32:
            saliency[i] = e[2]
    index = []
    for i in range(n):
        if not saliency[i] > 0.0 or balls[i].size < min_neighbors:
            continue
        if not any(saliency[j] > saliency[i] for j in balls[i]):
            index.append(i)
    index = np.array(index, np.int32)
    return {"n_keypoints": int(index.size), "keypoint_index": index, "keypoints": cloud[index].copy(), "n_salient": n_salient,
            "scatter6": scatter6, "eigenvalues3": eig, "saliency": saliency}


FIELDS = ("keypoint_index", "keypoints", "n_salient", "scatter6", "eigenvalues3", "saliency")


def same_bits(a: dict, b: dict) -> list:
    """The names of the fields whose bits differ (NaN payloads and signed zeros included)."""
    bad = [] if a["n_keypoints"] == b["n_keypoints"] else ["n_keypoints"]
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(f)
    return bad
