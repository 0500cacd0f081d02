"""The plane segmentation's rules (include/icpgpu.h, "plane segmentation") restated in NumPy / Python, operation for operation:

    samples   splitmix64 of the counter 3 t + c + 1 in uint64 arithmetic; sample[c] = ((z >> 32) * n) >> 32
    model     float32, every operation rounded on its own: the cross product of p1 - p0 and p2 - p0, its length by sqrtf, a division per
              component, d = -((n.x p0.x + n.y p0.y) + n.z p0.z); INVALID: equal indices, a non-finite point, a squared norm that is 0 or
              not finite, and with an axis |a . n| < cos(eps_angle) in double
    inlier    s = fmaf(n.z, q.z, fmaf(n.y, q.y, n.x * q.x)) + d with the fused operations emulated exactly (symmetric_restated.fma_f32);
              a finite q is an inlier iff (double)|s| < distance_threshold
    loop      the sequential RANSAC loop with k = log(1 - probability) / log(1 - w^3), math.log being the host's libm
    refine    the nine sums by math.fsum (exact, rounded once), means and covariances in double, normals_restated.jacobi3, the sign
              by the unrefined normal, d in double, and the selection again

segment() is the vectorised form the device is compared with; segment_literal() beside it is a per-hypothesis, per-point Python loop
with Python integers for the generator -- tests/test_sac_host.py holds the two against each other."""
from __future__ import annotations

import math
import sys

import numpy as np

import normals_restated as NR
from symmetric_restated import fma_f32

F32, F64 = np.float32, np.float64
MASK = (1 << 64) - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MAX_ITERATIONS = 1 << 20
DBL_EPSILON = sys.float_info.epsilon


class Refused(Exception):
    """What the library answers with ICPGPU_ERR_INVALID_ARG."""


# ---- the generator ---------------------------------------------------------------------------------------------------------
def sample_int(seed: int, t: int, c: int, n: int) -> int:
    """sample[c] of hypothesis t in Python integers."""
    z = (seed + (3 * t + c + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * MIX1) & MASK
    z = ((z ^ (z >> 27)) * MIX2) & MASK
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def samples(seed: int, t0: int, m: int, n: int) -> np.ndarray:
    """(m, 3) int64: the samples of hypotheses t0 .. t0 + m - 1, in uint64 arithmetic (NumPy's wraps modulo 2^64)."""
    with np.errstate(over="ignore"):
        t = np.arange(t0, t0 + m, dtype=np.uint64)[:, None]
        c = np.arange(3, dtype=np.uint64)[None, :]
        z = np.uint64(seed & MASK) + (np.uint64(3) * t + c + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


# ---- arguments -------------------------------------------------------------------------------------------------------------
def unit_axis(axis):
    """The axis normalised in double, a / sqrt((x x + y y) + z z); Refused when it is not finite or has zero length."""
    a = [float(v) for v in np.asarray(axis, F64).reshape(3)]
    if not all(math.isfinite(v) for v in a):
        raise Refused("axis not finite")
    with np.errstate(over="ignore"):
        length = float(np.sqrt((F64(a[0]) * F64(a[0]) + F64(a[1]) * F64(a[1])) + F64(a[2]) * F64(a[2])))
    if not length > 0.0:
        raise Refused("axis of zero length")
    return [v / length for v in a]


def check(threshold, max_iterations, probability, axis, eps_angle):
    if not (math.isfinite(threshold) and threshold >= 0.0):
        raise Refused("distance_threshold")
    if not 0 <= max_iterations <= MAX_ITERATIONS:
        raise Refused("max_iterations")
    if not 0.0 < probability < 1.0:
        raise Refused("probability")
    if axis is None:
        return None, 0.0
    a = unit_axis(axis)
    if not (math.isfinite(eps_angle) and eps_angle >= 0.0):
        raise Refused("eps_angle")
    return a, math.cos(eps_angle)


# ---- model, inliers ----------------------------------------------------------------------------------------------------------
def models(cloud, S, axis=None, cos_eps: float = 0.0):
    """(planes (m, 4) float32 -- NaN where INVALID --, valid (m,) bool) of the sample rows S (m, 3)."""
    xyz = np.asarray(cloud, F32).reshape(-1, 4)[:, :3]
    m = S.shape[0]
    planes = np.full((m, 4), np.nan, F32)
    valid = (S[:, 0] != S[:, 1]) & (S[:, 0] != S[:, 2]) & (S[:, 1] != S[:, 2])
    if m == 0:
        return planes, valid
    p0, p1, p2 = xyz[S[:, 0]], xyz[S[:, 1]], xyz[S[:, 2]]
    valid &= np.isfinite(p0).all(axis=1) & np.isfinite(p1).all(axis=1) & np.isfinite(p2).all(axis=1)
    with np.errstate(all="ignore"):
        u, v = p1 - p0, p2 - p0
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        l2 = (cx * cx + cy * cy) + cz * cz
        valid &= (l2 != 0) & np.isfinite(l2)
        l = np.sqrt(l2)
        nx, ny, nz = cx / l, cy / l, cz / l
        d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
        if axis is not None:
            dot = (F64(axis[0]) * nx.astype(F64) + F64(axis[1]) * ny.astype(F64)) + F64(axis[2]) * nz.astype(F64)
            valid &= np.abs(dot) >= cos_eps
    for e, col in enumerate((nx, ny, nz, d)):
        planes[:, e] = np.where(valid, col, F32(np.nan))
    return planes, valid


def inlier_mask(cloud, plane, threshold: float) -> np.ndarray:
    """(n,) bool: the points within the threshold of `plane` (4 float32) under the inlier rule."""
    c = np.asarray(cloud, F32).reshape(-1, 4)
    p = np.asarray(plane, F32)
    with np.errstate(all="ignore"):
        s = fma_f32(p[2], c[:, 2], fma_f32(p[1], c[:, 1], (p[0] * c[:, 0]).astype(F32))) + p[3]
        return np.isfinite(c[:, :3]).all(axis=1) & (np.abs(s.astype(F32)).astype(F64) < threshold)


def next_k(count: int, n: int, probability: float) -> float:
    w = count / float(n)
    p = 1.0 - w * w * w
    p = max(p, DBL_EPSILON)
    p = min(p, 1.0 - DBL_EPSILON)
    return math.log(1.0 - probability) / math.log(p)


# ---- refinement ------------------------------------------------------------------------------------------------------------
def moments_of(cloud, inliers, k_index: int) -> np.ndarray:
    """The nine sums about K = cloud[k_index] over the inliers: float32 differences, exact float64 terms, math.fsum."""
    xyz = np.asarray(cloud, F32).reshape(-1, 4)[:, :3]
    d = (xyz[inliers] - xyz[k_index]).astype(F64)      # (the subtraction in float32, then widened)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    terms = (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz, dx, dy, dz)
    return np.array([math.fsum(t.tolist()) for t in terms], F64)


def refine(moments, K, m: int, unrefined) -> np.ndarray:
    """The refined coefficients (4 float32) from the nine sums, K (3 float32), the inlier count and the unrefined coefficients."""
    S = np.asarray(moments, F64)
    dm = F64(m)
    with np.errstate(all="ignore"):
        mean = S[6:9] / dm
        a = np.zeros((1, 3, 3))
        for e, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            a[0, i, j] = a[0, j, i] = S[e] / dm - mean[i] * mean[j]
        d, V = NR.jacobi3(a)
        col = 0
        for j in (1, 2):
            if d[0, j, j] < d[0, col, col]:
                col = j
        nrm = V[0, :, col].astype(F32)
        u = np.asarray(unrefined, F32)
        if (nrm[0] * u[0] + nrm[1] * u[1]) + nrm[2] * u[2] < 0:
            nrm = -nrm
        c = np.asarray(K, F32).astype(F64) + mean
        n64 = nrm.astype(F64)
        dd = F32(-((n64[0] * c[0] + n64[1] * c[1]) + n64[2] * c[2]))
    return np.array([nrm[0], nrm[1], nrm[2], dd], F32)


# ---- the call --------------------------------------------------------------------------------------------------------------
def _finish(cloud, out, threshold, optimize, inliers_of):
    """The part behind the loop, shared by both forms: out holds counts, iterations, best_t, sample, coeff_unrefined."""
    out["found"] = int(out["best_t"] >= 0)
    out["moments"] = np.zeros(9, F64)
    out["coeff"] = np.zeros(4, F32)
    out["inliers"] = np.zeros(0, np.int32)
    out["n_unrefined"] = 0
    if not out["found"]:
        out["coeff_unrefined"] = np.zeros(4, F32)
        return out
    inliers = inliers_of(out["coeff_unrefined"])
    out["n_unrefined"] = int(inliers.size)
    out["coeff"] = out["coeff_unrefined"].copy()
    if optimize and inliers.size >= 3:
        k_index = int(out["sample"][0])
        out["moments"] = moments_of(cloud, inliers, k_index)
        out["coeff"] = refine(out["moments"], np.asarray(cloud, F32).reshape(-1, 4)[k_index, :3], inliers.size, out["coeff_unrefined"])
        inliers = inliers_of(out["coeff"])
    out["inliers"] = inliers.astype(np.int32)
    return out


def segment(cloud, threshold: float, max_iterations: int = 50, probability: float = 0.99, seed: int = 0, optimize: bool = True,
            axis=None, eps_angle: float = 0.0) -> dict:
    """counts (iterations,) int32, iterations, best_t (-1: none), sample (3,) int32, coeff_unrefined, n_unrefined, moments (9,)
    float64, coeff (4,) float32, inliers int32 ascending, found."""
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    a, cos_eps = check(threshold, max_iterations, probability, axis, eps_angle)
    n = cloud.shape[0]
    counts, k, best, best_count, t = [], math.inf, -1, 0, 0
    sample, plane = np.full(3, -1, np.int32), np.zeros(4, F32)
    chunk_S = chunk_planes = chunk_valid = None
    while n > 0 and t < max_iterations and float(t) < k:
        if t % 64 == 0:                                        # (the models 64 at a time: cheaper in NumPy, nothing else)
            chunk_S = samples(seed, t, min(64, max_iterations - t), n)
            chunk_planes, chunk_valid = models(cloud, chunk_S, a, cos_eps)
        h = t % 64
        count = int(inlier_mask(cloud, chunk_planes[h], threshold).sum()) if chunk_valid[h] else -1
        counts.append(count)
        if count > 0 and count > best_count:
            best, best_count = t, count
            sample, plane = chunk_S[h].astype(np.int32), chunk_planes[h].copy()
            k = next_k(count, n, probability)
        t += 1
    out = {"counts": np.array(counts, np.int32), "iterations": t, "best_t": best, "sample": sample, "coeff_unrefined": plane}
    return _finish(cloud, out, threshold, optimize, lambda p: np.flatnonzero(inlier_mask(cloud, p, threshold)))


def segment_literal(cloud, threshold: float, max_iterations: int = 50, probability: float = 0.99, seed: int = 0, optimize: bool = True,
                    axis=None, eps_angle: float = 0.0) -> dict:
    """The same answer by the rules' letter: one hypothesis and one point at a time, scalars only."""
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    a, cos_eps = check(threshold, max_iterations, probability, axis, eps_angle)
    n = cloud.shape[0]

    def is_inlier(p, q):
        if not (math.isfinite(q[0]) and math.isfinite(q[1]) and math.isfinite(q[2])):
            return False
        with np.errstate(all="ignore"):
            s = F32(fma_f32(p[2], q[2], fma_f32(p[1], q[1], F32(p[0] * q[0])))) + p[3]
            return float(abs(F32(s))) < threshold

    def inliers_of(p):
        return np.array([i for i in range(n) if is_inlier(p, cloud[i])], np.int64)

    def model(t):
        s = [sample_int(seed, t, c, n) for c in range(3)]
        if s[0] == s[1] or s[0] == s[2] or s[1] == s[2]:
            return s, None
        p0, p1, p2 = (cloud[i, :3] for i in s)
        if not all(math.isfinite(float(v)) for p in (p0, p1, p2) for v in p):
            return s, None
        with np.errstate(all="ignore"):
            u = [F32(p1[e] - p0[e]) for e in range(3)]
            v = [F32(p2[e] - p0[e]) for e in range(3)]
            c = [F32(F32(u[1] * v[2]) - F32(u[2] * v[1])), F32(F32(u[2] * v[0]) - F32(u[0] * v[2])), F32(F32(u[0] * v[1]) - F32(u[1] * v[0]))]
            l2 = F32(F32(F32(c[0] * c[0]) + F32(c[1] * c[1])) + F32(c[2] * c[2]))
            if l2 == 0 or not math.isfinite(float(l2)):
                return s, None
            l = F32(np.sqrt(l2))
            nrm = [F32(c[e] / l) for e in range(3)]
            d = F32(-F32(F32(F32(nrm[0] * p0[0]) + F32(nrm[1] * p0[1])) + F32(nrm[2] * p0[2])))
        if a is not None and not abs((a[0] * float(nrm[0]) + a[1] * float(nrm[1])) + a[2] * float(nrm[2])) >= cos_eps:
            return s, None
        return s, np.array([nrm[0], nrm[1], nrm[2], d], F32)

    counts, k, best, best_count, t = [], math.inf, -1, 0, 0
    sample, plane = np.full(3, -1, np.int32), np.zeros(4, F32)
    while n > 0 and t < max_iterations and float(t) < k:
        s, p = model(t)
        count = -1 if p is None else sum(is_inlier(p, cloud[i]) for i in range(n))
        counts.append(count)
        if count > 0 and count > best_count:
            best, best_count, sample, plane = t, count, np.array(s, np.int32), p
            k = next_k(count, n, probability)
        t += 1
    out = {"counts": np.array(counts, np.int32), "iterations": t, "best_t": best, "sample": sample, "coeff_unrefined": plane}
    return _finish(cloud, out, threshold, optimize, inliers_of)


def extract(cloud, inliers, negative: bool) -> np.ndarray:
    """pcl::ExtractIndices: the rows whose index is (negative: is not) among the inliers, in cloud order."""
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    mask = np.zeros(cloud.shape[0], bool)
    mask[np.asarray(inliers, np.int64)] = True
    return cloud[~mask if negative else mask]
