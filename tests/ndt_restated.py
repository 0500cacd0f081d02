"""An independent NumPy restatement of the NDT mode (include/icpgpu.h: ICPGPU_NDT; DESIGN.md, "NDT"): PCL 1.8's
NormalDistributionsTransform over VoxelGridCovariance, rule by rule as DESIGN.md states them.  It never calls the library.

    lattice / cells          the voxel filter's keys at leaf = resolution, per-cell float centroids and double sums in input order,
                             PCL's covariance, the same cyclic Jacobi as the device (so validity decisions agree), the eigenvalue
                             floor, the cofactor inverse and the validity rule
    neighbourhoods           cKDTree over the valid centroids at a slightly inflated radius, then the exact float predicate
    derivatives              PCL's updateDerivatives pair by pair, J and H written out analytically (Magnusson 2009, 6.17-6.21)
    step / align             JacobiSVD's pseudo-inverse by numpy's SVD, PCL 1.8's step rule and Newton loop, eulerAngles(0, 1, 2)
"""
from __future__ import annotations

import math

import numpy as np
from scipy.spatial import cKDTree

F32, F64 = np.float32, np.float64
INT32_MAX = 2**31 - 1
MIN_POINTS = 6
EIG_RATIO = 0.01
JACOBI_SWEEPS = 8
TERMS = 29
NOT_CONVERGED, CONV_ITERATIONS, CONV_TRANSFORM, CONV_NO_CORRESPONDENCES = 0, 1, 2, 5


class Overflow(ValueError):
    """The cell index would overflow int32 at this resolution (the library refuses with ICPGPU_ERR_INVALID_ARG)."""


def gauss_constants(resolution: float, outlier_ratio: float):
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / (resolution * resolution * resolution)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


# ---- float32 arithmetic the device uses ------------------------------------------------------------------------------
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


def transform_f32(T, xyz):
    """xform_point (icp_device.h): p_r = fma(T[r,2], z, fma(T[r,1], y, fma(T[r,0], x, T[r,3]))) in float32."""
    T = np.asarray(T, F32)
    x, y, z = (np.asarray(xyz[:, k], F32) for k in range(3))
    out = np.empty((xyz.shape[0], 3), F32)
    for r in range(3):
        out[:, r] = fma32(T[r, 2], z, fma32(T[r, 1], y, fma32(T[r, 0], x, T[r, 3])))
    return out


def _angle_axis_f(angle, axis):
    a = F32(angle)
    s, c = F32(math.sin(float(a))), F32(math.cos(float(a)))
    ax = [F32(1.0) if k == axis else F32(0.0) for k in range(3)]
    sa = [s * ax[k] for k in range(3)]
    ca = [(F32(1.0) - c) * ax[k] for k in range(3)]
    R = np.zeros((3, 3), F32)
    for i in range(3):
        R[i, i] = ca[i] * ax[i] + c
    R[0, 1] = ca[0] * ax[1] - sa[2]
    R[1, 0] = ca[0] * ax[1] + sa[2]
    R[0, 2] = ca[0] * ax[2] + sa[1]
    R[2, 0] = ca[0] * ax[2] - sa[1]
    R[1, 2] = ca[1] * ax[2] - sa[0]
    R[2, 1] = ca[1] * ax[2] + sa[0]
    return R


def _mul3f(A, B):
    C = np.zeros((3, 3), F32)
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return C


def transform_float(p):
    """Translation3f(p0..2) * AngleAxisf(p3, X) * AngleAxisf(p4, Y) * AngleAxisf(p5, Z), a 4x4 float32."""
    R = _mul3f(_mul3f(_angle_axis_f(p[3], 0), _angle_axis_f(p[4], 1)), _angle_axis_f(p[5], 2))
    T = np.eye(4, dtype=F32)
    T[:3, :3] = R
    T[:3, 3] = [F32(p[0]), F32(p[1]), F32(p[2])]
    return T


def transform_double(p):
    """T(p) = Translation * Rx * Ry * Rz in exact double arithmetic (for finite differences)."""
    cx, sx, cy, sy, cz, sz = math.cos(p[3]), math.sin(p[3]), math.cos(p[4]), math.sin(p[4]), math.cos(p[5]), math.sin(p[5])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = p[:3]
    return T


def euler_angles(R):
    """Eigen's MatrixBase::eulerAngles(0, 1, 2) of a 3x3 (double): ranges [0, pi] x [-pi, pi] x [-pi, pi]."""
    m = np.asarray(R, F64)
    r0 = math.atan2(m[1, 2], m[2, 2])
    c2 = math.hypot(m[0, 0], m[0, 1])
    if r0 > 0.0:
        r0 = r0 - math.pi
        r1 = math.atan2(-m[0, 2], -c2)
    else:
        r1 = math.atan2(-m[0, 2], c2)
    s1, c1 = math.sin(r0), math.cos(r0)
    r2 = math.atan2(s1 * m[2, 0] - c1 * m[1, 0], c1 * m[1, 1] - s1 * m[2, 1])
    return np.array([-r0, -r1, -r2])


def initial_pose(guess):
    """p0 of computeTransformation: the guess's translation and eulerAngles(0, 1, 2), both as float (Vector3f)."""
    if guess is None:
        return np.zeros(6)
    g = np.asarray(guess, F32)
    ang = euler_angles(g[:3, :3].astype(F64))
    return np.concatenate([g[:3, 3].astype(F64), ang.astype(F32).astype(F64)])


# ---- cells -------------------------------------------------------------------------------------------------------------
def lattice(pts, resolution):
    """The voxel filter's min_b / div_b at leaf = resolution (float arithmetic), or None when no point is finite."""
    xyz = np.asarray(pts, F32)[:, :3]
    fin = np.isfinite(xyz).all(axis=1)
    if not fin.any():
        return None
    leaf = F32(resolution)
    inv = F32(1.0) / leaf
    lo, hi = xyz[fin].min(axis=0), xyz[fin].max(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = [F32(F32(hi[a] - lo[a]) * inv) for a in range(3)] + [F32(lo[a] * inv) for a in range(3)] + [F32(hi[a] * inv) for a in range(3)]
    if not all(np.isfinite(v) for v in scaled):      # an extent or a bound beyond float: beyond every integer index too
        raise Overflow(resolution)
    d = [int(F32((hi[a] - lo[a]) * inv)) + 1 for a in range(3)]
    minb = [int(np.floor(F32(lo[a] * inv))) for a in range(3)]
    divb = [int(np.floor(F32(hi[a] * inv))) - minb[a] + 1 for a in range(3)]
    if d[0] * d[1] * d[2] > INT32_MAX or divb[0] * divb[1] * divb[2] > INT32_MAX:
        raise Overflow(resolution)
    return dict(inv=inv, minb=minb, divb=divb, mul_y=divb[0], mul_z=divb[0] * divb[1])


def _jacobi3(a):
    """The device's cyclic Jacobi (icp_ndt.hip: jacobi3), vectorised over cells: a (m, 3, 3) -> eigenvalues (diagonal), V."""
    a = a.copy()
    m = a.shape[0]
    v = np.broadcast_to(np.eye(3), (m, 3, 3)).copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(JACOBI_SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = a[:, p, q].copy()
                nz = apq != 0.0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                app = a[:, p, p] - t * apq
                aqq = a[:, q, q] + t * apq
                nrp = c * arp - s * arq
                nrq = s * arp + c * arq
                a[:, p, p] = np.where(nz, app, a[:, p, p])
                a[:, q, q] = np.where(nz, aqq, a[:, q, q])
                for (i, j) in ((p, q), (q, p)):
                    a[:, i, j] = np.where(nz, 0.0, a[:, i, j])
                for (i, j) in ((r, p), (p, r)):
                    a[:, i, j] = np.where(nz, nrp, a[:, i, j])
                for (i, j) in ((r, q), (q, r)):
                    a[:, i, j] = np.where(nz, nrq, a[:, i, j])
                for k in range(3):
                    vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
                    v[:, k, p] = np.where(nz, c * vkp - s * vkq, vkp)
                    v[:, k, q] = np.where(nz, s * vkp + c * vkq, vkq)
    return a, v


def cells(pts, resolution):
    """Every occupied cell of the target at `resolution`, ascending key: key, n, centroid (float32 xyz), mean, raw cov (the ones
    with n >= 6; NaN otherwise), icov, valid.  `lattice` is the lattice (None: no finite point)."""
    pts = np.asarray(pts, F32)
    L = lattice(pts, resolution)
    empty = dict(lattice=L, key=np.zeros(0, np.int64), n=np.zeros(0, np.int64), centroid=np.zeros((0, 3), F32),
                 mean=np.zeros((0, 3)), cov=np.zeros((0, 3, 3)), icov=np.zeros((0, 3, 3)), valid=np.zeros(0, bool))
    if L is None:
        return empty
    xyz = pts[:, :3]
    fin = np.isfinite(xyz).all(axis=1)
    inv = L["inv"]
    with np.errstate(invalid="ignore"):
        ijk = np.floor(xyz * inv).astype(F64)
    key = np.full(len(xyz), -1, np.int64)
    k3 = ijk[fin].astype(np.int64) - np.array(L["minb"], np.int64)
    key[fin] = k3[:, 0] + k3[:, 1] * L["mul_y"] + k3[:, 2] * L["mul_z"]
    idx = np.nonzero(fin)[0]
    order = idx[np.argsort(key[idx], kind="stable")]
    ks = key[order]
    if len(ks) == 0:
        return empty
    starts = np.concatenate([[0], np.nonzero(np.diff(ks))[0] + 1])
    counts = np.diff(np.concatenate([starts, [len(ks)]]))
    m = len(starts)
    fsum = np.zeros((m, 3), F32)
    S = np.zeros((m, 3))
    Q = np.zeros((m, 6))
    for r in range(int(counts.max())):
        sel = counts > r
        p = xyz[order[starts[sel] + r]]
        fsum[sel] = fsum[sel] + p
        pd = p.astype(F64)
        S[sel] = S[sel] + pd
        Q[sel] = Q[sel] + np.stack([pd[:, 0] * pd[:, 0], pd[:, 0] * pd[:, 1], pd[:, 0] * pd[:, 2], pd[:, 1] * pd[:, 1],
                                    pd[:, 1] * pd[:, 2], pd[:, 2] * pd[:, 2]], axis=1)
    cent = (fsum / counts.astype(F32)[:, None]).astype(F32)
    nd = counts.astype(F64)
    mean = S / nd[:, None]
    f = (nd - 1.0) / nd
    cov = np.full((m, 3, 3), np.nan)
    for e, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        v = ((Q[:, e] - 2.0 * (S[:, c] * mean[:, r])) / nd + mean[:, c] * mean[:, r]) * f
        cov[:, r, c] = v
        cov[:, c, r] = v
    big = counts >= MIN_POINTS
    icov = np.full((m, 3, 3), np.nan)
    valid = np.zeros(m, bool)
    if big.any():
        a, V = _jacobi3(cov[big])
        lam = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1)
        ordr = np.argsort(lam, axis=1, kind="stable")
        ls = np.take_along_axis(lam, ordr, axis=1)
        ok = ~((ls[:, 0] < 0.0) | (ls[:, 1] < 0.0) | (ls[:, 2] <= 0.0))
        fl = EIG_RATIO * ls[:, 2]
        infl = ok & (ls[:, 0] < fl)
        ls2 = ls.copy()
        ls2[:, 0] = np.where(infl, fl, ls[:, 0])
        ls2[:, 1] = np.where(infl & (ls[:, 1] < fl), fl, ls[:, 1])
        Vs = np.take_along_axis(V, ordr[:, None, :], axis=2)   # eigenvector columns in ascending order
        C = cov[big].copy()
        rebuilt = np.zeros_like(C)
        for r in range(3):
            for c in range(3):
                s = np.zeros(len(C))
                for e in range(3):
                    s = s + Vs[:, r, e] * ls2[:, e] * Vs[:, c, e]
                rebuilt[:, r, c] = s
        C = np.where(infl[:, None, None], rebuilt, C)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            c00 = C[:, 1, 1] * C[:, 2, 2] - C[:, 1, 2] * C[:, 2, 1]
            c01 = C[:, 1, 2] * C[:, 2, 0] - C[:, 1, 0] * C[:, 2, 2]
            c02 = C[:, 1, 0] * C[:, 2, 1] - C[:, 1, 1] * C[:, 2, 0]
            det = C[:, 0, 0] * c00 + C[:, 0, 1] * c01 + C[:, 0, 2] * c02
            ic = np.stack([c00 / det, (C[:, 0, 2] * C[:, 2, 1] - C[:, 0, 1] * C[:, 2, 2]) / det,
                           (C[:, 0, 1] * C[:, 1, 2] - C[:, 0, 2] * C[:, 1, 1]) / det,
                           (C[:, 0, 0] * C[:, 2, 2] - C[:, 0, 2] * C[:, 2, 0]) / det,
                           (C[:, 0, 2] * C[:, 1, 0] - C[:, 0, 0] * C[:, 1, 2]) / det,
                           (C[:, 0, 0] * C[:, 1, 1] - C[:, 0, 1] * C[:, 1, 0]) / det], axis=1)
        ok = ok & np.isfinite(ic).all(axis=1)
        icov[big] = ic[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
        valid[big] = ok
    return dict(lattice=L, key=ks[starts], n=counts, centroid=cent, mean=mean, cov=cov, icov=icov, valid=valid)


def valid_cells(C):
    v = C["valid"]
    return dict(key=C["key"][v], n=C["n"][v], centroid=C["centroid"][v], mean=C["mean"][v], icov=C["icov"][v])


# ---- neighbourhoods and derivatives ---------------------------------------------------------------------------------------
class Target:
    """The valid cells of a target and a kd-tree over their float centroids."""

    def __init__(self, pts, resolution: float, outlier_ratio: float = 0.55):
        self.resolution = float(resolution)
        self.all = cells(pts, resolution)
        self.v = valid_cells(self.all)
        self.tree = cKDTree(self.v["centroid"].astype(F64)) if len(self.v["key"]) else None
        self.d1, self.d2 = gauss_constants(self.resolution, outlier_ratio)

    def pairs(self, q):
        """(point, cell) index pairs: every valid cell whose centroid has float (dx^2 + dy^2) + dz^2 <= float(r^2) from q (float32)."""
        if self.tree is None or len(q) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        fin = np.isfinite(q).all(axis=1)
        qi = np.nonzero(fin)[0]
        lists = self.tree.query_ball_point(q[qi].astype(F64), self.resolution * (1 + 1e-5))
        pi = np.repeat(qi, [len(x) for x in lists])
        ci = np.concatenate([np.asarray(x, np.int64) for x in lists]) if len(pi) else np.zeros(0, np.int64)
        c = self.v["centroid"][ci]
        d = q[pi] - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 <= F32(self.resolution * self.resolution)
        pi, ci = pi[keep], ci[keep]
        o = np.lexsort((ci, pi))
        return pi[o], ci[o]


def angle_terms(p, small_angle_rule: bool = True):
    """PCL's j_ang_a .. h (8 x 3) and h_ang_a2 .. f3 (15 x 3) at the angles of p."""
    cs = []
    for a in p[3:6]:
        if small_angle_rule and abs(a) < 10e-5:
            cs.append((1.0, 0.0))
        else:
            cs.append((math.cos(a), math.sin(a)))
    (cx, sx), (cy, sy), (cz, sz) = cs
    j = np.array([[-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy],
                  [cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy],
                  [-sy * cz, sy * sz, cy],
                  [sx * cy * cz, -sx * cy * sz, sx * sy],
                  [-cx * cy * cz, cx * cy * sz, -cx * sy],
                  [-cy * sz, -cy * cz, 0.0],
                  [cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0.0],
                  [sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0.0]])
    h = np.array([[-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, sx * cy],
                  [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, -cx * cy],
                  [cx * cy * cz, -cx * cy * sz, cx * sy],
                  [sx * cy * cz, -sx * cy * sz, sx * sy],
                  [-sx * cz - cx * sy * sz, sx * sz - cx * sy * cz, 0.0],
                  [cx * cz - sx * sy * sz, -sx * sy * cz - cx * sz, 0.0],
                  [-cy * cz, cy * sz, -sy],
                  [-sx * sy * cz, sx * sy * sz, sx * cy],
                  [cx * sy * cz, -cx * sy * sz, -cx * cy],
                  [sy * sz, sy * cz, 0.0],
                  [-sx * cy * sz, -sx * cy * cz, 0.0],
                  [cx * cy * sz, cx * cy * cz, 0.0],
                  [-cy * cz, cy * sz, 0.0],
                  [-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, 0.0],
                  [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, 0.0]])
    return j, h


def point_derivatives(x, j, h):
    """computePointDerivatives for points x (m, 3) double: J (m, 6, 3) with J[:, k] = d(T x)/dp_k, and H (m, 6, 6, 3)."""
    m = x.shape[0]
    J = np.zeros((m, 6, 3))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    xd = lambda v: x @ v  # noqa: E731
    J[:, 3, 1], J[:, 3, 2] = xd(j[0]), xd(j[1])
    J[:, 4, 0], J[:, 4, 1], J[:, 4, 2] = xd(j[2]), xd(j[3]), xd(j[4])
    J[:, 5, 0], J[:, 5, 1], J[:, 5, 2] = xd(j[5]), xd(j[6]), xd(j[7])
    a = np.stack([np.zeros(m), xd(h[0]), xd(h[1])], axis=1)
    b = np.stack([np.zeros(m), xd(h[2]), xd(h[3])], axis=1)
    c = np.stack([np.zeros(m), xd(h[4]), xd(h[5])], axis=1)
    d = np.stack([xd(h[6]), xd(h[7]), xd(h[8])], axis=1)
    e = np.stack([xd(h[9]), xd(h[10]), xd(h[11])], axis=1)
    f = np.stack([xd(h[12]), xd(h[13]), xd(h[14])], axis=1)
    H = np.zeros((m, 6, 6, 3))
    H[:, 3, 3], H[:, 4, 3], H[:, 5, 3] = a, b, c
    H[:, 3, 4], H[:, 4, 4], H[:, 5, 4] = b, d, e
    H[:, 3, 5], H[:, 4, 5], H[:, 5, 5] = c, e, f
    return J, H


def pair_terms(tg: Target, q, x, pi, ci, p, small_angle_rule=True):
    """The 29 sums over the given pairs: q (transformed points, any float type), x (untransformed, double)."""
    j, h = angle_terms(p, small_angle_rule)
    qp = q[pi].astype(F64) - tg.v["mean"][ci]
    ic = tg.v["icov"][ci]
    icq = np.einsum("mrc,mc->mr", ic, qp)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-tg.d2 * np.einsum("mr,mr->m", qp, icq) / 2.0)
        de = tg.d2 * e
        use = ~((de > 1.0) | (de < 0.0) | (de != de))
    pi, qp, ic, icq, e, de = pi[use], qp[use], ic[use], icq[use], e[use], de[use]
    w = de * tg.d1
    J, H = point_derivatives(x[pi].astype(F64), j, h)
    icJ = np.einsum("mrc,mkc->mkr", ic, J)                 # icov J_k
    aq = np.einsum("mr,mkr->mk", qp, icJ)                  # q'^T icov J_k
    out = np.zeros(TERMS)
    out[0] = len(pi)
    out[1] = np.sum(-tg.d1 * e)
    out[2:8] = np.sum(aq * w[:, None], axis=0)
    qH = np.einsum("mr,mklr->mkl", icq, H)                  # q'^T icov H_kl
    JJ = np.einsum("mlr,mkr->mkl", J, icJ)                  # J_l^T icov J_k
    Hs = w[:, None, None] * (-tg.d2 * aq[:, :, None] * aq[:, None, :] + qH + JJ)
    out[8:] = np.sum(Hs, axis=0)[np.triu_indices(6)]
    return out


def derivatives(tg: Target, src, T, p):
    """One evaluation as the library runs it: q = the float transform T of the source, neighbourhoods of q, the 29 sums at p."""
    xyz = np.asarray(src, F32)[:, :3]
    q = transform_f32(T, xyz)
    pi, ci = tg.pairs(q)
    return pair_terms(tg, q, xyz.astype(F64), pi, ci, p)


def symmetric(sums):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = sums[8:29]
    return H + np.triu(H, 1).T


# ---- the Newton loop --------------------------------------------------------------------------------------------------------
STEP, ZERO, NAN = 0, 1, 2


def step(sums, p, step_size, eps):
    """One Newton step (PCL 1.8): -> (status, p_out, a, T_out float32, evaluate)."""
    p = np.asarray(p, F64)
    g = np.asarray(sums[2:8], F64)
    H = symmetric(sums)
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return NAN, p.copy(), 0.0, transform_float(p), False
    U, S, Vt = np.linalg.svd(H)
    thr = max(S[0] * 6 * 2.0**-52, np.finfo(F64).tiny)
    keep = S > thr
    delta = Vt[keep].T @ ((U[:, keep].T @ -g) / S[keep])
    norm = math.sqrt(float(np.sum(delta * delta)))
    if norm == 0.0:
        return ZERO, p.copy(), 0.0, transform_float(p), False
    if norm != norm:
        return NAN, p.copy(), 0.0, transform_float(p), False
    d = delta / norm
    d_phi_0 = -float(g @ d)
    if d_phi_0 >= 0:
        if d_phi_0 == 0:
            return STEP, p.copy(), 0.0, transform_float(p), False
        d = -d
    a = max(min(norm, step_size), eps / 2.0)
    p_out = p + d * a
    return STEP, p_out, a, transform_float(p_out), True


def align(tg: Target, src, max_iterations=35, transformation_epsilon=0.1, step_size=0.1, guess=None):
    """NormalDistributionsTransform::computeTransformation -> dict(T, iterations, state, converged, n_corr, probability)."""
    src = np.asarray(src, F32)
    Tf = np.eye(4, dtype=F32) if guess is None else np.asarray(guess, F32).copy()
    p = initial_pose(guess)
    sums = derivatives(tg, src, Tf, p)
    nr, state, converged = 0, NOT_CONVERGED, False
    if sums[0] == 0:
        converged, state = True, CONV_NO_CORRESPONDENCES
    else:
        while True:
            st, p_new, a, T_new, evaluate = step(sums, p, step_size, transformation_epsilon)
            if st == ZERO:
                converged, state = True, CONV_TRANSFORM
                break
            if st == NAN:
                converged, state = False, NOT_CONVERGED
                break
            if evaluate:
                p, Tf = p_new, T_new
                sums = derivatives(tg, src, Tf, p)
            cap = nr > max_iterations
            if cap or (nr and abs(a) < transformation_epsilon):
                converged, state = True, (CONV_ITERATIONS if cap else CONV_TRANSFORM)
                nr += 1
                break
            nr += 1
    return dict(T=Tf, iterations=nr, state=state, converged=converged, n_corr=int(sums[0]), probability=sums[1] / len(src), p=p)
