"""Hand clouds for region growing (include/icpgpu.h, "region growing"), shared by tests/test_region_host.py (where what each must
give is asserted) and tests/test_gpu_region.py (where the device is compared with the restatement on every one of them).

A case is (cloud (n, 4) float32, normals (n, 4) float32 {nx, ny, nz, curvature}, k, cos, threshold, lo, hi): the arguments of one call.
"""
from __future__ import annotations

import collections
import math

import numpy as np

F32 = np.float32
INT_MAX = 2**31 - 1
Case = collections.namedtuple("Case", "cloud normals k cos threshold lo hi")
UP, SIDE, TILT = (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.70710677, 0.70710677)


def cos_of(degrees: float) -> np.float32:
    return F32(math.cos(math.radians(degrees)))


def build(xyz, normals, curvature, k, cos, threshold=0.05, lo=1, hi=INT_MAX) -> Case:
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    cloud = np.ones((len(xyz), 4), F32)
    cloud[:, :3] = xyz.astype(F32)
    nrm = np.empty((len(xyz), 4), F32)
    nrm[:, :3] = np.asarray(normals, np.float64).reshape(-1, 3).astype(F32)
    nrm[:, 3] = np.broadcast_to(np.asarray(curvature, np.float64), (len(xyz),)).astype(F32)
    return Case(cloud, nrm, int(k), F32(cos), F32(threshold), int(lo), int(hi))


def shuffled(case: Case, seed: int):
    """(the case with its indices shuffled by a fixed seed, order): order[p] = the new index of point p."""
    order = np.random.default_rng(seed).permutation(len(case.cloud))
    cloud, normals = np.empty_like(case.cloud), np.empty_like(case.normals)
    cloud[order], normals[order] = case.cloud, case.normals
    return case._replace(cloud=cloud, normals=normals), order


# ---- two lattice planes meeting at 90 degrees ---------------------------------------------------------------------------------
def two_planes(cos=None, threshold=0.05, k=9, lo=1, hi=INT_MAX) -> Case:
    """A: (x, 0.9 + y, 0), x 0..9, y 0..8, normal UP, indices 9 x + y.  B: (x, 0, 1 + z), normal SIDE, indices 90 + 9 x + z.  The
    crease (x, 0, 0), indices 180 + x, normal TILT (45 degrees from both), curvature 0.2: 0.9 from A's edge, 1.0 from B's.  At the
    default 50 degrees the crease is smooth with both planes and the planes are not smooth with each other."""
    xyz = [[x, 0.9 + y, 0] for x in range(10) for y in range(9)] + [[x, 0, 1 + z] for x in range(10) for z in range(9)]
    xyz += [[x, 0, 0] for x in range(10)]
    normals = [UP] * 90 + [SIDE] * 90 + [TILT] * 10
    return build(xyz, normals, [0.0] * 180 + [0.2] * 10, k, cos_of(50) if cos is None else cos, threshold, lo, hi)


# ---- one crease point between a core of each plane ----------------------------------------------------------------------------
def crease_tie(one_ulp: bool = False, k=3) -> Case:
    """0: a core with normal UP; 1: a core with normal SIDE at (1, 0, 0), d2 = 1 from the crease point 2 at the origin (TILT, not
    core).  a is at d2 = 1 as well (a tie: the lower index wins), or with one_ulp at d2 = nextafter(1, 2): the nearer, 1, wins."""
    a = [-1.0, float(F32(2.0 ** -11.5)), 0.0] if one_ulp else [-1.0, 0.0, 0.0]
    return build([a, [1, 0, 0], [0, 0, 0]], [UP, SIDE, TILT], [0.0, 0.0, 1.0], k, 0.5)


def dot_on_threshold(above: bool = False) -> Case:
    """Normals (1, 0, 0) and (0.5, 0.8660254, 0): dot = 0.5 exactly.  Joined at 0.5, apart at nextafter(0.5, 1)."""
    return build([[0, 0, 0], [1, 0, 0]], [(1, 0, 0), (0.5, 0.8660254, 0.0)], 0.0, 2, np.nextafter(F32(0.5), F32(1)) if above else F32(0.5))


def curvature_on_threshold() -> Case:
    """Curvatures threshold, 0, nextafter(threshold, 1): core, core, border."""
    t = F32(0.05)
    c = build([[0, 0, 0], [1, 0, 0], [2, 0, 0]], [UP] * 3, 0.0, 3, cos_of(30), t)
    c.normals[:, 3] = [t, F32(0), np.nextafter(t, F32(1))]
    return c


def antiparallel() -> Case:
    return build([[0, 0, 0], [1, 0, 0]], [UP, (0, 0, -1)], 0.0, 2, cos_of(30))


# ---- a plane and a far point that lists it but is listed by none of it --------------------------------------------------------
def far_point(core: bool) -> Case:
    """A 5 x 5 plane of cores (indices 0..24) and point 25 ten units above it, k = 5: its row is itself and four plane points, no
    plane point's row has it.  Not core: it is single.  Core (curvature 0.01, so PCL seeds it after the plane): it joins the plane
    through its OWN row -- the symmetrisation; PCL's loop keeps it apart."""
    xyz = [[x, y, 0] for x in range(5) for y in range(5)] + [[2, 2, 10]]
    return build(xyz, [UP] * 26, [0.0] * 25 + [0.01 if core else 1.0], 5, cos_of(30))


def chain_with_nan_normal(nan: bool = True) -> Case:
    """Seven points in a line, k = 3 (itself and both neighbours); the middle one's normal is NaN: it cannot bridge the halves."""
    c = build([[x, 0, 0] for x in range(7)], [UP] * 7, 0.0, 3, cos_of(30))
    if nan:
        c.normals[3, 1] = np.nan
    return c


def duplicates() -> Case:
    """A 4 x 4 lattice three times over (copy c of point p: 16 c + p), k = 5; the third copy is not core: every point of it is at
    d2 = 0 from two cores and goes to the lower one, p."""
    xyz = [[x, y, 0] for x in range(4) for y in range(4)] * 3
    return build(xyz, [UP] * 48, [0.0] * 32 + [1.0] * 16, 5, cos_of(30))


def cylinder(degrees: float, lo=1, hi=INT_MAX) -> Case:
    """A patch of a cylinder of radius 5: 31 columns 2 degrees apart (0.1745 along the arc), 8 points 0.17 apart in each, index
    8 column + row, radial normals, k = 9.  One region at 30 degrees; at 1 degree a column is smooth with itself alone: 31 regions
    of 8 points, all tied."""
    xyz, normals = [], []
    for col in range(31):
        a = math.radians(2.0 * col)
        for row in range(8):
            xyz.append([5 * math.cos(a), 5 * math.sin(a), 0.17 * row])
            normals.append([math.cos(a), math.sin(a), 0.0])
    return build(xyz, normals, 0.01, 9, cos_of(degrees), 0.05, lo, hi)


# ---- shapes for the device's launch geometry ------------------------------------------------------------------------------------
def strip(n: int, seed: int, k=4) -> tuple:
    """n cores in a line 0.1 apart with one normal, the indices shuffled: one region whose graph has diameter ~n / 2."""
    return shuffled(build([[0.1 * i, 0, 0] for i in range(n)], [UP] * n, 0.0, k, cos_of(30)), seed)


def interleaved_strips(m: int, k=6) -> Case:
    """Even indices on one line with normal UP, odd ones on a line 0.05 beside it with normal (1, 0, 0): every point's nearest
    neighbour is in the other strip and is not smooth with it; its own strip's neighbours, 0.1 away, are in its row too."""
    order = np.random.default_rng(23).permutation(m)
    xyz, normals = np.zeros((2 * m, 3)), np.zeros((2 * m, 3))
    xyz[0::2, 0], xyz[1::2, 0], xyz[1::2, 1] = 0.1 * order, 0.1 * order[::-1], 0.05
    normals[0::2], normals[1::2] = UP, (1, 0, 0)
    return build(xyz, normals, 0.0, k, cos_of(30))


def tied_regions(m: int, seed: int) -> tuple:
    """m isolated pairs of cores and 40 far points that are not core, k = 2: with the window 2 .. 2 exactly m regions, all tied."""
    xyz = [[10.0 * i, 0, 0] for i in range(m)] + [[10.0 * i + 0.1, 0, 0] for i in range(m)] + [[10.0 * i, 50, 0] for i in range(40)]
    return shuffled(build(xyz, [UP] * (2 * m + 40), [0.0] * (2 * m) + [1.0] * 40, 2, cos_of(30), 0.05, 2, 2), seed)


# every hand case by name: what the device is compared with the restatement on
CASES = {
    "two_planes": two_planes(),
    "two_planes_k1": two_planes(k=1),
    "two_planes_no_curvature_test": two_planes(threshold=math.inf),
    "two_planes_cos_zero": two_planes(cos=0.0),
    "two_planes_cos_negative": two_planes(cos=-1.0),
    "two_planes_window": two_planes(lo=91, hi=100),
    "crease_tie": crease_tie(),
    "crease_one_ulp": crease_tie(one_ulp=True),
    "crease_k_above_n": crease_tie(k=64),
    "dot_on_threshold": dot_on_threshold(),
    "dot_above_threshold": dot_on_threshold(above=True),
    "curvature_on_threshold": curvature_on_threshold(),
    "antiparallel": antiparallel(),
    "far_noncore": far_point(core=False),
    "far_core": far_point(core=True),
    "nan_normal": chain_with_nan_normal(),
    "chain": chain_with_nan_normal(nan=False),
    "duplicates": duplicates(),
    "cylinder_30": cylinder(30),
    "cylinder_1": cylinder(1),
    "cylinder_1_window": cylinder(1, 8, 8),
    "cylinder_1_above": cylinder(1, 9, INT_MAX),
    "cylinder_1_max_below_min": cylinder(1, 3, 2),
}
