"""Hand clouds for the segment moments (include/icpgpu.h, "segment moments"), shared by tests/test_segment_host.py (where what each
must give is asserted) and tests/test_gpu_segment.py (where the device is compared with the restatement on every one of them).

A case is (cloud (n, 4) float32, segments: a list of index lists): the arguments of one call with a HOST source.
"""
from __future__ import annotations

import collections
import math

import numpy as np

F32 = np.float32
Case = collections.namedtuple("Case", "cloud segments")


def cloud_of(xyz) -> np.ndarray:
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    cloud = np.ones((len(xyz), 4), F32)
    cloud[:, :3] = xyz.astype(F32)
    return cloud


def whole(xyz) -> Case:
    cloud = cloud_of(xyz)
    return Case(cloud, [list(range(len(cloud)))])


def lattice(nx, ny, nz, sx, sy, sz, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
    return np.array([[origin[0] + sx * i, origin[1] + sy * j, origin[2] + sz * k] for i in range(nx) for j in range(ny) for k in range(nz)], np.float64)


def yawed(xyz, degrees: float, centre=(0.0, 0.0, 0.0)) -> np.ndarray:
    a = math.radians(degrees)
    R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = np.asarray(centre, np.float64)
    return (np.asarray(xyz, np.float64) - c) @ R.T + c


BOX = lattice(4, 4, 4, 2.0, 3.0, 5.0, origin=(1.0, -2.0, 0.5))   # extents 6 x 9 x 15 about (4, 2.5, 8): every coordinate a small dyadic
BOX_CENTRE = (4.0, 2.5, 8.0)


def box_lattice() -> Case:
    return whole(BOX)


def box_yawed() -> Case:
    return whole(yawed(BOX, 30.0, BOX_CENTRE))


def cube_lattice() -> Case:
    return whole(lattice(3, 3, 3, 1.0, 1.0, 1.0))


def plane_axis_parallel() -> Case:
    return whole(lattice(5, 4, 1, 1.0, 0.5, 1.0, origin=(0.0, 0.0, 2.0)))


def plane_tilted() -> Case:
    p = lattice(6, 5, 1, 0.3, 0.2, 1.0)
    p[:, 2] = 0.37 * p[:, 0] - 0.21 * p[:, 1] + 1.3
    return whole(p)


def collinear() -> Case:
    return whole([[0.25 * t, 0.5 * t, 0.75 * t] for t in range(9)])


def coincident() -> Case:
    return whole([[1.5, -2.25, 3.0]] * 5)


def single_point() -> Case:
    return Case(cloud_of([[1.0, 2.0, 3.0], [7.0, -8.0, 9.5]]), [[1]])


def nan_segments() -> Case:
    """0..2 NaN rows (one coordinate each), 3..7 a small lattice.  Segments: only NaN rows; NaN first; NaN in the middle and at the end;
    an empty one."""
    cloud = cloud_of([[0, 0, 0]] * 3 + [[1, 0, 0], [2, 1, 0], [3, 0, 1], [4, 2, 2], [5, 1, 3]])
    cloud[0, 0], cloud[1, 1], cloud[2, 2] = np.nan, np.inf, -np.inf
    return Case(cloud, [[0, 1, 2], [0, 3, 4, 5], [3, 1, 4, 5, 6, 2], [], [2, 7]])


def repeated_and_overlapping() -> Case:
    """A 3 x 3 x 2 lattice; a segment with repeats (an index counts as often as it is listed), two that overlap, one unsorted and the
    same one sorted (another K, the same centroid to rounding)."""
    cloud = cloud_of(lattice(3, 3, 2, 0.7, 1.1, 0.4))
    n = len(cloud)
    perm = np.random.default_rng(7).permutation(n).tolist()
    return Case(cloud, [[0, 5, 5, 5, 9, 0, 17], list(range(0, 12)), list(range(6, 18)), perm, sorted(perm)])


def signed_zeros() -> Case:
    """-0 against +0: x holds both zeros (the minimum is -0, the maximum +0), y only -0, z only +0."""
    cloud = cloud_of([[0.0, 0.0, 0.0]] * 4)
    cloud[:, 0] = [0.0, -0.0, 0.0, -0.0]
    cloud[:, 1] = -0.0
    return Case(cloud, [[0, 1, 2, 3], [2, 3], [1, 0]])


def far_from_origin(seed: int = 11, n: int = 400) -> Case:
    """A 2 x 1 x 0.5 m blob 3 km from the origin."""
    rng = np.random.default_rng(seed)
    return whole(np.array([3000.0, -2100.0, 150.0]) + rng.uniform(-1, 1, (n, 3)) * np.array([1.0, 0.5, 0.25]))


def wide_sum() -> Case:
    """24 entries whose dx runs from 1e-5 to 100 m about K = the origin: the terms of the dx dx sum span 1e-10 .. 1e4 m^2, inside the
    header's RANGE (25 * 1e7 < 2^28)."""
    x = np.concatenate([[0.0], np.logspace(-5, 2, 24)])
    return whole(np.stack([x, -x, np.zeros_like(x)], axis=1))


CASES = {
    "box_lattice": box_lattice(),
    "box_yawed": box_yawed(),
    "cube_lattice": cube_lattice(),
    "plane_axis_parallel": plane_axis_parallel(),
    "plane_tilted": plane_tilted(),
    "collinear": collinear(),
    "coincident": coincident(),
    "single_point": single_point(),
    "nan_segments": nan_segments(),
    "repeated_and_overlapping": repeated_and_overlapping(),
    "signed_zeros": signed_zeros(),
    "far_from_origin": far_from_origin(),
    "wide_sum": wide_sum(),
}
