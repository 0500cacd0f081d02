"""The hand clouds of the cropping and sampling filters' tests (tests/test_sampling_host.py, tests/test_gpu_sampling.py)."""
from __future__ import annotations

import numpy as np

from icpslam_amd import synth

F32 = np.float32
# the sizes every filter is run at: a lane, a wave and a workgroup of the flag kernels and the tile of launch_compact (icp_scan.hip:
# SC_TILE = 4096), each with its neighbours
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
EGO_MIN, EGO_MAX = (-1.5, -1.0, -2.0), (2.5, 1.0, 0.5)  # the vehicle's own body in the sensor frame


def rows(xyz) -> np.ndarray:
    xyz = np.asarray(xyz, np.float64)
    cloud = np.ones((len(xyz), 4), F32)
    cloud[:, :3] = xyz.astype(F32)
    cloud[:, 3] = np.arange(len(xyz), dtype=F32) * F32(0.25)  # (w is carried through: make it tell the rows apart)
    return cloud


_SCANS = {}


def scan(n: int, seed: int = 5) -> np.ndarray:
    """n returns of a synthetic street scan in the sensor frame (a prefix of one 5 000-return scan per seed, w = the row's number / 4)."""
    if seed not in _SCANS:
        _SCANS[seed] = synth.scan(synth.make_scene(3), np.eye(4), 5000, seed)
    if n > 5000:
        return rows(synth.scan(synth.make_scene(3), np.eye(4), n, seed)[:, :3])
    return rows(_SCANS[seed][:n, :3])


def with_bad_rows(cloud, where) -> np.ndarray:
    """NaN / +inf / -inf in x, y or z of the rows `where`, in turn."""
    out = np.array(cloud, F32)
    bad = (np.nan, np.inf, -np.inf)
    for k, i in enumerate(where):
        out[i, k % 3] = bad[(k // 3) % 3]
    return out


def one_wave_of_bad_rows(n: int):
    """The first row, the last row and every position of the wave that starts at row 64 (as far as the cloud has them)."""
    return sorted({i for i in [0, n - 1] + list(range(64, 128)) if 0 <= i < n})


def faces(mn=EGO_MIN, mx=EGO_MAX) -> np.ndarray:
    """Rows exactly ON each of the box's six faces, and one float32 step outside each: 12 rows around a centre row."""
    mn, mx = np.asarray(mn, F32), np.asarray(mx, F32)
    centre = ((mn + mx) * F32(0.5)).astype(F32)
    out = [centre]
    for a in range(3):
        for bound, away in ((mn[a], F32(-np.inf)), (mx[a], F32(np.inf))):
            on, off = centre.copy(), centre.copy()
            on[a] = bound
            off[a] = np.nextafter(bound, away)
            out += [on, off]
    return rows(np.array(out))


def lattice444() -> np.ndarray:
    """The 4 x 4 x 4 integer lattice, x fastest: row i = (i % 4, (i // 4) % 4, i // 16)."""
    i = np.arange(64)
    return rows(np.stack((i % 4, (i // 4) % 4, i // 16), axis=1))


def tie_cells() -> np.ndarray:
    """Leaf 1: cell centres are exact (k + 0.5).  Rows 0 and 1 tie in cell (0, 0, 0) at d2 = 1 / 16, row 2 of the same cell is farther;
    row 3 lies exactly on the face x = 1 and so in cell (1, 0, 0); rows 4 and 5 tie in cell (-1, -1, -1), the later one first in memory
    order of nothing: the lower index wins."""
    return rows([(0.25, 0.5, 0.5), (0.75, 0.5, 0.5), (0.5, 0.5, 0.125), (1.0, 0.5, 0.5), (-0.5, -0.25, -0.5), (-0.5, -0.75, -0.5)])


def duplicated(n: int, seed: int = 3) -> np.ndarray:
    """n rows of which every third repeats an earlier one bit for bit."""
    cloud = scan(n, seed).copy()
    r = np.random.default_rng(seed)
    for i in range(2, n, 3):
        cloud[i, :3] = cloud[int(r.integers(0, i)), :3]
    return cloud


def far_away(n: int = 3000) -> np.ndarray:
    """A scan 3 km from the origin: the cell centres' products and the differences to them round."""
    cloud = scan(n, 6).copy()
    cloud[:, :3] += F32([3000.0, -3000.0, 40.0])
    return cloud
