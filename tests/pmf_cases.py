"""Hand clouds of the ground filter's tests, shared by the host tests (restatement against its literal loop) and the GPU tests (kernels
against the restatement).  CASES: name -> (cloud (n, 4) float32, the filter's keyword arguments, the operator's windows)."""
import functools

import numpy as np

F32 = np.float32


def points(xyz) -> np.ndarray:
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = np.asarray(xyz, F32).reshape(-1, 3)
    return c


def lattice(nx: int, ny: int, spacing: float, z=0.0, origin=(0.0, 0.0)) -> np.ndarray:
    """nx x ny points spacing apart, x fastest; z: a constant or a function of (ix, iy)."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
    ix, iy = ix.reshape(-1), iy.reshape(-1)
    zz = z(ix, iy) if callable(z) else np.full(ix.size, z)
    xyz = np.stack([F32(origin[0]) + F32(spacing) * ix.astype(F32), F32(origin[1]) + F32(spacing) * iy.astype(F32), zz.astype(F32)], axis=1)
    return points(xyz)


def rippled(ix, iy):
    return 0.01 * ((7 * ix + 3 * iy) % 11)


def edge_lattice() -> np.ndarray:
    """Spacing 1.5 = h of window 3: every neighbour sits exactly on lo / hi of the first pass and must be in; spacing 2.5 etc. follow
    for the later windows only approximately.  All coordinates are exact."""
    return lattice(9, 7, 1.5, rippled)


def offset_lattice() -> np.ndarray:
    """A lattice of spacing 1 around x = 2^24, where float32's spacing changes from 1 to 2: p - h and q + h round apart, and the box
    relation is not symmetric (tests/test_pmf_host.py shows a pair)."""
    c = lattice(12, 3, 1.0, rippled, origin=(2.0**24 - 6.0, 0.0))
    return c


def block(width: int) -> np.ndarray:
    """A flat 21 x 21 lattice of spacing 1 with a width x width block raised by 2 in its middle."""
    lo = 10 - width // 2

    def z(ix, iy):
        return np.where((ix >= lo) & (ix < lo + width) & (iy >= lo) & (iy < lo + width), 2.0, 0.0)
    return lattice(21, 21, 1.0, z)


def signed_zeros() -> np.ndarray:
    rng = np.random.default_rng(11)
    c = lattice(8, 8, 1.0)
    c[:, 2] = np.where(rng.random(64) < 0.5, F32(-0.0), F32(0.0))
    return c


def duplicates() -> np.ndarray:
    rng = np.random.default_rng(12)
    base = points(np.concatenate([rng.uniform(-6, 6, (40, 2)), rng.normal(0, 0.1, (40, 1))], axis=1))
    c = np.concatenate([base, base[::2], base[::5]])
    c[40:60, 2] += F32(0.5)          # the same x, y with another z
    return c


def nan_rows() -> np.ndarray:
    c = lattice(10, 10, 1.0, rippled)
    c[::7, 1] = np.nan
    c[5, 2] = np.inf
    c[11, 0] = -np.inf
    c[50, 2] = 3.0
    return c


def vertical_line() -> np.ndarray:
    rng = np.random.default_rng(13)
    return points(np.concatenate([np.full((70, 2), 2.5), rng.normal(0, 1, (70, 1))], axis=1))


BOXES = ((-12.0, -10.0, 0.8, 1.0), (-3.0, 9.0, 1.0, 1.6), (6.0, -4.0, 1.2, 2.0), (13.0, 12.0, 0.9, 1.2), (2.0, -15.0, 1.1, 1.8))  # cx, cy, half, height


@functools.lru_cache(maxsize=None)
def graded_scene(n: int = 3000, seed: int = 21):
    """(cloud, is_box): a 40 m x 40 m street crowned along x = 0 with a 5 % grade to either side and a 5 cm ripple, and the tops of five
    boxes 1 - 2 m high and about 2 m wide standing on it, 60 points each; n points in all, shuffled."""
    rng = np.random.default_rng(seed)

    def ground(x, y):
        return -0.05 * np.abs(x) + 0.05 * np.sin(1.3 * x) * np.cos(0.9 * y)
    xy = [rng.uniform(-20, 20, (n - 300, 2))]
    lift = [np.zeros(n - 300)]
    for cx, cy, half, height in BOXES:
        xy.append(np.array([cx, cy]) + rng.uniform(-half, half, (60, 2)))
        lift.append(np.full(60, height))
    xy, lift = np.concatenate(xy), np.concatenate(lift)
    order = rng.permutation(n)
    xy, lift = xy[order], lift[order]
    is_box = lift > 0
    cloud = points(np.concatenate([xy, (ground(xy[:, 0], xy[:, 1]) + lift)[:, None]], axis=1))
    cloud.setflags(write=False)
    is_box.setflags(write=False)
    return cloud, is_box


SMALL = dict(max_window_size=5)      # windows 3 and 5
CASES = {
    "edge_lattice": (edge_lattice(), SMALL, (3.0, 6.0)),
    "offset_lattice": (offset_lattice(), SMALL, (2.0, 5.0)),
    "block_narrow": (block(3), SMALL, (3.0, 5.0)),
    "block_wide": (block(7), SMALL, (3.0, 5.0)),
    "signed_zeros": (signed_zeros(), dict(max_window_size=3, initial_distance=0.0), (2.0, 3.0)),
    "duplicates": (duplicates(), SMALL, (0.5, 3.0)),
    "nan_rows": (nan_rows(), SMALL, (3.0,)),
    "vertical_line": (vertical_line(), SMALL, (3.0,)),
    "slope_zero": (block(3), dict(max_window_size=9, slope=0.0), (9.0,)),
    "initial_zero": (lattice(6, 6, 1.0, rippled), dict(max_window_size=3, initial_distance=0.0), (3.0,)),
    "linear": (block(3), dict(max_window_size=8, exponential=False, base=1.0), (7.0,)),
}
for _cloud, _, _ in CASES.values():
    _cloud.setflags(write=False)
