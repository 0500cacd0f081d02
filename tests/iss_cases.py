"""The ISS keypoints' hand-made clouds (include/icpgpu.h, "ISS keypoints"), shared by tests/test_iss_host.py -- which checks what the
restatement says about each against an answer known by hand -- and tests/test_gpu_iss.py, which compares the device with the
restatement on every one of them.  A case is (name, cloud, arguments): arguments = (salient_radius, non_max_radius, gamma_21,
gamma_32, min_neighbors)."""
import functools
import itertools

import numpy as np

from icpslam_amd import synth

F32 = np.float32


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def points(xyz) -> np.ndarray:
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = np.asarray(xyz, F32).reshape(-1, 3)
    return c


def lattice(nx, ny, nz, spacing=1.0) -> np.ndarray:
    g = [np.arange(m, dtype=F32) * F32(spacing) for m in (nx, ny, nz)]
    return points(np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3))


def three_faces(m=7) -> np.ndarray:
    """The m x m lattice faces x = 0, y = 0 and z = 0 of a cube, each point once, sorted: point 0 is the corner."""
    pts = set()
    for a, b in itertools.product(range(m), range(m)):
        pts |= {(0, a, b), (a, 0, b), (a, b, 0)}
    return points(sorted(pts))


CORNER_ARGS = (2.5, 1.5, 0.45, 10.0, 5)
TIES_ARGS = (1.1, 1.1, 10.0, 10.0, 4)   # (a corner's ball holds four points)


def two_groups() -> np.ndarray:
    """Four points around the origin and five around (100, 0, 0), each group well inside a ball of 1 m."""
    a = [[0, 0, 0], [0.1, 0, 0], [0, 0.2, 0], [0, 0, 0.3]]
    b = [[100, 0, 0], [100.1, 0, 0.05], [100, 0.2, 0], [100, 0.05, 0.3], [100.2, 0.2, 0.2]]
    return points(a + b)


def on_the_radius() -> np.ndarray:
    """Pairs (p, p + d): d = 0.5 exactly (d2 == r2 for radius 0.5: outside) and d = the float below 0.5 (inside)."""
    below = float(np.nextafter(F32(0.5), F32(0)))
    return points([[0, 0, 0], [0.5, 0, 0], [0, 10, 0], [below, 10, 0]])


def with_nan_rows() -> np.ndarray:
    c = scan(257).copy()
    c[[0, 64, 200], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    c[100] = np.nan
    return c


def hand_cases() -> list:
    oblique = points([[0.25 * i, 0.5 * i, -0.125 * i] for i in range(12)])
    return [
        ("planar_lattice", lattice(7, 7, 1), (1.5, 1.5, 0.975, 0.975, 1)),
        ("line", lattice(1, 12, 1, 0.25), (1.0, 1.0, 10.0, 10.0, 1)),
        ("oblique_line", oblique, (1.0, 1.0, 10.0, 10.0, 1)),
        ("coincident", points([[3, -2, 7]] * 9), (0.5, 0.5, 10.0, 10.0, 1)),
        ("corner", three_faces(7), CORNER_ARGS),
        ("ties", lattice(5, 5, 5), TIES_ARGS),
        ("two_groups", two_groups(), (1.0, 1.0, 10.0, 10.0, 5)),
        ("on_the_radius", on_the_radius(), (0.5, 0.5, 10.0, 10.0, 1)),
        ("nan_rows", with_nan_rows(), (1.5, 1.0, 0.975, 0.975, 5)),
        ("non_max_smaller", scan(600), (1.5, 0.6, 0.975, 0.975, 5)),
        ("non_max_larger", scan(600), (1.0, 2.5, 0.975, 0.975, 5)),
    ]
