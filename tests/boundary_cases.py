"""The boundary estimation's hand-made clouds (include/icpgpu.h, "boundary estimation"), shared by tests/test_boundary_host.py -- which
checks what the restatement says about each against an answer known by hand -- and tests/test_gpu_boundary.py, which compares the
device with the restatement on every one of them.  A case is (name, cloud, queries or None, normals, k, radius, angle_threshold)."""
import functools
import math

import numpy as np

import iss_cases as K

F32 = np.float32
HALF_PI = math.pi / 2
ABOVE_HALF_PI = math.nextafter(HALF_PI, 4.0)
points, lattice, scan = K.points, K.lattice, K.scan


def normals_of(n, direction=(0.0, 0.0, 1.0)) -> np.ndarray:
    out = np.zeros((n, 4), F32)
    out[:, :3] = np.asarray(direction, F32)
    return out


@functools.lru_cache(maxsize=None)
def scan_normals(n: int, k: int = 12) -> np.ndarray:
    """The restated normals of scan(n) from k neighbours."""
    import normals_restated as N
    nrm = N.estimate(scan(n), None, k, 0.0)[0]
    nrm.setflags(write=False)
    return nrm


def ring(m: int, radius: float = 1.0, first: float = 0.0, arc: float = 2 * math.pi) -> np.ndarray:
    """The origin, then m points on a circle in the plane z = 0, spread evenly over `arc` radians from angle `first`."""
    a = first + arc * np.arange(m) / m
    return points([[0, 0, 0]] + [[radius * math.cos(t), radius * math.sin(t), 0] for t in a])


def hand_cases() -> list:
    tilted = np.array([1.0, 2.0, 2.0]) / 3.0
    # a lattice patch in the plane through the origin with normal `tilted`, spanned by two orthogonal in-plane vectors
    e1 = np.array([2.0, -1.0, 0.0]) / math.sqrt(5.0)
    e2 = np.cross(tilted, e1)
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    tilted_patch = points(g[:, :1] * e1 + g[:, 1:] * e2)
    pair = points([[0, 0, 0], [0, 0, 0], [1, 0, 0]])
    dup = points([[0, 0, 0], [1, 0, 0], [2, 0, 0], [-1, 0, 0], [3, 0, 0]])
    return [
        ("lattice_8", lattice(7, 7, 1), None, normals_of(49), 0, 1.5, HALF_PI),
        ("lattice_4_at", lattice(7, 7, 1), None, normals_of(49), 0, 1.1, HALF_PI),
        ("lattice_4_above", lattice(7, 7, 1), None, normals_of(49), 0, 1.1, ABOVE_HALF_PI),
        ("opposite_pi", points([[0, 0, 0], [1, 0, 0], [-1, 0, 0]]), None, normals_of(3), 3, 0.0, math.pi),
        ("opposite_3", points([[0, 0, 0], [1, 0, 0], [-1, 0, 0]]), None, normals_of(3), 3, 0.0, 3.0),
        ("single_direction", pair, None, normals_of(3), 3, 0.0, HALF_PI),
        ("rows_of_1_and_2", points([[0, 0, 0], [1, 0, 0], [50, 0, 0]]), None, normals_of(3), 0, 2.0, HALF_PI),
        ("along_the_normal", points([[0, 0, 0], [0, 0, 1], [0, 0, -2], [0, 0, 3]]), None, normals_of(4), 4, 0.0, HALF_PI),
        ("coincident", points([[3, -2, 7]] * 9), None, normals_of(9), 0, 0.5, HALF_PI),
        ("duplicated_directions", dup, None, normals_of(5), 5, 0.0, math.pi),
        ("zero_normal", lattice(3, 3, 1), None, normals_of(9, (0, 0, 0)), 0, 1.5, HALF_PI),
        ("nan_normal", lattice(3, 3, 1), None, normals_of(9, (np.nan, 0, 1)), 0, 1.5, HALF_PI),
        ("frame_far_branch", lattice(1, 5, 5), None, normals_of(25, (1, 0, 0)), 0, 1.5, HALF_PI),
        ("frame_tilted", tilted_patch, None, normals_of(25, tilted), 0, 1.5, HALF_PI),
        ("witness_ties", ring(3, 1.0, 0.3)[[0, 3, 1, 2]], None, normals_of(4), 4, 0.0, HALF_PI),
        ("ring_full", ring(12), None, normals_of(13), 0, 1.01, 0.6),
        ("ring_half", ring(12, 1.0, 0.2, math.pi), None, normals_of(13), 0, 1.01, 0.6),
    ]
