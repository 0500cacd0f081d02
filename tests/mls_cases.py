"""The moving least squares' clouds (include/icpgpu.h, "moving least squares"), shared by tests/test_mls_host.py -- which checks what
the restatement says about each against an answer known by hand or against the exact loop -- and tests/test_gpu_mls.py, which
compares the device with the restatement on every one of them.  A hand case is (name, cloud, queries or None, radius,
sqr_gauss_param); the tests run it for the orders they name."""
import functools

import numpy as np

from icpslam_amd import synth

F32 = np.float32
HEMISPHERE_CENTRE = np.array([5.0, -3.0, 1.0])
HEMISPHERE_RADIUS = 2.0
PARABOLOID = (0.25, -0.5)             # z = a x^2 + b y^2 (with the lattice's spacing of 1/8 every z is a float32 exactly)
BLOB_SIZES = (1, 2, 3, 5, 6, 7, 9, 10, 11, 63, 64, 65, 128, 129, 300)
BLOB_RADIUS = 0.5


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


@functools.lru_cache(maxsize=None)
def hemisphere(seed: int, noise: float = 0.01) -> np.ndarray:
    """The cap x[:, 2] > 0.2 of 1 500 random unit vectors, scaled to 2 m with 1 cm of radial noise, about (5, -3, 1): some 600 points."""
    r = np.random.default_rng(seed)
    d = r.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d = d[d[:, 2] > 0.2]
    rad = HEMISPHERE_RADIUS + r.normal(0.0, noise, len(d))
    c = points(HEMISPHERE_CENTRE + rad[:, None] * d)
    c.setflags(write=False)
    return c


def radial_rms(cloud) -> float:
    return float(np.sqrt(np.mean((np.linalg.norm(np.asarray(cloud)[:, :3].astype(np.float64) - HEMISPHERE_CENTRE, axis=1) - HEMISPHERE_RADIUS) ** 2)))


def radial_angle_deg(pts, normals) -> np.ndarray:
    """The angle between each normal's line and the radial direction at its point, in degrees."""
    n = np.asarray(normals)[:, :3].astype(np.float64)
    d = np.asarray(pts)[:, :3].astype(np.float64) - HEMISPHERE_CENTRE
    cos = np.abs((n * d).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1))
    return np.degrees(np.arccos(np.clip(cos, 0.0, 1.0)))


def paraboloid(m=9, spacing=0.125) -> np.ndarray:
    """z = a x^2 + b y^2 on an m x m lattice centred on the apex (m odd): the apex is point (m * m) // 2."""
    a, b = PARABOLOID
    g = (np.arange(m) - m // 2) * spacing
    x, y = (v.reshape(-1) for v in np.meshgrid(g, g, indexing="ij"))
    return points(np.stack([x, y, a * x * x + b * y * y], 1))


def blobs(sizes=BLOB_SIZES, seed=31) -> np.ndarray:
    """Groups of exactly the given numbers of points, each within 10 cm of its centre on a gently curved patch, 50 m apart: with
    BLOB_RADIUS a point's row is its group."""
    r = np.random.default_rng(seed)
    out = []
    for g, m in enumerate(sizes):
        xy = r.uniform(-0.1, 0.1, (m, 2))
        z = 0.4 * xy[:, 0] ** 2 - 0.3 * xy[:, 0] * xy[:, 1] + r.normal(0, 0.002, m)
        out.append(np.array([50.0 * g, 3.0, -2.0]) + np.stack([xy[:, 0], xy[:, 1], z], 1))
    return points(np.concatenate(out))


def with_nan_rows() -> np.ndarray:
    c = scan(257).copy()
    c[[0, 64, 200], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    c[100] = np.nan
    return c


def nan_queries() -> np.ndarray:
    q = scan(257)[:40].copy()
    q[[3, 17], [0, 2]] = [np.nan, np.inf]
    q[30] = np.nan
    return q


def hand_cases() -> list:
    oblique = points([[0.25 * i, 0.5 * i, -0.125 * i] for i in range(40)])
    plane_x = lattice(1, 9, 9, 0.25)
    return [
        ("planar_lattice", lattice(9, 9, 1, 0.25), None, 0.6, 0.0),            # N along z exactly: the frame's second branch
        ("plane_x", plane_x, None, 0.6, 0.0),                                   # N along x exactly: its first branch
        ("paraboloid", paraboloid(), None, 0.3, 0.0),
        ("line", lattice(1, 40, 1, 0.25), None, 1.6, 0.0),
        ("oblique_line", oblique, None, 3.2, 0.0),
        ("coincident", points([[3, -2, 7]] * 9), None, 0.5, 0.0),
        ("blobs", blobs(), None, BLOB_RADIUS, 0.0),
        ("explicit_s", lattice(9, 9, 1, 0.25), None, 0.6, 0.36),                # the default, spelled out: the same bits
        ("tiny_s", paraboloid(), None, 0.3, 1e-7),                             # every weight but the query's own underflows to 0
        ("small_s", paraboloid(), None, 0.3, 2.5e-5),                          # the nearest ring at e^-625, the next one gone
        ("nan_rows", with_nan_rows(), None, 1.5, 0.0),
        ("nan_queries", scan(257), nan_queries(), 1.5, 0.0),
        ("far_from_origin", points(hemisphere(1)[:, :3] + F32(120.0)), None, 0.45, 0.0),
    ]
