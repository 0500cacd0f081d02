"""The hand clouds of the segmentation from normals, shared by tests/test_sac_normals_host.py and tests/test_gpu_sac_normals.py.
Every case is (cloud (n, 4) float32, normals (n, 4) float32 rows nx, ny, nz, curvature); analytic normals unless it says otherwise."""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32


def rows(xyz, w=1.0) -> np.ndarray:
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.concatenate((xyz, np.full((xyz.shape[0], 1), w)), axis=1).astype(F32)


def cylinder(axis_point, axis_dir, radius, n, rng, length=2.0, arc=2 * np.pi, noise=0.0):
    """n points on a cylinder's surface with outward normals; arc < 2 pi: a part of the circumference."""
    d = np.asarray(axis_dir, np.float64) / np.linalg.norm(axis_dir)
    e1 = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    phi, s = rng.uniform(0, arc, n), rng.uniform(0, length, n)
    radial = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    r = radius + (rng.normal(0, noise, n) if noise else np.zeros(n))
    pts = np.asarray(axis_point, np.float64) + s[:, None] * d + r[:, None] * radial
    return rows(pts), rows(radial, 0.0)


def floor_and_wall(n_floor=300, n_wall=200, seed=4):
    """A floor z = 0 (normals +z) meeting a wall x = 0 (normals +x) whose lowest points lie within a few centimetres of the floor."""
    rng = np.random.default_rng(seed)
    floor = np.stack((rng.uniform(0.05, 4, n_floor), rng.uniform(-2, 2, n_floor), rng.normal(0, 0.004, n_floor)), axis=1)
    z = np.concatenate((rng.uniform(0.0, 0.04, n_wall // 4), rng.uniform(0.04, 2.0, n_wall - n_wall // 4)))
    wall = np.stack((rng.normal(0, 0.004, n_wall), rng.uniform(-2, 2, n_wall), z), axis=1)
    cloud = np.concatenate((rows(floor), rows(wall)))
    normals = np.concatenate((rows(np.tile([0.0, 0.0, 1.0], (n_floor, 1)), 0.01), rows(np.tile([1.0, 0.0, 0.0], (n_wall, 1)), 0.01)))
    return cloud, normals, n_floor


def pole_and_pipe(seed=6, n_each=160):
    """A vertical pole (axis z through (1, 1, 0), radius 0.15) beside a horizontal pipe (axis x through (0, -1, 0.5), radius 0.10)."""
    rng = np.random.default_rng(seed)
    pole, pole_n = cylinder((1.0, 1.0, 0.0), (0, 0, 1), 0.15, n_each, rng)
    pipe, pipe_n = cylinder((0.0, -1.0, 0.5), (1, 0, 0), 0.10, n_each + 40, rng)
    return np.concatenate((pole, pipe)), np.concatenate((pole_n, pipe_n)), n_each


def half_cylinder(noise=0.0, seed=8, n=240):
    """Half of a cylinder's circumference about the axis through (0.5, -0.25, 0) along (0.1, 0.2, 1), radius 0.25."""
    rng = np.random.default_rng(seed)
    return cylinder((0.5, -0.25, 0.0), (0.1, 0.2, 1.0), 0.25, n, rng, arc=np.pi, noise=noise)


def with_non_finite(cloud, normals):
    """The case with a NaN point, an infinite point, a NaN normal and an infinite curvature planted in it."""
    cloud, normals = cloud.copy(), normals.copy()
    n = cloud.shape[0]
    cloud[n // 7, 0] = np.nan
    cloud[n // 3, 2] = np.inf
    normals[n // 5, 1] = np.nan
    normals[n // 2, 3] = np.inf
    return cloud, normals


POLES = ((3.0, 2.0, 0.10), (-2.5, 4.0, 0.15), (1.0, -3.5, 0.20))     # x, y, radius


@functools.lru_cache(maxsize=None)
def street(seed=1):
    """A synthetic street: a crowned ground, five boxes and three poles of radius 0.10 .. 0.20 m, 3 450 points; the normals
    are tests/normals_restated.py's over 12 neighbours with the viewpoint 3 m above the origin."""
    import normals_restated as NR
    rng = np.random.default_rng(seed)
    g = np.stack((rng.uniform(-6, 6, 1500), rng.uniform(-6, 6, 1500)), axis=1)
    ground = np.concatenate((g, (0.05 - 0.002 * g[:, :1] ** 2) + rng.normal(0, 0.004, (1500, 1))), axis=1)
    parts = [ground]
    for cx, cy in ((-4, -4), (4, 4), (-4, 2), (4.5, -2), (0, 5)):
        u, v, f = rng.uniform(-0.5, 0.5, 150), rng.uniform(0, 1.2, 150), rng.integers(0, 4, 150)
        bx = np.where(f < 2, u, np.where(f == 2, -0.5, 0.5))
        by = np.where(f < 2, np.where(f == 0, -0.5, 0.5), u)
        parts.append(np.stack((cx + bx, cy + by, v), axis=1))
    for x, y, r in POLES:
        phi, z = rng.uniform(0, 2 * np.pi, 400), rng.uniform(0.0, 2.5, 400)
        rr = r + rng.normal(0, 0.002, 400)
        parts.append(np.stack((x + rr * np.cos(phi), y + rr * np.sin(phi), z), axis=1))
    cloud = rows(np.concatenate(parts))
    normals = NR.estimate(cloud, None, k=12, viewpoint=(0.0, 0.0, 3.0))[0]
    return cloud, normals
