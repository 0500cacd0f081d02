"""The C++ shim's region growing (include/icpgpu_registration.hpp: icpgpu::RegionGrowing) with PCL's spelling of every call:
tests/cpp/region_demo.cpp runs VoxelGrid -> NormalEstimation -> RegionGrowing -> extract on a ground plane with five boxes standing on
it.  The ground must come out as one region and every box face as a region of its own -- where EuclideanClusterExtraction at twice the
leaf size leaves boxes and ground in one component -- and the regions must be the restatement's for the demo's own cloud and normals."""
import math
import os
import subprocess

import numpy as np
import pytest

import region_restated as R
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS = [(-7.0, -6.0), (-3.0, 5.0), (2.0, -2.0), (6.0, 6.0), (8.0, -7.0)]
SIDES = ((0, -1), (0, 1), (1, -1), (1, 1))      # (axis, sign) of a box's four standing faces; face 4 is its top


def street_scene(seed=4) -> np.ndarray:
    """A 24 m x 24 m patch of ground (z = 0 within a centimetre) and the SURFACES of five boxes of 1.2 m x 1.2 m x 1.8 m standing on it:
    four sides and the top each, within half a centimetre."""
    r = np.random.default_rng(seed)
    parts = [np.concatenate([r.uniform(-12, 12, (30000, 2)), r.normal(0, 0.01, (30000, 1))], axis=1)]
    for centre in OBJECTS:
        for axis, sign in SIDES:
            p = np.zeros((1500, 3))
            p[:, axis] = sign * 0.6 + r.normal(0, 0.005, 1500) + centre[axis]
            p[:, 1 - axis] = r.uniform(-0.6, 0.6, 1500) + centre[1 - axis]
            p[:, 2] = r.uniform(0.0, 1.8, 1500)
            parts.append(p)
        parts.append(np.concatenate([r.uniform(-0.6, 0.6, (1000, 2)) + centre, 1.8 + r.normal(0, 0.005, (1000, 1))], axis=1))
    cloud = np.ones((sum(len(p) for p in parts), 4), np.float32)
    cloud[:, :3] = r.permutation(np.concatenate(parts)).astype(np.float32)
    return cloud


def surface_of(cloud, edge=0.15) -> np.ndarray:
    """Per point: 0 the ground away from the boxes, 1 + 5 b + f face f of box b away from its edges, -1 the rest."""
    s = np.full(len(cloud), -1)
    x, y, z = (cloud[:, a].astype(np.float64) for a in range(3))
    by_a_box = np.zeros(len(cloud), bool)
    for b, (cx, cy) in enumerate(OBJECTS):
        d = (x - cx, y - cy)
        near = (abs(d[0]) < 0.9) & (abs(d[1]) < 0.9)
        by_a_box |= near
        for f, (axis, sign) in enumerate(SIDES):
            s[near & (abs(d[axis] - sign * 0.6) < 0.05) & (abs(d[1 - axis]) < 0.6 - edge) & (z > edge) & (z < 1.8 - edge)] = 1 + 5 * b + f
        s[near & (z > 1.7) & (abs(d[0]) < 0.6 - edge) & (abs(d[1]) < 0.6 - edge)] = 1 + 5 * b + 4
    s[~by_a_box & (abs(z) < 0.1)] = 0
    return s


def _build(tmp_path):
    exe = tmp_path / "region_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "region_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


def ints(line):
    return [] if line == "-" else [int(v) for v in line.split()]


def floats(line):
    words = line.split()
    return np.array([int(w, 16) for w in words[1:]], np.uint32).view(np.float32).reshape(int(words[0]), 4)


@pytest.mark.gpu
def test_demo_separates_the_faces_where_the_distance_does_not(built, ctx, tmp_path):
    exe = _build(tmp_path)
    raw = street_scene()
    a = tmp_path / "cloud.bin"
    raw.tofile(a)
    leaf, k_normals, k, degrees, curvature, lo = 0.15, 20, 30, 30.0, 0.05, 20
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(leaf), str(k_normals), str(k), str(degrees), str(curvature), str(lo), str(2 * leaf)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    cloud, normals = floats(lines[0]), floats(lines[1])
    m = len(cloud)
    assert cloud.tobytes() == ctx.voxel_grid(raw, leaf).tobytes() and 20000 < m < len(raw) and len(normals) == m
    # the restatement's regions of the demo's own cloud and normals (theta travels as a float, as in PCL)
    cos = R.smoothness_cos(np.float32(degrees / 180.0 * math.pi))
    start, indices, labels, _, _, _ = R.grow(cloud, normals, k, cos, np.float32(curvature), lo, 1000000)
    n_regions = int(lines[2])
    assert n_regions == start.size - 1
    for q in range(n_regions):
        assert ints(lines[3 + q]) == indices[start[q]:start[q + 1]].tolist()
    assert ints(lines[3 + n_regions]) == labels.tolist()
    # the ground is one region, every face of every box a region of its own
    surface = surface_of(cloud)
    homes = []
    for s in range(1 + 5 * len(OBJECTS)):
        on = labels[surface == s]
        assert on.size >= 50 and (on == on[0]).all() and on[0] >= 0, s
        homes.append(int(on[0]))
    assert homes[0] == 0 and len(set(homes)) == len(homes)
    # getSegmentFromPoint agrees with extract
    at = 4 + n_regions
    for i in range(0, m, 97):
        head, _, rest = lines[at].partition(": ")
        assert int(head) == i
        assert ints(rest) == ([] if labels[i] < 0 else indices[start[labels[i]]:start[labels[i] + 1]].tolist())
        at += 1
    # ... where the distance alone leaves every box and the ground in one component
    sizes = ints(lines[at])
    assert sizes[0] > m - 10 and (surface >= 0).sum() > 0.9 * m
