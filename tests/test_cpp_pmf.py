"""The C++ shim's ground filter (include/icpgpu_registration.hpp: icpgpu::ProgressiveMorphologicalFilter,
icpgpu::applyMorphologicalOperator) with PCL's spelling of every call: tests/cpp/pmf_demo.cpp runs VoxelGrid ->
ProgressiveMorphologicalFilter -> ExtractIndices(negative) -> EuclideanClusterExtraction on a street scene whose ground is crowned and
rippled.  The five objects must come out as five clusters and the ground must be the restatement's ground of the filtered cloud; with
SACSegmentation in the filter's place at the same threshold they do not."""
import os
import subprocess

import numpy as np
import pytest

import pmf_restated as R
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS = ((-6.0, -5.0), (-1.0, 4.0), (4.0, -4.0), (7.0, 5.0), (0.5, -7.5))       # the footprints' centres, metres apart


def graded_street_scene(seed=4) -> np.ndarray:
    """A 24 m x 24 m street crowned along x = 0 with a 5 % grade to either side, a 5 cm ripple and a centimetre of noise, and five boxes
    of 1.2 m x 1.2 m x 1.8 m standing on it."""
    r = np.random.default_rng(seed)

    def street(x, y):
        return -0.05 * np.abs(x) + 0.05 * np.sin(1.3 * x) * np.cos(0.9 * y)
    xy = r.uniform(-12, 12, (12000, 2))
    parts = [np.concatenate([xy, (street(xy[:, 0], xy[:, 1]) + r.normal(0, 0.01, 12000))[:, None]], axis=1)]
    for c in OBJECTS:
        bxy = r.uniform(-0.6, 0.6, (500, 2)) + c
        parts.append(np.concatenate([bxy, (street(bxy[:, 0], bxy[:, 1]) + r.uniform(0, 1.8, 500))[:, None]], axis=1))
    cloud = np.ones((12000 + 500 * len(OBJECTS), 4), np.float32)
    cloud[:, :3] = r.permutation(np.concatenate(parts)).astype(np.float32)
    return cloud


def _build(tmp_path):
    exe = tmp_path / "pmf_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pmf_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_demo_separates_the_objects_where_the_plane_does_not(built, ctx, tmp_path):
    exe = _build(tmp_path)
    raw = graded_street_scene()
    a = tmp_path / "cloud.bin"
    raw.tofile(a)
    leaf, threshold, seed, tolerance, min_size = 0.3, 0.15, 7, 0.5, 20
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(leaf), str(threshold), str(seed), str(tolerance), str(min_size), str(len(OBJECTS))],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr, r.stdout[-400:])
    lines = r.stdout.split("\n")
    words = lines[0].split()
    m = int(words[0])
    filtered = np.array([int(w, 16) for w in words[1:]], np.uint32).view(np.float32).reshape(m, 4)
    assert filtered.tobytes() == ctx.voxel_grid(raw, leaf).tobytes() and 3000 < m < 9000
    want = R.run(filtered)
    assert [int(v) for v in lines[1].split()] == [5, want["ground"].size]
    assert [int(v) for v in lines[2].split()] == want["ground"].tolist()
    assert np.array([int(w, 16) for w in lines[3].split()], np.uint32).view(np.float32).tobytes() == R.operator(filtered, 3.0, R.OPEN).tobytes()
    n_left, n_clusters = (int(v) for v in lines[4].split())
    assert n_left == m - want["ground"].size and n_clusters == len(OBJECTS)
    seen = set()
    for k in range(n_clusters):                                                      # every cluster inside one object's footprint
        size, x0, x1, y0, y1 = (float(v) for v in lines[5 + k].split())
        inside = [j for j, (cx, cy) in enumerate(OBJECTS) if cx - 0.8 <= x0 and x1 <= cx + 0.8 and cy - 0.8 <= y0 and y1 <= cy + 0.8]
        assert len(inside) == 1 and size >= min_size
        seen.add(inside[0])
    assert seen == set(range(len(OBJECTS)))
    plane = [int(v) for v in lines[5 + n_clusters].split()]                          # inliers, points left, cluster sizes
    assert plane[0] + plane[1] == m and plane[0] < 0.8 * want["ground"].size         # the plane misses a fifth of the ground at least
    assert len(plane) - 2 != len(OBJECTS) and max(plane[2:]) > 1000                  # ... and what it leaves joins objects to ground
