"""The C++ shim's ground removal (include/icpgpu_registration.hpp: icpgpu::SACSegmentation, icpgpu::ModelCoefficients,
icpgpu::ExtractIndices) with PCL's spelling of every call: tests/cpp/sac_demo.cpp runs VoxelGrid -> SACSegmentation ->
ExtractIndices(negative) -> EuclideanClusterExtraction on a synthetic street scene.  The objects must come out as separate clusters,
the same scene without the ground removal as one component, and the plane must be the restatement's plane of the filtered cloud."""
import os
import subprocess

import numpy as np
import pytest

import sac_restated as R
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS = ((-6.0, -5.0), (-1.0, 4.0), (4.0, -4.0), (7.0, 5.0), (0.5, -7.5))       # the footprints' centres, metres apart


def street_scene(seed=4) -> np.ndarray:
    """A 24 m x 24 m patch of ground (z = 0 within a centimetre) and five boxes of 1.2 m x 1.2 m x 1.8 m standing on it."""
    r = np.random.default_rng(seed)
    ground = np.concatenate([r.uniform(-12, 12, (30000, 2)), r.normal(0, 0.01, (30000, 1))], axis=1)
    boxes = [np.concatenate([r.uniform(-0.6, 0.6, (900, 2)) + c, r.uniform(0, 1.8, (900, 1))], axis=1) for c in OBJECTS]
    cloud = np.ones((30000 + 900 * len(OBJECTS), 4), np.float32)
    cloud[:, :3] = r.permutation(np.concatenate([ground] + boxes)).astype(np.float32)
    return cloud


def _build(tmp_path):
    exe = tmp_path / "sac_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sac_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_demo_separates_the_objects_and_matches_the_restatement(built, ctx, tmp_path):
    exe = _build(tmp_path)
    raw = street_scene()
    a = tmp_path / "cloud.bin"
    raw.tofile(a)
    leaf, threshold, seed, tolerance, min_size = 0.2, 0.15, 7, 0.5, 20
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(leaf), str(threshold), str(seed), str(tolerance), str(min_size), str(len(OBJECTS))],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr, r.stdout[-400:])
    lines = r.stdout.split("\n")
    words = lines[0].split()
    m = int(words[0])
    filtered = np.array([int(w, 16) for w in words[1:]], np.uint32).view(np.float32).reshape(m, 4)
    assert filtered.tobytes() == ctx.voxel_grid(raw, leaf).tobytes() and 5000 < m < len(raw)
    want = R.segment(filtered, threshold, 100, 0.99, seed, True)
    plane = lines[1].split()
    assert np.array([int(w, 16) for w in plane[:4]], np.uint32).view(np.float32).tobytes() == want["coeff"].tobytes()
    assert (int(plane[4]), int(plane[5])) == (want["iterations"], want["inliers"].size)
    assert [int(v) for v in lines[2].split()] == want["inliers"].tolist()
    assert abs(want["coeff"][2]) > 0.999 and abs(want["coeff"][3]) < 0.05            # the ground
    n_left, n_clusters = (int(v) for v in lines[3].split())
    assert n_left == m - want["inliers"].size and n_clusters == len(OBJECTS)
    seen = set()
    for k in range(n_clusters):                                                      # every cluster inside one object's footprint
        size, x0, x1, y0, y1 = (float(v) for v in lines[4 + k].split())
        inside = [j for j, (cx, cy) in enumerate(OBJECTS) if cx - 0.8 <= x0 and x1 <= cx + 0.8 and cy - 0.8 <= y0 and y1 <= cy + 0.8]
        assert len(inside) == 1 and size >= min_size
        seen.add(inside[0])
    assert seen == set(range(len(OBJECTS)))
    assert [int(v) for v in lines[4 + n_clusters].split()] == [m]                    # without the ground removal: one component
