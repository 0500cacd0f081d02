"""The C++ shim's moving least squares (include/icpgpu_registration.hpp: icpgpu::MovingLeastSquares) with PCL's spelling of every
call: tests/cpp/mls_demo.cpp runs VoxelGrid -> MovingLeastSquares -> NormalEstimation -> FPFHEstimation on the ground plane with boxes
of tests/test_cpp_iss.py, and the same chain without the smoothing beside it.  Its indices, points and normals must be the
restatement's over the filtered cloud it prints, bit for bit, and inside the planes the signatures must be the hand answer of
tests/test_cpp_fpfh.py for at least as many points as without MovingLeastSquares."""
import os
import subprocess

import numpy as np
import pytest

import mls_restated as R
import normals_restated as N
from icpslam_amd import _lib
from test_cpp_fpfh import SUM_TOL
from test_cpp_iss import plane_interior, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LEAF, SEARCH_RADIUS, ORDER, NORMALS_RADIUS, FPFH_RADIUS = 0.1, 0.25, 2, 0.2, 0.2


def _build(tmp_path):
    exe = tmp_path / "mls_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mls_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to link without icpgpu_moving_least_squares in the library."""
    assert _build(tmp_path).exists()


def parse(line, width):
    words = line.split()
    return int(words[0]), np.array([int(w, 16) for w in words[1:]], np.uint32).view(F32).reshape(-1, width)


def hand_answer(signatures):
    """True where a signature is the plane's: bins 5, 16 and 27 hold 100 each, the others nothing."""
    others = np.ones(33, bool)
    others[[5, 16, 27]] = False
    return ~signatures[:, others].any(axis=1) & (np.abs(signatures[:, [5, 16, 27]] - 100.0) <= SUM_TOL).all(axis=1)


@pytest.mark.gpu
def test_demo_matches_the_restatement_and_keeps_the_planes(built, tmp_path):
    exe = _build(tmp_path)
    raw = scene()
    a = tmp_path / "raw.bin"
    raw.tofile(a)
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(LEAF), str(SEARCH_RADIUS), str(ORDER), str(NORMALS_RADIUS), str(FPFH_RADIUS)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")
    n_f, filtered = parse(lines[0], 4)
    assert n_f == len(filtered) and 3000 < n_f < len(raw) // 3
    want = R.project(filtered, None, SEARCH_RADIUS, ORDER)
    index = np.array(lines[1].split()[1:], np.int32)
    assert int(lines[1].split()[0]) == index.size == want["n_out"] and np.array_equal(index, want["index"])
    width, smoothed = parse(lines[2], 7)
    assert width == index.size == n_f                                            # every point of this scene has three neighbours
    assert np.array_equal(smoothed[:, :3].view(np.uint32), np.ascontiguousarray(want["points"][:, :3]).view(np.uint32))
    assert np.array_equal(smoothed[:, 3:].view(np.uint32), want["normals"].view(np.uint32))
    assert (want["status"] == 2).sum() > n_f // 2
    # the descriptors over the smoothed cloud
    surface = np.ones((n_f, 4), F32)
    surface[:, :3] = smoothed[:, :3]
    dense, normals = parse(lines[3], 4)
    assert np.array_equal(normals.view(np.uint32), N.estimate(surface, None, radius=NORMALS_RADIUS)[0].view(np.uint32))
    _, with_mls = parse(lines[4], 33)
    _, without = parse(lines[5], 33)
    assert len(with_mls) == len(without) == n_f
    # inside a plane -- everything a signature reads lies on it -- the smoothing moves nothing, and the hand answer survives
    interior = plane_interior(filtered[:, :3].astype(np.float64), SEARCH_RADIUS + NORMALS_RADIUS + 2 * FPFH_RADIUS + 0.06)
    on_ground = interior & (filtered[:, 2] == 0)
    assert on_ground.sum() > 150 and np.array_equal(smoothed[on_ground, :3].view(np.uint32), np.ascontiguousarray(filtered[on_ground, :3]).view(np.uint32))
    kept, before = hand_answer(with_mls) & interior, hand_answer(without) & interior
    print("plane-interior points", int(interior.sum()), "hand answers with MLS", int(kept.sum()), "without", int(before.sum()))
    assert before[on_ground].all() and kept.sum() >= before.sum() >= on_ground.sum()
