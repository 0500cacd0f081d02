"""The C++ shim's normal estimation (include/icpgpu_registration.hpp: icpgpu::NormalEstimation) with PCL's spelling of every call:
tests/cpp/normals_demo.cpp must print the restatement's normals in both modes and over a search surface, and its chain
NormalEstimation -> setTargetNormals -> IterativeClosestPointWithNormals::align must give the transform a Python Context gives with
the same normals handed to set_target_normals."""
import os
import subprocess

import numpy as np
import pytest

import normals_restated as R
from icpslam_amd import P2PLANE, Context, _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = tmp_path / "normals_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "normals_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to link without icpgpu_normal_estimation in the library."""
    assert _build(tmp_path).exists()


def parse(line):
    words = line.split()
    return int(words[0]), np.array([int(w, 16) for w in words[1:]], np.uint32).view(np.float32).reshape(-1, 4)


@pytest.mark.gpu
def test_demo_matches_the_restatement_and_the_python_chain(built, tmp_path):
    exe = _build(tmp_path)
    src, tgt, _ = synth.make_pair(1500, 1500, seed=7)
    surface = synth.scan(synth.make_scene(3), np.eye(4), 3000, 5).copy()
    surface[11, 0] = np.nan
    a, b, c = tmp_path / "tgt.bin", tmp_path / "surface.bin", tmp_path / "src.bin"
    tgt.tofile(a)
    surface.tofile(b)
    src.tofile(c)
    k, radius, vp, iters = 12, 0.25, (0.5, -1.0, 2.0), 10
    r = subprocess.run([str(exe), str(a), str(len(tgt)), str(b), str(len(surface)), str(k), str(radius)] + [str(v) for v in vp]
                       + [str(c), str(len(src)), str(iters)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")
    by_k = R.estimate(tgt, None, k=k, viewpoint=vp)[0]
    by_r = R.estimate(tgt, None, radius=radius, viewpoint=vp)[0]
    over = R.estimate(surface, tgt, k=k, viewpoint=vp)[0]
    assert np.isnan(by_r).any() and not np.isnan(by_r).all()  # the radius leaves some points without three neighbours: is_dense = 0
    for line, want in zip(lines, (by_k, by_r, over)):
        dense, got = parse(line)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert dense == int(not np.isnan(want).any())
    with Context(0) as ctx:
        ctx.set_params(method=P2PLANE, max_iterations=iters, transformation_epsilon=1e-6, max_correspondence_distance=1.0)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_target_normals(by_k)
        want = ctx.align()
    words = lines[3].split()
    assert int(words[0]) == int(want["converged"]) and int(words[1]) == want["iterations"] and want["iterations"] > 1
    T = np.array([np.float32(w) for w in words[2:]], np.float32).reshape(4, 4).T
    assert T.tobytes() == np.asarray(want["T"], np.float32).tobytes()
