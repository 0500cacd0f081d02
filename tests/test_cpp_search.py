"""The C++ shim's neighbour search (include/icpgpu_registration.hpp: icpgpu::search::KdTree, icpgpu::KdTreeFLANN) with PCL's
spelling of every call: tests/cpp/search_demo.cpp must print the restatement's rows for its single-point, by-index and batched
calls."""
import os
import subprocess

import numpy as np
import pytest

import search_restated as R
from icpslam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = tmp_path / "search_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "search_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


def ints(line):
    return [] if line == "-" else [int(v) for v in line.split()]


def floats(line):
    return np.array([] if line == "-" else [np.float32(v) for v in line.split()], np.float32)


@pytest.mark.gpu
def test_demo_matches_the_restatement(built, tmp_path):
    exe = _build(tmp_path)
    scene = synth.make_scene(3)
    cloud = synth.scan(scene, np.eye(4), 3000, 5).copy()
    cloud[11, 0] = np.nan
    queries = synth.scan(scene, np.eye(4), 37, 9).copy()
    queries[5, 1] = np.inf
    a, b = tmp_path / "cloud.bin", tmp_path / "queries.bin"
    cloud.tofile(a)
    queries.tofile(b)
    k, radius, max_nn, index = 12, 0.8, 5, 1234
    r = subprocess.run([str(exe), str(a), str(len(cloud)), str(b), str(len(queries)), str(k), str(radius), str(max_nn), str(index)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    q1 = np.concatenate([queries[:1], cloud[index:index + 1]])
    q1[:, 3] = 1.0
    widx, wd2, wn = R.knn(cloud, q1, k)
    for row in (0, 1):
        assert ints(lines[2 * row]) == widx[row, :wn[row]].tolist()
        assert floats(lines[2 * row + 1]).tobytes() == wd2[row, :wn[row]].tobytes()
    assert widx[1, 0] == index
    rs, ridx, rd2 = R.radius(cloud, q1[:1], radius, 0)
    assert ints(lines[4]) == ridx.tolist() and floats(lines[5]).tobytes() == rd2.tobytes() and len(ridx) > max_nn
    rs2, ridx2, rd22 = R.radius(cloud, q1[1:], radius, max_nn)
    assert ints(lines[6]) == ridx2.tolist() and floats(lines[7]).tobytes() == rd22.tobytes() and len(ridx2) == max_nn
    assert ints(lines[8]) == [k, k, len(ridx), max_nn]
    widx, wd2, wn = R.knn(cloud, queries, k)
    assert ints(lines[9]) == wn.tolist() and wn[5] == 0
    assert ints(lines[10]) == widx.reshape(-1).tolist()
    assert floats(lines[11]).tobytes() == wd2.reshape(-1).tobytes()
    rs, ridx, rd2 = R.radius(cloud, queries, radius, max_nn)
    assert ints(lines[12]) == rs.tolist() and ints(lines[13]) == ridx.tolist() and floats(lines[14]).tobytes() == rd2.tobytes()
