"""The C++ shim's euclidean clustering (include/icpgpu_registration.hpp: icpgpu::EuclideanClusterExtraction, icpgpu::PointIndices)
with PCL's spelling of every call: tests/cpp/cluster_demo.cpp runs VoxelGrid -> EuclideanClusterExtraction -> extract and must print
the restatement's clusters of the filtered cloud."""
import os
import subprocess

import numpy as np
import pytest

import cluster_restated as R
from icpslam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = tmp_path / "cluster_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cluster_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


def ints(line):
    return [] if line == "-" else [int(v) for v in line.split()]


@pytest.mark.gpu
def test_demo_matches_the_restatement(built, ctx, tmp_path):
    exe = _build(tmp_path)
    raw = synth.scan(synth.make_scene(3), np.eye(4), 20000, 6).copy()
    raw[11, 0] = np.nan
    a = tmp_path / "cloud.bin"
    raw.tofile(a)
    leaf, tolerance, lo, hi = 0.4, 0.8, 3, 200
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(leaf), str(tolerance), str(lo), str(hi)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    words = lines[0].split()
    m = int(words[0])
    filtered = np.array([int(w, 16) for w in words[1:]], np.uint32).view(np.float32).reshape(m, 4)
    assert filtered.tobytes() == ctx.voxel_grid(raw, leaf).tobytes() and 1000 < m < len(raw)
    start, indices, labels, _ = R.extract(filtered, tolerance, lo, hi)
    n_clusters = int(lines[1])
    assert n_clusters == start.size - 1 and n_clusters > 3
    for k in range(n_clusters):
        assert ints(lines[2 + k]) == indices[start[k]:start[k + 1]].tolist()
    assert ints(lines[2 + n_clusters]) == labels.tolist()
    sizes = np.unique(R.components(filtered, tolerance), return_counts=True)[1]
    assert (sizes < lo).any() and (sizes > hi).any()  # the window cut on both sides
