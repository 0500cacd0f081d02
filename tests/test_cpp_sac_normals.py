"""The C++ shim's segmentation from normals (include/icpgpu_registration.hpp: icpgpu::SACSegmentationFromNormals) with PCL's spelling
of every call: tests/cpp/sac_normals_demo.cpp runs VoxelGrid -> NormalEstimation -> SACSegmentationFromNormals(NORMAL_PLANE) ->
ExtractIndices(negative) -> NormalEstimation -> SACSegmentationFromNormals(CYLINDER, a vertical axis, radius limits) on the street
with poles.  The ground comes out, the cylinder is one of the poles within the bounds measured on the host
(tests/test_sac_normals_host.py::test_the_street_end_to_end), and both results equal the restatement's."""
import math
import os
import subprocess

import numpy as np
import pytest

import normals_restated as NR
import sac_normals_cases as CS
import sac_normals_restated as R
import sac_restated as SR
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = tmp_path / "sac_normals_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sac_normals_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


def hex_floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


@pytest.mark.gpu
def test_demo_finds_the_ground_and_a_pole_and_matches_the_restatement(built, ctx, tmp_path):
    exe = _build(tmp_path)
    raw = CS.street(1)[0]
    a = tmp_path / "cloud.bin"
    raw.tofile(a)
    leaf, k, plane_thr, cyl_thr, rmin, rmax, eps, seed = 0.01, 12, 0.08, 0.03, 0.05, 0.3, 0.1, 1
    r = subprocess.run([str(exe), str(a), str(len(raw))] + [str(v) for v in (leaf, k, plane_thr, cyl_thr, rmin, rmax, eps, seed)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr, r.stdout[-400:])
    lines = r.stdout.split("\n")
    words = lines[0].split()
    m = int(words[0])
    filtered = hex_floats(words[1:]).reshape(m, 4)
    assert filtered.tobytes() == ctx.voxel_grid(raw, leaf).tobytes() and 3000 < m <= len(raw)
    normals = NR.estimate(filtered, None, k=k, viewpoint=(0.0, 0.0, 3.0))[0]
    want = R.segment(R.NORMAL_PLANE, filtered, normals, plane_thr, 0.1, 0.0, 0.0, 100, 0.99, seed, True)
    words = lines[1].split()
    assert hex_floats(words[:4]).tobytes() == want["coeff"].tobytes()
    assert (int(words[4]), int(words[5])) == (want["iterations"], want["inliers"].size)
    assert [int(v) for v in lines[2].split()] == want["inliers"].tolist()
    assert abs(want["coeff"][2]) > 0.999 and want["inliers"].size >= 1400                # the ground
    rest = SR.extract(filtered, want["inliers"], True)
    rest_normals = NR.estimate(rest, None, k=k, viewpoint=(0.0, 0.0, 3.0))[0]
    words = lines[3].split()
    co = hex_floats(words[:7])
    # the unrefined stages are the restatement's bit for bit; the refined coefficients stand on the device's double-double sums, so
    # they are held to the restatement's within float32 rounding of a coefficient of this size and to the host-measured bounds
    cyl = R.segment(R.CYLINDER, rest, rest_normals, cyl_thr, 0.1, rmin, rmax, 1000, 0.99, seed, True, (0, 0, 1), eps)
    assert int(words[7]) == cyl["iterations"]
    assert np.abs(co.astype(np.float64) - cyl["coeff"].astype(np.float64)).max() <= 4 * 2.0 ** -23 * 4.0
    got_inliers = np.array([int(v) for v in lines[4].split()])
    assert np.array_equal(got_inliers, np.flatnonzero(R.inlier_mask(R.CYLINDER, rest, rest_normals, co, cyl_thr, 0.1)))
    assert int(words[8]) == got_inliers.size > 300
    centre, radius = min((math.hypot(co[0] - x, co[1] - y), rr) for x, y, rr in CS.POLES)
    assert centre <= 2e-3 and abs(co[6] - radius) <= 1e-3 and math.degrees(math.acos(min(1.0, abs(float(co[5]))))) <= 0.25
