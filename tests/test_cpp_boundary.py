"""The C++ shim's boundary estimation and ISS border estimation (include/icpgpu_registration.hpp: icpgpu::BoundaryEstimation,
icpgpu::ISSKeypoint3DBorder) with PCL's spelling of every call: tests/cpp/boundary_demo.cpp runs VoxelGrid -> NormalEstimation ->
BoundaryEstimation -> ISSKeypoint3DBorder -> FPFHEstimation on tests/test_cpp_iss.py's ground plane with boxes, the ground rippled by
a centimetre: on an exact plane the smallest eigenvalue is 0 and plain ISS has no keypoint to lose, on the rippled one it places
keypoints along the patch's rim, where the ball is half empty.  Every output must be the restatements' over the filtered cloud it
prints, bit for bit; the ground patch's rim must come out as boundary, plain ISS's keypoints along that rim must be gone with the
border on, and every box must still contribute a keypoint."""
import os
import subprocess

import numpy as np
import pytest

import boundary_restated as B
import fpfh_restated as FR
import iss_border_restated as IB
import iss_restated as R
import normals_restated as N
import test_cpp_iss as TI
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LEAF, ARGS, NORMALS_K, BORDER_RADIUS, FPFH_RADIUS = TI.LEAF, TI.ARGS, TI.NORMALS_K, 0.3, TI.FPFH_RADIUS
HALF_PI = float(np.float32(np.pi / 2))                                          # the shim keeps PCL's float threshold
RIPPLE = 0.01


def scene():
    """tests/test_cpp_iss.py's scene with the ground lifted to z = 1 cm * sin(2 pi x / 1.3 m) * cos(2 pi y / 0.9 m)."""
    raw = TI.scene().copy()
    ground = raw[:, 2] == 0
    x, y = raw[ground, 0].astype(np.float64), raw[ground, 1].astype(np.float64)
    raw[ground, 2] = (RIPPLE * np.sin(2 * np.pi * x / 1.3) * np.cos(2 * np.pi * y / 0.9)).astype(F32)
    return raw


def check_scene(filtered, normals, flags, n_neighbours, plain, index, edge, border):
    """What the scene is for: the rim is boundary, the interiors are not, plain ISS's rim keypoints go, the boxes stay."""
    n_f = len(filtered)
    xyz = filtered[:, :3].astype(np.float64)
    ground = np.abs(xyz[:, 2]) <= RIPPLE + 1e-6
    to_rim = np.minimum(xyz[:, :2].min(axis=1), TI.GROUND - xyz[:, :2].max(axis=1))
    on_rim = ground & (to_rim <= LEAF / 2)                                      # the ground's outermost voxels
    margin = BORDER_RADIUS + 0.06
    off_boxes = np.ones(n_f, bool)
    for box in TI.BOXES:
        p = TI.box_frame(box, xyz)
        off_boxes &= ~((np.abs(p[:, 0]) <= box[2] + margin) & (np.abs(p[:, 1]) <= box[3] + margin))
    deep = TI.plane_interior(xyz, margin) | (ground & off_boxes & (to_rim >= margin))
    assert on_rim.sum() > 200 and flags[on_rim].all()
    assert deep.sum() > n_f // 4 and not flags[deep].any()
    assert np.array_equal(np.flatnonzero(flags.astype(bool) & (n_neighbours >= ARGS[4])), edge)   # the same rule over the same rows
    near_rim = ground & (to_rim <= BORDER_RADIUS - LEAF)                        # within the border radius of an outermost voxel
    assert near_rim[plain].sum() >= 4 and not near_rim[index].any()             # plain ISS's rim keypoints are gone
    assert np.isin(np.flatnonzero(near_rim), border).all()
    assert np.isin(np.setdiff1d(plain, index), border).all() and np.isin(index, plain).all()
    for box in TI.BOXES:                                                        # every box is still found
        p = TI.box_frame(box, xyz[index])
        at_box = (np.abs(p[:, 0]) <= box[2] + 0.15) & (np.abs(p[:, 1]) <= box[3] + 0.15)
        assert at_box.sum() >= 1, box


def _build(tmp_path):
    exe = tmp_path / "boundary_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "boundary_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to link without icpgpu_boundary_estimation and icpgpu_iss_keypoints_border in the library."""
    assert _build(tmp_path).exists()


def indices_of(line):
    words = line.split()
    assert int(words[0]) == len(words) - 1
    return np.array(words[1:], np.int32)


@pytest.mark.gpu
def test_demo_matches_the_restatements_and_clears_the_rim(built, tmp_path):
    exe = _build(tmp_path)
    raw = scene()
    a = tmp_path / "raw.bin"
    raw.tofile(a)
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(LEAF)] + [str(v) for v in ARGS] + [str(NORMALS_K), str(BORDER_RADIUS), str(FPFH_RADIUS)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")
    n_f, filtered = TI.parse(lines[0], 4)
    assert n_f == len(filtered) and 3000 < n_f < len(raw) // 3
    dense, normals = TI.parse(lines[1], 4)
    assert dense == 1 and np.array_equal(normals.view(np.uint32), N.estimate(filtered, None, k=NORMALS_K)[0].view(np.uint32))
    # the boundary flags, and the ground's rim among them
    flags = np.array(lines[2].split()[1:], np.uint8)
    want = B.estimate(filtered, None, normals, 0, BORDER_RADIUS, HALF_PI)
    assert flags.size == n_f and flags.tobytes() == want["boundary"].tobytes()
    # plain ISS, then with the border on
    plain = indices_of(lines[3])
    assert np.array_equal(plain, R.keypoints(filtered, *ARGS)["keypoint_index"])
    got = IB.keypoints_border(filtered, *ARGS, BORDER_RADIUS, HALF_PI, normals)
    index, edge, border = indices_of(lines[4]), indices_of(lines[5]), indices_of(lines[6])
    assert np.array_equal(index, got["keypoint_index"]) and np.array_equal(edge, np.flatnonzero(got["edge"]))
    assert np.array_equal(border, np.flatnonzero(got["border"]))
    check_scene(filtered, normals, flags, want["n_neighbours"], plain, index, edge, border)
    assert np.array_equal(indices_of(lines[7]), plain)                          # border radius 0: plain ISS
    dense, at_keys = TI.parse(lines[8], 33)
    assert dense == 1 and np.array_equal(at_keys.view(np.uint32), FR.estimate(filtered, normals, filtered[index], radius=FPFH_RADIUS)[0].view(np.uint32))
