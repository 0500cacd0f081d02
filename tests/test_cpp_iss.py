"""The C++ shim's ISS keypoints (include/icpgpu_registration.hpp: icpgpu::ISSKeypoint3D) with PCL's spelling of every call:
tests/cpp/iss_demo.cpp runs VoxelGrid -> ISSKeypoint3D -> NormalEstimation -> FPFHEstimation at the keypoints over the filtered surface,
on a ground plane with boxes.  Its indices and keypoints must be the restatement's over the filtered cloud it prints, bit for bit; no
keypoint may lie in a plane's interior, every box must contribute one, and the signatures at the keypoints must be fpfh_restated's."""
import os
import subprocess

import numpy as np
import pytest

import fpfh_restated as FR
import iss_restated as R
import normals_restated as N
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LEAF, ARGS, NORMALS_K, FPFH_RADIUS = 0.1, (0.45, 0.3, 0.975, 0.975, 5), 12, 0.35
# (centre x, y; half sizes x, y; height; yaw)
BOXES = ((1.5, 1.6, 0.5, 0.35, 0.8, 0.3), (4.4, 1.4, 0.3, 0.6, 1.1, -0.5), (3.0, 4.3, 0.7, 0.4, 0.6, 1.1))
GROUND = 6.0


def _build(tmp_path):
    exe = tmp_path / "iss_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "iss_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to link without icpgpu_iss_keypoints in the library."""
    assert _build(tmp_path).exists()


def parse(line, width):
    words = line.split()
    return int(words[0]), np.array([int(w, 16) for w in words[1:]], np.uint32).view(F32).reshape(-1, width)


def box_frame(box, xyz):
    """The points in the box's own frame: (along x, along y, z), the centre of its footprint at the origin."""
    cx, cy, _, _, _, yaw = box
    c, s = np.cos(yaw), np.sin(yaw)
    dx, dy = xyz[:, 0] - cx, xyz[:, 1] - cy
    return np.stack([c * dx + s * dy, -s * dx + c * dy, xyz[:, 2]], -1)


def scene(step=0.04):
    """A 6 m x 6 m ground lattice at z = 0 and three boxes standing on it (four walls and a lid each, no two alike, each turned about
    z by an angle of its own), sampled every 4 cm, as a raw cloud in a fixed random order."""
    g = np.arange(0, GROUND + 1e-9, step)
    parts = [np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3)]
    for cx, cy, hx, hy, height, yaw in BOXES:
        u, v, w = np.arange(-hx, hx + 1e-9, step), np.arange(-hy, hy + 1e-9, step), np.arange(step, height + 1e-9, step)
        faces = [np.stack(np.meshgrid(u, v, [w[-1]], indexing="ij"), -1).reshape(-1, 3)]
        for side in (-hx, hx):
            faces.append(np.stack(np.meshgrid([side], v, w, indexing="ij"), -1).reshape(-1, 3))
        for side in (-hy, hy):
            faces.append(np.stack(np.meshgrid(u, [side], w, indexing="ij"), -1).reshape(-1, 3))
        local = np.unique(np.concatenate(faces).round(9), axis=0)
        c, s = np.cos(yaw), np.sin(yaw)
        parts.append(np.stack([cx + c * local[:, 0] - s * local[:, 1], cy + s * local[:, 0] + c * local[:, 1], local[:, 2]], -1))
    raw = np.ones((sum(map(len, parts)), 4), F32)
    raw[:, :3] = np.concatenate(parts).astype(F32)
    return raw[np.random.default_rng(1).permutation(len(raw))]


def plane_interior(xyz, margin):
    """True where a point lies on the ground or on a box's face with nothing else -- no other face, no box, no border of the ground --
    within `margin` of it: its ball of that radius is a piece of one plane."""
    inside = np.zeros(len(xyz), bool)
    near_box = np.zeros(len(xyz), bool)
    for box in BOXES:
        _, _, hx, hy, height, _ = box
        p = box_frame(box, xyz)
        ax, ay = np.abs(p[:, 0]), np.abs(p[:, 1])
        near_box |= (ax <= hx + margin) & (ay <= hy + margin) & (p[:, 2] <= height + margin)
        tol = 0.06                                                   # (a voxel's centroid lies within half a leaf of its face)
        on_lid = (np.abs(p[:, 2] - height) <= tol) & (ax <= hx - margin) & (ay <= hy - margin)
        on_x = (np.abs(ax - hx) <= tol) & (ay <= hy - margin) & (p[:, 2] >= margin) & (p[:, 2] <= height - margin)
        on_y = (np.abs(ay - hy) <= tol) & (ax <= hx - margin) & (p[:, 2] >= margin) & (p[:, 2] <= height - margin)
        inside |= on_lid | on_x | on_y
    on_ground = (xyz[:, 2] == 0) & ~near_box & (np.minimum(xyz[:, :2].min(axis=1), GROUND - xyz[:, :2].max(axis=1)) >= margin)
    return inside | on_ground


@pytest.mark.gpu
def test_demo_matches_the_restatement_and_finds_the_boxes(built, tmp_path):
    exe = _build(tmp_path)
    raw = scene()
    a = tmp_path / "raw.bin"
    raw.tofile(a)
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(LEAF)] + [str(v) for v in ARGS] + [str(NORMALS_K), str(FPFH_RADIUS)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")
    n_f, filtered = parse(lines[0], 4)
    assert n_f == len(filtered) and 3000 < n_f < len(raw) // 3
    want = R.keypoints(filtered, *ARGS)
    index = np.array(lines[1].split()[1:], np.int32)
    assert int(lines[1].split()[0]) == index.size == want["n_keypoints"] and np.array_equal(index, want["keypoint_index"])
    width, keypoints = parse(lines[2], 4)
    assert width == index.size and np.array_equal(keypoints.view(np.uint32), want["keypoints"].view(np.uint32))
    assert np.array_equal(keypoints.view(np.uint32), filtered[index].view(np.uint32))
    # no keypoint inside a plane; every box found
    interior = plane_interior(filtered[:, :3].astype(np.float64), ARGS[0] + 0.06)
    assert interior.sum() > n_f // 4 and not interior[index].any()
    for box in BOXES:
        p = box_frame(box, keypoints[:, :3].astype(np.float64))
        at_box = (np.abs(p[:, 0]) <= box[2] + 0.15) & (np.abs(p[:, 1]) <= box[3] + 0.15)
        assert at_box.sum() >= 1, box
    assert 3 <= index.size < n_f // 10
    # the descriptors at the keypoints
    dense, normals = parse(lines[3], 4)
    assert dense == 1 and np.array_equal(normals.view(np.uint32), N.estimate(filtered, None, k=NORMALS_K)[0].view(np.uint32))
    dense, at_keys = parse(lines[4], 33)
    assert dense == 1 and np.array_equal(at_keys.view(np.uint32), FR.estimate(filtered, normals, keypoints, radius=FPFH_RADIUS)[0].view(np.uint32))
