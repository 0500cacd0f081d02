"""The C++ shim's cropping and sampling filters (include/icpgpu_registration.hpp: icpgpu::PassThrough, CropBox, UniformSampling,
FarthestPointSampling) with PCL's spelling of every call: tests/cpp/sampling_demo.cpp runs the front end of a descriptor pipeline on a
street scene -- PassThrough(z) -> CropBox(negative, the vehicle's own box) -> VoxelGrid -> NormalEstimation -> UniformSampling ->
FPFHEstimation at the sampled points over the filtered surface -- and FarthestPointSampling over the same surface."""
import os
import subprocess

import numpy as np
import pytest

import sampling_cases as SC
import sampling_restated as R
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
Z_LIMITS = (-2.5, 3.0)


def _build(tmp_path):
    exe = tmp_path / "sampling_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sampling_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to link without the cropping and sampling entry points in the library."""
    assert _build(tmp_path).exists()


def street_scene(seed=4) -> np.ndarray:
    """A 24 m x 24 m patch of ground 1.8 m below the sensor, five boxes standing on it, the returns of the vehicle's own body inside
    its box, a few returns far above the range, and two rows that are not finite."""
    r = np.random.default_rng(seed)
    parts = [np.concatenate([r.uniform(-12, 12, (9000, 2)), r.normal(-1.8, 0.01, (9000, 1))], axis=1)]
    for c in ((5, 5), (-6, 3), (7, -4), (-3, -7), (0, 8)):
        parts.append(np.concatenate([r.uniform(-0.6, 0.6, (500, 2)) + c, r.uniform(-1.8, 0.0, (500, 1))], axis=1))
    parts.append(r.uniform(SC.EGO_MIN, SC.EGO_MAX, (400, 3)))                       # the vehicle itself
    parts.append(np.concatenate([r.uniform(-12, 12, (60, 2)), r.uniform(3.5, 9.0, (60, 1))], axis=1))   # overhead returns
    cloud = SC.rows(r.permutation(np.concatenate(parts)))
    cloud[[17, 4000], :3] = F32([[np.nan, 1, 1], [2, np.inf, 0]])
    return cloud


def parse_cloud(line):
    words = line.split()
    return int(words[0]), np.array([int(w, 16) for w in words[1:]], np.uint32).view(F32).reshape(-1, 4)


@pytest.mark.gpu
def test_demo_crops_samples_and_describes(built, tmp_path):
    exe = _build(tmp_path)
    raw = street_scene()
    path = tmp_path / "raw.bin"
    raw.tofile(path)
    leaf, sample_leaf, normals_k, fpfh_radius, n_far, seed = 0.1, 1.5, 12, 0.4, 64, 7
    r = subprocess.run([str(exe), str(path), str(len(raw)), str(Z_LIMITS[0]), str(Z_LIMITS[1]), str(leaf), str(sample_leaf), str(normals_k),
                        str(fpfh_radius), str(n_far), str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")
    # the crop: the restatement's rows, none of them in the vehicle's box or outside the z range
    n_c, cropped = parse_cloud(lines[0])
    in_range = raw[R.pass_through(raw, 2, *Z_LIMITS)]
    want = in_range[R.crop_box(in_range, SC.EGO_MIN, SC.EGO_MAX, None, True)]
    assert n_c == len(cropped) and cropped.tobytes() == want.tobytes()
    assert 8000 < n_c <= len(raw) - 400 - 60                                      # (the ground under the vehicle goes with it)
    xyz = cropped[:, :3]
    assert np.isfinite(xyz).all() and (xyz[:, 2] >= F32(Z_LIMITS[0])).all() and (xyz[:, 2] <= F32(Z_LIMITS[1])).all()
    assert not ((xyz >= F32(SC.EGO_MIN)) & (xyz <= F32(SC.EGO_MAX))).all(axis=1).any()
    pass_removed, crop_removed = (np.array(part.split(), np.int64) for part in lines[1].split("|"))
    assert pass_removed.tolist() == R.removed_of(len(raw), R.pass_through(raw, 2, *Z_LIMITS)).tolist()
    assert crop_removed.tolist() == R.removed_of(len(in_range), R.crop_box(in_range, SC.EGO_MIN, SC.EGO_MAX, None, True)).tolist()
    # the sampled rows of the filtered surface: the restatement's, one signature each
    n_s, surface = parse_cloud(lines[2])
    assert n_s == len(surface) and 2000 < n_s < n_c
    key_index = np.array(lines[3].split(), np.int32)
    assert key_index.tolist() == R.uniform_sampling(surface, sample_leaf)[0].tolist() and 100 < len(key_index) < n_s // 4
    sig = lines[4].split()
    assert int(sig[0]) == len(key_index) and len(sig) == 1 + 33 * len(key_index)
    hist = np.array([int(w, 16) for w in sig[1:]], np.uint32).view(F32).reshape(-1, 3, 11)
    assert np.isfinite(hist).all() and (np.abs(hist.sum(axis=2) - 100.0) <= 1e-2).all(axis=1).mean() > 0.9
    # the farthest points: the restatement's from the seeded row, within twice the cover radius of 64 strided rows
    far_index = np.array(lines[5].split(), np.int32)
    assert far_index.tolist() == R.farthest_point_sampling(surface, n_far, R.seeded_first_row(surface, seed))[0].tolist()
    r_fps, r_strided = R.cover_radius(surface, far_index), R.cover_radius(surface, np.arange(n_far) * (n_s // n_far))
    print(f"cover radius: farthest point sampling {r_fps:.4f}, strided {r_strided:.4f}, ratio {r_fps / r_strided:.4f}")
    assert r_fps <= 2.0 * r_strided
