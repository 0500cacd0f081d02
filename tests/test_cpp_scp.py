"""The C++ shim's global registration (include/icpgpu_registration.hpp: icpgpu::SampleConsensusPrerejective, icpgpu::FeatureKdTree)
with PCL's spelling of every call: tests/cpp/scp_demo.cpp runs NormalEstimation -> FPFHEstimation -> SampleConsensusPrerejective ->
IterativeClosestPoint on the end-to-end scene.  The alignment must be the Python front end's over the signatures the demo prints, bit
for bit, within the scene's two bounds of the truth, and ICP from it must end on the truth."""
import os
import subprocess

import numpy as np
import pytest

import scp_restated as R
import scp_scenes as S
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _build(tmp_path):
    exe = tmp_path / "scp_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scp_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to link without icpgpu_feature_knn and icpgpu_scp_align in the library."""
    assert _build(tmp_path).exists()


def words(line, width, skip=0):
    w = line.split()
    return [int(v) for v in w[:skip]], np.array([int(v, 16) for v in w[skip:]], np.uint32).view(F32).reshape(-1, width)


@pytest.mark.gpu
def test_demo_relocalises_and_matches_the_python_front_end(built, ctx, tmp_path):
    exe = _build(tmp_path)
    source, target, truth = S.e2e_clouds()
    a, b = tmp_path / "source.bin", tmp_path / "target.bin"
    source.tofile(a)
    target.tofile(b)
    E, seed = S.E2E, S.E2E_SEEDS[0]
    r = subprocess.run([str(exe), str(a), str(len(source)), str(b), str(len(target)), str(S.E2E_NORMAL_K), str(S.E2E_FPFH_RADIUS), str(E["nr"]),
                        str(E["kc"]), str(E["similarity"]), str(E["distance"]), str(E["fraction"]), str(E["max_iterations"]), str(seed)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr, r.stdout[-400:])
    lines = r.stdout.split("\n")
    (dense_s,), sf = words(lines[0], 33, 1)
    (dense_t,), tf = words(lines[1], 33, 1)
    assert dense_s == dense_t == 1 and sf.shape == tf.shape == (1500, 33)
    ctx.search_set_input(target)                                                       # the Python front end over the demo's own signatures
    similarity, fraction = float(F32(E["similarity"])), float(F32(E["fraction"]))      # (setSimilarityThreshold / setInlierFraction take floats)
    want = ctx.scp_align(source, sf, tf, nr_samples=E["nr"], k_correspondences=E["kc"], similarity_threshold=similarity,
                         max_correspondence_distance=E["distance"], inlier_fraction=fraction, max_iterations=E["max_iterations"], seed=seed)
    (converged, n_inliers), rest = words(lines[2], 17, 2)
    fitness, T = rest[0, 0], rest[0, 1:].reshape(4, 4).T
    assert converged == 1 == int(want["converged"]) and n_inliers == want["inliers"].size and fitness == F32(want["fitness"])
    assert T.tobytes() == want["T"].tobytes()
    assert [int(v) for v in lines[3].split()] == want["inliers"].tolist()
    assert words(lines[4], 4)[1].tobytes() == want["cloud"].tobytes()
    rot, trans = S.pose_error(T, truth)
    assert rot <= 2.0 and trans <= E["distance"]
    rows = R.feature_knn(tf, sf, E["kc"])[0]                                           # the feature tree against the restatement
    assert [int(v) for v in lines[5].split()] == rows.reshape(-1).tolist()
    assert [int(v) for v in lines[6].split()] == [E["kc"]] + rows[0].tolist()
    (icp_converged,), Ti = words(lines[7], 16, 1)
    Ti = Ti.reshape(4, 4).T.astype(np.float64)
    assert icp_converged == 1 and np.abs(Ti[:3, :3] - truth[:3, :3]).max() <= 1e-4 and np.linalg.norm(Ti[:3, 3] - truth[:3, 3]) <= 1e-3
