"""The C++ shim's sample-consensus rejector (include/icpgpu_registration.hpp: icpgpu::registration::CorrespondenceRejectorSampleConsensus,
icpgpu::Correspondence) with PCL's spelling of every call, both ways: in an IterativeClosestPoint's chain on the moved-block scene
and alone behind matches.  tests/cpp/rsac_demo.cpp must print what the Python front end gives, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import rsac_scenes as S
import scp_scenes as SC
from icpslam_amd import Context, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _build(tmp_path):
    exe = tmp_path / "rsac_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rsac_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to compile without the class and to link without icpgpu_correspondence_rejector_sample_consensus in the library."""
    assert _build(tmp_path).exists()


def mat(words):
    return np.array([F32(x) for x in words], F32).reshape(4, 4).T


@pytest.mark.gpu
def test_demo_in_a_chain_on_the_moved_block(built, tmp_path):
    exe = _build(tmp_path)
    src, tgt, truth, _ = S.moved_block()
    a, b = tmp_path / "src.bin", tmp_path / "tgt.bin"
    src.tofile(a)
    tgt.tofile(b)
    thr, it = S.BLOCK_STAGE
    r = subprocess.run([str(exe), "chain", str(a), str(len(src)), str(b), str(len(tgt)), str(S.BLOCK_KW["max_iterations"]), str(thr), str(it)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    f = r.stdout.split()
    with Context(0) as ctx:
        ctx.set_params(**S.BLOCK_KW)
        ctx.set_target(tgt)
        ctx.set_source(src)
        ctx.set_correspondence_rejectors([(_lib.REJECT_SAMPLE_CONSENSUS, thr, it)])
        ref = ctx.align()
        best = ctx.rejector_sac_fetch(per_hypothesis=False)["best_T"]
    assert (int(f[0]), int(f[1]), int(f[2])) == (int(ref["converged"]), ref["iterations"], ref["n_corr"])
    assert mat(f[3:19]).tobytes() == ref["T"].tobytes() and mat(f[19:35]).tobytes() == best.tobytes()
    rot, trans = SC.pose_error(mat(f[3:19]), truth)
    assert rot <= S.E2E_BOUND[0] and trans <= S.E2E_BOUND[1]


@pytest.mark.gpu
def test_demo_alone_behind_matches(built, tmp_path):
    exe = _build(tmp_path)
    source, target, truth = SC.e2e_clouds()
    rng = np.random.default_rng(3)
    iq = np.arange(len(source), dtype=np.int32)
    im = iq.copy()
    wrong = rng.permutation(len(source))[:1000]                     # two thirds of the matches are wrong
    im[wrong] = rng.integers(0, len(target), wrong.size)
    a, b, p = tmp_path / "src.bin", tmp_path / "tgt.bin", tmp_path / "pairs.bin"
    source.tofile(a)
    target.tofile(b)
    np.stack([iq, im], 1).astype(np.int32).tofile(p)
    r = subprocess.run([str(exe), "alone", str(a), str(len(source)), str(b), str(len(target)), str(p), str(len(iq)), "0.05", "1000"],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")
    head = lines[0].split()
    with Context(0) as ctx:
        want = ctx.reject_sample_consensus(source, target, iq, im, 0.05, 1000, 12345)
    assert int(head[0]) == want["n_kept"] and mat(head[1:17]).tobytes() == want["best_T"].tobytes()
    assert np.array_equal(np.array(lines[1].split(), np.int64), np.flatnonzero(want["kept"]))
    rot, trans = SC.pose_error(mat(head[1:17]), truth)
    assert rot <= S.MATCH_BOUND[0] and trans <= S.MATCH_BOUND[1] and want["n_kept"] >= 500 and want["kept"][im == iq].all()
