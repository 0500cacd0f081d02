"""The C++ shim's setUseReciprocalCorrespondences (include/icpgpu_registration.hpp) driven with PCL's spelling of the calls:
tests/cpp/reciprocal_demo.cpp must print the transform the C-ABI gives for the same flag and chain, and the same GICP result with
the flag on and off."""
import os
import subprocess

import numpy as np
import pytest

from icpslam_amd import Context, _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = tmp_path / "reciprocal_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "reciprocal_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["p2p", "p2plane"])
def test_demo_prints_the_c_abi_transform(built, tmp_path, method):
    exe = _build(tmp_path)
    src, tgt, _ = synth.make_pair(5000, 5000, seed=2)
    a, b = tmp_path / "src.bin", tmp_path / "tgt.bin"
    src.tofile(a)
    tgt.tofile(b)
    cmd = [str(exe), str(a), str(src.shape[0]), str(b), str(tgt.shape[0]), "10"] + (["p2plane"] if method == "p2plane" else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2
    f = lines[0].split()
    with Context(0) as ctx:
        ctx.set_params(method=_lib.P2PLANE if method == "p2plane" else _lib.P2P_SVD, max_iterations=10)
        ctx.set_target(tgt)
        ctx.set_source(src)
        ctx.set_reciprocal_correspondences(True)
        ctx.set_correspondence_rejectors([(_lib.REJECT_TRIMMED, float(np.float32(0.9)))])
        ref = ctx.align()
        st = ctx.reciprocal_stats()
        ctx.set_reciprocal_correspondences(False)
        plain = ctx.align()
    assert st["pairs_out"] < st["pairs_in"] and plain["n_corr"] != ref["n_corr"]      # the flag did something
    assert (int(f[0]), int(f[1]), int(f[2])) == (int(ref["converged"]), ref["iterations"], ref["n_corr"])
    T = np.array([np.float32(x) for x in f[3:19]], np.float32).reshape(4, 4).T
    assert T.tobytes() == ref["T"].tobytes()
    g = lines[1].split()
    assert len(g) == 38 and g[:19] == g[19:]                                          # GICP: the flag changes nothing
