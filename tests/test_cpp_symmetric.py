"""The C++ shim's chain for clouds with normals (include/icpgpu_registration.hpp), with PCL's spelling of every call:
tests/cpp/symmetric_demo.cpp -- NormalEstimation on both clouds -> setSourceNormals / setTargetNormals ->
IterativeClosestPointWithNormals with setUseSymmetricObjective(true) and a CorrespondenceRejectorSurfaceNormal -> align -- must give
the transform a Python Context gives through the C-ABI with the same normals, flag and chain."""
import numpy as np
import pytest

from icpslam_amd import P2PLANE, Context, synth
from test_symmetric_host import build_demo


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    """Fails to compile without the shim's new names, and to link without the library's new symbols."""
    assert build_demo(tmp_path).exists()


@pytest.mark.gpu
def test_demo_equals_the_c_abi(built, tmp_path):
    import subprocess
    exe = build_demo(tmp_path)
    src, tgt, _ = synth.make_pair(1500, 1500, seed=7)
    a, b = tmp_path / "src.bin", tmp_path / "tgt.bin"
    src.tofile(a)
    tgt.tofile(b)
    k, iters, threshold = 12, 10, 0.5
    r = subprocess.run([str(exe), str(a), str(len(src)), str(b), str(len(tgt)), str(iters), str(k), str(threshold)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    with Context(0) as ctx:
        ctx.search_set_input(src)
        sn = ctx.normal_estimation(None, k=k)[0]                    # {nx, ny, nz, curvature}: the fourth float is ignored
        ctx.search_set_input(tgt)
        tn = ctx.normal_estimation(None, k=k)[0]
        ctx.set_params(method=P2PLANE, max_iterations=iters, transformation_epsilon=1e-6, max_correspondence_distance=1.0)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_source_normals(sn)
        ctx.set_target_normals(tn)
        ctx.set_p2plane_symmetric(True, True)
        ctx.set_correspondence_rejectors([(4, threshold)])
        want = ctx.align()
        stats = ctx.rejector_stats()
        ctx.set_p2plane_symmetric(False)
        plain = ctx.align()
    words = r.stdout.split()
    assert int(words[0]) == int(want["converged"]) and int(words[1]) == want["iterations"] and want["iterations"] > 1
    T = np.array([np.float32(w) for w in words[2:]], np.float32).reshape(4, 4).T
    assert T.tobytes() == np.asarray(want["T"], np.float32).tobytes()
    assert T.tobytes() != np.asarray(plain["T"], np.float32).tobytes()          # the objective is the symmetric one
    assert 0 < stats[0]["pairs_out"] < stats[0]["pairs_in"]                     # ... and the stage had something to reject
