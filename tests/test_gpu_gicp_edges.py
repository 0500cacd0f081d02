"""GICP ALIGNMENT pinned to the oracle at its edges (the covariance kernels have tests/test_gpu_gicp.py): every case of
tests/gicp_edge_cases.py -- source sizes on the launch boundaries, initial guesses, pairs exactly on the gate, 3 / 4 / 5
correspondences, non-finite points, clouds of fewer than 20 finite points, identical / far / planar / duplicated clouds -- through
every path that can take it:
  (a) the default context: the host loop over the resident evaluation server (gicp_server_kernel);
  (b) ICPGPU_GICP_DEVICE=1: the device solver (gicp_solve_kernel);
  (c) ICPGPU_GICP_SERVER=0: one launch per evaluation (gicp_cost_kernel);
  (d) align_batch: resumable runs, gicp_solve_batch_kernel (the cases without a guess or an output cloud, in ONE call, twice);
  (e) development flavour, ICPGPU_GICP_RESIDENT_MAX=0 ICPGPU_GICP_SOLVE_BLOCKS=1: the streaming server and, with
      ICPGPU_GICP_DEVICE=1, the streaming solver, on the cases of at most 1025 sources.
Per case, the project's GICP standard and no other tolerance: converged, iterations, state and n_corr equal the oracle's, T its
bits, fitness within 1e-9 * max(1, reference), the output cloud (guess cases) its bits.  Across paths: T, counts and fitness the same
bits, mse to 1e-12 relative (its float64 sum is rounded in workgroup order).  The profile says which solver ran.  The switches are
read once per process: (b), (c), (e) are one fresh child process each, run one after the other; a child that fails ends the module's
child runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gicp_edge_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [c.name for c in ec.cases()]
_child_failed = []


def _compare_with_oracle(name, got):
    case = ec.by_name(ec.AFTER_REFUSED if name.startswith("after:") else name)   # (after:<refused>: the ordinary pair that followed it)
    ref = ec.reference(case.name)
    print("%-30s state %d/%d iterations %d/%d n_corr %d/%d fitness %.17g/%.17g device %d host %d" % (
        name, got["state"], ref["state"], got["iterations"], ref["iterations"], got["n_corr"], ref["n_corr"], got["fitness"], ref["fitness"],
        got["device_solves"], got["host_solves"]))
    assert (got["converged"], got["iterations"], got["state"], got["n_corr"]) == (ref["converged"], ref["iterations"], ref["state"], ref["n_corr"]), name
    assert np.array_equal(np.asarray(got["T"], np.float32).view(np.uint32), np.asarray(ref["T"], np.float32).view(np.uint32)), (name, got["T"], ref["T"])
    if np.isnan(ref["fitness"]):
        assert np.isnan(got["fitness"]), name
    else:
        assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"]), (name, got["fitness"], ref["fitness"])
    if ec.wants_cloud(case) and not name.startswith("after:"):
        assert got["cloud"] is not None and np.array_equal(got["cloud"].view(np.uint32), ref["cloud"].view(np.uint32)), name
    ec.check_exit(case, got)


def _compare_paths(name, got, base):
    assert np.array_equal(got["T"].view(np.uint32), base["T"].view(np.uint32)), name
    assert (got["converged"], got["iterations"], got["state"], got["n_corr"]) == (base["converged"], base["iterations"], base["state"], base["n_corr"]), name
    assert got["fitness"] == base["fitness"] or (np.isnan(got["fitness"]) and np.isnan(base["fitness"])), (name, got["fitness"], base["fitness"])
    assert abs(got["mse"] - base["mse"]) <= 1e-12 * abs(base["mse"]), (name, got["mse"], base["mse"])


def _solves(name, got, device):
    """The solves the profile must show for this alignment on the solver that ran it: one per outer iteration; none for a refused
    cloud.  A registration that ends with fewer than 4 correspondences completes no iteration: the host loop sees the count in its
    first evaluation and never starts its solver, the device solver is the launch that finds it out -- one solve more."""
    if not name.startswith("after:") and ec.by_name(name).exit.get("refused"):
        return 0
    return got["iterations"] + (1 if device and got["state"] == ec.NO_CORRESPONDENCES else 0)


@pytest.fixture(scope="module")
def default_path(ctx):
    """(a): the whole table on the session's context, in this process"""
    return ec.run_table(ctx, set(ALL))


def _child(tmp_path, tag, env, which="all"):
    if _child_failed:
        pytest.fail("not started: the child process of %s failed" % _child_failed[0])
    path = str(tmp_path / (tag + ".npz"))
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gicp_edge_cases.py"), "--child", path, which], env=e, capture_output=True,
                             text=True, timeout=300, cwd=ROOT)
    except subprocess.TimeoutExpired as t:   # a child that hung: nothing further is started either
        _child_failed.append(tag)
        pytest.fail("child %s: no result after %d s\n%s" % (tag, t.timeout, (t.stderr or b"")[-3000:]))
    if res.returncode != 0:
        _child_failed.append(tag)
        pytest.fail("child %s: exit %d\n%s" % (tag, res.returncode, res.stderr[-3000:]))
    return ec.load_results(path)


def test_default_path_host_loop_over_the_evaluation_server(default_path):
    assert set(ALL) <= set(default_path) and sum(k.startswith("after:") for k in default_path) == 3
    for name, got in default_path.items():
        _compare_with_oracle(name, got)
        assert got["device_solves"] == 0 and got["host_solves"] == _solves(name, got, False), (name, got["device_solves"], got["host_solves"])


@pytest.mark.parametrize("r", [1.0, 0.5, 0.3])
def test_gate_is_strict(default_path, r):
    """a pair exactly on r^2 (or on the first float above it) is rejected, one float inside accepted; the gate one step wider
    takes exactly the three on-gate points more"""
    a, b = default_path["gate_%g" % r], default_path["gate_%g_wide" % r]
    assert a["n_corr"] == ec.reference("gate_%g" % r)["n_corr"] and b["n_corr"] - a["n_corr"] == len(ec.gate_points(r)["on"]) == 3


def test_device_solver(default_path, tmp_path):
    got = _child(tmp_path, "device", {"ICPGPU_GICP_DEVICE": "1"})
    assert set(got) == set(default_path)
    for name, g in got.items():
        _compare_with_oracle(name, g)
        _compare_paths(name, g, default_path[name])
        assert g["device_solves"] == _solves(name, g, True) and g["host_solves"] == 0, (name, g["device_solves"], g["host_solves"], g["iterations"])
        if g["converged"]:
            assert g["device_solves"] == g["iterations"], name


def test_single_launches(default_path, tmp_path):
    got = _child(tmp_path, "launches", {"ICPGPU_GICP_SERVER": "0"})
    assert set(got) == set(default_path)
    for name, g in got.items():
        _compare_with_oracle(name, g)
        _compare_paths(name, g, default_path[name])
        assert g["device_solves"] == 0 and g["host_solves"] == _solves(name, g, False), name


def test_batch(built, default_path):
    """the cases without a guess or an output cloud share one parameter set: ONE align_batch call holds small, boundary, refused and
    degenerate pairs side by side; the second call meets warm workers"""
    from icpslam_amd import Context, GICP
    cs = [c for c in ec.cases() if c.guess is None and not ec.wants_cloud(c)]
    assert all(c.params == ec.COMMON for c in cs) and len(cs) >= 35 and any(c.exit.get("refused") for c in cs)
    with Context(0) as c:
        c.set_params(c.default_params(), method=GICP, **ec.COMMON)
        for _ in range(2):
            c.profile_reset()
            got = c.align_batch([x.src for x in cs], [x.tgt for x in cs], want_fitness=True)
            prof = c.profile()
            assert prof.gicp_device_solves > 0 and prof.gicp_host_solves == 0
            for case, g in zip(cs, got):
                g = dict(g, device_solves=-1, host_solves=-1)
                _compare_with_oracle(case.name, g)
                _compare_paths(case.name, g, default_path[case.name])


def test_forced_streaming_server_and_solver(built, dev_flavour, tmp_path):
    if dev_flavour.delegated:
        return
    if _child_failed:
        pytest.fail("not started: the child process of %s failed" % _child_failed[0])
    from icpslam_amd import Context
    small = {c.name for c in ec.cases() if ec.is_small(c)}
    assert {"ns_20", "ns_513", "ns_1025", "min_3", "min_4", "min_5"} <= small
    with Context(0) as ctx:
        base = ec.run_table(ctx, small)
    forced = {"ICPGPU_GICP_RESIDENT_MAX": "0", "ICPGPU_GICP_SOLVE_BLOCKS": "1"}
    for tag, env in (("streamed_server", forced), ("streamed_solver", dict(forced, ICPGPU_GICP_DEVICE="1"))):
        got = _child(tmp_path, tag, env, which="small")
        assert set(got) == small
        for name, g in got.items():
            _compare_with_oracle(name, g)
            _compare_paths(name, g, base[name])
            if "ICPGPU_GICP_DEVICE" in env:
                assert g["device_solves"] == _solves(name, g, True) and g["host_solves"] == 0, name
            else:
                assert g["device_solves"] == 0 and g["host_solves"] == _solves(name, g, False), name
