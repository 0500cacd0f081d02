"""NDT with the More-Thuente step rule (icpgpu_set_ndt_line_search(ctx, ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE)) on the device,
against the NumPy restatement in tests/ndt_line_search_restated.py (on tests/ndt_restated.py's derivatives; neither calls the
library).  The alignments pinned here are those whose every line-search decision the restatement finds clear of its threshold."""
import os
import subprocess

import numpy as np
import pytest

import ndt_line_search_restated as ls
import ndt_restated as nr
from icpslam_amd import NDT, NDT_LINE_SEARCH_MORE_THUENTE, NDT_LINE_SEARCH_PCL18, Context, NormalDistributionsTransform, _lib, synth
from icpslam_amd._lib import IcpGpuError
from icpslam_amd.sequence import run_odometry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MT = NDT_LINE_SEARCH_MORE_THUENTE
MARGIN = 1e-6      # least relative margin of a pinned alignment's line-search decisions (the sums agree to ~1e-12)


def _ctx(resolution=1.0, line_search=MT, **kw):
    c = Context(0)
    kw.setdefault("max_iterations", 35)
    kw.setdefault("transformation_epsilon", 0.1)
    c.set_params(c.default_params(), method=NDT, **kw)
    c.set_ndt_params(resolution, 0.1, 0.55, line_search=line_search)
    return c


def _cloud(xyz):
    xyz = np.asarray(xyz, F)
    return np.c_[xyz, np.ones(len(xyz), F)].astype(F)


# ---- the trial pass ------------------------------------------------------------------------------------------------------------
def _boundary_clouds():
    """test_gpu_ndt's radius-boundary scene: exact centroids, source points exactly `resolution` from them and one ulp further."""
    offs = np.array([[dx, dy, dz] for dx in (-0.25, 0.25) for dy in (-0.25, 0.25) for dz in (-0.125, 0.125)], F)
    centres = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 3.5, 2.5], [-2.5, -1.5, 0.5]], F)
    tgt = _cloud(np.concatenate([c + offs for c in centres]))
    src = []
    for c in centres:
        for a in range(3):
            for s in (-1, 1):
                q = c.copy()
                q[a] = c[a] + s * F(1.0)
                src.append(q.copy())
                q[a] = np.nextafter(q[a], F(s * np.inf))
                src.append(q.copy())
        src.append(c + F(0.5))
    return _cloud(np.array(src)), tgt


def test_trial_pass_is_the_first_8_sums_bit_for_bit():
    src, tgt, T_gt = synth.make_pair(20000, 40000, seed=4)
    rng = np.random.default_rng(1)
    poses = [np.zeros(6), np.r_[T_gt[:3, 3], 0.0, 0.0, 0.02], np.r_[rng.normal(0, 0.3, 3), rng.uniform(-5e-5, 5e-5, 3)],
             np.r_[rng.normal(0, 0.3, 3), rng.normal(0, 0.05, 3)], np.r_[0.2, -0.1, 0.0, 3.0, -1.2, 2.0]]
    bsrc, btgt = _boundary_clouds()
    with _ctx() as ctx:
        for s, t, ps in ((src, tgt, poses), (bsrc, btgt, [np.zeros(6), np.r_[0.01, 0.0, 0.0, 0.0, 0.0, 1e-3]])):
            ctx.set_target(t)
            ctx.set_source(s)
            for p in ps:
                full = ctx.ndt_derivatives(p)
                g = ctx.ndt_gradient(p)
                assert g.shape == (8,) and g[0] > 0
                assert np.array_equal(g.view(np.uint64), full[:8].view(np.uint64)), (p, g, full[:8])
                assert np.array_equal(ctx.ndt_gradient(p).view(np.uint64), g.view(np.uint64))


# ---- alignments ------------------------------------------------------------------------------------------------------------------
def _same(got, ref, trace=None, prob=None):
    assert (got["iterations"], got["state"], got["converged"]) == (ref["iterations"], ref["state"], ref["converged"]), (got, ref)
    assert got["n_corr"] == ref["n_corr"]
    assert np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max() <= 1e-4
    assert np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]) <= 1e-3
    if trace is not None:
        assert len(trace["step"]) == ref["trials"]
        want = np.array(ref["trace"], np.float64).reshape(-1, 4)
        assert np.array_equal(trace["iteration"], want[:, 0].astype(np.int32))
        assert np.allclose(trace["step"], want[:, 1], rtol=1e-6, atol=1e-9)
        assert np.allclose(trace["phi"], want[:, 2], rtol=1e-9, atol=0)
        assert np.allclose(trace["d_phi"], want[:, 3], rtol=1e-5, atol=1e-6 * np.abs(want[:, 3]).max())
    if prob is not None:
        assert abs(prob - ref["probability"]) <= 1e-9 * abs(ref["probability"])


# (n, seeds, eps): seeds of synth.make_pair(n, n, seed=100 + s) whose restated decisions all clear MARGIN
PINNED = [(5000, (0, 1, 2, 3), 0.1), (5000, (0, 1, 2), 1e-3), (50000, (0, 1), 0.1), (50000, (0,), 1e-3)]


@pytest.mark.parametrize("n,seeds,eps", PINNED)
def test_alignment_matches_the_restatement(n, seeds, eps):
    with _ctx(transformation_epsilon=eps) as ctx:
        assert ctx.get_ndt_line_search() == MT
        for seed in seeds:
            src, tgt, _ = synth.make_pair(n, n, seed=100 + seed)
            ctx.set_target(tgt)
            ctx.set_source(src)
            got = ctx.align()
            ref = ls.align_mt(nr.Target(tgt, 1.0), src, transformation_epsilon=eps)
            assert ref["min_margin"] > MARGIN, (seed, ref["min_margin"])
            _same(got, ref, ctx.ndt_line_search_trace(), ctx.ndt_transformation_probability())


@pytest.mark.parametrize("eps", [0.1, 1e-3])
def test_alignment_at_200k(eps):
    src, tgt, _ = synth.make_pair(200000, 60000, seed=77)
    with _ctx(transformation_epsilon=eps) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        got = ctx.align(want_fitness=True)
        ref = ls.align_mt(nr.Target(tgt, 1.0), src, transformation_epsilon=eps)
        assert ref["min_margin"] > MARGIN, ref["min_margin"]
        _same(got, ref, ctx.ndt_line_search_trace(), ctx.ndt_transformation_probability())
        assert np.isfinite(got["fitness"]) and got["converged"]


def test_switching_to_more_thuente_and_back_gives_the_default_bits():
    src, tgt, _ = synth.make_pair(20000, 20000, seed=5)
    with _ctx(line_search=NDT_LINE_SEARCH_PCL18, transformation_epsilon=0.01) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        assert ctx.get_ndt_line_search() == NDT_LINE_SEARCH_PCL18
        base = ctx.align()
        base_prob = ctx.ndt_transformation_probability()
        assert len(ctx.ndt_line_search_trace()["step"]) == 0                   # no trial is traced under PCL 1.8's rule
        ctx.set_ndt_line_search(MT)
        mt = ctx.align()
        assert len(ctx.ndt_line_search_trace()["step"]) >= mt["iterations"]
        ctx.set_ndt_params(1.0, 0.1, 0.55, line_search=NDT_LINE_SEARCH_PCL18)
        again = ctx.align()
        assert np.array_equal(again["T"].view(np.uint32), base["T"].view(np.uint32))
        assert (again["iterations"], again["n_corr"], again["state"]) == (base["iterations"], base["n_corr"], base["state"])
        assert ctx.ndt_transformation_probability() == base_prob
        assert len(ctx.ndt_line_search_trace()["step"]) == 0
        # the same context under MT again: the same bits as its first MT alignment
        ctx.set_ndt_line_search(MT)
        assert np.array_equal(ctx.align()["T"].view(np.uint32), mt["T"].view(np.uint32))


def test_mode_errors_and_batches():
    with _ctx() as ctx:
        for bad in (-1, 2, 7):
            with pytest.raises(IcpGpuError):
                ctx.set_ndt_line_search(bad)
        assert ctx.get_ndt_line_search() == MT                                 # a refused mode changes nothing
        src, tgt, _ = synth.make_pair(3000, 3000, seed=1)
        with pytest.raises(IcpGpuError) as e:
            ctx.align_batch([src], [tgt])
        assert e.value.code == _lib.ERR_UNSUPPORTED
    with Context(0) as ctx:
        assert ctx.get_ndt_line_search() == NDT_LINE_SEARCH_PCL18              # a new context: PCL 1.8's rule


_SHIM = r'''
#include <cstdio>
#include <memory>
#include <vector>
#include "icpgpu_registration.hpp"
struct alignas(16) P { float x, y, z, w; };
struct Cloud { std::vector<P> points; std::size_t size() const { return points.size(); } using Ptr = std::shared_ptr<Cloud>; };
static Cloud::Ptr load(const char* path, std::size_t n) {
  auto c = std::make_shared<Cloud>();
  c->points.resize(n);
  FILE* f = std::fopen(path, "rb");
  if (!f || std::fread(c->points.data(), sizeof(P), n, f) != n) std::exit(2);
  std::fclose(f);
  return c;
}
int main(int argc, char** argv) {
  if (argc < 5) return 2;
  icpgpu::NormalDistributionsTransform<Cloud> ndt;
  if (ndt.getMoreThuenteLineSearch()) return 4;
  ndt.setMoreThuenteLineSearch(true);
  if (!ndt.getMoreThuenteLineSearch()) return 4;
  Cloud::Ptr src = load(argv[1], std::strtoull(argv[2], nullptr, 10)), tgt = load(argv[3], std::strtoull(argv[4], nullptr, 10));
  ndt.setInputSource(src);  // (the shim keeps the clouds by address, as PCL keeps the shared pointers: they must outlive align)
  ndt.setInputTarget(tgt);
  Cloud out;
  ndt.align(out);
  const auto T = ndt.getFinalTransformation();
  std::printf("%d %d %.17g", ndt.hasConverged() ? 1 : 0, ndt.getFinalNumIteration(), ndt.getTransformationProbability());
  for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
  std::printf("\n");
  return 0;
}
'''


def test_cpp_shim_and_python_front_end(tmp_path):
    src, tgt, _ = synth.make_pair(20000, 20000, seed=6)
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        got = ctx.align()
        prob = ctx.ndt_transformation_probability()
    ref = ls.align_mt(nr.Target(tgt, 1.0), src)
    _same(got, ref)
    ndt = NormalDistributionsTransform()
    assert ndt.getMoreThuenteLineSearch() is False
    ndt.setMoreThuenteLineSearch(True)
    ndt.setInputSource(src)
    ndt.setInputTarget(tgt)
    ndt.align()
    assert np.array_equal(ndt.getFinalTransformation().view(np.uint32), got["T"].view(np.uint32))
    assert ndt.getFinalNumIteration() == got["iterations"] and ndt.getTransformationProbability() == prob
    code = tmp_path / "mt.cpp"
    code.write_text(_SHIM)
    exe = tmp_path / "mt"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(code),
                           "-o", str(exe), "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    a, b = tmp_path / "s.bin", tmp_path / "t.bin"
    src.tofile(a)
    tgt.tofile(b)
    r = subprocess.run([str(exe), str(a), str(len(src)), str(b), str(len(tgt))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    vals = r.stdout.split()
    assert (int(vals[0]), int(vals[1])) == (int(got["converged"]), got["iterations"])
    T_cpp = np.array([float(v) for v in vals[3:19]], F).reshape(4, 4).T
    assert np.array_equal(T_cpp.view(np.uint32), got["T"].view(np.uint32))
    assert float(vals[2]) == pytest.approx(prob, rel=1e-12)


# ---- a drive at PCL's defaults ---------------------------------------------------------------------------------------------------
def _drive(n_scans, n_pts=60000, seed=8):
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(321)
    poses = [np.eye(4)]
    for _ in range(n_scans - 1):
        poses.append(poses[-1] @ synth.pose_matrix(0.3, rng.uniform(-0.03, 0.03), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-2, 2))))
    return [synth.scan(scene, P, n_pts, seed=900 + k) for k, P in enumerate(poses)], poses


# The restatement's drift on this drive (ndt_line_search_restated.align_mt on the 0.2 m voxel filter's clouds, chained the way the
# test chains the device's; computed on a CPU before any device run): see DESIGN.md f6.
RESTATED_DRIFT_AT_PCL_DEFAULTS = 11.11      # 11.106 m (1.8's rule: 11.1 m)


def test_drive_of_40_scans_through_run_odometry_at_pcl_defaults():
    """The reference's online loop with NDT at PCL's defaults (resolution 1.0, step size 0.1, 35 iterations, transformation epsilon
    0.1) and the More-Thuente rule; the drift is bounded by the restatement's on the same drive (+ 5 cm)."""
    scans, poses = _drive(40)
    with _ctx() as ctx:
        graph, recs = run_odometry(ctx, scans, voxel_leaf=0.2)
    assert len(recs) == 39 and all(r["accepted"] for r in recs)
    P = np.eye(4)
    for r in recs:
        P = P @ r["T"].astype(np.float64)
    drift = float(np.linalg.norm(P[:3, 3] - poses[-1][:3, 3]))
    assert drift <= RESTATED_DRIFT_AT_PCL_DEFAULTS + 0.05, drift
