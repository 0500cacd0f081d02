"""NDT registration (method NDT: pcl::NormalDistributionsTransform over pcl::VoxelGridCovariance, PCL 1.8) on the device, against
the NumPy restatement in tests/ndt_restated.py (which never calls the library).  Parity against PCL binaries is unpinned, as for
every other mode."""
import os
import subprocess

import numpy as np
import pytest

import ndt_restated as nr
from icpslam_amd import NDT, Context, NormalDistributionsTransform, _lib, synth
from icpslam_amd._lib import IcpGpuError
from icpslam_amd.sequence import run_odometry
from icpslam_amd.sharding import COMM_NONE, align_batch_multi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NOT_CONVERGED, ITERATIONS, TRANSFORM, NO_CORRESPONDENCES = 0, 1, 2, 5


def _ctx(resolution=1.0, **kw):
    c = Context(0)
    kw.setdefault("max_iterations", 35)
    kw.setdefault("transformation_epsilon", 0.1)
    c.set_params(c.default_params(), method=NDT, **kw)
    c.set_ndt_params(resolution, 0.1, 0.55)
    return c


def _cloud(xyz):
    xyz = np.asarray(xyz, F)
    return np.c_[xyz, np.ones(len(xyz), F)].astype(F)


# ---- cells -------------------------------------------------------------------------------------------------------------------
def _cell_scene(seed=0):
    """Noisy planes (the eigenvalue floor fires), a blob, a cell of exactly 5 points and one of 6, collinear points along an axis,
    duplicates, and non-finite points."""
    rng = np.random.default_rng(seed)
    parts = [np.c_[rng.uniform(-6, 6, (4000, 2)), rng.normal(0.3, 0.01, 4000)],                 # floor
             np.c_[rng.uniform(-6, 6, 3000), rng.normal(4.4, 0.02, 3000), rng.uniform(0, 3, 3000)],  # wall
             rng.normal([2.5, -2.5, 1.5], 0.3, (1500, 3)),                                          # blob
             rng.uniform([10.1, 10.1, 10.1], [10.9, 10.9, 10.9], (5, 3)),                           # exactly 5: no cell
             rng.uniform([12.1, 10.1, 10.1], [12.9, 10.9, 10.9], (6, 3)),                           # exactly 6: a cell
             np.c_[np.linspace(14.05, 14.95, 12), np.full(12, 10.5), np.full(12, 10.5)],            # collinear (x axis)
             np.tile([[16.25, 10.5, 10.5], [16.75, 10.5, 10.5]], (5, 1)), [[16.5, 10.75, 10.5]] * 2,  # duplicates, a plane
             np.tile([[18.5, 10.5, 10.5]], (8, 1))]                                                 # one point, eight times
    pts = _cloud(np.concatenate(parts))
    pts = pts[rng.permutation(len(pts))]
    bad = rng.choice(len(pts), 7, replace=False)
    pts[bad[:3], 0] = np.nan
    pts[bad[3:5], 1] = np.inf
    pts[bad[5:], 2] = -np.inf
    return pts


def _check_cells(ctx, tgt, resolution):
    ctx.set_ndt_params(resolution, 0.1, 0.55)
    ctx.set_target(tgt)
    got = ctx.ndt_cells()
    C = nr.cells(tgt, resolution)
    ref = nr.valid_cells(C)
    assert len(got["n_points"]) == len(ref["n"]) > 0
    assert np.array_equal(got["n_points"], ref["n"])
    assert np.array_equal(got["centroid"][:, :3].view(np.uint32), ref["centroid"].view(np.uint32))
    assert (got["centroid"][:, 3] == 1).all()
    assert np.array_equal(got["mean"].view(np.uint64), ref["mean"].view(np.uint64))
    scale = np.abs(ref["icov"]).reshape(-1, 9).max(axis=1)
    assert (np.abs(got["icov"] - ref["icov"]).reshape(-1, 9).max(axis=1) <= 1e-12 * scale).all()
    # the centroids are the voxel filter's rows of the same cells, bit for bit
    vox = ctx.voxel_grid(tgt, resolution)
    assert len(vox) == len(C["key"])
    rows = vox[C["valid"], :3]
    assert np.array_equal(got["centroid"][:, :3].view(np.uint32), rows.view(np.uint32))
    return C


def test_cells_match_the_restatement():
    tgt = _cell_scene()
    with _ctx() as ctx:
        C = _check_cells(ctx, tgt, 1.0)
        key = {int(k): i for i, k in enumerate(C["key"])}
        L = C["lattice"]
        def cell_of(x, y, z):
            ijk = np.floor(np.array([x, y, z], F) * L["inv"]).astype(np.int64) - L["minb"]
            return key[int(ijk[0] + ijk[1] * L["mul_y"] + ijk[2] * L["mul_z"])]
        assert C["n"][cell_of(10.5, 10.5, 10.5)] == 5 and not C["valid"][cell_of(10.5, 10.5, 10.5)]
        assert C["n"][cell_of(12.5, 10.5, 10.5)] == 6 and C["valid"][cell_of(12.5, 10.5, 10.5)]
        assert C["valid"][cell_of(14.5, 10.5, 10.5)]                    # collinear: two zero eigenvalues raised
        assert not C["valid"][cell_of(18.5, 10.5, 10.5)]                # one point eight times: all eigenvalues zero
        assert C["n"].sum() == np.isfinite(tgt[:, :3]).all(axis=1).sum()
        # planes: the floor fired (smallest eigenvalue raised to 0.01 x the largest)
        ev = np.linalg.eigvalsh(np.linalg.inv(C["icov"][C["valid"]]))
        assert (np.abs(ev[:, 0] / ev[:, 2] - 0.01) < 1e-9).sum() > 20
        # other resolutions and a raw synthetic scan
        _check_cells(ctx, tgt, 0.5)
        _check_cells(ctx, tgt, 2.3)
        _check_cells(ctx, synth.scan(synth.make_scene(5), np.eye(4), 60000, seed=3), 1.0)


def test_cells_overflow_is_refused():
    tgt = _cloud([[-1e6, 0, 0], [1e6, 0, 0], [0, -1e6, 0], [0, 1e6, 0], [0, 0, -1e5], [0, 0, 1e5]] * 2)
    with pytest.raises(nr.Overflow):
        nr.cells(tgt, 0.05)
    with _ctx(resolution=0.05) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(tgt)
        for call in (ctx.ndt_cells, ctx.align):
            with pytest.raises(IcpGpuError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARG
        ctx.set_ndt_params(1000.0, 0.1, 0.55)                            # a coarser lattice fits
        assert len(ctx.ndt_cells()["n_points"]) == 0
    # extents beyond int64 on ONE axis (2e30 cells: a float-to-int64 cast of that is undefined, and negative where it is not), beyond
    # float on one axis (hi - lo = inf), and three ordinary extents whose int64 product wraps (2^22 cells cubed, times 8): all refused
    for box, res in (([[-1e30, 0, 0], [1e30, 1, 1]], 1.0), ([[-3e38, 0, 0], [3e38, 1, 1]], 1.0), ([[-4e4, -4e4, -4e4], [4e4, 4e4, 4e4]], 0.01)):
        far = _cloud(box * 6)
        with pytest.raises(nr.Overflow):
            nr.cells(far, res)
        with _ctx(resolution=res) as ctx:
            ctx.set_target(far)
            ctx.set_source(far)
            for call in (ctx.ndt_cells, ctx.align):
                with pytest.raises(IcpGpuError) as e:
                    call()
                assert e.value.code == _lib.ERR_INVALID_ARG


# ---- derivatives ----------------------------------------------------------------------------------------------------------------
def _check_terms(got, ref):
    assert got[0] == ref[0]
    assert abs(got[1] - ref[1]) <= 1e-9 * abs(ref[1])
    assert np.abs(got[2:8] - ref[2:8]).max() <= 1e-9 * np.abs(ref[2:8]).max()
    assert np.abs(got[8:] - ref[8:]).max() <= 1e-9 * np.abs(ref[8:]).max()


def test_derivatives_match_the_restatement_and_are_deterministic():
    src, tgt, T_gt = synth.make_pair(20000, 40000, seed=4)
    tg = nr.Target(tgt, 1.0)
    rng = np.random.default_rng(1)
    poses = [np.zeros(6), np.r_[T_gt[:3, 3], 0.0, 0.0, 0.02], np.r_[rng.normal(0, 0.3, 3), rng.uniform(-5e-5, 5e-5, 3)],
             np.r_[rng.normal(0, 0.3, 3), rng.normal(0, 0.05, 3)], np.r_[0.2, -0.1, 0.0, 3.0, -1.2, 2.0]]
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        for p in poses:
            got = ctx.ndt_derivatives(p)
            ref = nr.derivatives(tg, src, nr.transform_float(p), p)
            assert ref[0] > 1000 or np.abs(p[3:]).max() > 1
            _check_terms(got, ref)
            assert np.array_equal(ctx.ndt_derivatives(p).view(np.uint64), got.view(np.uint64))


def test_derivatives_on_the_radius_boundary():
    """Cells whose float centroids are exact, source points exactly `resolution` from them (and one ulp further) in the next cells:
    the device's stencil finds every pair the float predicate accepts."""
    offs = np.array([[dx, dy, dz] for dx in (-0.25, 0.25) for dy in (-0.25, 0.25) for dz in (-0.125, 0.125)], F)
    centres = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 3.5, 2.5], [-2.5, -1.5, 0.5]], F)
    tgt = _cloud(np.concatenate([c + offs for c in centres]))
    one = F(1.0)
    src = []
    for c in centres:
        for a in range(3):
            for s in (-1, 1):
                q = c.copy()
                q[a] = c[a] + s * one
                src.append(q.copy())
                q[a] = np.nextafter(q[a], F(s * np.inf))
                src.append(q.copy())
        src.append(c + F(0.5))                                              # inside, on the diagonal
    src = _cloud(np.array(src))
    tg = nr.Target(tgt, 1.0)
    assert sorted(map(tuple, tg.v["centroid"].tolist())) == sorted(map(tuple, centres.tolist()))
    ref = nr.derivatives(tg, src, np.eye(4, dtype=F), np.zeros(6))
    assert ref[0] >= len(centres) * 7                                     # (one-ulp-further points can round onto the radius)
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        _check_terms(ctx.ndt_derivatives(np.zeros(6)), ref)


# ---- alignments ------------------------------------------------------------------------------------------------------------------
def _same(got, ref, prob=None):
    assert (got["iterations"], got["state"], got["converged"]) == (ref["iterations"], ref["state"], ref["converged"]), (got, ref)
    assert got["n_corr"] == ref["n_corr"]
    assert np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max() <= 1e-4
    assert np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]) <= 1e-3
    if prob is not None:
        assert abs(prob - ref["probability"]) <= 1e-9 * abs(ref["probability"])


@pytest.mark.parametrize("n,seeds,eps", [(5000, range(6), 0.1), (5000, range(3), 1e-3), (50000, range(2), 0.1)])
def test_alignment_matches_the_restatement(n, seeds, eps):
    with _ctx(transformation_epsilon=eps) as ctx:
        for seed in seeds:
            src, tgt, _ = synth.make_pair(n, n, seed=100 + seed)
            ctx.set_target(tgt)
            ctx.set_source(src)
            got = ctx.align()
            assert np.isnan(got["mse"])
            _same(got, nr.align(nr.Target(tgt, 1.0), src, transformation_epsilon=eps), ctx.ndt_transformation_probability())


def test_alignment_at_200k():
    src, tgt, _ = synth.make_pair(200000, 60000, seed=77)
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        got = ctx.align(want_fitness=True)
        _same(got, nr.align(nr.Target(tgt, 1.0), src), ctx.ndt_transformation_probability())
        assert np.isfinite(got["fitness"]) and got["converged"]


def test_known_answer_and_a_guess():
    for seed in range(3):
        src, tgt, T_gt = synth.make_known_answer_pair(8000, seed=seed)
        with _ctx(max_iterations=100, transformation_epsilon=1e-4) as ctx:
            ctx.set_target(tgt)
            ctx.set_source(src)
            got = ctx.align()
            _same(got, nr.align(nr.Target(tgt, 1.0), src, max_iterations=100, transformation_epsilon=1e-4),
                  ctx.ndt_transformation_probability())
            assert np.abs(got["T"][:3, :3] - T_gt[:3, :3]).max() <= 2e-4, seed
            assert np.linalg.norm(got["T"][:3, 3] - T_gt[:3, 3]) <= 2e-3, seed
            # a non-identity guess near the answer: p0 from its eulerAngles(0, 1, 2)
            guess = (T_gt @ synth.pose_matrix(0.05, -0.04, 0.01, 0.0, 0.0, np.deg2rad(1.0))).astype(F)
            got = ctx.align(guess=guess)
            _same(got, nr.align(nr.Target(tgt, 1.0), src, max_iterations=100, transformation_epsilon=1e-4, guess=guess),
                  ctx.ndt_transformation_probability())
            assert np.linalg.norm(got["T"][:3, 3] - T_gt[:3, 3]) <= 2e-3, seed


# ---- a drive -----------------------------------------------------------------------------------------------------------------------
def _drive(n_scans, n_pts=60000, seed=8):
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(321)
    poses = [np.eye(4)]
    for _ in range(n_scans - 1):
        poses.append(poses[-1] @ synth.pose_matrix(0.3, rng.uniform(-0.03, 0.03), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-2, 2))))
    return [synth.scan(scene, P, n_pts, seed=900 + k) for k, P in enumerate(poses)], poses


def _demo(tmp_path):
    exe = tmp_path / "ndt_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ndt_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_drive_of_10_scans_and_the_cpp_shim(tmp_path):
    """voxel filter -> NDT -> promote, scan by scan, against the restatement; on some pairs the C++ shim's
    NormalDistributionsTransform and the Python front end give the context's T bit for bit."""
    scans, _ = _drive(10)
    exe = _demo(tmp_path)
    with _ctx() as ctx:
        prev = None
        for k, raw in enumerate(scans):
            vox = ctx.voxel_grid(raw, 0.2)
            ctx.set_source(vox)
            if prev is None:
                ctx.promote_source_to_target()
                prev = vox
                continue
            got = ctx.align(want_fitness=True)
            ref = nr.align(nr.Target(prev, 1.0), vox)
            _same(got, ref, ctx.ndt_transformation_probability())
            assert got["converged"]
            if k in (3, 9):
                ndt = NormalDistributionsTransform()
                ndt.setInputSource(vox)
                ndt.setInputTarget(prev)
                ndt.align()
                assert np.array_equal(ndt.getFinalTransformation().view(np.uint32), got["T"].view(np.uint32))
                assert ndt.getFinalNumIteration() == got["iterations"]
                assert ndt.getTransformationProbability() == pytest.approx(ref["probability"], rel=1e-9)
                a, b, g = tmp_path / "s.bin", tmp_path / "t.bin", tmp_path / "g.bin"
                vox.tofile(a)
                prev.tofile(b)
                for guess in (None, synth.pose_matrix(0.25, 0.0, 0.0, 0.0, 0.0, 0.0).astype(F)):
                    args = [str(exe), str(a), str(vox.shape[0]), str(b), str(prev.shape[0]), "1.0"]
                    if guess is not None:
                        np.ascontiguousarray(guess.T).tofile(g)
                        args.append(str(g))
                    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
                    assert r.returncode == 0, r.stderr
                    vals = r.stdout.split()
                    T_cpp = np.array([float(v) for v in vals[4:20]], F).reshape(4, 4).T
                    want = ref if guess is None else nr.align(nr.Target(prev, 1.0), vox, guess=guess)
                    _same(dict(T=T_cpp, iterations=int(vals[1]), state=want["state"], converged=bool(int(vals[0])),
                               n_corr=want["n_corr"]), want, float(vals[2]))
                    if guess is None:
                        assert np.array_equal(T_cpp.view(np.uint32), got["T"].view(np.uint32))
            ctx.promote_source_to_target()
            prev = vox


def test_drive_of_40_scans_through_run_odometry():
    """The reference's online loop with the method through the params, at resolution 0.5 and transformation epsilon 1e-3 (PCL
    1.8's Newton loop takes no line-search trial and, at its defaults, stops after about two clamped steps on this drive: DESIGN.md).
    Drift bound: the end of the 40-scan drive (11.66 m) lies within 1.2 m of synth's ground truth; one MI355X measured 0.945 m
    (the restatement gives the same)."""
    scans, poses = _drive(40)
    with _ctx(resolution=0.5, transformation_epsilon=1e-3) as ctx:
        graph, recs = run_odometry(ctx, scans, voxel_leaf=0.2)
    assert len(recs) == 39 and all(r["accepted"] for r in recs)
    P = np.eye(4)
    for r in recs:
        P = P @ r["T"].astype(np.float64)
    drift = float(np.linalg.norm(P[:3, 3] - poses[-1][:3, 3]))
    assert drift <= 1.2, drift


# ---- errors and edges ------------------------------------------------------------------------------------------------------------
def test_a_target_without_a_cell_returns_the_guess():
    rng = np.random.default_rng(2)
    sparse = _cloud(np.arange(40)[:, None] * np.array([[1.5, 0.0, 0.0]]) + rng.uniform(0, 0.1, (40, 3)))   # 1 point per cell
    src = _cloud(rng.uniform(0, 60, (500, 3)))
    guess = synth.pose_matrix(0.3, 0.1, 0.0, 0.0, 0.0, 0.2).astype(F)
    with _ctx() as ctx:
        ctx.set_target(sparse)
        ctx.set_source(src)
        assert len(ctx.ndt_cells()["n_points"]) == 0
        for g in (None, guess):
            r = ctx.align(guess=g)
            assert r["state"] == NO_CORRESPONDENCES and r["iterations"] == 0 and r["converged"] and r["n_corr"] == 0
            assert np.array_equal(r["T"], np.eye(4, dtype=F) if g is None else g)


def test_errors_and_edges():
    src, tgt, _ = synth.make_pair(3000, 3000, seed=6)
    with _ctx() as ctx, Context(0) as p2p:
        # missing inputs and empty clouds: what the other methods do
        for c in (ctx, p2p):
            with pytest.raises(IcpGpuError) as e:
                c.align()
            assert e.value.code == _lib.ERR_NO_INPUT
        with pytest.raises(IcpGpuError) as e:
            ctx.ndt_derivatives(np.zeros(6))
        assert e.value.code == _lib.ERR_NO_INPUT
        for c in (ctx, p2p):
            c.set_source(src)
            c.set_target(np.zeros((0, 4), F))
        r, r_p2p = ctx.align(), p2p.align()
        assert not r["converged"] and not r_p2p["converged"] and np.array_equal(r["T"], r_p2p["T"])
        ctx.set_target(tgt)
        ctx.set_source(np.zeros((0, 4), F))
        r = ctx.align()
        assert r["state"] == NO_CORRESPONDENCES and r["n_corr"] == 0
        # bad parameters
        for bad in ((0.0, 0.1, 0.55), (-1.0, 0.1, 0.55), (1.0, 0.0, 0.55), (1.0, -0.1, 0.55), (1.0, 0.1, 0.0), (1.0, 0.1, 1.0),
                    (1.0, 0.1, 1.5), (np.nan, 0.1, 0.55)):
            with pytest.raises(IcpGpuError) as e:
                ctx.set_ndt_params(*bad)
            assert e.value.code == _lib.ERR_INVALID_ARG
        assert ctx.get_ndt_params() == dict(resolution=1.0, step_size=0.1, outlier_ratio=0.55)
        # no batch path
        ctx.set_source(src)
        with pytest.raises(IcpGpuError) as e:
            ctx.align_batch([src], [tgt])
        assert e.value.code == _lib.ERR_UNSUPPORTED
    params = _lib.Params()
    _lib.load().icpgpu_default_params(params)
    params.method = NDT
    with pytest.raises(IcpGpuError) as e:
        align_batch_multi([0], [src], [tgt], params=params, communicator=COMM_NONE)
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_cell_lifetime():
    """Cells are kept while the target is the same cloud (recognised included); a new or promoted target or another resolution
    rebuilds them.  Observed through icpgpu_ndt_cells: what it returns is always the current target's cells."""
    a, b, _ = synth.make_pair(6000, 6000, seed=12)
    with _ctx() as ctx:
        ctx.set_target(b)
        ctx.set_source(a)
        cb = ctx.ndt_cells()
        r1 = ctx.align()
        ctx.set_target(b)                                              # the same cloud: recognised, cells kept
        assert ctx.profile().targets_recognised >= 1
        assert np.array_equal(ctx.ndt_cells()["mean"], cb["mean"])
        r2 = ctx.align()
        assert np.array_equal(r1["T"], r2["T"])
        ctx.promote_source_to_target()                                 # a is the target now
        ca = ctx.ndt_cells()
        assert np.array_equal(ca["mean"], nr.valid_cells(nr.cells(a, 1.0))["mean"])
        ctx.set_ndt_params(0.7, 0.1, 0.55)                             # another resolution
        c07 = ctx.ndt_cells()
        assert np.array_equal(c07["mean"], nr.valid_cells(nr.cells(a, 0.7))["mean"])
        ctx.set_target(b)                                              # a new target
        ctx.set_ndt_params(1.0, 0.1, 0.55)
        assert np.array_equal(ctx.ndt_cells()["mean"], cb["mean"])
