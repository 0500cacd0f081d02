"""Point-to-plane ICP (method P2PLANE: pcl::IterativeClosestPointWithNormals + TransformationEstimationPointToPlaneLLS) on the device.

The restatements are written here, from the oracle's pieces: its normals (oracle.gicp_normals), its nearest neighbours and its float32
transform (the reduction), and the point-to-point restatement's DefaultConvergenceCriteria (the loop).  Parity against PCL binaries is
unpinned, as for every other mode."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from icpslam_amd import P2PLANE, Context, IterativeClosestPointWithNormals, _lib, synth
from icpslam_amd._lib import IcpGpuError
from icpslam_amd.registration import solve_point_to_plane

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3                                        # PCL gicp_epsilon_
F = np.float32
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)


def _ctx(**kw):
    c = Context(0)
    c.set_params(c.default_params(), method=P2PLANE, **kw)
    return c


# ---- normals ---------------------------------------------------------------------------------------------------------------------
def _check_normals(cloud, nrm, gicp_cov):
    """nrm against the oracle's normals bit for bit (direction and orientation: oracle.gicp_normals, itself pinned to a NumPy
    restatement in tests/test_oracle.py), the oracle's covariances (finite points: I - C = (1 - eps) n n^T) and the orientation
    rule; NaN exactly where the covariance kernels write their identity marker (gicp_cov: the device's GICP covariances, C == I bit
    for bit), which is where the point is not finite (the oracle computes a covariance there: it is compared on finite points only)."""
    assert np.array_equal(nrm.view(np.uint32), oracle.gicp_normals(cloud).view(np.uint32))
    finite = np.isfinite(cloud[:, :3]).all(axis=1)
    marker = np.all(gicp_cov.reshape(-1, 9) == np.eye(3).reshape(9), axis=1)
    nan = np.isnan(nrm[:, :3]).any(axis=1)
    assert np.array_equal(marker, nan) and np.array_equal(nan, ~finite), (int(marker.sum()), int(nan.sum()), int((~finite).sum()))
    assert np.isnan(nrm[nan, :3]).all() and (nrm[~nan, 3] == 0).all()
    C = oracle.gicp_covariances(cloud)
    ok = finite
    n = nrm[ok, :3].astype(np.float64)
    want = (np.eye(3) - C[ok]) / (1.0 - EPS)
    assert float(np.abs(n[:, :, None] * n[:, None, :] - want).max()) <= 1e-6
    # flipNormalTowardsViewpoint, viewpoint (0, 0, 0): ((vx nx + vy ny) + vz nz) in float32, v = 0 - p, flipped when < 0
    v = (F(0) - cloud[ok, :3]).astype(F)
    m = nrm[ok, :3]
    cos = ((v[:, 0] * m[:, 0] + v[:, 1] * m[:, 1]).astype(F) + v[:, 2] * m[:, 2]).astype(F)
    assert not (cos < 0).any()
    return int(ok.sum())


def test_normals_match_the_oracle_covariances():
    raw = synth.scan(synth.make_scene(21), np.eye(4), 200000, seed=9)
    raw[::997, 1] = np.nan                                             # non-finite points: the marker (the filter keeps some)
    vox = oracle.voxel_grid(raw, 0.2)
    small = synth.make_pair(4000, 4000, seed=3)[1]
    with Context(0) as ctx:
        for cloud in (small, vox, raw):
            ctx.set_target(cloud)
            got = ctx.normals(of_target=True)
            assert got.shape == cloud.shape and _check_normals(cloud, got, ctx.gicp_covariances(of_target=True)) > 0.99 * cloud.shape[0]
            ctx.set_source(cloud)                                      # the source's estimate is the same computation
            assert np.array_equal(ctx.normals(of_target=False).view(np.uint32), got.view(np.uint32))
        assert 15000 < vox.shape[0] < 40000 and not np.isfinite(raw).all()


def test_normals_on_the_wall_through_the_sensor_and_at_the_origin():
    """A wall y ~ 0 through the sensor: the normal (~ +-y) is nearly perpendicular to the view ray, so the flip depends on the last
    bits of U, and the moment sums round (their order shows); a point exactly at the viewpoint has cos = 0 and is never flipped;
    a plane through the origin.  Bit for bit the oracle's normals."""
    wall = synth.wall_through_sensor(40000, seed=2)
    wall[123, :3] = 0.0
    plane = synth.plane_through_origin(40000, seed=3)
    plane[7, :3] = 0.0
    with Context(0) as ctx:
        for cloud in (wall, plane):
            ctx.set_target(cloud)
            got = ctx.normals(of_target=True)
            assert _check_normals(cloud, got, ctx.gicp_covariances(of_target=True)) == cloud.shape[0]


def test_normals_of_a_cloud_with_fewer_than_20_finite_points_are_nan():
    cloud = synth.make_pair(40, 40, seed=2)[0]
    cloud[::2, 0] = np.nan                                             # 20 of 40 non-finite: 20 finite points left, still enough
    cloud[1, 2] = np.inf                                               # 19
    with Context(0) as ctx:
        ctx.set_target(cloud)
        nrm = ctx.normals()
        # GICP's own covariances of such a cloud are an argument error (fewer than 20 FINITE points is too small, include/icpgpu.h;
        # they used to come back as identity markers), before and after the normals were asked for; the normals keep their rule
        for _ in range(2):
            with pytest.raises(IcpGpuError) as e:
                ctx.gicp_covariances(of_target=True)
            assert e.value.code == _lib.ERR_INVALID_ARG and "20" in str(e.value)
        again = ctx.normals()
    assert np.isnan(nrm[:, :3]).all()
    assert np.array_equal(nrm.view(np.uint32), oracle.gicp_normals(cloud).view(np.uint32))
    assert np.array_equal(again.view(np.uint32), nrm.view(np.uint32))


# ---- the reduction ---------------------------------------------------------------------------------------------------------------
def _terms(s, d, n):
    """TransformationEstimationPointToPlaneLLS's float terms (each operation rounded to float32), widened to double."""
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    a = (nz * sy).astype(F) - (ny * sz).astype(F)
    b = (nx * sz).astype(F) - (nz * sx).astype(F)
    c = (ny * sx).astype(F) - (nx * sy).astype(F)
    r = ((nx * d[:, 0]).astype(F) + (ny * d[:, 1]).astype(F)).astype(F) + (nz * d[:, 2]).astype(F)
    r = (r.astype(F) - (nx * sx).astype(F)).astype(F)
    r = (r - (ny * sy).astype(F)).astype(F)
    r = (r - (nz * sz).astype(F)).astype(F)
    A = np.column_stack([a, b, c, nx, ny, nz]).astype(F).astype(np.float64)
    return A, r.astype(np.float64)


def _restated_sums(src, tgt, nrm, T, max_dist):
    """(sums[29], abs-sums[29], n) over oracle.nn's correspondences under T: the accept rule (double)d2 <= max_dist^2."""
    idx, d2 = oracle.nn(src, tgt, T)
    keep = (idx >= 0) & (d2.astype(np.float64) <= max_dist * max_dist)
    s = oracle.transform_cloud(src, T)[keep, :3].astype(F)
    j = idx[keep]
    d, n = tgt[j, :3].astype(F), nrm[j, :3].astype(F)
    fin = np.isfinite(n).all(axis=1)
    A, r = _terms(s[fin], d[fin], n[fin])
    iu = np.triu_indices(6)
    P = (A[:, :, None] * A[:, None, :])[:, iu[0], iu[1]]
    R = A * r[:, None]
    dd = d2[keep].astype(np.float64)
    sums = np.concatenate([[keep.sum(), dd.sum()], P.sum(0), R.sum(0)])
    mags = np.concatenate([[keep.sum(), dd.sum()], np.abs(P).sum(0), np.abs(R).sum(0)])
    return sums, mags, int(keep.sum()), idx


def test_reduction_matches_the_restatement_and_is_deterministic():
    src, tgt, T_gt = synth.make_pair(20000, 20000, seed=4)
    tgt[::501, 0] = np.nan
    T = np.asarray(T_gt, np.float32)
    T[:3, 3] += F(0.05)
    with _ctx() as c1, _ctx() as c2:
        for c in (c1, c2):
            c.set_source(src)
            c.set_target(tgt)
        nrm = c1.normals()
        ref, mags, n, idx = _restated_sums(src, tgt, nrm, T, 1.0)
        idx_dev, _ = c1.nn(T)
        assert np.array_equal(idx_dev, idx)
        got = c1.reduce_point_to_plane(T, 1.0)
        assert int(got[0]) == n and got[0] == ref[0]
        assert np.all(np.abs(got[1:] - ref[1:]) <= 1e-12 * mags[1:]), np.abs(got - ref) / np.maximum(mags, 1e-300)
        assert np.array_equal(got.view(np.uint64), c1.reduce_point_to_plane(T, 1.0).view(np.uint64))
        c2.nn(T)
        assert np.array_equal(got.view(np.uint64), c2.reduce_point_to_plane(T, 1.0).view(np.uint64))


# ---- the whole loop --------------------------------------------------------------------------------------------------------------
def restated_align(src, tgt, nrm, max_iterations=10, eps=1e-6, max_dist=1.0, min_corr=3, guess=None):
    """pcl::IterativeClosestPointWithNormals::align restated: the point-to-point loop (oracle/icp_oracle_np.py's convergence
    criteria) with the point-to-plane solve; the 6 x 6 solve itself is the library's host function (tested against NumPy in
    tests/test_point_to_plane_host.py)."""
    final = np.eye(4) if guess is None else np.asarray(guess, np.float64)
    mse_prev, nr, state, conv, n_c, mse = np.finfo(np.float64).max, 0, NOT_CONVERGED, False, 0, 0.0
    while True:
        sums, _, n_c, _ = _restated_sums(src, tgt, nrm, final.astype(F), max_dist)
        if n_c < min_corr:
            state, conv = NO_CORRESPONDENCES, False
            break
        Tk = solve_point_to_plane(sums)
        if Tk is None:
            state, conv = NOT_CONVERGED, False
            break
        final = Tk @ final
        mse = sums[1] / sums[0]
        nr += 1
        if nr >= max_iterations:
            conv, state = True, ITERATIONS
        else:
            cos_angle = 0.5 * (np.trace(Tk[:3, :3]) - 1.0)
            if cos_angle >= 1.0 - eps and float(Tk[:3, 3] @ Tk[:3, 3]) <= eps:
                conv, state = True, TRANSFORM
            elif abs(mse - mse_prev) < 1e-12:
                conv, state = True, ABS_MSE
            mse_prev = mse
        if conv:
            break
    return dict(T=final.astype(F), converged=conv, iterations=nr, state=state, n_corr=n_c)


def _supplied_normals(cloud):
    """Normals a PointNormal cloud could carry: the oracle covariance's plane direction (eigh), NaN at the markers."""
    C = oracle.gicp_covariances(cloud)
    w, V = np.linalg.eigh(np.eye(3) - C)
    n = np.zeros((cloud.shape[0], 4), F)
    n[:, :3] = V[:, :, 2]
    n[np.all(C.reshape(-1, 9) == np.eye(3).reshape(9), axis=1), :3] = np.nan
    return n


def _same(got, ref):
    assert (got["iterations"], got["state"], got["n_corr"]) == (ref["iterations"], ref["state"], ref["n_corr"]), (got, ref)
    assert got["converged"] == ref["converged"]
    assert np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max() <= 1e-4
    assert np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]) <= 1e-3


@pytest.mark.parametrize("n", [5000, 50000])
def test_alignment_matches_the_restatement(n):
    with _ctx() as ctx:
        for seed in range(20):
            src, tgt, _ = synth.make_pair(n, n, seed=100 + seed)
            ctx.set_target(tgt)
            ctx.set_source(src)
            got = ctx.align()
            ref = restated_align(src, tgt, oracle.gicp_normals(tgt))
            _same(got, ref)
            sup = _supplied_normals(tgt)
            ctx.set_target_normals(sup)
            _same(ctx.align(), restated_align(src, tgt, sup))


def test_alignment_at_200k():
    src, tgt, _ = synth.make_pair(200000, 200000, seed=77)
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        got = ctx.align(want_fitness=True)
        _same(got, restated_align(src, tgt, oracle.gicp_normals(tgt)))
        assert np.isfinite(got["fitness"])


def test_known_answer():
    for seed in range(3):
        src, tgt, T_gt = synth.make_known_answer_pair(8000, seed=seed)
        with _ctx(max_iterations=50) as ctx:
            ctx.set_target(tgt)
            ctx.set_source(src)
            got = ctx.align()
        assert np.abs(got["T"][:3, :3] - T_gt[:3, :3]).max() <= 1e-4, seed
        assert np.linalg.norm(got["T"][:3, 3] - T_gt[:3, 3]) <= 1e-3, seed


# ---- a drive ---------------------------------------------------------------------------------------------------------------------
def _drive(n_scans, n_pts=60000, seed=8):
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(321)
    poses = [np.eye(4)]
    for _ in range(n_scans - 1):
        poses.append(poses[-1] @ synth.pose_matrix(0.3, rng.uniform(-0.03, 0.03), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-2, 2))))
    return [synth.scan(scene, P, n_pts, seed=900 + k) for k, P in enumerate(poses)]


def _demo(tmp_path):
    exe = tmp_path / "p2plane_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "p2plane_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_drive_of_40_scans_and_the_cpp_shim(tmp_path):
    """voxel filter -> P2PLANE -> promote, scan by scan, against the restatement; on some pairs the C++ shim's
    IterativeClosestPointWithNormals gives the Python front end's T bit for bit (estimated and supplied normals)."""
    scans = _drive(40)
    exe = _demo(tmp_path)
    shim_pairs = {5, 20, 39}
    with _ctx() as ctx:
        prev = None
        for k, raw in enumerate(scans):
            vox = ctx.voxel_grid(raw, 0.2)
            assert np.array_equal(vox, oracle.voxel_grid(raw, 0.2))
            ctx.set_source(vox)
            if prev is None:
                ctx.promote_source_to_target()
                prev = vox
                continue
            got = ctx.align(want_fitness=True)
            nrm = ctx.normals()
            _same(got, restated_align(vox, prev, nrm))
            assert got["converged"]
            if k in shim_pairs:
                icp = IterativeClosestPointWithNormals()
                icp.setMaximumIterations(10)
                icp.setTransformationEpsilon(1e-6)
                icp.setMaxCorrespondenceDistance(1.0)
                a, b, nb = tmp_path / "s.bin", tmp_path / "t.bin", tmp_path / "n.bin"
                vox.tofile(a)
                prev.tofile(b)
                for normals in (None, _supplied_normals(prev)):
                    icp.setInputSource(vox)
                    icp.setInputTarget(prev, normals=normals)
                    icp.align()
                    T_py = icp.getFinalTransformation()
                    args = [str(exe), str(a), str(vox.shape[0]), str(b), str(prev.shape[0]), "10"]
                    if normals is not None:
                        normals.tofile(nb)
                        args.append(str(nb))
                    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
                    assert r.returncode == 0, r.stderr
                    vals = r.stdout.split()
                    T_cpp = np.array([float(v) for v in vals[3:19]], np.float32).reshape(4, 4).T
                    assert np.array_equal(T_cpp.view(np.uint32), T_py.view(np.uint32)), k
                    assert int(vals[1]) == icp.result["iterations"]
            ctx.promote_source_to_target()
            prev = vox


def test_sequence_and_mapper_take_the_method():
    from icpslam_amd.mapper import OctreeMapper
    from icpslam_amd.sequence import pose_from_matrix, run_odometry
    scans = _drive(6, n_pts=20000, seed=3)
    with _ctx() as ctx:
        graph, recs = run_odometry(ctx, scans, voxel_leaf=0.2)
        assert len(recs) == 5 and all(r["accepted"] for r in recs)
        assert all(r["iterations"] >= 1 for r in recs)
    with Context(0) as ctx:
        mapper = OctreeMapper(ctx, octree_resolution=0.5, method=P2PLANE)
        poses = [synth.pose_matrix(0.3 * k, 0.0, 0.0, 0.0, 0.0, 0.0) for k in range(4)]
        oks = [mapper.refineTransformAndGrowMap(s, pose_from_matrix(P.astype(np.float32)))[0] for s, P in zip(scans, poses)]
        assert oks[0] is False and all(oks[1:])
        assert ctx.get_params().method == P2PLANE


# ---- errors and edges ------------------------------------------------------------------------------------------------------------
def test_errors_and_edges():
    src, tgt, _ = synth.make_pair(3000, 3000, seed=6)
    with _ctx() as ctx:
        ctx.set_source(src)
        ctx.set_target(tgt)
        with pytest.raises(IcpGpuError) as e:
            ctx.set_target_normals(np.zeros((2999, 4), F))
        assert e.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(IcpGpuError) as e:
            ctx.align_batch([src], [tgt])
        assert e.value.code == _lib.ERR_UNSUPPORTED
        # fewer than 20 points and no normals: GICP's covariances fail with the same code
        tiny = tgt[:19].copy()
        ctx.set_target(tiny)
        with pytest.raises(IcpGpuError) as e_gicp:
            ctx.gicp_covariances(of_target=True)
        for call in (lambda: ctx.normals(), lambda: ctx.align()):
            with pytest.raises(IcpGpuError) as e:
                call()
            assert e.value.code == e_gicp.value.code == _lib.ERR_INVALID_ARG
        ctx.set_target_normals(np.tile(np.array([0, 0, 1, 0], F), (19, 1)))   # ... with normals it runs
        ctx.align()


def test_a_single_plane_stops_with_a_finite_transform():
    g = np.arange(-20, 20, 0.5, dtype=F)
    xx, yy = np.meshgrid(g, g)
    plane = np.column_stack([xx.ravel(), yy.ravel(), np.zeros(xx.size, F), np.ones(xx.size, F)]).astype(F)
    src = plane.copy()
    src[:, 0] += F(0.1)
    src[:, 1] -= F(0.05)
    with _ctx() as ctx:
        ctx.set_target(plane)
        ctx.set_source(src)
        nrm = ctx.normals()
        assert np.array_equal(np.abs(nrm[:, :3]), np.tile(np.array([0, 0, 1], F), (plane.shape[0], 1)))
        r = ctx.align()
    assert not r["converged"] and r["state"] == NOT_CONVERGED and r["iterations"] == 0
    assert np.isfinite(r["T"]).all() and np.array_equal(r["T"], np.eye(4, dtype=F))


def test_normals_lifetime():
    """A recognised target keeps its estimated normals (no covariance pass), a promoted one re-estimates them; supplied normals are
    dropped by set_target, recognised or not."""
    a, b, _ = synth.make_pair(6000, 6000, seed=12)
    with _ctx() as ctx, Context(0) as fresh:
        ctx.set_target(b)
        ctx.set_source(a)
        ctx.align()
        launches = ctx.profile().gicp_cov_launches
        ctx.set_target(b)                                                  # the same cloud: recognised
        assert ctx.profile().targets_recognised >= 1
        ctx.align()
        assert ctx.profile().gicp_cov_launches == launches
        sup = _supplied_normals(b)
        ctx.set_target_normals(sup)
        assert np.array_equal(ctx.normals().view(np.uint32), sup.view(np.uint32))
        ctx.set_target(b)                                                  # recognised again: the caller's normals are gone
        fresh.set_target(b)
        est = fresh.normals()
        assert np.array_equal(ctx.normals().view(np.uint32), est.view(np.uint32))
        assert ctx.profile().gicp_cov_launches == launches
        ctx.set_source(a)
        ctx.promote_source_to_target()                                     # a is the target now: its normals are estimated
        fresh.set_target(a)
        assert np.array_equal(ctx.normals().view(np.uint32), fresh.normals().view(np.uint32))
        assert ctx.profile().gicp_cov_launches == launches + 1
