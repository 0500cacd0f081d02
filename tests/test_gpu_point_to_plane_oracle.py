"""Point-to-plane ICP on the device against its C restatement (oracle/p2plane_oracle.c, pinned to the NumPy one in
tests/test_oracle.py), never against the library itself.

replay: every sweep of an oracle alignment (each iteration's float transform, and the last one) is fed to ctx.nn and
        ctx.reduce_point_to_plane: the keys equal oracle.nn's, sums[0] is exact and every other sum is within
        1e-12 * sum |terms| of the oracle's EXACT sum (the device adds in its own order).
whole:  ctx.align against oracle.p2plane_align: converged, iterations, state and n_corr exact, T within the point-to-point
        parity tolerances, mse and fitness within 1e-9 relative."""
import numpy as np
import pytest

import oracle
from icpslam_amd import P2PLANE, Context, IterativeClosestPointWithNormals, _lib, synth

pytestmark = pytest.mark.gpu
F = np.float32
R_TOL, T_TOL = 1e-4, 1e-3                                          # BASELINE.json / DESIGN.md section 3
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
WORST = {"sum_ulps": 0.0, "dR": 0.0, "dt": 0.0}                    # reported at the end of the module (-s)


def _ctx(**kw):
    c = Context(0)
    c.set_params(c.default_params(), method=P2PLANE, **kw)
    return c


def _oparams(kw):
    o = {k: v for k, v in kw.items() if k != "nn_mode"}
    if kw.get("nn_mode") == _lib.NN_BRUTE:
        o["nn_mode"] = oracle.NN_BRUTE
    return oracle.default_params(**o)


def replay(ctx, src, tgt, nrm_used, ref, max_dist=1.0, guess=None):
    """ref = oracle.p2plane_align(..., trace=True): its sweeps on the device; returns the device sums of every sweep"""
    sweeps = [t["final"].astype(F) for t in ref["trace"]] + [ref["T"]]
    if not ref["trace"]:
        sweeps = [np.eye(4, dtype=F) if guess is None else np.asarray(guess, F)]
    out = []
    for T in sweeps:
        idx_dev, d2_dev = ctx.nn(T)
        idx, d2 = oracle.nn(src, tgt, T)
        assert np.array_equal(idx_dev, idx)
        got = ctx.reduce_point_to_plane(T, max_dist)
        want = oracle.p2plane_sums(src, tgt, nrm_used, T, idx, d2, max_dist)
        mag = oracle.p2plane_sums(src, tgt, nrm_used, T, idx, d2, max_dist, mode=oracle.P2PLANE_SUMS_ABS)
        assert got[0] == want[0]
        err = np.abs(got - want)
        assert np.all(err <= 1e-12 * mag), (err / np.maximum(mag, 1e-300)).max()
        nz = mag > 0
        if nz.any():
            WORST["sum_ulps"] = max(WORST["sum_ulps"], float((err[nz] / (mag[nz] * 2.0 ** -53)).max()))
        out.append(got)
    return out


def whole(got, ref, fitness=True):
    assert (got["converged"], got["iterations"], got["state"], got["n_corr"]) == \
        (ref["converged"], ref["iterations"], ref["state"], ref["n_corr"]), (got, {k: ref[k] for k in ("converged", "iterations", "state", "n_corr")})
    dR = float(np.abs(got["T"][:3, :3].astype(np.float64) - ref["T"][:3, :3]).max())
    dt = float(np.linalg.norm(got["T"][:3, 3].astype(np.float64) - ref["T"][:3, 3]))
    WORST["dR"], WORST["dt"] = max(WORST["dR"], dR), max(WORST["dt"], dt)
    assert dR <= R_TOL and dt <= T_TOL, (dR, dt)
    assert abs(got["mse"] - ref["mse"]) <= 1e-9 * abs(ref["mse"]), (got["mse"], ref["mse"])
    if fitness:
        assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * abs(ref["fitness"]), (got["fitness"], ref["fitness"])


def check(src, tgt, normals=None, guess=None, **kw):
    """replay + whole for one case; normals None: the device's estimate (bit for bit oracle.gicp_normals, test_gpu_point_to_plane)"""
    max_dist = kw.get("max_correspondence_distance", 1.0)
    nrm_used = oracle.gicp_normals(tgt) if normals is None else np.ascontiguousarray(normals, F)
    ref = oracle.p2plane_align(src, tgt, _oparams(kw), guess=guess, normals=nrm_used, want_fitness=True)
    with _ctx(**kw) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        if normals is not None:
            ctx.set_target_normals(normals)
        got = ctx.align(guess=guess, want_fitness=True)
        whole(got, ref)
        sums = replay(ctx, src, tgt, nrm_used, ref, max_dist, guess)
    return ref, got, sums


# ---- source sizes: partial workgroups, partial 4-point unrolls, the capped grid's stride loop -----------------------------------
@pytest.mark.parametrize("n_s", [1, 3, 255, 257, 1023, 1025, 4097])
def test_source_sizes(n_s):
    src, tgt, _ = synth.make_pair(max(n_s, 64), 20000, seed=500 + n_s)
    ref, got, _ = check(src[:n_s].copy(), tgt)
    if n_s < 3:
        assert ref["state"] == NO_CORRESPONDENCES


def test_source_of_1_5m_points_runs_the_stride_loop_twice():
    """p2plane_blocks caps the grid at 1024 workgroups of 256 lanes, four points a lane per trip: 1.5M points take two trips"""
    src, tgt, _ = synth.make_pair(1_500_000, 200_000, seed=71)
    assert src.shape[0] > 1024 * 256 * 4
    ref, _, _ = check(src, tgt, max_iterations=3)
    assert ref["n_corr"] > 1_000_000


# ---- the search: brute force, grid and auto give the same keys, the same sum bits, the same result ------------------------------
def test_nn_modes_agree_bit_for_bit():
    src, tgt, _ = synth.make_pair(6000, 6000, seed=72)
    runs = [check(src, tgt, nn_mode=m) for m in (_lib.NN_BRUTE, _lib.NN_GRID, _lib.NN_AUTO)]
    for _, got, sums in runs[1:]:
        assert np.array_equal(np.array(sums).view(np.uint64), np.array(runs[0][2]).view(np.uint64))
        assert np.array_equal(got["T"].view(np.uint32), runs[0][1]["T"].view(np.uint32))


# ---- guesses and the loop's parameters ---------------------------------------------------------------------------------------
def test_guess():
    src, tgt, _ = synth.make_pair(20000, 20000, seed=73)
    check(src, tgt, guess=synth.pose_matrix(0.15, -0.1, 0.03, 0.01, -0.02, 0.03).astype(F))
    far = synth.pose_matrix(500.0, 0.0, 0.0, 0.0, 0.0, 0.0).astype(F)    # no pair within 1 m: fewer than min_correspondences
    ref, got, _ = check(src, tgt, guess=far)
    assert ref["state"] == NO_CORRESPONDENCES and ref["iterations"] == 0 and np.array_equal(got["T"], far)


def test_min_correspondences_at_its_boundary():
    src, tgt, _ = synth.make_pair(3000, 3000, seed=74)
    n0 = oracle.p2plane_align(src, tgt)["trace"][0]["n_corr"]
    ref, _, _ = check(src, tgt, min_correspondences=n0)
    assert ref["iterations"] >= 1
    ref, _, _ = check(src, tgt, min_correspondences=n0 + 1)
    assert ref["state"] == NO_CORRESPONDENCES and ref["iterations"] == 0


@pytest.mark.parametrize("kw,state", [(dict(max_iterations=1), ITERATIONS),
                                      (dict(max_iterations=6, force_iterations=1), ITERATIONS),
                                      (dict(transformation_epsilon=1e-1), TRANSFORM),
                                      (dict(euclidean_fitness_epsilon=5e-2, max_iterations=30), REL_MSE)])
def test_loop_parameters(kw, state):
    src, tgt, _ = synth.make_pair(8000, 8000, seed=75)
    ref, got, _ = check(src, tgt, **kw)
    assert ref["state"] == state
    if kw.get("force_iterations"):
        assert ref["iterations"] == 6


# ---- accept threshold, non-finite points ---------------------------------------------------------------------------------------
def test_pairs_exactly_on_the_accept_threshold():
    """A lattice at 0.5 m (six layers) and its top layer lifted by 0.25 m: every d2 is exactly 0.0625 = r^2 (accepted); every
    other point lifted one ulp more lies just outside.  Normals supplied (a lattice's planes are degenerate)."""
    g = np.arange(0, 10, 0.5, dtype=F)
    xx, yy, zz = np.meshgrid(g, g, g[:6], indexing="ij")
    tgt = np.column_stack([xx.ravel(), yy.ravel(), zz.ravel(), np.ones(xx.size, F)]).astype(F)
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=(tgt.shape[0], 4)).astype(F)
    nrm[:, :3] /= np.linalg.norm(nrm[:, :3], axis=1, keepdims=True)
    src = tgt[tgt[:, 2] == g[5]].copy()
    src[:, 2] += F(0.25)
    src[1::2, 2] = np.nextafter(src[1::2, 2], F(100))
    _, d2 = oracle.nn(src, tgt)
    assert (d2 == F(0.0625)).sum() == (src.shape[0] + 1) // 2 and (d2 > F(0.0625)).sum() == src.shape[0] // 2
    ref, _, _ = check(src, tgt, normals=nrm, max_correspondence_distance=0.25, max_iterations=1)
    assert ref["trace"][0]["n_corr"] == (src.shape[0] + 1) // 2


def test_non_finite_points():
    src, tgt, _ = synth.make_pair(10000, 10000, seed=76)
    src[::97, 1] = np.nan
    src[5::101, 0] = np.inf
    tgt[::89, 2] = np.nan
    tgt[7::103, 1] = -np.inf
    check(src, tgt)


# ---- supplied normals ----------------------------------------------------------------------------------------------------------
def _normals_case(kind, tgt):
    n = oracle.gicp_normals(tgt)
    n[np.isnan(n)] = 0.0
    n[:, 3] = 0.0
    if kind == "scaled":
        n[:, :3] *= F(3.0)
    elif kind == "zero":
        n[::4, :3] = 0.0
    elif kind == "one_nan":
        n[::5, 1] = np.nan
    elif kind == "inf":
        n[::6, 0] = np.inf
        n[3::6, 2] = -np.inf
    elif kind == "w_garbage":
        n[:, 3] = np.random.default_rng(0).normal(size=n.shape[0]).astype(F) * F(1e30)
        n[::7, 3] = np.nan
    return n


@pytest.mark.parametrize("kind", ["scaled", "zero", "one_nan", "inf", "w_garbage"])
def test_supplied_normals(kind):
    src, tgt, _ = synth.make_pair(12000, 12000, seed=77)
    check(src, tgt, normals=_normals_case(kind, tgt))


@pytest.mark.parametrize("with_guess", [False, True])
def test_all_normals_nan_is_singular(with_guess):
    src, tgt, _ = synth.make_pair(5000, 5000, seed=78)
    guess = synth.pose_matrix(0.1, 0.0, 0.0, 0.0, 0.0, 0.02).astype(F) if with_guess else None
    ref, got, _ = check(src, tgt, normals=np.full((tgt.shape[0], 4), np.nan, F), guess=guess)
    assert (ref["state"], ref["iterations"], ref["converged"]) == (NOT_CONVERGED, 0, False)
    assert np.array_equal(got["T"], np.eye(4, dtype=F) if guess is None else guess)


# ---- cancellation: far from the origin, a wall through the sensor --------------------------------------------------------------
def test_clouds_3km_from_the_origin():
    src, tgt, _ = synth.make_pair(20000, 20000, seed=79)
    off = np.array([3000.0, -1200.0, 40.0, 0.0], F)
    check(src + off, tgt + off)


def test_wall_through_the_sensor():
    wall = synth.wall_through_sensor(30000, seed=4)
    scene = synth.make_pair(20000, 20000, seed=80)[1]
    tgt = np.concatenate([wall, scene]).astype(F)
    src = oracle.transform_cloud(tgt[::2], synth.pose_matrix(0.05, 0.02, 0.0, 0.0, 0.0, 0.01))
    check(src, tgt)


# ---- the mapper and the C++-style front end -------------------------------------------------------------------------------------
def test_mapper_against_the_oracle_octree():
    from icpslam_amd.mapper import OctreeMapper
    from icpslam_amd.sequence import pose_from_matrix, pose_inverse, pose_to_matrix
    rng = np.random.default_rng(5)
    scene = synth.make_scene(321)
    poses = [np.eye(4)]
    for _ in range(4):
        poses.append(poses[-1] @ synth.pose_matrix(0.3, rng.uniform(-0.03, 0.03), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-2, 2))))
    scans = [oracle.voxel_grid(synth.scan(scene, P, 60000, seed=40 + k), 0.2) for k, P in enumerate(poses)]
    octree = oracle.PclOctreeMap(0.5)
    with Context(0) as ctx:
        mapper = OctreeMapper(ctx, octree_resolution=0.5, method=P2PLANE, pcl_approx_search=True)
        for k, (scan, P) in enumerate(zip(scans, poses)):
            raw = pose_from_matrix(P.astype(F))
            Pm, Pinv = pose_to_matrix(raw), pose_to_matrix(pose_inverse(raw))
            if k == 0:
                mapper.refineTransformAndGrowMap(scan, raw)
                octree.add_points(scan, Pm)
            else:
                nn_dev = mapper.approxNearestNeighbors(scan, raw, want_cloud=True)
                nn = octree.nn_cloud(scan, Pm, Pinv)
                assert np.array_equal(nn_dev.view(np.uint32), nn.view(np.uint32)), k
                ok, transform, refined, info = mapper.refineTransformAndGrowMap(scan, raw)
                ref = oracle.p2plane_align(scan, nn, oracle.default_params(max_iterations=30, transformation_epsilon=1e-6))
                whole(info["icp"], ref, fitness=False)
                assert ok == ref["converged"]
                if ok:
                    octree.add_points(scan, pose_to_matrix(refined))
            assert np.array_equal(ctx.map_points().view(np.uint32), octree.points().view(np.uint32)), k


def test_front_end_with_a_guess_and_fitness():
    src, tgt, _ = synth.make_pair(15000, 15000, seed=81)
    guess = synth.pose_matrix(0.1, -0.05, 0.0, 0.0, 0.0, 0.02).astype(F)
    nrm = _normals_case("scaled", tgt)
    for normals in (None, nrm):
        icp = IterativeClosestPointWithNormals()
        icp.setMaximumIterations(10)
        icp.setTransformationEpsilon(1e-6)
        icp.setMaxCorrespondenceDistance(1.0)
        icp.setInputSource(src)
        icp.setInputTarget(tgt, normals=normals)
        icp.align(guess)
        ref = oracle.p2plane_align(src, tgt, guess=guess, normals=normals, want_fitness=True)
        r = icp.result
        assert (r["iterations"], r["state"], r["n_corr"]) == (ref["iterations"], ref["state"], ref["n_corr"])
        T = icp.getFinalTransformation()
        assert np.abs(T[:3, :3] - ref["T"][:3, :3]).max() <= R_TOL and np.linalg.norm(T[:3, 3] - ref["T"][:3, 3]) <= T_TOL
        fit = icp.getFitnessScore()
        assert abs(fit - ref["fitness"]) <= 1e-9 * ref["fitness"]


def test_zz_report_worst_differences():
    """(the largest differences against the oracle seen by this module; printed with -s)"""
    print(f"\nP2PLANE vs oracle: worst |dR| {WORST['dR']:.3g}, |dt| {WORST['dt']:.3g} m, "
          f"worst sum error {WORST['sum_ulps']:.3g} x sum|terms| 2^-53")
