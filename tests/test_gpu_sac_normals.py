"""The segmentation from normals on the device (icpgpu_sac_segmentation_from_normals / icpgpu_sac_normals_fetch / icpgpu_sac_extract;
icp_sac_normals.hip) against the NumPy restatement (tests/sac_normals_restated.py), bit for bit at every stage and for both models:
the count of every iteration, the iterations, the best hypothesis and its sample, the unrefined coefficients and inlier count, the
final coefficients and the inlier indices.  The refinement's sums -- the plane's nine, exact, and the 21 of every cylinder pass,
within 1e-12 of the sum of their terms' magnitudes of math.fsum -- and then the restatement's refinement run on the device's own
sums, which must give the device's coefficients bit for bit."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import sac_normals_cases as CS
import sac_normals_restated as R
import sac_restated as SR
from icpslam_amd import Context, IcpGpuError, SACSegmentationFromNormals, _lib, synth
from icpslam_amd import SAC_RANSAC, SACMODEL_CYLINDER, SACMODEL_NORMAL_PLANE

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "sac_normals_2k.npz")
BLOCK_POINTS, GRID_CAP = 512, 1024          # icp_kernels.h: kSacnBlockPoints, kSacnGridCap
PLANE, CYL = SACMODEL_NORMAL_PLANE, SACMODEL_CYLINDER
STAGES = ("counts", "sample", "coeff_unrefined", "coeff", "inliers")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5):
    """A scan and pseudo-normals for it: unit vectors scattered about +z with curvatures in [0, 0.3) -- any finite rows serve a
    bit-for-bit comparison."""
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    rng = np.random.default_rng(seed + 100)
    v = rng.normal(0, 0.35, (n, 3)) + [0.0, 0.0, 1.0]
    nr = np.concatenate((v / np.linalg.norm(v, axis=1, keepdims=True), rng.uniform(0, 0.3, (n, 1))), axis=1).astype(F32)
    c.setflags(write=False)
    nr.setflags(write=False)
    return c, nr


def device(ctx, model, normals, threshold, weight=0.1, rmin=0.0, rmax=0.0, max_iterations=50, probability=0.99, seed=0, optimize=True, axis=None,
           eps_angle=0.0) -> dict:
    rc, coeff, n_coeff, n_inliers, iterations, found = ctx.sac_segmentation_from_normals_raw(model, normals, threshold, weight, rmin, rmax,
                                                                                            max_iterations, probability, seed, optimize, axis, eps_angle)
    assert rc == 0, ctx._L.icpgpu_last_error(ctx._h)
    nc = 4 if model == PLANE else 7
    assert n_coeff == (nc if found else 0) and not coeff[nc:].any()
    rc, f = ctx.sac_normals_fetch_raw(n_inliers, iterations)
    assert rc == 0
    passes = f["cylinder_passes"]
    assert not f["cylinder_sums"][passes:].any()
    return {"counts": f["counts"], "iterations": iterations, "best_t": f["best_t"], "sample": f["sample"], "coeff_unrefined": f["coeff_unrefined"][:nc],
            "n_unrefined": f["n_unrefined"], "moments": f["moments"], "cylinder_sums": f["cylinder_sums"][:passes], "cylinder_stop": f["cylinder_stop"],
            "coeff": coeff[:nc], "inliers": f["inliers"], "found": found}


def assert_same(got: dict, want: dict, what=""):
    for name in ("iterations", "best_t", "n_unrefined", "found"):
        assert got[name] == want[name], (what, name, got[name], want[name])
    for name in STAGES:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, g[:8], w[:8])


def check(ctx, model, cloud, normals, threshold, weight=0.1, rmin=0.0, rmax=0.0, max_iterations=50, probability=0.99, seed=0, optimize=True,
          axis=None, eps_angle=0.0, want=None) -> dict:
    """The device against the restatement; then the sums, the refinement from the device's own sums, the selection under the
    device's own coefficients and the host waits.  A refined cylinder's sums may differ from math.fsum's in the last bits (they are
    double-double sums of inexact terms), so its final stages are held to the restatement run on the device's own sums, and to the
    restatement's own answer wherever the sums agree."""
    args = (threshold, weight, rmin, rmax, max_iterations, probability, seed, optimize, axis, eps_angle)
    got = device(ctx, model, normals, *args)
    want = R.segment(model, cloud, normals, *args) if want is None else want
    what = f"model {model} n {len(cloud)} args {args}"
    xyz = np.asarray(cloud, F32).reshape(-1, 4)
    if model == CYL and optimize and want["n_unrefined"] >= 5:
        for name in ("iterations", "best_t", "n_unrefined", "found"):
            assert got[name] == want[name], (what, name)
        for name in ("counts", "sample", "coeff_unrefined"):
            assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), (what, name)
        unrefined = np.flatnonzero(R.inlier_mask(model, cloud, normals, got["coeff_unrefined"], threshold, weight))
        assert unrefined.size == got["n_unrefined"]
        # every pass's sums against math.fsum of the terms at the chart point the DEVICE's sums lead to
        fs = R.fsum_pass(cloud, unrefined)
        device_sums = iter(got["cylinder_sums"])
        index = [0]

        def replay(P, D, ia, ib, r):
            S = next(device_sums)
            T = R.cyl_terms(P, D, ia, ib, r, xyz[unrefined, :3])
            ref = np.array(fs(P, D, ia, ib, r))
            bound = 1e-12 * np.abs(T).sum(axis=0)
            assert (np.abs(S - ref) <= bound).all(), (what, "pass", index[0], S, ref)
            index[0] += 1
            return S
        coeff, sums, stop = R.cyl_refine(got["coeff_unrefined"], xyz[got["sample"][0], :3], replay)
        assert sums.shape == got["cylinder_sums"].shape and stop == got["cylinder_stop"], (what, stop, got["cylinder_stop"])
        assert coeff.tobytes() == got["coeff"].tobytes(), (what, coeff, got["coeff"])
        kept = sums[-2] if stop == R.STOP_NO_DECREASE else sums[-1]                    # (a refused step's pass is the last one)
        assert 1 <= sums.shape[0] <= R.CYLINDER_ITERATIONS and kept[20] <= sums[0, 20]
        if sums.tobytes() == want["cylinder_sums"].tobytes():
            assert_same(got, want, what)
    else:
        assert_same(got, want, what)
        assert got["cylinder_sums"].shape[0] == 0 and got["cylinder_stop"] == 0
    if model == PLANE and optimize and got["n_unrefined"] >= 3:
        assert got["moments"].tobytes() == want["moments"].tobytes(), what           # (exact sums: equal to math.fsum's)
        assert SR.refine(got["moments"], xyz[got["sample"][0], :3], got["n_unrefined"], got["coeff_unrefined"]).tobytes() == got["coeff"].tobytes()
    else:
        assert not got["moments"].any()
    if got["found"]:
        assert np.array_equal(np.flatnonzero(R.inlier_mask(model, cloud, normals, got["coeff"], threshold, weight)), got["inliers"]), what
        assert (np.diff(got["inliers"]) > 0).all()
    assert ctx.sac_normals_host_waits() == R.expected_waits(got, optimize, model), what
    return got


# ---- sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [PLANE, CYL])
@pytest.mark.parametrize("n", [2, 3, 4, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 3000])
def test_sizes(ctx, model, n):
    cloud, normals = (a[:n] for a in scan(3000))
    ctx.search_set_input(cloud)
    for seed, optimize, threshold in ((0, True, 0.2), (11, False, 0.2), (2**64 - 3, True, 0.05)):
        got = check(ctx, model, cloud, normals, threshold, 0.1, 0.0, 0.0, 50, 0.99, seed, optimize)
        assert got["iterations"] == got["counts"].size
    if n == 3000 and model == PLANE:
        assert got["found"] == 1
    if n == 2 and model == PLANE:
        assert got["found"] == 0 and (got["counts"] == -1).all()


@pytest.mark.parametrize("model", [PLANE, CYL])
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_sizes_around_the_compactions_tile(ctx, model, n):
    cloud, normals = (a[:n] for a in scan(4097))
    ctx.search_set_input(cloud)
    got = check(ctx, model, cloud, normals, 0.3, 0.1, 0.0, 0.0, 50, 0.99, 0, True)
    assert got["found"] == 1
    mask = np.zeros(n, bool)
    mask[got["inliers"]] = True
    for negative in (False, True):
        for view in (False, True):
            assert ctx.sac_extract(negative, view).tobytes() == cloud[mask != negative].tobytes()
    rc, f = ctx.sac_normals_fetch_raw(got["inliers"].size, got["iterations"])        # the extracts left the result alone
    assert rc == 0 and np.array_equal(f["inliers"], got["inliers"])


@pytest.mark.parametrize("n", [BLOCK_POINTS * GRID_CAP, BLOCK_POINTS * GRID_CAP + 1])
def test_either_side_of_the_counting_grids_cap(ctx, n):
    """At 512 * 1024 points every workgroup takes one step; one point more and the first takes a second one."""
    base, base_n = scan(4096)
    reps = -(-n // 4096)
    rng = np.random.default_rng(1)
    cloud = np.tile(base, (reps, 1))[:n].copy()
    cloud[:, :3] += rng.normal(0, 0.01, (n, 3)).astype(F32)
    normals = np.tile(base_n, (reps, 1))[:n]
    ctx.search_set_input(cloud)
    for model in (PLANE, CYL):
        got = check(ctx, model, cloud, normals, 0.2, 0.1, 0.0, 0.0, 3, 0.99, 4, False)
        assert got["iterations"] == 3


# ---- the loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [PLANE, CYL])
@pytest.mark.parametrize("max_iterations", [0, 1, 63, 64, 65, 129])
def test_iteration_limits_on_a_low_inlier_scene(ctx, model, max_iterations):
    """Scattered points with random normals: no hypothesis gathers enough inliers to stop the loop, which runs across batches."""
    rng = np.random.default_rng(7)
    cloud = CS.rows(rng.uniform(-5, 5, (700, 3)))
    normals = scan(700)[1]
    ctx.search_set_input(cloud)
    got = check(ctx, model, cloud, normals, 0.05, 0.1, 0.0, 0.0, max_iterations, 0.99, 3, True)
    assert got["iterations"] == max_iterations
    assert ctx.sac_normals_host_waits() >= -(-max_iterations // 64)


def test_a_high_inlier_scene_stops_in_the_first_batch(ctx):
    cloud, normals, n_floor = CS.floor_and_wall(900, 100)
    ctx.search_set_input(cloud)
    got = check(ctx, PLANE, cloud, normals, 0.05, 0.1, 0.0, 0.0, 1000, 0.99, 1, True)
    assert got["found"] == 1 and got["iterations"] < 64 and (got["inliers"] < n_floor).all()
    pole, pole_n = CS.cylinder((0, 0, 0), (0, 0, 1), 0.2, 500, np.random.default_rng(2))
    ctx.search_set_input(pole)
    got = check(ctx, CYL, pole, pole_n, 0.02, 0.1, 0.0, 0.0, 1000, 0.99, 1, True)
    assert got["found"] == 1 and got["iterations"] < 64 and got["inliers"].size == 500


# ---- the hand cases ----------------------------------------------------------------------------------------------------------
def test_floor_and_wall(ctx):
    """At the same threshold the plain plane takes in the wall's foot and NORMAL_PLANE does not; weight 0 is the plane call byte for
    byte; weight 1 lets the angle alone decide."""
    cloud, normals, n_floor = CS.floor_and_wall()
    ctx.search_set_input(cloud)
    got = check(ctx, PLANE, cloud, normals, 0.05, 0.1, 0.0, 0.0, 50, 0.99, 0, True)
    assert (got["inliers"] < n_floor).all() and got["inliers"].size == n_floor
    for optimize in (True, False):
        rc, coeff, n_in, it, found = ctx.sac_segment_raw(0.05, 50, 0.99, 0, optimize)
        assert rc == 0
        rc, plain = ctx.sac_fetch_raw(n_in, it)
        assert rc == 0 and (plain["inliers"] >= n_floor).sum() > 10
        zero = check(ctx, PLANE, cloud, normals, 0.05, 0.0, 0.0, 0.0, 50, 0.99, 0, optimize)
        assert zero["coeff"].tobytes() == coeff.tobytes() and zero["iterations"] == it and zero["found"] == found
        for name in ("inliers", "counts", "sample", "moments"):
            assert zero[name].tobytes() == plain[name].tobytes(), name
        assert zero["coeff_unrefined"].tobytes() == plain["coeff_unrefined"].tobytes() and zero["n_unrefined"] == plain["n_unrefined"]
    one = check(ctx, PLANE, cloud, normals, 0.05, 1.0, 0.0, 0.0, 50, 0.99, 0, False)
    # curvature 0.01 everywhere: w = 0.99; theta is 0 on the floor for a floor hypothesis, so the floor's points pass at any height
    assert one["found"] == 1


def test_pole_and_pipe_axis_and_radius_limits(ctx):
    cloud, normals, n_pole = CS.pole_and_pipe()
    ctx.search_set_input(cloud)
    free = check(ctx, CYL, cloud, normals, 0.02, 0.1, 0.05, 0.3, 200, 0.99, 3, True)
    assert (free["inliers"] >= n_pole).all()                                          # the pipe has more points
    pole = check(ctx, CYL, cloud, normals, 0.02, 0.1, 0.05, 0.3, 200, 0.99, 3, True, (0, 0, 2), 0.2)
    assert (pole["inliers"] < n_pole).all() and pole["inliers"].size == n_pole
    assert abs(abs(pole["coeff"][5]) - 1) < 1e-5 and abs(pole["coeff"][6] - 0.15) < 1e-5
    pipe = check(ctx, CYL, cloud, normals, 0.02, 0.1, 0.05, 0.3, 200, 0.99, 3, True, (1, 0, 0), 0.2)
    assert (pipe["inliers"] >= n_pole).all() and abs(pipe["coeff"][6] - 0.10) < 1e-5
    thin = check(ctx, CYL, cloud, normals, 0.02, 0.1, 0.05, 0.12, 200, 0.99, 3, True)
    assert thin["found"] == 1 and (thin["inliers"] >= n_pole).all()
    thick = check(ctx, CYL, cloud, normals, 0.02, 0.1, 0.13, 0.3, 200, 0.99, 3, True)
    assert thick["found"] == 1 and (thick["inliers"] < n_pole).all()
    none = check(ctx, CYL, cloud, normals, 0.02, 0.1, 5.0, 6.0, 64, 0.99, 3, True)
    assert none["found"] == 0 and (none["counts"] == -1).all() and none["iterations"] == 64


@pytest.mark.parametrize("noise", [0.0, 0.003])
@pytest.mark.parametrize("weight", [0.0, 0.1, 1.0])
def test_half_cylinder(ctx, noise, weight):
    cloud, normals = CS.half_cylinder(noise)
    ctx.search_set_input(cloud)
    got = check(ctx, CYL, cloud, normals, 0.02, weight, 0.0, 0.0, 100, 0.99, 1, True)
    assert got["found"] == 1
    if weight < 1.0:
        assert abs(got["coeff"][6] - 0.25) < (1e-5 if noise == 0 else 2e-3)


@pytest.mark.parametrize("model", [PLANE, CYL])
def test_non_finite_rows_and_duplicated_points(ctx, model):
    base = CS.floor_and_wall()[:2] if model == PLANE else CS.pole_and_pipe()[:2]
    cloud, normals = CS.with_non_finite(*base)
    cloud = np.concatenate((cloud, cloud[:50], cloud[:50]))
    normals = np.concatenate((normals, normals[:50], normals[:50]))
    ctx.search_set_input(cloud)
    for seed in (0, 5):
        got = check(ctx, model, cloud, normals, 0.03, 0.1, 0.0, 0.0, 130, 0.999, seed, True)
        bad = ~(np.isfinite(cloud[:, :3]).all(axis=1) & np.isfinite(normals).all(axis=1))
        assert bad.sum() == 4 and not bad[got["inliers"]].any()
    everything = np.full_like(normals, np.nan)
    got = check(ctx, model, cloud, everything, 0.03, 0.1, 0.0, 0.0, 70, 0.99, 0, True)
    assert got["found"] == 0                                                          # valid plane hypotheses count nothing


def test_a_cloud_the_grid_refuses(ctx):
    """Every point in one spot but a few: the k-NN grid gives up on such a cloud; the segmentation needs none."""
    cloud, normals = (a.copy() for a in scan(3000))
    cloud[20:, :3] = cloud[7, :3]
    ctx.search_set_input(cloud)
    for model in (PLANE, CYL):
        check(ctx, model, cloud, normals, 0.1, 0.1, 0.0, 0.0, 70, 0.99, 2, True)


def test_the_devices_own_normals_fed_back(ctx):
    cloud, _ = CS.street(1)
    ctx.search_set_input(cloud)
    normals = ctx.normal_estimation(None, k=12, viewpoint=(0.0, 0.0, 3.0))[0]
    ground = check(ctx, PLANE, cloud, normals, 0.08, 0.1, 0.0, 0.0, 100, 0.99, 1, True)
    assert (ground["inliers"] < 1500).sum() > 1350
    rest = ctx.sac_extract(negative=True)
    assert rest.shape[0] == cloud.shape[0] - ground["inliers"].size
    ctx.search_set_input(rest)
    normals = ctx.normal_estimation(None, k=12, viewpoint=(0.0, 0.0, 3.0))[0]
    pole = check(ctx, CYL, rest, normals, 0.03, 0.1, 0.05, 0.3, 1000, 0.99, 1, True, (0, 0, 1), 0.1)
    assert pole["found"] == 1 and pole["inliers"].size > 100
    assert min(math.hypot(pole["coeff"][0] - x, pole["coeff"][1] - y) for x, y, _ in CS.POLES) < 0.05


# ---- the interface -------------------------------------------------------------------------------------------------------------
def refusals(n):
    nan, inf = math.nan, math.inf
    ok = dict(model=PLANE, threshold=0.1, weight=0.1, rmin=0.0, rmax=0.0, max_iterations=10, probability=0.9, axis=None, eps_angle=0.0)
    for change in (dict(model=0), dict(model=15), dict(model=6), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf), dict(weight=-0.01),
                   dict(weight=1.01), dict(weight=nan), dict(rmin=-1.0), dict(rmax=-1.0), dict(rmin=nan), dict(rmax=inf), dict(rmin=2.0, rmax=1.0),
                   dict(rmin=1.0, rmax=0.0), dict(max_iterations=-1), dict(max_iterations=(1 << 20) + 1), dict(probability=0.0),
                   dict(probability=1.0), dict(probability=nan), dict(axis=(0, 0, 1)), dict(model=CYL, axis=(0, 0, 0)),
                   dict(model=CYL, axis=(nan, 0, 1)), dict(model=CYL, axis=(0, 0, 1), eps_angle=-0.1), dict(model=CYL, axis=(0, 0, 1), eps_angle=nan)):
        yield {**ok, **change}


def test_refusals_leave_no_result(ctx):
    cloud, normals, _ = CS.pole_and_pipe()
    ctx.search_set_input(cloud)
    n_cases = 0
    for a in refusals(len(cloud)):
        assert device(ctx, CYL, normals, 0.02, 0.1, 0.0, 0.0, 20)["found"] == 1       # a result to lose
        with pytest.raises(SR.Refused):
            R.segment(a["model"], cloud, normals, a["threshold"], a["weight"], a["rmin"], a["rmax"], a["max_iterations"], a["probability"], 0, True,
                      a["axis"], a["eps_angle"])
        rc, coeff, n_coeff, n_in, it, found = ctx.sac_segmentation_from_normals_raw(a["model"], normals, a["threshold"], a["weight"], a["rmin"], a["rmax"],
                                                                                   a["max_iterations"], a["probability"], 0, True, a["axis"], a["eps_angle"])
        assert rc == _lib.ERR_INVALID_ARG and not coeff.any() and (n_coeff, n_in, it, found) == (0, 0, 0, 0), a
        assert ctx.sac_normals_fetch_raw(0, 0)[0] == _lib.ERR_INVALID_ARG
        with pytest.raises(IcpGpuError):
            ctx.sac_extract()
        with pytest.raises(IcpGpuError):
            ctx.sac_normals_host_waits()
        n_cases += 1
    assert n_cases == 25
    assert ctx.sac_segmentation_from_normals_raw(CYL, None, 0.02)[0] == _lib.ERR_INVALID_ARG     # null normals
    L, h = ctx._L, ctx._h
    out = (C.c_float * 7)()
    nc, it, found, n_in = C.c_int32(), C.c_int32(), C.c_int32(), C.c_size_t()
    nrm = np.ascontiguousarray(normals)
    fp = nrm.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, C.byref(nc), C.byref(n_in), C.byref(it), C.byref(found)), (out, None, C.byref(n_in), C.byref(it), C.byref(found)),
                 (out, C.byref(nc), None, C.byref(it), C.byref(found)), (out, C.byref(nc), C.byref(n_in), None, C.byref(found)),
                 (out, C.byref(nc), C.byref(n_in), C.byref(it), None)):
        assert L.icpgpu_sac_segmentation_from_normals(h, CYL, fp, 0.02, 0.1, 0.0, 0.0, 10, 0.9, 0, 1, None, 0.0, *args) == _lib.ERR_INVALID_ARG
    with Context(0) as fresh:                                                        # no search cloud
        assert fresh.sac_segmentation_from_normals_raw(CYL, normals, 0.02)[0] == _lib.ERR_INVALID_ARG


def test_degenerate_inputs_are_ok_without_a_model(ctx):
    cloud, normals, _ = CS.pole_and_pipe()
    for model in (PLANE, CYL):
        size = 3 if model == PLANE else 2
        for c, nr, kw in ((cloud[:0], normals[:1], {}), (cloud, normals, dict(max_iterations=0)), (cloud, normals, dict(threshold=0.0)),
                          (cloud[:size - 1], normals[:size - 1], {})):
            ctx.search_set_input(c)
            a = dict(threshold=0.02, max_iterations=20)
            a.update(kw)
            got = check(ctx, model, c, nr, a["threshold"], 0.1, 0.0, 0.0, a["max_iterations"], 0.99, 0, True)
            assert got["found"] == 0 and got["inliers"].size == 0 and not got["coeff"].any()
            assert ctx.sac_extract(False).shape[0] == 0 and ctx.sac_extract(True).shape[0] == len(c)


def test_fetch_capacities_null_subsets_and_the_cross_refusal(ctx):
    cloud, normals, _ = CS.pole_and_pipe()
    ctx.search_set_input(cloud)
    got = device(ctx, CYL, normals, 0.02, 0.1, 0.05, 0.3, 200, 0.99, 3, True)
    n_in, it = got["inliers"].size, got["iterations"]
    assert n_in > 0 and it > 0
    for cap_in, cap_counts in ((n_in - 1, it), (n_in, it - 1), (0, 0)):
        rc, f = ctx.sac_normals_fetch_raw(cap_in, cap_counts)
        assert rc == _lib.ERR_INVALID_ARG and (f["inliers"] == -2).all() and (f["counts"] == -2).all() and f["best_t"] == -2
        assert (f["coeff_unrefined"] == -2).all() and (f["cylinder_sums"] == -2).all() and f["cylinder_passes"] == -2
    rc, f = ctx.sac_normals_fetch_raw(n_in + 3, it + 2)                                # room to spare: the tail untouched
    assert rc == 0 and (f["inliers"][n_in:] == -2).all() and (f["counts"][it:] == -2).all() and np.array_equal(f["inliers"][:n_in], got["inliers"])
    L, h = ctx._L, ctx._h
    assert L.icpgpu_sac_normals_fetch(h, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0      # all NULL
    best_t = C.c_int32(-2)
    assert L.icpgpu_sac_normals_fetch(h, 0, 0, None, None, None, C.byref(best_t), None, None, None, None, None, None) == 0
    assert best_t.value == got["best_t"]
    # the plane's fetch refuses this result, nothing written; and the other way round
    rc, f = ctx.sac_fetch_raw(n_in, it)
    assert rc == _lib.ERR_INVALID_ARG and (f["inliers"] == -2).all() and (f["moments"] == -2).all() and f["best_t"] == -2
    assert ctx.sac_host_waits() == ctx.sac_normals_host_waits()
    rc, _, n_in, it, found = ctx.sac_segment_raw(0.02, 20)
    assert rc == 0
    rc, f = ctx.sac_normals_fetch_raw(n_in, it)
    assert rc == _lib.ERR_INVALID_ARG and (f["inliers"] == -2).all() and (f["counts"] == -2).all() and f["cylinder_stop"] == -2
    with pytest.raises(IcpGpuError):
        ctx.sac_normals_host_waits()
    assert ctx.sac_fetch_raw(n_in, it)[0] == 0


@pytest.mark.parametrize("model", [PLANE, CYL])
def test_extract_both_ways(ctx, model):
    cloud, normals = CS.with_non_finite(*CS.street(1))
    ctx.search_set_input(cloud)
    got = device(ctx, model, normals, 0.06, 0.1, 0.05, 0.4, 100, 0.99, 2, True)
    assert got["found"] == 1
    mask = np.zeros(len(cloud), bool)
    mask[got["inliers"]] = True
    for negative in (False, True, False):
        for view in (False, True):
            assert ctx.sac_extract(negative, view).tobytes() == cloud[mask != negative].tobytes()


def test_five_identical_runs(ctx):
    cloud, normals = CS.street(1)
    ctx.search_set_input(cloud)
    for model in (PLANE, CYL):
        runs = [device(ctx, model, normals, 0.05, 0.1, 0.05, 0.3, 150, 0.99, 9, True) for _ in range(5)]
        for r in runs[1:]:
            for name in STAGES + ("moments", "cylinder_sums"):
                assert r[name].tobytes() == runs[0][name].tobytes(), name


def test_the_golden_fixture(ctx):
    g = np.load(GOLDEN)
    cloud, normals = g["cloud"], g["normals"]
    ctx.search_set_input(cloud)
    for model, tag in ((PLANE, "plane"), (CYL, "cyl")):
        a = g[tag + "_args"]
        axis = None if model == PLANE else (0.0, 0.0, 1.0)
        want = {name: g[f"{tag}_{name}"] for name in STAGES + ("moments", "cylinder_sums")}
        for name in ("iterations", "best_t", "n_unrefined", "found", "cylinder_stop"):
            want[name] = int(g[f"{tag}_{name}"])
        check(ctx, model, cloud, normals, float(a[0]), float(a[1]), float(a[2]), float(a[3]), int(a[4]), float(a[5]), int(a[6]), True, axis, float(a[7]),
              want=want)


def test_the_python_class():
    cloud, normals = CS.street(1)
    seg = SACSegmentationFromNormals()
    assert (seg.getModelType(), seg.getMethodType(), seg.getNormalDistanceWeight(), seg.getRadiusLimits(), seg.getMaxIterations()) == \
        (SACMODEL_NORMAL_PLANE, SAC_RANSAC, 0.1, (0.0, 0.0), 50)
    with pytest.raises(IcpGpuError):
        seg.segment()
    for bad in (0, 15, 1):
        with pytest.raises(IcpGpuError):
            seg.setModelType(bad)
    with pytest.raises(IcpGpuError):
        seg.setMethodType(1)
    seg.setInputCloud(cloud)
    seg.setInputNormals(normals)
    seg.setDistanceThreshold(0.08)
    seg.setMaxIterations(100)
    seg.setSeed(1)
    inliers, coeff = seg.segment()
    want = R.segment(R.NORMAL_PLANE, cloud, normals, 0.08, 0.1, 0.0, 0.0, 100, 0.99, 1, True)
    assert coeff.shape == (4,) and coeff.tobytes() == want["coeff"].tobytes() and np.array_equal(inliers, want["inliers"])
    rest = seg.extractCloud(negative=True)
    assert rest.shape[0] == len(cloud) - inliers.size
    seg.setModelType(SACMODEL_CYLINDER)
    seg.setAxis((0, 0, 1))
    seg.setEpsAngle(0.1)
    seg.setRadiusLimits(0.05, 0.3)
    seg.setNormalDistanceWeight(0.2)
    seg.setDistanceThreshold(0.03)
    seg.setOptimizeCoefficients(False)
    inliers, coeff = seg.segment()
    want = R.segment(R.CYLINDER, cloud, normals, 0.03, 0.2, 0.05, 0.3, 100, 0.99, 1, False, (0, 0, 1), 0.1)
    assert coeff.shape == (7,) and coeff.tobytes() == want["coeff"].tobytes() and np.array_equal(inliers, want["inliers"])
    seg.setRadiusLimits(50.0, 60.0)
    inliers, coeff = seg.segment()
    assert inliers.size == 0 and coeff.size == 0
