"""The plane segmentation's rules on the host (include/icpgpu.h, "plane segmentation"): the NumPy restatement (tests/sac_restated.py)
against its literal per-hypothesis, per-point loop, the generator against Python integers, answers known by hand, the golden fixture,
and the ABI of the new entry points, which needs no GPU."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import sac_restated as R
from icpslam_amd import _lib, synth

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rows_f", "sac_2k.npz")
SYMBOLS = ("icpgpu_sac_plane_segmentation", "icpgpu_sac_fetch", "icpgpu_sac_stats", "icpgpu_sac_extract", "icpgpu_sac_extract_view")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def points(xyz) -> np.ndarray:
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = np.asarray(xyz, F32).reshape(-1, 3)
    return c


def floor_and_scatter(n_floor=40, n_scatter=12, seed=3) -> np.ndarray:
    """n_floor points exactly on z = 0 and n_scatter at least a metre above it, shuffled."""
    rng = np.random.default_rng(seed)
    floor = np.concatenate([rng.uniform(-8, 8, (n_floor, 2)), np.zeros((n_floor, 1))], axis=1)
    scatter = np.concatenate([rng.uniform(-8, 8, (n_scatter, 2)), rng.uniform(1, 4, (n_scatter, 1))], axis=1)
    return points(rng.permutation(np.concatenate([floor, scatter])))


def same(a: dict, b: dict):
    assert a.keys() == b.keys()
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), key


# ---- the restatement and its literal loop --------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("case", ["scan", "floor", "nan", "axis"])
def test_restatement_equals_the_literal_loop(case, optimize):
    kw = dict(threshold=0.15, max_iterations=12, probability=0.99, seed=7, optimize=optimize)
    if case == "scan":
        cloud = scan(90)
    elif case == "floor":
        cloud = floor_and_scatter()
    elif case == "nan":
        cloud = scan(90).copy()
        cloud[::7, 1] = np.nan
        cloud[5, 2] = np.inf
    else:
        cloud = floor_and_scatter()
        kw.update(axis=(0.0, 0.2, 3.0), eps_angle=0.3)
    same(R.segment(cloud, **kw), R.segment_literal(cloud, **kw))


def test_generator_against_python_integers():
    for n in (1, 2, 3, 64, 1000, 2**31 - 1):
        for seed in (0, 1, 2**64 - 1, 0x123456789ABCDEF0):
            got = R.samples(seed, 0, 70, n)
            want = [[R.sample_int(seed, t, c, n) for c in range(3)] for t in range(70)]
            assert got.tolist() == want
            assert (got >= 0).all() and (got < n).all()
    assert R.samples(5, 1000, 3, 99).tolist() == [[R.sample_int(5, t, c, 99) for c in range(3)] for t in (1000, 1001, 1002)]
    assert (R.samples(9, 0, 50, 1) == 0).all()
    # the largest 32-bit draw still lands below n
    assert ((2**32 - 1) * (2**31 - 1)) >> 32 == 2**31 - 2


# ---- answers known by hand ---------------------------------------------------------------------------------------------------
def test_a_floor_known_by_hand():
    """40 points exactly on z = 0 among 12 above it.  Seed 1 was chosen by running the restatement here: its loop ends on a sample of
    three floor points, so the plane's points are exactly the inliers and the refined coefficients are (0, 0, +-1, 0)."""
    cloud = floor_and_scatter()
    on_floor = np.flatnonzero(cloud[:, 2] == 0)
    r = R.segment(cloud, 0.05, 50, 0.99, seed=1)
    assert r["found"] == 1 and r["inliers"].tolist() == on_floor.tolist() and r["n_unrefined"] == on_floor.size
    assert np.array_equal(np.abs(r["coeff"]), F32([0, 0, 1, 0]))
    assert np.array_equal(np.abs(r["coeff_unrefined"]), F32([0, 0, 1, 0]))
    assert r["coeff"][2] == r["coeff_unrefined"][2]                      # the refinement keeps the unrefined normal's side
    assert r["counts"][r["best_t"]] == on_floor.size and r["iterations"] == r["counts"].size < 50
    assert (cloud[r["sample"], 2] == 0).all()
    assert np.array_equal(R.extract(cloud, r["inliers"], False), cloud[on_floor])
    assert np.array_equal(R.extract(cloud, r["inliers"], True), cloud[cloud[:, 2] != 0])


def test_a_point_exactly_on_the_threshold_is_out():
    plane = F32([0, 0, 1, 0])
    thr = float(F32(0.25))
    cloud = points([[0, 0, 0.25], [1, 1, -0.25], [2, 0, np.nextafter(F32(0.25), F32(0))], [0, 3, 0.0], [np.nan, 0, 0], [0, 0, np.inf]])
    assert R.inlier_mask(cloud, plane, thr).tolist() == [False, False, True, True, False, False]
    assert R.inlier_mask(cloud, plane, float(np.nextafter(thr, 1.0))).tolist() == [True, True, True, True, False, False]
    assert not R.inlier_mask(cloud, plane, 0.0).any()                    # threshold 0: nothing is below it


def test_collinear_and_coincident_clouds_have_no_model():
    line = points([[0.5 * i, 1.0 * i, -0.25 * i] for i in range(40)])
    spot = points([[1.5, -2.0, 0.75]] * 40)
    for cloud in (line, spot):
        r = R.segment(cloud, 0.1, 30, 0.99, seed=2)
        assert (r["counts"] == -1).all() and r["iterations"] == 30
        assert r["found"] == 0 and r["best_t"] == -1 and r["inliers"].size == 0 and not r["coeff"].any() and not r["moments"].any()
        same(r, R.segment_literal(cloud, 0.1, 30, 0.99, seed=2))


def test_degenerate_inputs_are_ok_without_a_model():
    for cloud, kw in ((np.empty((0, 4), F32), {}), (scan(63), {"max_iterations": 0}), (scan(63), {"threshold": 0.0}),
                      (np.full((9, 4), np.nan, F32), {}), (points([[0, 0, 0], [1, 0, 0]]), {})):
        args = {"threshold": 0.2, "max_iterations": 20, "seed": 3, **kw}
        r = R.segment(cloud, **args)
        assert r["found"] == 0 and r["inliers"].size == 0 and r["iterations"] == (0 if len(cloud) == 0 else args["max_iterations"])
        assert (r["counts"] <= 0).all()


def test_the_k_rule():
    # w = 1: p clamps to DBL_EPSILON, k = log(0.01) / log(2^-52) = 0.1277...: the loop stops before t = 1
    assert R.next_k(10, 10, 0.99) == math.log(1 - 0.99) / math.log(R.DBL_EPSILON) and 0 < R.next_k(10, 10, 0.99) < 1
    flat = points([[x, y, 0] for x in range(6) for y in range(6)])
    r = R.segment(flat, 0.01, 50, 0.99, seed=4)
    first = int(np.flatnonzero(r["counts"] > 0)[0])
    assert r["iterations"] == first + 1 and r["best_t"] == first and r["counts"][first] == 36
    # small w: w^3 underflows the clamp's upper end only below w ~ 6e-6; at w = 0.01, k = log(0.01) / log(1 - 1e-6) ~ 4.6e6
    k = R.next_k(1, 100, 0.99)
    assert k == math.log(0.01) / math.log(1.0 - 0.01 * 0.01 * 0.01) and 4.6e6 < k < 4.61e6
    assert R.next_k(1, 10**6, 0.99) == math.log(0.01) / math.log(1.0 - R.DBL_EPSILON)   # the upper clamp
    # k only ever changes when the best changes: a worse or equal later count leaves it alone
    r = R.segment(scan(200), 0.3, 40, 0.9, seed=1)
    best = np.maximum.accumulate(np.maximum(r["counts"], 0))
    assert r["best_t"] == int(np.flatnonzero(r["counts"] == best[-1])[0])


def test_the_axis_picks_the_floor_over_a_larger_wall():
    rng = np.random.default_rng(8)
    wall = np.stack([np.full(80, 5.0), rng.uniform(-6, 6, 80), rng.uniform(0, 4, 80)], axis=1)      # x = 5: 80 points
    floor = np.stack([rng.uniform(-6, 6, 50), rng.uniform(-6, 6, 50), np.zeros(50)], axis=1)        # z = 0: 50 points
    cloud = points(rng.permutation(np.concatenate([wall, floor])))
    plain = R.segment(cloud, 0.05, 200, 0.99, seed=6)
    assert plain["inliers"].size >= 80 and abs(plain["coeff"][0]) > 0.99         # without an axis the wall wins
    with_axis = R.segment(cloud, 0.05, 200, 0.99, seed=6, axis=(0, 0, 2.5), eps_angle=math.radians(10))
    assert with_axis["found"] == 1 and abs(with_axis["coeff"][2]) > 0.99 and with_axis["inliers"].size >= 50
    assert (cloud[with_axis["inliers"], 2] == 0).sum() == 50
    wall_hypotheses = np.flatnonzero(plain["counts"][:with_axis["iterations"]] >= 80)
    assert wall_hypotheses.size and (with_axis["counts"][wall_hypotheses] == -1).all()   # the wall's hypotheses are INVALID there
    sideways = R.segment(cloud, 0.05, 200, 0.99, seed=6, axis=(1, 0, 0), eps_angle=math.radians(10))
    assert abs(sideways["coeff"][0]) > 0.99


def test_refusals():
    ok = dict(threshold=0.1, max_iterations=10, probability=0.9)
    for bad in (dict(threshold=-0.1), dict(threshold=math.nan), dict(threshold=math.inf), dict(max_iterations=-1),
                dict(max_iterations=(1 << 20) + 1), dict(probability=0.0), dict(probability=1.0), dict(probability=math.nan),
                dict(axis=(0, 0, 0)), dict(axis=(math.nan, 0, 1)), dict(axis=(0, 0, 1), eps_angle=-0.1), dict(axis=(0, 0, 1), eps_angle=math.inf)):
        with pytest.raises(R.Refused):
            R.segment(scan(63), **{**ok, **bad})
    R.segment(scan(63), **{**ok, "eps_angle": -1.0})                     # (without an axis eps_angle is not looked at)
    R.segment(scan(63), **{**ok, "max_iterations": 0})


# ---- the golden fixture and the ABI ------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    r = R.segment(g["cloud"], float(g["threshold"]), int(g["max_iterations"]), float(g["probability"]), int(g["seed"]), True)
    for name in ("counts", "sample", "coeff_unrefined", "moments", "coeff", "inliers"):
        assert r[name].dtype == g[name].dtype and r[name].tobytes() == g[name].tobytes(), name
    assert (r["iterations"], r["best_t"], r["n_unrefined"]) == (int(g["iterations"]), int(g["best_t"]), int(g["n_unrefined"]))
    assert 100 < r["inliers"].size < 2000 and r["n_unrefined"] != r["inliers"].size
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "rows_f", "normals_2k.npz"))


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in SYMBOLS:
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS
    assert f"#define ICPGPU_SAC_MAX_ITERATIONS (1 << 20)" in header and _lib.SAC_MAX_ITERATIONS == R.MAX_ITERATIONS == 1 << 20


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_sac_plane_segmentation(None, 0.1, 50, 0.99, 0, 1, None, 0.0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_sac_fetch(None, 0, 0, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_sac_stats(None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_sac_extract(None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_sac_extract_view(None, 1, None, None) == _lib.ERR_INVALID_ARG


def test_extract_indices_front_end_and_the_constants():
    import icpslam_amd as pkg
    ex = pkg.ExtractIndices()
    cloud = scan(63)
    ex.setInputCloud(cloud)
    ex.setIndices([3, 1, 60])
    assert np.array_equal(ex.filter(), cloud[[1, 3, 60]])
    ex.setNegative(True)
    assert np.array_equal(ex.filter(), np.delete(cloud, [1, 3, 60], axis=0))
    assert (pkg.SACMODEL_PLANE, pkg.SACMODEL_PERPENDICULAR_PLANE, pkg.SAC_RANSAC) == (0, 15, 0)
