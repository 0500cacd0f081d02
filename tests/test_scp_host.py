"""The feature-space k-nearest search's and the sample-consensus alignment's rules on the host (include/icpgpu.h, "feature-space
k-nearest" and "sample-consensus alignment"): the NumPy restatement (tests/scp_restated.py) against its literal per-pair,
per-hypothesis, per-point loop, the generator against Python integers, the 33-term chain against exact rational arithmetic, answers
known by hand, the end-to-end scene, and the ABI of the new entry points, which needs no GPU."""
import functools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fpfh_restated as FR
import normals_restated as NR
import scp_restated as R
import scp_scenes as S
from icpslam_amd import _lib

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("icpgpu_feature_knn", "icpgpu_scp_align", "icpgpu_scp_fetch", "icpgpu_scp_stats")


def points(xyz) -> np.ndarray:
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = np.asarray(xyz, F32).reshape(-1, 3)
    return c


def same(a: dict, b: dict, names):
    for key in names:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.dtype == y.dtype and (x.tobytes() == y.tobytes() or np.array_equal(x, y, equal_nan=True)), key


# ---- the restatement and its literal loop --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "ties", "non_finite", "overflow", "short"])
def test_feature_knn_equals_the_literal_loop(case):
    rng = np.random.default_rng(3)
    target, query, k = S.descriptors(40, 1).copy(), S.descriptors(7, 2).copy(), 5
    if case == "ties":
        base = rng.integers(0, 3, (6, 33)).astype(F32)
        target, query = base[rng.integers(0, 6, 40)], base
    elif case == "non_finite":
        target[::5, 4] = np.nan
        target[3, 0] = np.inf
        query[2, 7] = np.nan
        query[5, 32] = -np.inf
    elif case == "overflow":
        target[::3] *= F32(1e19)
        target[1, 0] = F32(3e38)
        query[0, 0] = F32(-3e38)
        query[3] *= F32(1e19)
    elif case == "short":
        target, k = target[:3], 5
    got, want = R.feature_knn(target, query, k), R.feature_knn_literal(target, query, k)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


def small_scene(seed=0, n=24):
    """n matched points with noisy descriptors, a NaN source point and an infinite target point."""
    rng = np.random.default_rng(seed)
    target = points(rng.uniform(-3, 3, (n, 3)))
    source = S.moved(target, np.linalg.inv(S.rigid(0.7, 0.05, -0.03, (1.0, 2.0, 0.5))))
    tf = S.descriptors(n, seed + 10)
    sf = (tf + rng.normal(0, 1, (n, 33))).astype(F32)
    source[3, 1] = np.nan
    target[7, 0] = np.inf
    return source, sf, target, tf


@pytest.mark.parametrize("kw", [dict(), dict(nr=4, kc=1), dict(similarity=0.0, max_iterations=20), dict(similarity=1.0), dict(distance=0.0),
                                dict(fraction=1.0), dict(nr=8, kc=1, similarity=0.5, max_iterations=40)])
def test_alignment_equals_the_literal_loop(kw):
    args = {**dict(nr=3, kc=2, similarity=0.8, distance=0.3, fraction=0.2, max_iterations=60, seed=5), **kw}
    scene = small_scene()
    a, b = R.align(*scene, **args), R.align_literal(*scene, **args)
    same(a, b, ("status", "source_idx", "target_idx", "transforms", "count", "sum", "error", "best_t", "converged", "T", "fitness", "inliers", "cloud"))
    if not kw:
        assert a["converged"] == 1 and (a["status"] == R.EVALUATED).sum() > 3 and (a["status"] == R.INVALID).any()


def test_generator_against_python_integers():
    for nr in (3, 4, 8):
        for seed in (0, 1, 2**64 - 1, 0x123456789ABCDEF0):
            got = R.draws(seed, 0, 40, nr)
            assert got.tolist() == [[R.draw_int(seed, t, c, nr) for c in range(2 * nr)] for t in range(40)]
            assert (got < 2**32).all()
    assert R.draws(5, 1000, 3, 3).tolist() == [[R.draw_int(5, t, c, 3) for c in range(6)] for t in (1000, 1001, 1002)]
    # hypothesis t of nr samples owns the counters (2 nr) t + 1 .. (2 nr)(t + 1): consecutive hypotheses never share a draw
    assert R.draw_int(9, 0, 5, 3) != R.draw_int(9, 1, 0, 3) and R.draw_int(9, 1, 0, 3) == R.draw_int(9, 0, 6, 3)
    for n in (1, 2, 2**31 - 1):                                           # the scaling: always below n, m = 1 always picks entry 0
        picks = [R.scale_int(R.draw_int(3, t, 0, 3), n) for t in range(200)]
        assert min(picks) >= 0 and max(picks) < n
        assert ((R.draws(3, 0, 200, 3)[:, 0] * np.uint64(n)) >> np.uint64(32)).tolist() == picks
    assert R.scale_int(2**32 - 1, 1) == 0 and R.scale_int(2**32 - 1, 2**31 - 1) == 2**31 - 2


def test_the_chain_against_exact_rational_arithmetic():
    """Every fused step rounds the EXACT a * b + c once: replayed with Fractions on a few rows, tie cases included."""
    rng = np.random.default_rng(4)
    q = np.concatenate([S.descriptors(3, 5), rng.integers(0, 9, (2, 33)).astype(F32), (S.descriptors(1, 6) * F32(1e-20))])
    t = np.concatenate([S.descriptors(3, 7), rng.integers(0, 9, (2, 33)).astype(F32), (S.descriptors(1, 8) * F32(1e18))])
    D = R.feature_d2(q, t)
    for i in range(len(q)):
        for j in range(len(t)):
            acc = Fraction(0)
            for b in range(33):
                d = Fraction(float(F32(q[i, b] - t[j, b])))
                acc = Fraction(R.round_f32(d * d + acc)) if math.isfinite(R.round_f32(d * d + acc)) else None
                if acc is None:
                    break
            want = math.inf if acc is None else float(acc)
            assert float(D[i, j]) == want == R.feature_d2_literal(q[i], t[j]), (i, j)
    # the rounding helper itself: halfway cases go to the even neighbour, the largest finite value's upper half goes to infinity
    one, ulp = Fraction(1), Fraction(2) ** -23
    assert R.round_f32(one + ulp / 2) == 1.0 and R.round_f32(one + 3 * ulp / 2) == float(1 + 2 * ulp) and R.round_f32(one + ulp / 2 + ulp / 1024) == float(1 + ulp)
    assert R.round_f32(Fraction(R.FLT_MAX) + Fraction(2) ** 103) == math.inf and R.round_f32(Fraction(R.FLT_MAX) + Fraction(2) ** 103 - 1) == R.FLT_MAX


def test_key_ties_put_the_lowest_index_first():
    base = S.descriptors(4, 9)
    target = np.concatenate([base[[2, 0, 1, 0, 2, 3, 0]]])                # row 0 at 1, 3, 6; row 2 at 0, 4
    idx, d2, n_found = R.feature_knn(target, base, 4)
    assert idx[0, :3].tolist() == [1, 3, 6] and idx[2, :2].tolist() == [0, 4] and idx[1, 0] == 2 and idx[3, 0] == 5
    assert (d2[0, :3] == 0).all() and (d2[2, :2] == 0).all() and (n_found == 4).all()
    zeros = np.zeros((70, 33), F32)
    assert R.feature_knn(zeros, zeros[:2], 64)[0].tolist() == [list(range(64))] * 2


# ---- the pre-rejection -------------------------------------------------------------------------------------------------------------
IDENTITY_ROWS = (np.arange(3, dtype=np.int32)[:, None], np.ones(3, np.int32))


def statuses(source, target, similarity, m=40):
    return R.hypotheses(source, target, *IDENTITY_ROWS, 3, similarity, 1, 0, m)[0]


def test_an_edge_ratio_exactly_on_the_threshold_passes():
    source = points([[0, 0, 0], [1, 0, 0], [0, 1, 0]])                    # squared edges 1, 2, 1
    target = points([[0, 0, 0], [2, 0, 0], [0, 2, 0]])                    # ... 4, 8, 4: every ratio is exactly 0.25
    st = statuses(source, target, 0.5)
    assert (st == R.EVALUATED).sum() > 3 and set(st.tolist()) == {R.INVALID, R.EVALUATED}
    above = math.sqrt(float(np.nextafter(F32(0.25), F32(1)))) * (1 + 1e-9)   # the first similarity whose float32 square is above 0.25
    assert F32(above * above) == np.nextafter(F32(0.25), F32(1))
    assert set(statuses(source, target, above).tolist()) == {R.INVALID, R.PREREJECTED}
    assert ((statuses(source, target, 0.5) == R.INVALID) == (statuses(source, target, above) == R.INVALID)).all()
    assert set(statuses(source, target, float(np.nextafter(0.5, 1.0))).tolist()) == {R.INVALID, R.EVALUATED}   # (its float32 square is still 0.25)


def test_zero_over_zero_fails_even_at_similarity_zero():
    source = points([[1, 1, 1], [1, 1, 1], [0, 1, 0]])                    # points 0 and 1 coincide in both clouds: that edge is 0 / 0
    target = points([[5, 0, 2], [5, 0, 2], [0, 2, 0]])
    assert set(statuses(source, target, 0.0).tolist()) == {R.INVALID, R.PREREJECTED}
    target = points([[5, 0, 2], [5, 1, 2], [0, 2, 0]])                    # 0 / 1 = 0: passes at similarity 0 only
    assert set(statuses(source, target, 0.0).tolist()) == {R.INVALID, R.EVALUATED}
    assert set(statuses(source, target, 1e-3).tolist()) == {R.INVALID, R.PREREJECTED}


def test_a_cloud_matched_with_itself_passes_at_every_similarity():
    cloud = points(np.random.default_rng(6).uniform(-4, 4, (3, 3)))
    for similarity in (0.0, 0.5, 1.0):
        assert set(statuses(cloud, cloud, similarity).tolist()) == {R.INVALID, R.EVALUATED}
    for bad in (-0.1, 1.0000001, math.nan, math.inf):
        with pytest.raises(R.Refused):
            R.check(3, 2, bad, 0.5, 0.25, 10)


# ---- the fitness and the choice ----------------------------------------------------------------------------------------------------
def test_a_point_exactly_on_the_distance_is_no_inlier():
    target = points([[0, 0, 0], [4, 0, 0]])
    source = points([[0.5, 0, 0], [4, 0.25, 0], [np.nan, 0, 0], [0, 0, 0.5000001], [30, 0, 0]])
    identity = np.eye(4, dtype=F32).reshape(16)
    mask, d2 = R.inlier_d2(identity, source, target, 0.5)
    assert mask.tolist() == [False, True, False, False, False] and d2[1] == F32(0.0625) and np.isposinf(d2[[0, 2, 3, 4]]).all()
    mask, d2 = R.inlier_d2(identity, source, target, float(np.nextafter(F32(0.5), F32(1))))     # the next float32 r2 up
    assert mask.tolist() == [True, True, False, False, False] and d2[0] == F32(0.25)
    assert not R.inlier_d2(identity, source, target, 0.0)[0].any()                              # r2 = 0: nothing is below it
    assert R.inlier_d2(identity, points([[0, 0, 0]]), target, 0.5)[0].tolist() == [True]        # d2 = 0 < r2


def test_the_inlier_fraction_is_compared_in_float32_and_met_exactly():
    for count, n_s in ((27, 35), (1, 3), (2, 3), (5, 7), (999, 1500)):
        error = np.full(1, 0.5, F32)
        exact = float(F32(count) / F32(n_s))
        assert R.choose([count], error, n_s, exact) == 0                                        # count / n_s itself is enough
        assert R.choose([count], error, n_s, float(np.nextafter(F32(exact), F32(2)))) == -1
        assert R.choose([count], error, n_s, 0.0) == 0 and R.choose([count], error, n_s, 1.0) == -1
        assert R.choose([n_s], error, n_s, 1.0) == 0
    assert R.choose([0], np.zeros(1, F32), 10, 0.0) == -1                                       # no inliers: never the best, whatever the fraction


def test_equal_errors_keep_the_lower_t():
    error = F32([0.5, 0.25, 0.25, 0.3, 0.25])
    assert R.choose([5, 5, 9, 9, 9], error, 10, 0.5) == 1
    assert R.choose([5, 4, 9, 9, 9], error, 10, 0.5) == 2                                       # t = 1 has too few inliers
    assert R.choose([5, 5, 5], F32([R.FLT_MAX] * 3), 10, 0.0) == -1                             # FLT_MAX is not below the start


# ---- the end-to-end scene -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_descriptors():
    source, target, _ = S.e2e_clouds()
    return tuple(FR.estimate(c, NR.estimate(c, None, k=S.E2E_NORMAL_K)[0], None, radius=S.E2E_FPFH_RADIUS)[0] for c in (source, target))


@functools.lru_cache(maxsize=None)
def restated_rows():
    sf, tf = restated_descriptors()
    return R.feature_knn(tf, sf, S.E2E["kc"])


@pytest.mark.parametrize("seed", S.E2E_SEEDS)
def test_end_to_end_relocalisation(seed):
    """A 1500-point scan seen again from 1.2 rad of yaw and (4, -2, 0.1) m away, no guess: normals (k = 10), FPFH (radius 2.0), 3
    samples, randomness 5, similarity 0.9, distance 0.5 m, inlier fraction 0.25, 3000 hypotheses.  The restatement's pose must be within
    2 degrees and the correspondence distance (0.5 m) of the truth.  Attained: seed 1: 0.000 degrees, 4.6e-8 m (51 hypotheses scored
    of 3000); seed 2: 0.319 degrees, 0.065 m (44 scored); seed 3: 0.077 degrees, 0.026 m (60 scored).  The conditioning cut of the
    device test's transform comparison leaves out at most 10 % of the scored hypotheses here."""
    source, target, truth = S.e2e_clouds()
    sf, tf = restated_descriptors()
    r = R.align(source, sf, target, tf, seed=seed, rows=restated_rows(), **S.E2E)
    rot, trans = S.pose_error(r["T"], truth)
    scored = np.flatnonzero(r["status"] == R.EVALUATED)
    print(f"seed {seed}: {rot:.4f} degrees, {trans:.4g} m, {scored.size} scored, best_t {r['best_t']}, {r['inliers'].size} inliers")
    assert r["converged"] == 1 and rot <= 2.0 and trans <= S.E2E["distance"]
    assert (r["status"] == R.PREREJECTED).mean() > 0.9                                          # the pre-rejection does the work
    thin = sum(not S.well_spread(r["sums17"][e]) for e in scored)
    assert thin <= 0.10 * scored.size, (thin, scored.size)


@pytest.mark.parametrize("case", range(len(S.CUT_CASES)))
def test_the_device_tests_scenes_keep_the_conditioning_cut_under_ten_percent(case):
    """tests/test_gpu_scp.py compares the host solve's transforms on well-spread samples only (sigma_2 >= 1e-3 sigma_1); the cut may
    leave out at most 10 % of the scored hypotheses of every scene it uses.  The samples are a function of the scene and the arguments
    alone, so the restatement decides this without a device."""
    n_s, n, scene_kw, kw = S.CUT_CASES[case]
    args = {**S.GPU_KW, **kw}
    source, sf, target, tf, _ = S.matched(n_s, n, **scene_kw)
    rows, _, found = R.feature_knn(tf, sf, args["kc"])
    status, _, _, sums = R.hypotheses(source, target, rows, found, args["nr"], args["similarity"], args["seed"], 0, args["max_iterations"])
    scored = np.flatnonzero(R.solve(status, sums)[1] == R.EVALUATED)
    thin = sum(not S.well_spread(sums[e]) for e in scored)
    assert thin <= 0.10 * scored.size, (thin, scored.size)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in SYMBOLS:
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS
    assert "#define ICPGPU_SCP_MAX_ITERATIONS (1 << 20)" in header and _lib.SCP_MAX_ITERATIONS == R.MAX_ITERATIONS == 1 << 20
    assert "#define ICPGPU_SCP_CHUNK 65536" in header and _lib.SCP_CHUNK == R.CHUNK == 65536
    assert "#define ICPGPU_SCP_MAX_SAMPLES 8" in header and _lib.SCP_MAX_SAMPLES == R.MAX_SAMPLES == 8
    for value, name in enumerate(("INVALID", "PREREJECTED", "NO_TRANSFORM", "EVALUATED")):
        assert f"#define ICPGPU_SCP_{name} {value}" in header and getattr(_lib, f"SCP_{name}") == getattr(R, name) == value


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_feature_knn(None, None, 0, None, 0, 1, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_scp_align(None, None, 0, None, None, 3, 2, 0.9, 0.5, 0.25, 10, 0, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_scp_fetch(None, 0, 0, None, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_scp_stats(None, None, None, None) == _lib.ERR_INVALID_ARG


def test_front_ends_and_their_defaults():
    import icpslam_amd as pkg
    assert "SampleConsensusPrerejective" in pkg.__all__ and "FeatureKdTree" in pkg.__all__
    with pytest.raises(R.Refused):
        R.align(*small_scene(), nr=2)
    with pytest.raises(R.Refused):
        R.align(*small_scene(), max_iterations=(1 << 20) + 1)
    for bad in (dict(kc=0), dict(kc=65), dict(distance=-1.0), dict(distance=math.inf), dict(fraction=1.5), dict(nr=9)):
        with pytest.raises(R.Refused):
            R.align(*small_scene(), **bad)
