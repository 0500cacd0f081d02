"""The rules of the segmentation from normals on the host (include/icpgpu.h, "segmentation from normals"): the NumPy restatement
(tests/sac_normals_restated.py) against its literal per-hypothesis, per-point loop, the angle against math.atan2, the inlier decisions
against PCL's acos form, answers known by hand, the refinement and each of its stop reasons, the refusals, the golden fixture, the
ABI, and the street scene end to end."""
import math
import os
import subprocess

import numpy as np
import pytest

import normals_restated as NR
import sac_normals_cases as CS
import sac_normals_restated as R
import sac_restated as SR
from icpslam_amd import _lib

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rows_f", "sac_normals_2k.npz")
SYMBOLS = ("icpgpu_sac_segmentation_from_normals", "icpgpu_sac_normals_fetch", "icpgpu_sac_normals_stats")
PLANE, CYL = R.NORMAL_PLANE, R.CYLINDER


def same(a: dict, b: dict):
    assert set(a) == set(b)
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, x, y)


# ---- the two restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimize", [True, False])
@pytest.mark.parametrize("case", ["floor", "pole", "half", "noisy", "bad"])
def test_restatement_equals_the_literal_loop(case, optimize):
    if case == "floor":
        cloud, normals = (a[::4] for a in CS.floor_and_wall()[:2])
        runs = [(PLANE, 0.05, 0.1, 0.0, 0.0, None, 0.0), (PLANE, 0.05, 1.0, 0.0, 0.0, None, 0.0)]
    elif case == "pole":
        cloud, normals = (a[::3] for a in CS.pole_and_pipe()[:2])
        runs = [(CYL, 0.02, 0.1, 0.05, 0.3, None, 0.0), (CYL, 0.02, 0.1, 0.0, 0.0, (0, 0, 1), 0.2)]
    elif case in ("half", "noisy"):
        cloud, normals = (a[:70] for a in CS.half_cylinder(0.0 if case == "half" else 0.003))
        runs = [(CYL, 0.02, 0.1, 0.0, 0.0, None, 0.0), (CYL, 0.02, 0.0, 0.0, 0.0, None, 0.0)]
    else:
        cloud, normals = CS.with_non_finite(*(a[::3] for a in CS.pole_and_pipe()[:2]))
        runs = [(CYL, 0.02, 0.1, 0.0, 0.0, None, 0.0), (PLANE, 0.05, 0.1, 0.0, 0.0, None, 0.0)]
    for model, thr, w, rmin, rmax, axis, eps in runs:
        for seed in (0, 7):
            args = (model, cloud, normals, thr, w, rmin, rmax, 25, 0.99, seed, optimize, axis, eps)
            same(R.segment(*args), R.segment_literal(*args))


def test_generators():
    for seed in (0, 12345, 2**64 - 1):
        S = R.samples2(seed, 5, 70, 1000)
        assert S.shape == (70, 2)
        assert all(int(S[i, c]) == R.sample2_int(seed, 5 + i, c, 1000) for i in range(70) for c in range(2))
    # NORMAL_PLANE proposes the plane segmentation's triples: with weight 0 the whole run is the plane's, byte for byte
    cloud, normals, _ = CS.floor_and_wall()
    for optimize in (True, False):
        a, b = R.segment(PLANE, cloud, normals, 0.05, 0.0, 0.0, 0.0, 50, 0.99, 3, optimize), SR.segment(cloud, 0.05, 50, 0.99, 3, optimize)
        for name in ("counts", "sample", "coeff_unrefined", "moments", "coeff", "inliers"):
            assert a[name].tobytes() == b[name].tobytes(), name
        assert (a["iterations"], a["best_t"], a["n_unrefined"], a["found"]) == (b["iterations"], b["best_t"], b["n_unrefined"], b["found"])


# ---- the angle -----------------------------------------------------------------------------------------------------------------
def test_the_angle_against_atan2():
    """|A(y, x) - atan2(y, x)| <= 2^-22: 2 ulp of pi / 2 asserted, 1.31 measured (1.56e-7 over this sweep)."""
    rng = np.random.default_rng(0)
    t = np.linspace(0, 1, 1000001).astype(F32)
    one = np.ones_like(t)
    y = np.concatenate((t, one, rng.uniform(0, 1, 400000), 10.0 ** rng.uniform(-30, 30, 200000))).astype(F32)
    x = np.concatenate((one, t, rng.uniform(0, 1, 400000), 10.0 ** rng.uniform(-30, 30, 200000))).astype(F32)
    got = R.folded_angle(y, x).astype(F64)
    err = np.abs(got - np.arctan2(y.astype(F64), x.astype(F64))).max()
    print("angle: max error", err, "=", err / 2.0 ** -23, "ulp of pi / 2")
    assert err <= R.ANGLE_BOUND == 2.0 ** -22
    assert (got >= 0).all() and (got <= float(R.HALF_PI)).all()
    tiny, huge = F32(1e-38), F32(3e38)
    for yy, xx in ((0.5, 0.5), (tiny, huge), (huge, tiny), (tiny, tiny), (huge, huge), (1e-30, 1.0), (1.0, 1e-30), (3.0, 4.0)):
        a = float(R.folded_angle(F32(yy), F32(xx)))
        assert abs(a - math.atan2(float(F32(yy)), float(F32(xx)))) <= R.ANGLE_BOUND, (yy, xx)
        assert R.angle_literal(yy, xx).tobytes() == F32(a).tobytes()
    # exactly 0 for parallel, exactly the float32 image of pi / 2 for perpendicular directions; a zero direction gives 0
    assert R.folded_angle(F32(0), F32(2)).tobytes() == F32(0).tobytes() and R.folded_angle(F32(0), F32(0)).tobytes() == F32(0).tobytes()
    assert R.folded_angle(F32(2), F32(0)).tobytes() == F32(math.pi / 2).tobytes() == R.HALF_PI.tobytes()
    assert float(R.pair_angle(np.float32([[0, 0, 2]]), np.float32([0, 0, -3]))[0]) == 0.0
    assert R.pair_angle(np.float32([[0, 2, 0]]), np.float32([0, 0, -3]))[0].tobytes() == R.HALF_PI.tobytes()
    assert math.isnan(float(R.folded_angle(F32(np.nan), F32(1)))) and math.isnan(float(R.folded_angle(F32(np.inf), F32(np.inf))))


def test_inlier_decisions_against_pcls_acos_form():
    """PCL's weighted distance in float64 with acos of the normalised dot product, on 2 000 points of the street: points whose
    weighted distance lies within 1e-5 of the threshold are left out (at most 1 % of them), none of the rest may disagree."""
    keep = np.sort(np.random.default_rng(5).choice(CS.street(1)[0].shape[0], 2000, replace=False))
    cloud, normals = (a[keep] for a in CS.street(1))
    ok = np.isfinite(normals).all(axis=1)
    q, m, c = cloud[:, :3].astype(F64), normals[:, :3].astype(F64), normals[:, 3].astype(F64)
    plane = np.float32([0.0006, -0.00003, 0.9999998, -0.027])
    cyl = np.float32([3.0, 2.0, 0.0, 0.01, -0.02, 0.9997, 0.10])
    thr, W = 0.06, 0.1
    for model, co in ((PLANE, plane), (CYL, cyl)):
        co64 = co.astype(F64)
        with np.errstate(all="ignore"):
            if model == PLANE:
                de = np.abs(q @ co64[:3] + co64[3])
                g = np.broadcast_to(co64[:3], q.shape)
                w = W * (1 - c)
            else:
                v = q - co64[:3]
                d = co64[3:6]
                de = np.abs(np.linalg.norm(np.cross(v, d), axis=1) - co64[6])
                g = v - (v @ d)[:, None] * d
                w = np.full(len(q), W)
            cosine = np.abs((m * g).sum(axis=1)) / (np.linalg.norm(m, axis=1) * np.linalg.norm(g, axis=1))
            ref = w * np.arccos(np.clip(cosine, 0, 1)) + (1 - w) * de
        ours = R.inlier_mask(model, cloud, normals, co, thr, W)
        near = np.abs(ref - thr) <= 1e-5
        assert near[ok].sum() <= 0.01 * len(q)
        decided = ok & ~near
        assert np.array_equal(ours[decided], ref[decided] < thr) and 20 <= ours.sum() < 1900
        assert not ours[~ok].any()


# ---- hypotheses and scenes known by hand ---------------------------------------------------------------------------------------
def test_a_point_exactly_on_the_threshold_is_out():
    cloud = CS.rows([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0.25], [0.3, 0.3, 0.125]])
    normals = CS.rows(np.tile([0.0, 0.0, 1.0], (5, 1)), 0.0)
    plane = np.float32([0, 0, 1, 0])
    assert R.values(PLANE, cloud, normals, plane, 0.0).tolist() == [0, 0, 0, 0.25, 0.125]
    assert R.inlier_mask(PLANE, cloud, normals, plane, 0.25, 0.0).tolist() == [True, True, True, False, True]
    # weight 1 with curvature 0: the angle alone decides -- a point far off the plane with a parallel normal is in at any threshold
    assert R.inlier_mask(PLANE, cloud, normals, plane, 1e-30, 1.0).all()
    tilted = normals.copy()
    tilted[3, :3] = [0, 1, 1]
    v = R.values(PLANE, cloud, tilted, plane, 1.0)
    assert abs(float(v[3]) - math.pi / 4) <= R.ANGLE_BOUND and not R.inlier_mask(PLANE, cloud, tilted, plane, 0.7, 1.0)[3]
    # the curvature weighting: w = W (1 - c)
    curved = tilted.copy()
    curved[3, 3] = 0.5
    assert R.values(PLANE, cloud, curved, plane, 1.0)[3].tobytes() == F32(F32(F32(0.5) * v[3]) + F32(F32(0.5) * F32(0.25))).tobytes()


def test_floor_meeting_a_wall():
    cloud, normals, n_floor = CS.floor_and_wall()
    plain = SR.segment(cloud, 0.05, 50, 0.99, 0, True)
    aware = R.segment(PLANE, cloud, normals, 0.05, 0.1, 0.0, 0.0, 50, 0.99, 0, True)
    assert (plain["inliers"] >= n_floor).sum() > 10                                 # the wall's foot
    assert (aware["inliers"] < n_floor).all() and aware["inliers"].size == n_floor
    with pytest.raises(SR.Refused):
        R.segment(PLANE, cloud, normals, 0.05, 0.1, 0.0, 0.0, 50, 0.99, 0, True, (0, 0, 1), 0.1)


def test_cylinder_hypotheses_by_hand():
    p = CS.rows([[1, 0, 0], [0, 1, 0], [0, 1, 2], [1, 0, 5], [-1, 0, 3]])
    nr = CS.rows([[1, 0, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0]], 0.0)
    S = np.array([[0, 1], [0, 2], [0, 3], [0, 4], [2, 2], [0, 3]], np.int64)
    co, valid = R.cylinder_models(p, nr, S)
    assert valid.tolist() == [False, True, False, False, False, False]              # one cross-section; ok; parallel x 2; repeated; parallel
    assert co[1].tolist() == [0, 0, 0, 0, 0, 1, 1] and np.isnan(co[0]).all()
    assert R.cylinder_model_literal(p[0, :3], nr[0, :3], p[1, :3], nr[1, :3]) is None
    assert R.cylinder_model_literal(p[0, :3], nr[0, :3], p[2, :3], nr[2, :3]).tolist() == [0, 0, 0, 0, 0, 1, 1]
    S1 = S[1:2]
    for rmin, rmax, want in ((0.5, 1.0, True), (1.0, 1.5, True), (0.0, 0.99, False), (1.01, 2.0, False), (0.0, 0.0, True)):
        assert R.cylinder_models(p, nr, S1, rmin, rmax)[1][0] == want
    for axis, eps, want in (((0, 0, 1), 0.0, True), ((0, 0, -5), 0.1, True), ((1, 0, 0), 0.1, False), ((0, 1, 1), 0.7, False), ((0, 1, 1), 0.8, True)):
        assert R.cylinder_models(p, nr, S1, 0.0, 0.0, SR.unit_axis(axis), math.cos(eps))[1][0] == want
    bad = nr.copy()
    bad[2, 1] = np.nan
    assert not R.cylinder_models(p, bad, S1)[1][0]
    bad = p.copy()
    bad[0, 2] = np.inf
    assert not R.cylinder_models(bad, nr, S1)[1][0]
    # a point on the axis is never an inlier, whatever the threshold
    q = CS.rows([[0, 0, 1], [1, 0, 1]])
    assert R.inlier_mask(CYL, q, CS.rows([[1, 0, 0], [1, 0, 0]], 0.0), co[1], 10.0, 0.1).tolist() == [False, True]


def test_pole_beside_a_pipe():
    cloud, normals, n_pole = CS.pole_and_pipe()
    args = (CYL, cloud, normals, 0.02, 0.1, 0.05, 0.3, 200, 0.99, 3, True)
    assert (R.segment(*args)["inliers"] >= n_pole).all()
    pole = R.segment(*args, (0, 0, 1), 0.2)
    assert (pole["inliers"] < n_pole).all() and pole["inliers"].size == n_pole and abs(pole["coeff"][6] - 0.15) < 1e-5
    pipe = R.segment(*args, (1, 0, 0), 0.2)
    assert (pipe["inliers"] >= n_pole).all() and abs(pipe["coeff"][6] - 0.10) < 1e-5 and abs(abs(pipe["coeff"][3]) - 1) < 1e-5


def test_non_finite_rows():
    cloud, normals = CS.with_non_finite(*CS.pole_and_pipe()[:2])
    bad = ~(np.isfinite(cloud[:, :3]).all(axis=1) & np.isfinite(normals).all(axis=1))
    assert bad.sum() == 4
    for model in (PLANE, CYL):
        r = R.segment(model, cloud, normals, 0.05, 0.1, 0.0, 0.0, 150, 0.999, 0, True)
        assert r["found"] == 1 and not bad[r["inliers"]].any()
    S = np.array([[int(np.flatnonzero(bad)[k]), 0] for k in range(4)], np.int64)
    assert R.cylinder_models(cloud, normals, S)[1].tolist() == [False, False, False, True]   # (a sampled curvature is not read)
    assert not SR.models(cloud, np.array([[int(np.flatnonzero(bad)[0]), 0, 1]], np.int64))[1][0]
    r = R.segment(PLANE, cloud, np.full_like(normals, np.nan), 0.05, 0.1, 0.0, 0.0, 70, 0.99, 0, True)
    assert r["found"] == 0 and r["iterations"] == 70
    r = R.segment(CYL, cloud, np.full_like(normals, np.nan), 0.05, 0.1, 0.0, 0.0, 70, 0.99, 0, True)
    assert r["found"] == 0 and (r["counts"] == -1).all()


def test_degenerate_inputs_are_ok_without_a_model():
    cloud, normals, _ = CS.pole_and_pipe()
    for model, size in ((PLANE, 3), (CYL, 2)):
        for c, nr, thr, it in ((cloud[:0], normals[:0], 0.02, 20), (cloud, normals, 0.02, 0), (cloud, normals, 0.0, 20),
                               (cloud[:size - 1], normals[:size - 1], 0.02, 20)):
            r = R.segment(model, c, nr, thr, 0.1, 0.0, 0.0, it, 0.99, 0, True)
            assert r["found"] == 0 and r["inliers"].size == 0 and not r["coeff"].any() and r["best_t"] == -1


# ---- the cylinder's refinement -------------------------------------------------------------------------------------------------
def test_refinement_recovers_a_noise_free_half_cylinder():
    cloud, normals = CS.half_cylinder(0.0)
    r = R.segment(CYL, cloud, normals, 0.02, 0.1, 0.0, 0.0, 100, 0.99, 1, True)
    d = np.float64([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    co = r["coeff"].astype(F64)
    assert np.abs(np.abs(co[3:6]) - d).max() < 2e-7 and abs(co[6] - 0.25) < 1e-7
    off = co[:3] - np.float64([0.5, -0.25, 0.0])
    assert np.linalg.norm(off - (off @ d) * d) < 2e-7                                # the point lies on the true axis
    assert r["inliers"].size == 240 and r["cylinder_sums"][-1, 20] < 1e-11


def test_refinement_never_raises_the_sum_of_squares():
    for seed in range(6):
        cloud, normals = CS.half_cylinder(0.003, seed=seed + 20)
        r = R.segment(CYL, cloud, normals, 0.015, 0.1, 0.0, 0.0, 60, 0.99, seed, True)
        S = r["cylinder_sums"]
        kept = S[-2] if r["cylinder_stop"] == R.STOP_NO_DECREASE else S[-1]
        assert 1 <= S.shape[0] <= R.CYLINDER_ITERATIONS and kept[20] <= S[0, 20]
        assert (np.diff(S[:-1, 20]) < 0).all()                                        # every kept step lowered it strictly
        # the sums a refined model stands on are its own: a pass at the refined chart point gives the kept sum of squares
        assert r["cylinder_stop"] in (R.STOP_PASSES, R.STOP_SMALL_STEP, R.STOP_NO_DECREASE)


def test_every_stop_reason():
    u = np.float32([0, 0, 0, 0, 0, 1, 1])
    K = np.float32([1, 0, 0])
    good = [1.0 if i == j else 0.0 for i in range(5) for j in range(i, 5)]

    def script(rows):
        it = iter(rows)
        return lambda P, D, ia, ib, r: next(it)
    # a pivot that is not > 0
    assert R.cyl_refine(u, K, script([[0.0] * 21]))[2] == R.STOP_CHOLESKY
    assert R.cyl_refine(u, K, script([good[:14] + [-1.0] + [0.1] * 5 + [1.0]]))[2] == R.STOP_CHOLESKY
    # a step that is not finite
    assert R.cyl_refine(u, K, script([good + [math.inf, 0, 0, 0, 0, 1.0]]))[2] == R.STOP_NOT_FINITE
    # a small step: the gradient is zero
    co, S, stop = R.cyl_refine(u, K, script([good + [0.0] * 5 + [1.0]]))
    assert stop == R.STOP_SMALL_STEP and S.shape[0] == 1 and co.tolist() == u.tolist()
    # no decrease: the step is refused and the unrefined parameters stay
    co, S, stop = R.cyl_refine(u, K, script([good + [0.1] * 5 + [1.0], good + [0.1] * 5 + [1.0]]))
    assert stop == R.STOP_NO_DECREASE and S.shape[0] == 2 and co.tolist() == u.tolist()
    # the pass limit: every step lowers the sum
    rows = [good + [0.1] * 5 + [1.0 / (k + 1)] for k in range(R.CYLINDER_ITERATIONS)]
    co, S, stop = R.cyl_refine(u, K, script(rows))
    assert stop == R.STOP_PASSES and S.shape[0] == R.CYLINDER_ITERATIONS and abs(float(co[6]) - (1 - 0.1 * 9)) < 1e-6
    # the chart: e is the largest |dir_e|, the lowest index among equals
    assert R.chart_of(np.float32([0, 0, 0, 0.5, -0.5, 0.5, 1]), K)[:3] == (0, 1, 2)
    assert R.chart_of(np.float32([0, 0, 0, 0.1, -0.9, 0.5, 1]), K)[:3] == (1, 0, 2)
    assert R.chart_of(np.float32([0, 0, 0, 0.1, 0.2, -0.9, 1]), K)[:3] == (2, 0, 1)
    # a refined direction keeps the unrefined one's sense
    co = R.cyl_refine(np.float32([0, 0, 0, 0, 0, -1, 1]), K, script([good + [0.0] * 5 + [1.0]]))[0]
    assert co[5] == -1


def test_cholesky_solves():
    rng = np.random.default_rng(1)
    J = rng.normal(size=(40, 5))
    rho = rng.normal(size=40)
    A, g = J.T @ J, J.T @ rho
    S = [A[i, j] for i in range(5) for j in range(i, 5)] + list(g) + [float(rho @ rho)]
    assert np.allclose(R.cyl_step(S), np.linalg.solve(A, -g), rtol=1e-10, atol=1e-12)


def test_the_jacobian_is_the_residuals_derivative():
    P, D, r = [0.3, -0.2, 0.0], [0.1, 0.25, 1.0], 0.4
    q = np.float32([[1.0, 0.5, 0.7]])

    def rho(p):
        Pp, Dp = [p[0], p[1], 0.0], [p[2], p[3], 1.0]
        return -R.cyl_terms(Pp, Dp, 0, 1, p[4], q)[0, 19]                             # J_4 rho = -rho
    p0 = [P[0], P[1], D[0], D[1], r]
    T = R.cyl_terms(P, D, 0, 1, r, q)[0]
    for i in range(4):
        hi, lo = list(p0), list(p0)
        hi[i] += 1e-6
        lo[i] -= 1e-6
        assert abs((rho(hi) - rho(lo)) / 2e-6 - (-T[[4, 8, 11, 13][i]])) < 1e-8      # J_i J_4 = -J_i


# ---- refusals, the fixture, the ABI --------------------------------------------------------------------------------------------
def test_refusals():
    cloud, normals, _ = CS.pole_and_pipe()
    ok = dict(model=CYL, threshold=0.1, weight=0.1, radius_min=0.0, radius_max=0.0, max_iterations=10, probability=0.9, axis=None, eps_angle=0.0)
    nan, inf = math.nan, math.inf
    for change in (dict(model=0), dict(model=15), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf), dict(weight=-0.01), dict(weight=1.01),
                   dict(weight=nan), dict(radius_min=-1.0), dict(radius_max=-1.0), dict(radius_min=nan), dict(radius_max=inf),
                   dict(radius_min=2.0, radius_max=1.0), dict(radius_min=1.0), dict(max_iterations=-1), dict(max_iterations=(1 << 20) + 1),
                   dict(probability=0.0), dict(probability=1.0), dict(model=PLANE, axis=(0, 0, 1)), dict(axis=(0, 0, 0)), dict(axis=(nan, 0, 1)),
                   dict(axis=(0, 0, 1), eps_angle=-0.1), dict(axis=(0, 0, 1), eps_angle=nan)):
        a = {**ok, **change}
        with pytest.raises(SR.Refused):
            R.check(a["model"], normals, a["threshold"], a["weight"], a["radius_min"], a["radius_max"], a["max_iterations"], a["probability"],
                    a["axis"], a["eps_angle"])
    with pytest.raises(SR.Refused):
        R.check(CYL, None, 0.1, 0.1, 0.0, 0.0, 10, 0.9, None, 0.0)
    R.check(CYL, normals, 0.0, 1.0, 0.0, 0.0, 0, 0.5, (0, 0, 2), 0.0)
    R.check(PLANE, normals, 0.0, 0.0, 1.0, 1.0, 1 << 20, 0.5, None, nan)               # eps_angle is ignored without an axis


def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    for model, tag in ((PLANE, "plane"), (CYL, "cyl")):
        a = g[tag + "_args"]
        r = R.segment(model, g["cloud"], g["normals"], float(a[0]), float(a[1]), float(a[2]), float(a[3]), int(a[4]), float(a[5]), int(a[6]), True,
                      None if model == PLANE else (0.0, 0.0, 1.0), float(a[7]))
        for name in ("counts", "sample", "coeff_unrefined", "moments", "cylinder_sums", "coeff", "inliers"):
            assert r[name].dtype == g[f"{tag}_{name}"].dtype and r[name].tobytes() == g[f"{tag}_{name}"].tobytes(), (tag, name)
        for name in ("iterations", "best_t", "n_unrefined", "found", "cylinder_stop"):
            assert r[name] == int(g[f"{tag}_{name}"]), (tag, name)
        assert r["found"] == 1 and r["inliers"].size > 100
    assert int(g["cyl_cylinder_stop"]) != 0 and g["cyl_cylinder_sums"].shape[0] >= 2
    assert os.path.getsize(GOLDEN) < 1 << 17


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in SYMBOLS:
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS
    for name, value in (("SACMODEL_CYLINDER", 5), ("SACMODEL_NORMAL_PLANE", 11), ("SAC_CYLINDER_ITERATIONS", 10), ("SAC_STOP_PASSES", 1),
                        ("SAC_STOP_CHOLESKY", 2), ("SAC_STOP_NOT_FINITE", 3), ("SAC_STOP_SMALL_STEP", 4), ("SAC_STOP_NO_DECREASE", 5)):
        assert f"#define ICPGPU_{name} {value}" in header and getattr(_lib, name) == value
    assert (R.CYLINDER, R.NORMAL_PLANE, R.CYLINDER_ITERATIONS) == (5, 11, 10)
    assert (R.STOP_PASSES, R.STOP_CHOLESKY, R.STOP_NOT_FINITE, R.STOP_SMALL_STEP, R.STOP_NO_DECREASE) == (1, 2, 3, 4, 5)
    assert "#define ICPGPU_VERSION_MINOR 2" in header


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_sac_segmentation_from_normals(None, 11, None, 0.1, 0.1, 0.0, 0.0, 50, 0.99, 0, 1, None, 0.0, None, None, None, None,
                                                  None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_sac_normals_fetch(None, 0, 0, None, None, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_sac_normals_stats(None, None) == _lib.ERR_INVALID_ARG


def test_the_front_end_and_the_constants():
    import icpslam_amd as pkg
    assert (pkg.SACMODEL_CYLINDER, pkg.SACMODEL_NORMAL_PLANE, pkg.SACMODEL_PLANE, pkg.SACMODEL_PERPENDICULAR_PLANE) == (5, 11, 0, 15)
    assert "SACSegmentationFromNormals" in pkg.__all__ and hasattr(pkg.SACSegmentationFromNormals, "setNormalDistanceWeight")


# ---- the street, end to end ----------------------------------------------------------------------------------------------------
def test_the_street_end_to_end():
    """NORMAL_PLANE takes the crowned ground out of the street (threshold 0.08, weight 0.1), CYLINDER with a vertical axis (0.1 rad),
    radius limits 0.05 .. 0.3, threshold 0.03 and 1000 iterations then finds one of the three poles in what remains, the normals
    estimated again there.  Measured for seeds 1, 2, 3: ground inliers among the 1 500 ground points 1449, 1450, 1449, and no more
    than 17 others; the axis at the sample's height off the pole's centre by 0.28, 0.60, 0.37 mm; the radius off by 0.28, 0.23,
    0.15 mm; the axis off the vertical by 0.00, 0.07, 0.04 degrees.  Asserted with a margin of three over the worst: 1400 ground
    points, 50 others, 2 mm, 1 mm, 0.25 degrees."""
    cloud, normals = CS.street(1)
    for seed in (1, 2, 3):
        g = R.segment(PLANE, cloud, normals, 0.08, 0.1, 0.0, 0.0, 100, 0.99, seed, True)
        on_ground = int((g["inliers"] < 1500).sum())
        assert on_ground >= 1400 and g["inliers"].size - on_ground <= 50
        rest = SR.extract(cloud, g["inliers"], True)
        rest_normals = NR.estimate(rest, None, k=12, viewpoint=(0.0, 0.0, 3.0))[0]
        c = R.segment(CYL, rest, rest_normals, 0.03, 0.1, 0.05, 0.3, 1000, 0.99, seed, True, (0, 0, 1), 0.1)
        co = c["coeff"].astype(F64)
        centre, radius = min((math.hypot(co[0] - x, co[1] - y), r) for x, y, r in CS.POLES)
        tilt = math.degrees(math.acos(min(1.0, abs(co[5]))))
        print("seed", seed, "ground", on_ground, "others", g["inliers"].size - on_ground, "centre", centre, "radius", abs(co[6] - radius), "tilt", tilt)
        assert c["found"] == 1 and c["inliers"].size > 300
        assert centre <= 2e-3 and abs(co[6] - radius) <= 1e-3 and tilt <= 0.25


# ---- the shared host / device headers, compiled for the host -------------------------------------------------------------------
def _host_check(tmp_path, mode, records, dtype):
    exe = tmp_path / "sac_normals_host_check"
    if not exe.exists():
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                               os.path.join(HERE, "cpp", "sac_normals_host_check.cpp"), "-o", str(exe)])
    path = tmp_path / f"{mode}.bin"
    np.ascontiguousarray(records, dtype).tofile(path)
    out = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.strip().split("\n")]


def _f32(word):
    return np.array([int(word, 16)], np.uint32).view(F32)[0]


def test_the_shared_headers_compiled_for_the_host_equal_the_restatement(tmp_path):
    """tests/cpp/sac_normals_host_check.cpp: icp_angle.h and icp_sac_normals.h as a plain C++ compiler builds them, on the hand cases."""
    rng = np.random.default_rng(2)
    # the angle
    y = np.concatenate((rng.uniform(0, 1, 3000), 10.0 ** rng.uniform(-30, 30, 1000), [0, 0, 2, 1, np.nan, np.inf])).astype(F32)
    x = np.concatenate((rng.uniform(0, 1, 3000), 10.0 ** rng.uniform(-30, 30, 1000), [0, 2, 0, 1, 1, np.inf])).astype(F32)
    got = np.array([_f32(w[0]) for w in _host_check(tmp_path, "angle", np.stack((y, x), axis=1), F32)], F32)
    assert got.tobytes() == R.folded_angle(y, x).tobytes()
    # the plane's and the cylinder's pairs
    cloud, normals = CS.with_non_finite(*CS.street(1))
    cloud, normals = cloud[::5], normals[::5]
    ok = np.isfinite(cloud[:, :3]).all(axis=1) & np.isfinite(normals).all(axis=1)
    plane = np.float32([0.0006, -0.00003, 0.9999998, -0.027])
    w = (F32(0.1) * (F32(1) - normals[:, 3])).astype(F32)
    rec = np.concatenate((np.tile(plane, (len(cloud), 1)), cloud[:, :3], normals[:, :3], w[:, None]), axis=1)[ok]
    got = np.array([_f32(r[0]) for r in _host_check(tmp_path, "plane", rec, F32)], F32)
    assert got.tobytes() == R.values(PLANE, cloud, normals, plane, 0.1)[ok].tobytes()
    cyl = np.float32([3.0, 2.0, 0.5, 0.01, -0.02, 0.9997, 0.10])
    on_axis = np.float32([[3.0, 2.0, 0.5, 1.0], [3.01, 1.98, 1.4997, 1.0]])             # A, and A + dir
    c2 = np.concatenate((cloud[ok], on_axis))
    n2 = np.concatenate((normals[ok], normals[ok][:2]))
    rec = np.concatenate((np.tile(cyl, (len(c2), 1)), c2[:, :3], n2[:, :3], np.full((len(c2), 1), 0.25, F32)), axis=1)
    out = _host_check(tmp_path, "cyl", rec, F32)
    want = R.values(CYL, c2, n2, cyl, 0.25)
    off = np.array([int(r[1]) for r in out], bool)
    assert off[-2] and np.array_equal(off, np.isnan(want))
    got = np.array([_f32(r[0]) for r in out], F32)
    assert got[~off].tobytes() == want[~off].tobytes()
    # the cylinder's model
    pc, pn, _ = CS.pole_and_pipe()
    S = R.samples2(3, 0, 300, len(pc))
    hand = CS.rows([[1, 0, 0], [0, 1, 0], [0, 1, 2], [1, 0, 5]])
    hand_n = CS.rows([[1, 0, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0]], 0.0)
    pc, pn = np.concatenate((hand, pc)), np.concatenate((hand_n, pn))
    S = np.concatenate((np.array([[0, 1], [0, 2], [0, 3]]), S + 4))
    S = S[S[:, 0] != S[:, 1]]
    rec = np.concatenate((pc[S[:, 0], :3], pn[S[:, 0], :3], pc[S[:, 1], :3], pn[S[:, 1], :3]), axis=1)
    out = _host_check(tmp_path, "model", rec, F32)
    want, valid = R.cylinder_models(pc, pn, S)
    assert [int(r[0]) for r in out] == valid.astype(int).tolist() and valid[:3].tolist() == [False, True, False] and valid.sum() > 100
    got = np.array([[_f32(w) for w in r[1:]] for r in out], F32)
    assert got[valid].tobytes() == want[valid].tobytes()
    # the refinement's terms, a point on the axis among them
    P, D, r = [0.3, -0.2, 0.1], [0.1, 1.0, 0.25], 0.4
    q = np.concatenate((rng.uniform(-1, 1, (50, 3)), [[0.3, -0.2, 0.1]])).astype(F32)
    q[-1] = F32(0.3), F32(-0.2), F32(0.1)
    Pq = [float(F32(v)) for v in P]                                                    # (so that the last point lies exactly on the axis)
    rec = np.concatenate((np.tile(Pq + D + [r, 0.0, 2.0], (len(q), 1)), q.astype(F64)), axis=1)
    out = _host_check(tmp_path, "terms", rec, F64)
    got = np.array([[int(w, 16) for w in row] for row in out], np.uint64).view(F64)
    want = R.cyl_terms(Pq, D, 0, 2, r, q)
    assert got.tobytes() == want.tobytes() and got[-1, 14] == 1.0 and got[-1, 20] == r * r and not got[-1, :4].any()
