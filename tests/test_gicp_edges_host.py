"""The GICP edge-case table (tests/gicp_edge_cases.py) against the CPU oracle, the rule "fewer than 20 FINITE points is a cloud that
is too small" on the oracle's side, and the oracle against its NumPy restatement on the small cases.  No GPU."""
import numpy as np
import pytest

import gicp_edge_cases as ec
import oracle

CASES = [c.name for c in ec.cases()]


@pytest.mark.parametrize("name", CASES)
def test_every_case_ends_as_recorded(name):
    """state, converged, and iterations / n_corr where they are the point: a case that stops hitting what it was built for fails"""
    ec.check_exit(ec.by_name(name), ec.reference(name))


def test_the_table_holds_what_the_cases_need():
    names = set(CASES)
    assert {"ns_%d" % n for n in ec.SIZES} <= names and "nt_20" in names
    for c in ec.cases():
        fin_s, fin_t = (int(np.isfinite(x[:, :3]).all(axis=1).sum()) for x in (c.src, c.tgt))
        assert c.src.shape[0] >= 20 and c.tgt.shape[0] >= 20 and max(c.src.shape[0], c.tgt.shape[0]) <= 65537, c.name
        assert bool(c.exit.get("refused")) == (min(fin_s, fin_t) < 20), c.name
    assert int(np.isfinite(ec.by_name("finite_20_of_30").src[:, :3]).all(axis=1).sum()) == 20
    assert int(np.isfinite(ec.by_name("finite_19_of_30_src").src[:, :3]).all(axis=1).sum()) == 19
    assert int(np.isfinite(ec.by_name("finite_19_of_30_tgt").tgt[:, :3]).all(axis=1).sum()) == 19
    assert not np.isfinite(ec.by_name("nonfinite_last_of_1025").src[-1, :3]).all()
    # the float64 guess is not a float32 matrix in disguise, and both sides round it to the float32 case's matrix
    g64, g32 = ec.by_name("guess_small_f64").guess, ec.by_name("guess_small").guess
    assert g64.dtype == np.float64 and g32.dtype == np.float32 and not np.array_equal(g64, g32.astype(np.float64))
    a, b = ec.reference("guess_small_f64"), ec.reference("guess_small")
    assert np.array_equal(a["T"].view(np.uint32), b["T"].view(np.uint32)) and np.array_equal(a["cloud"], b["cloud"])
    # ~1 rad of yaw: R = transformation * guess is far from the identity in the Mahalanobis step
    assert abs(ec.by_name("guess_yaw_1rad").guess[0, 1]) > 0.8


@pytest.mark.parametrize("r", [1.0, 0.5, 0.3])
def test_gate_cases_sit_where_they_are_meant_to(r):
    """The oracle's own search gives the hand-built points the float d2 they were built for (one float below the gate, on it / the
    first float above it, the next one), all to the lone target point; the nominal gate keeps exactly the inner ones, the gate one
    step wider exactly the `on` points more."""
    c, w = ec.by_name("gate_%g" % r), ec.by_name("gate_%g_wide" % r)
    g = ec.gate_points(r)
    assert g["exact"] == (r != 0.3)
    k = sum(len(g[n]) for n in ("inside", "on", "outside"))
    idx, d2 = oracle.nn(c.src[-k:], c.tgt)
    assert (idx == c.tgt.shape[0] - 1).all()
    want = np.concatenate([np.full(len(g[n]), g["d2"][n], np.float32) for n in ("inside", "on", "outside")])
    assert np.array_equal(d2.view(np.uint32), want.view(np.uint32)), (d2, want)
    r2 = float(c.params["max_correspondence_distance"]) ** 2
    assert float(g["d2"]["inside"]) < r2 <= float(g["d2"]["on"]) < float(w.params["max_correspondence_distance"]) ** 2 < float(g["d2"]["outside"])
    assert (float(g["d2"]["on"]) == r2) == g["exact"]
    _, d2_all = oracle.nn(c.src, c.tgt)
    a, b = ec.reference(c.name), ec.reference(w.name)
    assert a["n_corr"] == int((d2_all.astype(np.float64) < r2).sum())
    assert b["n_corr"] - a["n_corr"] == len(g["on"]) == 3


def test_fewer_than_twenty_finite_points_is_too_small():
    """30 points of which 18 are finite: oracle.gicp_covariances used to read past a short neighbour list (a crash), the alignment
    returned converged with an all-NaN rotation.  Now: an exception, and the answer of a cloud of fewer than 20 points."""
    probe = ec.by_name("finite_18_of_30_src")
    for name in ("finite_18_of_30_src", "finite_19_of_30_src", "finite_19_of_30_tgt"):
        c = ec.by_name(name)
        r = ec.reference(name)
        assert not r["converged"] and r["iterations"] == 0 and r["n_corr"] == 0 and r["state"] == ec.NOT_CONVERGED
        assert np.array_equal(r["T"], np.eye(4, dtype=np.float32))
        small = c.src if name.endswith("src") else c.tgt
        for order in (False, True):
            with pytest.raises(RuntimeError, match="20"):
                oracle.gicp_covariances(small, pcl_order=order)
        with pytest.raises(RuntimeError, match="20"):
            oracle.gicp_neighbours(small)
    out = oracle.icp_align(probe.src, probe.tgt, oracle.default_params(method=oracle.GICP), want_cloud=True)
    ok = np.isfinite(probe.src[:, :3]).all(axis=1)
    assert np.array_equal(out["cloud"][ok], probe.src[ok]) and np.isnan(out["cloud"][~ok, :3]).any(axis=1).all()   # T = I
    legal = ec.by_name("finite_20_of_30")
    cov = oracle.gicp_covariances(legal.src)
    fin = np.isfinite(legal.src[:, :3]).all(axis=1)
    assert np.isfinite(cov[fin]).all() and np.isfinite(ec.reference(legal.name)["T"]).all()


SMALL_CASES = [c.name for c in ec.cases() if (ec.is_small(c) or c.name.startswith(("guess_", "gate_"))) and not c.exit.get("refused")]
# where the two restatements end on the same float32 pose (the others part ways inside an inner BFGS run, see below)
SAME_BITS = {"ns_21", "ns_63", "ns_64", "ns_513", "ns_1023", "ns_1024", "ns_1025", "min_3", "min_4", "min_5", "guess_small", "guess_small_f64",
             "guess_yaw_1rad", "guess_exact", "guess_far", "gate_1", "gate_1_wide", "gate_0.5", "gate_0.5_wide", "gate_0.3", "gate_0.3_wide"}


def _pose_gap(Ta, Tb):
    return (float(np.abs(np.asarray(Ta, np.float64)[:3, :3] - np.asarray(Tb, np.float64)[:3, :3]).max()),
            float(np.linalg.norm(np.asarray(Ta, np.float64)[:3, 3] - np.asarray(Tb, np.float64)[:3, 3])))


def test_the_small_cases_are_the_ones_the_issue_names():
    assert {"ns_%d" % n for n in ec.SIZES if n <= ec.SMALL} <= set(SMALL_CASES) and SAME_BITS <= set(SMALL_CASES)
    assert {"nt_20", "gate_0.3", "min_3", "min_4", "min_5", "guess_yaw_1rad", "guess_far"} <= set(SMALL_CASES)


@pytest.mark.parametrize("name", SMALL_CASES)
def test_numpy_restatement_agrees_on_the_small_cases(name):
    """oracle/gicp_oracle.c against oracle/gicp_oracle_np.py (SciPy kd-tree, LAPACK SVD and inverse, BFGS in Python; it has an align
    with guess and gate, no force_iterations -- the gate cases' one forced iteration is its max_iterations = 1 -- and no non-finite
    points) on every finite case of at most 1025 sources, the gate and the guess cases, at what
    tests/test_oracle.py::test_gicp_two_restatements_agree demands: same end, iterations within 3, correspondences within 0.1 %
    (below 1000 of them that is equality), rotation 1e-4, translation 1e-3, covariances 1e-9.

    (1) The FIRST outer iteration -- same start, the identity; the same correspondences, compared exactly -- to that pose
        tolerance, for every case.
    (2) EVERY outer iteration of the oracle, stepped through from the oracle's own transform before it (problem_at): the same number
        of correspondences, exactly; and the oracle's step judged by the restatement's independently computed objective: it
        descends, f(oracle's end) < f(start).
    (3) The whole registration: end, iterations and correspondences for every case; the pose to the same tolerance from 1000
        sources on, and the same float32 bits on the 21 cases of SAME_BITS.
    What is printed and not asserted is the final pose of ns_20, ns_65, ns_255, ns_256, ns_257, ns_511, ns_512 and nt_20, and the
    reason is measured here, not supposed: stepping through (2), all but eight of the 64 steps of these cases end within 1e-6 of
    each other in the state vector, and the others part ways INSIDE one inner BFGS run over identical correspondences from an identical
    start -- ns_255's second step by 2.4 cm, ns_256's third by 6.4 mm, ns_511's first by 0.2 mm, ns_512's second by 0.06 mm,
    nt_20's first two by 0.03 mm -- where both runs are cut off by PCL's cap of 20 inner iterations with a gradient norm of
    0.012 .. 0.3, above the 0.01 that would end them: a few hundred correspondences against a 4000-point target leave a valley
    the line search has not walked out of, and the two ends differ by 2e-3 of the objective at most (ns_255; both below the
    start by 15 %).  The next outer iteration starts from different correspondences.  A gap of that kind says nothing about
    either restatement; a wrong cost, gradient or search would show in (1) and (2)."""
    from oracle import gicp_oracle_np as gnp
    c, b = ec.by_name(name), ec.reference(name)
    kw = {k: v for k, v in c.params.items() if k != "force_iterations"}
    gate = c.params.get("max_correspondence_distance", 1.0)
    # (3) the whole registration
    a = gnp.gicp_align(c.src, c.tgt, guess=c.guess, sums="exact", **kw)
    assert a["converged"] == b["converged"] and abs(a["iterations"] - b["iterations"]) <= 3
    assert abs(a["n_corr"] - b["n_corr"]) <= 0.001 * b["n_corr"], (a["n_corr"], b["n_corr"])
    dR, dt = _pose_gap(a["T"], b["T"])
    print("%-18s whole: iterations %d / %d  n_corr %d / %d  dR %.2e  dt %.2e" % (name, a["iterations"], b["iterations"], a["n_corr"], b["n_corr"], dR, dt))
    if c.src.shape[0] >= 1000:
        assert dR <= 1e-4 and dt <= 1e-3, (dR, dt)
    if name in SAME_BITS:
        assert np.array_equal(np.asarray(a["T"], np.float32).view(np.uint32), np.asarray(b["T"], np.float32).view(np.uint32)), (dR, dt)
    if c.src.shape[0] <= ec.SMALL:
        assert np.abs(gnp.covariances(c.src) - oracle.gicp_covariances(c.src)).max() <= 1e-9
    # (1) the first outer iteration
    p1 = oracle.default_params(method=oracle.GICP, **dict(c.params, max_iterations=1))
    o1 = oracle.icp_align(c.src, c.tgt, p1, guess=c.guess)
    n1 = gnp.gicp_align(c.src, c.tgt, guess=c.guess, sums="exact", **dict(kw, max_iterations=1))
    assert (n1["n_corr"], n1["iterations"], n1["converged"]) == (o1["n_corr"], o1["iterations"], o1["converged"])
    dR, dt = _pose_gap(n1["T"], o1["T"])
    print("%-18s first iteration: n_corr %d  dR %.2e  dt %.2e" % (name, o1["n_corr"], dR, dt))
    assert dR <= 1e-4 and dt <= 1e-3, (dR, dt)
    # (2) every outer iteration of the oracle from its own start
    trace = oracle.icp_align(c.src, c.tgt, oracle.default_params(method=oracle.GICP, **c.params), guess=c.guess, want_trace=True)["trace"]
    assert len(trace) == b["iterations"]
    T0 = np.eye(4)
    for k, t in enumerate(trace):
        cost, x0, n = gnp.problem_at(c.src, c.tgt, T0, c.guess, gate)
        assert n == t["n_corr"], (k, n, t["n_corr"])
        f0, _ = cost.fdf(x0)
        xo = gnp._state_from_matrix(t["Tk"])
        fo, go = cost.fdf(xo)
        xn, ok = gnp._bfgs_minimize(cost, x0)
        fn, gn = cost.fdf(xn)
        print("%-18s step %d: n_corr %d  f start %.6e  oracle %.9e  restatement %.9e  |g| %.1e / %.1e  |x_o - x_n| %.1e" % (
            name, k, n, f0, fo, fn, np.linalg.norm(go), np.linalg.norm(gn), np.linalg.norm(xo - xn)))
        assert ok and (fo < f0 or np.array_equal(xo, x0)), (k, f0, fo)
        T0 = t["Tk"]
    if b["iterations"] == 0:   # the minimum and the hopeless guess: the count that ends the registration is the same
        assert gnp.problem_at(c.src, c.tgt, np.eye(4), c.guess, gate)[2] == b["n_corr"] < 4


def test_numpy_restatement_refuses_fewer_than_twenty_finite_points():
    from oracle import gicp_oracle_np as gnp
    few = ec.by_name("finite_19_of_30_src")
    with pytest.raises(ValueError):
        gnp.covariances(few.src)
    a = gnp.gicp_align(few.src, few.tgt)
    assert not a["converged"] and a["iterations"] == 0 and a["n_corr"] == 0 and np.array_equal(a["T"], np.eye(4, dtype=np.float32))
