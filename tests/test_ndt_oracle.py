"""The NDT C oracle (oracle/ndt_oracle.c) pinned to the NumPy restatement (tests/ndt_restated.py), which shares no code with it,
and to the library's host transform (icpgpu_ndt_step's T_out).  CPU only.

cells        keys, n, float centroids, means and raw covariances equal bit for bit; validity and floor decisions equal wherever
             the oracle's binary128 margin clears 1e-12 (the restatement copies the device's 8-sweep Jacobi, the oracle runs
             its own to convergence); icov within 1e-12 max|icov| per cell (every valid cell has condition <= 100 after the floor)
transform    bit for bit, ~10^4 random poses and the angles around the 1e-4 rule, +-pi and beyond 2 pi
derivatives  pair counts exact (brute force, position hash, cKDTree); the 29 sums within 1e-12 mag (mag = the sums of |factors|)
self-checks  binary128 eigen residuals, per-point sums against math.fsum"""
import math

import numpy as np
import pytest

import ndt_restated as nr
import oracle

F = np.float32
SPECIAL_ANGLES = [0.0, -0.0, 9.9999e-5, -9.9999e-5, 1e-4, -1e-4, 1.0001e-4, -1.0001e-4, math.pi, -math.pi, 7.0, -9.5, 100.0]


def cloud(xyz):
    xyz = np.asarray(xyz, F)
    return np.c_[xyz, np.ones(len(xyz), F)].astype(F)


def cell_scene(seed=0, offset=(0.0, 0.0, 0.0)):
    """Every decision category of the cell build: planes (the floor raises l0), a blob (no floor), needles (l0 and l1 raised),
    cells of 5 and 6 points, an axis-aligned line, a point repeated 8 times, duplicates and non-finite points.  `offset` moves the
    whole scene."""
    rng = np.random.default_rng(seed)
    o = np.asarray(offset, np.float64)
    parts = [np.c_[rng.uniform(-6, 6, (4000, 2)), rng.normal(0.3, 0.01, 4000)],
             np.c_[rng.uniform(-6, 6, 3000), rng.normal(4.4, 0.02, 3000), rng.uniform(0, 3, 3000)],
             rng.normal([2.5, -2.5, 1.5], 0.3, (1500, 3)),
             np.c_[rng.uniform(-6, 6, 1500), rng.normal(-5.5, 0.01, 1500), rng.normal(2.5, 0.01, 1500)],     # needles along x
             rng.uniform([10.1, 10.1, 10.1], [10.9, 10.9, 10.9], (5, 3)),
             rng.uniform([12.1, 10.1, 10.1], [12.9, 10.9, 10.9], (6, 3)),
             np.c_[np.linspace(14.05, 14.95, 12), np.full(12, 10.5), np.full(12, 10.5)],
             np.tile([[16.25, 10.5, 10.5], [16.75, 10.5, 10.5]], (5, 1)), [[16.5, 10.75, 10.5]] * 2,
             np.tile([[18.5, 10.5, 10.5]], (8, 1))]
    pts = cloud(np.concatenate(parts) + o)
    pts = pts[rng.permutation(len(pts))]
    bad = rng.choice(len(pts), 7, replace=False)
    pts[bad[:3], 0] = np.nan
    pts[bad[3:5], 1] = np.inf
    pts[bad[5:], 2] = -np.inf
    return pts


def far_scene(seed=0, n=3000, sigma=2e-5):
    """Thin planes and blobs 3 km from the origin: PCL's one-pass covariance cancels, down to negative eigenvalues."""
    rng = np.random.default_rng(seed)
    plane = np.c_[rng.uniform(-4, 4, (n, 2)), rng.normal(0.0, sigma, n)]
    blob = rng.normal(0.0, 0.2, (n // 2, 3)) + [0.5, 0.5, 2.5]
    return cloud(np.concatenate([plane, blob]) + [3000.2, -2999.7, 2000.4])


def check_cells_against_restatement(pts, resolution):
    """-> the oracle's cells; asserts the bitwise and the decision contract against ndt_restated.cells"""
    O = oracle.ndt_cells(pts, resolution)
    R = nr.cells(pts, resolution)
    c = O["cells"]
    assert np.array_equal(c["key"], R["key"]) and np.array_equal(c["n"], R["n"])
    assert np.array_equal(c["centroid"][:, :3].view(np.uint32), R["centroid"].view(np.uint32))
    assert (c["centroid"][:, 3] == 1).all()
    assert np.array_equal(c["mean"].view(np.uint64), R["mean"].view(np.uint64))
    big = c["n"] >= nr.MIN_POINTS
    assert np.array_equal(c["cov"][big].view(np.uint64), R["cov"][big].view(np.uint64))
    assert np.isnan(c["cov"][~big]).all() and not c["valid"][~big].any()
    assert (c["resid"] <= 1e-30).all(), c["resid"].max()
    clear = c["margin"] > 1e-12
    assert np.array_equal(c["valid"][clear] != 0, R["valid"][clear])
    # the restatement's floor decision, read from its icov: l0 of the floored covariance is 0.01 l2
    both = clear & (c["valid"] != 0) & R["valid"]
    if both.any():
        ev = np.linalg.eigvalsh(np.linalg.inv(R["icov"][both]))
        r_floored = np.abs(ev[:, 0] / ev[:, 2] - 0.01) < 1e-9
        assert np.array_equal(r_floored, c["floored"][both] > 0)
        scale = np.abs(c["icov"][both]).reshape(-1, 9).max(axis=1)
        assert (np.abs(c["icov"][both] - R["icov"][both]).reshape(-1, 9).max(axis=1) <= 1e-12 * scale).all()
        # condition <= 100 after the floor (the premise of the icov bound)
        ic_ev = np.linalg.eigvalsh(c["icov"][both])
        assert (ic_ev[:, 2] / ic_ev[:, 0] <= 100 * (1 + 1e-9)).all()
    return O


def categories(c):
    """the decision categories that occur: small, invalid (clear margin), valid, floored l0, floored l0 and l1"""
    clear = c["margin"] > 1e-12
    return dict(small=int((c["n"] < 6).sum()), invalid=int((clear & (c["n"] >= 6) & (c["valid"] == 0)).sum()),
                valid=int((clear & (c["valid"] != 0) & (c["floored"] == 0)).sum()),
                floored1=int((clear & (c["valid"] != 0) & (c["floored"] == 1)).sum()),
                floored2=int((clear & (c["valid"] != 0) & (c["floored"] == 2)).sum()))


# ---- cells ------------------------------------------------------------------------------------------------------------------
def test_cells_match_the_restatement_with_every_decision():
    pts = cell_scene()
    total = dict.fromkeys(("small", "invalid", "valid", "floored1", "floored2"), 0)
    for res in (0.3, 1.0, 2.5):
        cat = categories(check_cells_against_restatement(pts, res)["cells"])
        assert cat["valid"] and cat["floored1"] and cat["floored2"], (res, cat)
        far = check_cells_against_restatement(far_scene(), res)["cells"]
        for k, v in categories(far).items():
            total[k] += v + cat[k]
    assert all(v > 0 for v in total.values()), total     # (invalid: negative eigenvalues from the cancellation 3 km out)
    for res in (0.05, 5.0):                                   # (0.05: few cells reach 6 points; 5: few cells)
        check_cells_against_restatement(pts, res)


@pytest.mark.parametrize("seed", [1, 2])
def test_cells_on_synthetic_scans(seed):
    from icpslam_amd import synth
    scan = synth.scan(synth.make_scene(seed), np.eye(4), 60000, seed=seed)
    for res in (0.05, 0.3, 1.0, 2.5, 5.0):
        check_cells_against_restatement(scan, res)


def test_cells_edges():
    assert oracle.ndt_cells(np.zeros((0, 4), F), 1.0)["cells"].size == 0
    nan = cloud([[np.nan, 0, 0]] * 10)
    O = oracle.ndt_cells(nan, 1.0)
    assert O["cells"].size == 0 and not O["has_cells"]
    over = cloud([[-1e6, 0, 0], [1e6, 0, 0], [0, -1e6, 0], [0, 1e6, 0], [0, 0, -1e5], [0, 0, 1e5]] * 2)
    with pytest.raises(oracle.NdtOverflow):
        oracle.ndt_cells(over, 0.05)
    with pytest.raises(nr.Overflow):
        nr.cells(over, 0.05)


def excess_scene(resolution=0.7, cells=6, seed=0):
    """Cells whose float centroid lies outside the cell their points were keyed to (e > 0): points a few ulps below a boundary in x
    whose float sum rounds up past it ("up": keyed to b - 1, centroid on b's side), and points a few ulps above one whose sum
    rounds down ("dn"); y and z spread inside the cell.  -> (cloud, [(kind, boundary index)])"""
    rng = np.random.default_rng(seed)
    res = F(resolution)
    inv = F(F(1) / res)
    out, found = [], []
    while len(found) < cells:
        b = int(rng.integers(-400, 400))
        x = F(b * float(res))
        while np.floor(F(x * inv)) >= b:
            x = np.nextafter(x, F(-np.inf))
        while np.floor(F(np.nextafter(x, F(np.inf)) * inv)) < b:
            x = np.nextafter(x, F(np.inf))
        below = [x]
        for _ in range(3):
            below.append(np.nextafter(below[-1], F(-np.inf)))
        above = [np.nextafter(x, F(np.inf))]
        for _ in range(3):
            above.append(np.nextafter(above[-1], F(np.inf)))
        kind = ("up", "dn")[len(found) % 2]
        vals, cell = (below, b - 1) if kind == "up" else (above, b)
        n = int(rng.integers(6, 32))
        xs = rng.choice(np.array(vals, F), n)
        s = F(0)
        for v in xs:
            s = F(s + v)
        u = float(F(s / F(n))) * float(inv)
        if (kind == "up" and u < cell + 1) or (kind == "dn" and u >= cell):
            continue
        yz = rng.uniform(0.15, 0.85, (n, 2)) * float(res) + np.array([len(found) * 3, 5]) * float(res)
        out.append(np.c_[xs, yz].astype(F))
        found.append((kind, b))
    return cloud(np.concatenate(out)), found


def test_excess_is_measured():
    """Centroids past the upper and below the lower boundary of their cell: e > 0 in the oracle; the restatement agrees on every
    centroid bit (so the excursion is the contract's, not a rounding of either side)."""
    for res in (0.7, 0.3):
        pts, found = excess_scene(res)
        O = check_cells_against_restatement(pts, res)
        c = O["cells"]
        assert len(c) == len(found) and c["valid"].all()
        assert (c["excess"] > 0).all() and O["max_excess"] == c["excess"].max() > 0


# ---- the eigen-decomposition's own checks ---------------------------------------------------------------------------------------
def test_oracle_eigenvalues_against_numpy_on_random_symmetric_matrices():
    """The binary128 eigenvalues of random covariances (well and badly conditioned, repeated) against numpy's eigvalsh, within
    its own error bound, and the residual the oracle reports."""
    rng = np.random.default_rng(5)
    pts = []
    for k in range(200):
        scale = rng.choice([1e-3, 1e-2, 0.1, 0.3], 3) * rng.choice([1.0, 1e-3], 3)
        A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        blob = (rng.normal(size=(30, 3)) * scale) @ A.T * 0.1 + 0.5
        pts.append(blob + [2.0 * k, 0, 0])
    O = oracle.ndt_cells(cloud(np.concatenate(pts)), 2.0)
    c = O["cells"][O["cells"]["n"] >= 6]
    ev = np.linalg.eigvalsh(c["cov"])
    tol = 8 * np.finfo(float).eps * np.abs(ev).max(axis=1, keepdims=True)
    assert (np.abs(c["eig"] - ev) <= tol).all()
    assert (c["resid"] <= 1e-30).all()


# ---- transform ----------------------------------------------------------------------------------------------------------------------
def test_transform_bit_for_bit(built):
    from icpslam_amd.registration import ndt_step
    rng = np.random.default_rng(3)
    poses = [np.r_[rng.normal(0, 50, 3), rng.uniform(-4, 4, 3)] for _ in range(8000)]
    poses += [np.r_[rng.normal(0, 1e3, 3), rng.normal(0, 0.05, 3)] for _ in range(2000)]
    poses += [np.r_[0.5, -0.25, 3e3, a, b, c] for a in SPECIAL_ANGLES for b in SPECIAL_ANGLES[::3] for c in SPECIAL_ANGLES[1::3]]
    zero = np.zeros(29)
    for p in poses:
        T = oracle.ndt_transform(p)
        assert np.array_equal(T.view(np.uint32), nr.transform_float(p).view(np.uint32)), p
        st, p_out, _, T_lib = ndt_step(zero, p, 0.1, 0.1)          # |delta| = 0: T_out = T(p)
        assert st == 1 and np.array_equal(p_out, p)
        assert np.array_equal(T.view(np.uint32), T_lib.view(np.uint32)), p


def test_angle_terms_and_the_small_angle_rule():
    rng = np.random.default_rng(4)
    for p in [np.r_[0, 0, 0, a, b, c] for a in SPECIAL_ANGLES for b in SPECIAL_ANGLES[::2] for c in SPECIAL_ANGLES[1::2]] + \
             [np.r_[0, 0, 0, rng.uniform(-7, 7, 3)] for _ in range(200)]:
        j, h = oracle.ndt_angle_terms(p)
        jr, hr = nr.angle_terms(p)
        assert np.abs(j - jr).max() <= 4e-16 and np.abs(h - hr).max() <= 4e-16, p
        small = np.abs(p[3:]) < 1e-4
        if small.all():                                            # cos 1, sin 0: the tables are exact
            assert np.array_equal(j, jr) and np.array_equal(h, hr)


# ---- derivatives -------------------------------------------------------------------------------------------------------------------
def check_derivatives_against_restatement(tgt, src, resolution, ratio, poses):
    O = oracle.ndt_cells(tgt, resolution)
    tg = nr.Target(tgt, resolution, ratio)
    for p in poses:
        a = oracle.ndt_derivatives(O, src, p, resolution, ratio, search=oracle.NDT_SEARCH_HASH)
        b = oracle.ndt_derivatives(O, src, p, resolution, ratio, search=oracle.NDT_SEARCH_BRUTE)
        assert np.array_equal(a["sums"].view(np.uint64), b["sums"].view(np.uint64)) and a["pairs"] == b["pairs"]
        ref = nr.derivatives(tg, src, nr.transform_float(p), p)
        assert a["pairs"] == ref[0] and a["skipped"] == 0 and a["near"] == 0, (p, a["pairs"], ref[0])
        assert (np.abs(a["sums"] - ref) <= 1e-12 * a["mag"]).all(), (p, (np.abs(a["sums"] - ref) / a["mag"]).max())
        assert (a["mag"] >= np.abs(a["sums"])).all()


@pytest.mark.parametrize("resolution,ratio", [(0.3, 0.01), (1.0, 0.55), (2.5, 0.99), (0.05, 0.55)])
def test_derivatives_match_the_restatement(resolution, ratio):
    from icpslam_amd import synth
    src, tgt, T_gt = synth.make_pair(4000, 30000, seed=4)
    rng = np.random.default_rng(1)
    poses = [np.zeros(6), np.r_[T_gt[:3, 3], 0.0, 0.0, 0.02], np.r_[rng.normal(0, 0.2, 3), 9.9999e-5, -1e-4, 1.0001e-4],
             np.r_[rng.normal(0, 0.2, 3), rng.normal(0, 0.05, 3)], np.r_[0.2, -0.1, 0.0, 3.0, -1.2, 2.0]]
    check_derivatives_against_restatement(tgt, src, resolution, ratio, poses)


def test_pairs_match_a_kd_tree_on_the_cell_scene():
    pts = cell_scene(3)
    rng = np.random.default_rng(2)
    src = pts[rng.choice(len(pts), 3000, replace=False)]
    check_derivatives_against_restatement(pts, src, 1.0, 0.55, [np.zeros(6), np.r_[0.1, 0.2, -0.1, 0.01, -0.02, 0.03]])


def test_sums_against_fsum_per_point():
    """The pass over a cloud against math.fsum of the passes over its points one at a time (binary128 accumulation)."""
    from icpslam_amd import synth
    src, tgt, _ = synth.make_pair(60, 5000, seed=9)
    O = oracle.ndt_cells(tgt, 1.0)
    p = np.r_[0.05, -0.02, 0.01, 0.02, -0.01, 0.03]
    whole = oracle.ndt_derivatives(O, src, p, 1.0)
    per = [oracle.ndt_derivatives(O, src[i:i + 1], p, 1.0) for i in range(len(src))]
    assert whole["pairs"] == sum(x["pairs"] for x in per) > 100
    for k in range(29):
        s = math.fsum(x["sums"][k] for x in per)
        assert abs(whole["sums"][k] - s) <= 2 ** -50 * whole["mag"][k], k


def test_the_skip_rule_is_unreachable_for_psd_cells():
    """d2 < 1 over resolution {0.05 .. 5} x outlier ratio {0.01 .. 0.99}: with a PSD icov, q'^T icov q' >= 0, so d2 e <= d2 < 1 and
    PCL's `d2 e > 1 / < 0 / NaN` skip never fires (it would need a non-PSD or non-finite icov, which the cell build rejects).
    The near-zero-d1 corner (resolution 0.05, ratio 0.55: d2 ~ 0.9996, |d1| ~ 1e-3) keeps its sums meaningful only through mag."""
    d1s = []
    for res in (0.05, 0.3, 1.0, 2.5, 5.0):
        for ratio in (0.01, 0.55, 0.99):
            d1, d2 = nr.gauss_constants(res, ratio)
            assert 0.08 < d2 < 1.0, (res, ratio, d2)
            d1s.append(abs(d1))
    assert min(d1s) < 2e-3
