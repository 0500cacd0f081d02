"""The fast point feature histograms' rules on the host (tests/fpfh_restated.py; include/icpgpu.h, "fast point feature
histograms"): the vectorised restatement against the literal per-point, per-pair loop, the sector rule against float64 atan2, the
answers that can be derived by hand, the golden fixture and the symbol's ABI.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import fpfh_restated as R
import normals_restated as N
from icpslam_amd import _lib, synth

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rows_f", "fpfh_512.npz")
# A sub-histogram's bins are h[b] * f with f = float32(100 / s) and s the float64 sum of the h[b]: each product is off by at most
# 2^-24 relative, f by another 2^-24, so the eleven products sum to 100 within 100 * 2 * 2^-24 (1.2e-5) plus second-order terms.
SUM_TOL = 100.0 * 3 * 2.0 ** -24


def same(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).shape == np.asarray(w).shape
               and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def cloud_of(xyz):
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = np.asarray(xyz, F32)
    return c


def random_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 4)).astype(F32)
    v[:, :3] /= np.linalg.norm(v[:, :3], axis=1, keepdims=True).astype(F32)
    return v


# ---- the two forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_vectorised_and_literal_forms_agree(seed):
    rng = np.random.default_rng(seed)
    cloud = cloud_of(rng.normal(size=(150, 3)))
    cloud[7] = cloud[3]          # a duplicated point
    cloud[20, 1] = np.nan        # a non-finite row
    normals = N.estimate(cloud, None, k=8)[0].copy()  # estimated normals: NaN where the row is empty
    normals[50, 0] = np.inf
    queries = cloud_of(rng.normal(size=(30, 3)))
    queries[:5] = cloud[:5]      # coincident with cloud points
    queries[9, 2] = np.nan
    for q in (None, queries):
        for mode in (dict(k=2), dict(k=7), dict(radius=0.5), dict(radius=1.2)):
            assert same(R.estimate(cloud, normals, q, **mode), R.estimate_literal(cloud, normals, q, **mode)), (q is None, mode)


def test_scan_with_estimated_normals_and_the_sums():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 400, 5)
    normals = N.estimate(cloud, None, k=10)[0]
    for mode in (dict(k=10), dict(radius=0.8)):
        fpfh, counts, spfh = R.estimate(cloud, normals, None, **mode)
        assert same((fpfh, counts, spfh), R.estimate_literal(cloud, normals, None, **mode))
        sums = fpfh.astype(F64).reshape(len(fpfh), 3, 11).sum(axis=2)
        live = np.isfinite(fpfh).all(axis=1)[:, None] & (sums != 0)
        assert live.any() and (np.abs(sums[live] - 100.0) <= SUM_TOL).all(), np.abs(sums[live] - 100.0).max()
        # an SPFH sub-histogram counts every non-skipped pair once: count * incr with count <= m - 1
        ssum = spfh.astype(F64).reshape(len(spfh), 3, 11).sum(axis=2)
        assert (ssum <= 100.0 + 1e-3).all()


# ---- the sector rule --------------------------------------------------------------------------------------------------------
def test_sector_rule_equals_atan2_away_from_the_edges():
    rng = np.random.default_rng(11)
    ang = rng.uniform(-math.pi, math.pi, 200000)
    mag = 10.0 ** rng.uniform(-3, 3, ang.size)
    x, y = (mag * np.cos(ang)).astype(F32), (mag * np.sin(ang)).astype(F32)
    theta = np.arctan2(y.astype(F64), x.astype(F64)) + math.pi              # in [0, 2 pi]
    pos = theta * 11.0 / (2.0 * math.pi)
    away = np.abs(pos - np.round(pos)) * (2.0 * math.pi / 11.0) > 1e-5      # farther than 1e-5 rad from every edge, 0 and 2 pi included
    assert away.mean() > 0.999
    want = np.minimum(np.floor(pos), 10).astype(np.int64)
    got = R.angle_bin(y, x)
    assert np.array_equal(got[away], want[away])
    assert set(got.tolist()) == set(range(11))


def test_sector_rule_at_zero_and_on_the_axes():
    z, nz, one = F32(0.0), F32(-0.0), F32(1.0)
    # x = y = 0 of either sign: bin 5, where atan2f(+-0, +0) = +-0 puts it (PCL's atan2f(+-0, -0) = +-pi would go to bin 10 or 0)
    for y in (z, nz):
        for x in (z, nz):
            assert R.angle_bin([y], [x])[0] == 5, (y, x)
    by_hand = {(one, z): 5,      # +x: angle 0 -> 11 * 0.5 = 5.5
               (one, nz): 5,
               (z, one): 8,      # +y: pi / 2 -> 11 * 0.75 = 8.25
               (nz, one): 8,
               (z, -one): 2,     # -y: -pi / 2 -> 11 * 0.25 = 2.75
               (nz, -one): 2,
               (-one, nz): 0,    # -x from below: -pi -> 0
               (-one, z): 0}     # -x from above: +pi -> 11, PCL clamps to bin 10; DEVIATION: bin 0
    for (x, y), want in by_hand.items():
        assert R.angle_bin([y], [x])[0] == want, (x, y)
    for (x, y), want in by_hand.items():
        if not (x == -one and not np.signbit(y)):
            pos = (math.atan2(float(y), float(x)) + math.pi) * 11.0 / (2.0 * math.pi)
            assert min(int(math.floor(pos)), 10) == want
    assert R.angle_bin([F32(np.nan)], [one])[0] == 5 and R.angle_bin([one], [F32(np.nan)])[0] == 5  # (b NaN: edges 1..5 count, no test passes)


def test_unit_bins():
    f = F32([-1.0, -0.9999999, -0.82, 0.0, 0.09, 0.0910, 0.999, 1.0, 1.5, -1.5, np.inf, -np.inf, np.nan])
    assert R.unit_bin(f).tolist() == [0, 0, 0, 5, 5, 6, 10, 10, 10, 0, 10, 0, 0]


# ---- answers derived by hand ------------------------------------------------------------------------------------------------
def test_planar_lattice_has_its_whole_mass_in_three_bins():
    """z = 0 lattice, normals (0, 0, 1): d is in the plane, so a1 = a2 = 0 (no swap, f3 = 0 -> bin 22 + 5), v = d x n is a unit vector
    in the plane (f2 = v . n = 0 -> bin 11 + 5), w = n x v is in the plane too (y = w . n = 0) and x = n . n = 1: bin 5."""
    g = np.arange(7, dtype=F32)
    xyz = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    cloud = cloud_of(np.concatenate([xyz, np.zeros((len(xyz), 1), F32)], axis=1))
    cloud = np.concatenate([cloud, cloud[24:25]])  # the centre point twice: one entry of each copy's row is skipped (f4 = 0)
    normals = np.tile(F32([0, 0, 1, 0]), (len(cloud), 1))
    for mode in (dict(k=9), dict(radius=1.5), dict(radius=2.1)):
        for fpfh, counts, spfh in (R.estimate(cloud, normals, None, **mode), R.estimate_literal(cloud, normals, None, **mode)):
            others = np.ones(33, bool)
            others[[5, 16, 27]] = False
            assert not fpfh[:, others].any() and not spfh[:, others].any()
            assert (np.abs(fpfh[:, [5, 16, 27]] - 100.0) <= SUM_TOL).all()
            pairs = counts - 1                     # every row entry but the point itself ...
            pairs[[24, 49]] -= 1                   # ... and, for the two copies of the centre, but the other copy
            incr = F32(100.0) / (counts - 1).astype(F32)
            assert np.array_equal(spfh[:, 5], pairs.astype(F32) * incr)
            assert np.array_equal(spfh[:, 16], spfh[:, 5]) and np.array_equal(spfh[:, 27], spfh[:, 5])
            assert spfh[24, 5] < 100 and (np.delete(spfh[:, 5], [24, 49]) == 100).all()


def test_swap_rule_at_equal_angles():
    """|a1| == |a2| exactly: no swap (PCL swaps only on >), so f3 = a1 = 0.6 -> bin 8; a swap would give f3 = -a2 = -0.6 -> bin 2."""
    Pp, Pj = F32([0, 0, 0]), F32([1, 0, 0])
    Np, Nj = F32([0.6, 0.8, 0]), F32([0.6, 0, 0.8])
    ok, b1, b2, b3 = R.pair_bins(Pp, Np, Pj, Nj)
    assert ok[0] and b3[0] == 8
    assert R.pair_bins_literal(Pp, Np, Pj, Nj) == (b1[0], b2[0], 8)
    # just below and just above: |a1| < |a2| swaps, |a1| > |a2| does not
    lower = F32([np.nextafter(F32(0.6), F32(0)), 0.8, 0])
    assert R.pair_bins(Pp, lower, Pj, Nj)[3][0] == 2 and R.pair_bins_literal(Pp, lower, Pj, Nj)[2] == 2
    assert R.pair_bins(Pp, Np, Pj, F32([np.nextafter(F32(0.6), F32(0)), 0, 0.8]))[3][0] == 8
    # the frame by hand, without a swap: v = d x n1 = (0, 0, 0.8) -> (0, 0, 1); f2 = v . n2 = 0.8 -> floor(11 * 0.9) = 9;
    # w = n1 x v = (0.8, -0.6, 0); y = w . n2 = 0.48, x = n1 . n2 = 0.36: atan2 = 0.927 -> floor(11 * (0.927 + pi) / (2 pi)) = 7
    assert (b1[0], b2[0]) == (7, 9)


def test_skipped_pairs():
    Pp, Np = F32([1, 2, 3]), F32([1, 0, 0])
    good = F32([0, 1, 0])
    cases = {"f4 = 0": (Pp, good), "vn = 0": (F32([3, 2, 3]), F32([0, 1, 0])), "NaN normal": (F32([2, 3, 4]), F32([0, np.nan, 1]))}
    for name, (Pj, Nj) in cases.items():
        assert not R.pair_bins(Pp, Np, Pj, Nj)[0][0], name
        assert R.pair_bins_literal(Pp, Np, Pj, Nj) is None, name
    assert not R.pair_bins(Pp, F32([np.inf, 0, 0]), F32([2, 3, 4]), good)[0][0]
    assert R.pair_bins(Pp, Np, F32([2, 3, 4]), good)[0][0] and R.pair_bins_literal(Pp, Np, F32([2, 3, 4]), good) is not None
    # in a cloud: point 0 with a coincident copy (1), a neighbour along its normal (2), one with a NaN normal (3), a good one (4)
    cloud = cloud_of([[1, 2, 3], [1, 2, 3], [3, 2, 3], [2, 3, 4], [1, 3, 3]])
    normals = np.zeros((5, 4), F32)
    normals[:, :3] = F32([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, np.nan, 1], [0, 0, 1]])
    for est in (R.estimate, R.estimate_literal):
        fpfh, counts, spfh = est(cloud, normals, None, k=5)
        assert counts.tolist() == [5] * 5
        assert spfh[0].reshape(3, 11).sum(axis=1).tolist() == [25.0] * 3  # one pair of four counted: 1 * (100 / 4)
        assert not spfh[3].any()                                           # its own normal is NaN: every pair skipped


def test_rows_of_one_and_two_entries():
    one = cloud_of([[1, 2, 3]])
    for est in (R.estimate, R.estimate_literal):
        fpfh, counts, spfh = est(one, random_normals(1, 0), None, k=2)
        assert counts.tolist() == [1] and not fpfh.any() and not spfh.any()
        two = cloud_of([[0, 0, 0], [1, 0, 0]])
        normals = np.zeros((2, 4), F32)
        normals[:, :3] = F32([[0, 0, 1], [0, 0, 1]])
        fpfh, counts, spfh = est(two, normals, None, k=2)
        hand = np.zeros(33, F32)
        hand[[5, 16, 27]] = 100                     # m = 2: incr = 100 / 1, one pair; the FPFH is the other point's SPFH, renormalised
        assert counts.tolist() == [2, 2] and np.array_equal(spfh, [hand, hand]) and np.array_equal(fpfh, [hand, hand])
        fpfh, counts, spfh = est(two, normals, None, radius=0.5)  # rows of the point alone: m = 1
        assert counts.tolist() == [1, 1] and not fpfh.any() and not spfh.any()
        fpfh, counts, _ = est(two, normals, cloud_of([[0, 0, 0], [9, 9, 9], [np.nan, 0, 0]]), radius=0.5)
        assert counts.tolist() == [1, 0, 0] and not fpfh[:2].any() and np.isnan(fpfh[2]).all()


def test_refusals():
    cloud, normals = cloud_of(np.eye(3)), random_normals(3, 0)
    for mode in (dict(), dict(k=1), dict(k=65), dict(k=-2), dict(k=3, radius=1.0), dict(radius=-1.0), dict(radius=float("nan")),
                 dict(radius=float("inf"))):
        with pytest.raises(R.Refused):
            R.estimate(cloud, normals, None, **mode)
    with pytest.raises(R.Refused):
        R.estimate(cloud, None, None, k=2)


def test_edge_constants_are_the_float32_cosines_and_sines():
    k = np.arange(1, 11)
    assert np.array_equal(R.EDGE_COS, np.cos(2 * np.pi * k / 11).astype(F32)) and np.array_equal(R.EDGE_SIN, np.sin(2 * np.pi * k / 11).astype(F32))


# ---- the golden fixture and the ABI --------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    assert g["cloud"].shape == (512, 4) and g["normals"].shape == (512, 4)
    for name, kw in (("k", dict(k=int(g["k"]))), ("r", dict(radius=float(g["radius"])))):
        assert same(R.estimate(g["cloud"], g["normals"], None, **kw), (g[f"{name}_fpfh"], g[f"{name}_counts"], g[f"{name}_spfh"])), name
    assert os.path.getsize(GOLDEN) <= 95783  # no larger than the largest fixture beside it


def test_new_symbol_is_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    assert " T icpgpu_fpfh_estimation\n" in names
    assert "int icpgpu_fpfh_estimation(" in header and "icpgpu_fpfh_estimation" in _lib.EXPORTS
    assert "#define ICPGPU_FPFH_BINS 33" in header and R.BINS == 33


def test_entry_point_refuses_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_fpfh_estimation(None, None, None, 0, 10, 0.0, None, None, None) == _lib.ERR_INVALID_ARG
