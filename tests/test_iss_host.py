"""The ISS keypoints' rules on the host (include/icpgpu.h, "ISS keypoints"): the NumPy restatement (tests/iss_restated.py) against the
literal point-by-point loop with fractions.Fraction sums, against answers known by hand (the clouds of tests/iss_cases.py), and against
the golden fixture; and the ABI of the three entry points, which needs no GPU."""
import os
import subprocess

import numpy as np
import pytest

import iss_cases as K
import iss_restated as R
import search_restated as S
from icpslam_amd import _lib

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rows_f", "iss_2k.npz")
CASES = {name: (cloud, args) for name, cloud, args in K.hand_cases()}


def run(name):
    cloud, args = CASES[name]
    return cloud, args, R.keypoints(cloud, *args)


# ---- the two restatements ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(1.5, 1.0, 0.975, 0.975, 5), (0.8, 1.6, 0.9, 0.6, 3), (2.5, 2.5, 10.0, 10.0, 0)])
def test_restatement_and_literal_loop_agree_on_a_scan(args):
    cloud = K.scan(600).copy()
    cloud[[7, 300], [1, 0]] = [np.nan, np.inf]
    cloud[50:54] = cloud[400:404]
    a, b = R.keypoints(cloud, *args), R.keypoints_literal(cloud, *args)
    assert R.same_bits(a, b) == []
    if args[4]:
        assert a["n_keypoints"] > 0 and (a["saliency"] > 0).sum() > a["n_keypoints"]   # some points are suppressed, some survive


@pytest.mark.parametrize("name", ["ties", "corner", "planar_lattice", "oblique_line", "two_groups", "on_the_radius"])
def test_restatement_and_literal_loop_agree_on_the_hand_clouds(name):
    cloud, args, got = run(name)
    assert R.same_bits(got, R.keypoints_literal(cloud, *args)) == []


def test_balls_are_the_radius_search_rows():
    cloud, args, got = run("nan_rows")
    start, _, _ = S.radius(cloud, None, args[0], 0)
    assert np.array_equal(got["n_salient"], np.diff(start))
    lit_start, _, _ = S.radius_literal(cloud, None, args[0], 0)
    assert np.array_equal(start, lit_start)


# ---- answers known by hand ---------------------------------------------------------------------------------------------------
def test_planar_lattice_has_no_keypoints():
    cloud, args, got = run("planar_lattice")
    assert (got["n_salient"] >= 4).all() and got["n_salient"].max() == 9
    assert (got["scatter6"][:, [2, 4, 5]] == 0).all() and (got["scatter6"][:, 0] > 0).all()
    assert (got["eigenvalues3"][:, 2] == 0).all() and (got["eigenvalues3"][:, 1] > 0).all()
    assert not got["saliency"].any() and got["n_keypoints"] == 0


def test_points_on_a_line_have_no_keypoints():
    cloud, args, got = run("line")
    assert (got["eigenvalues3"][:, 0] > 0).all() and not got["eigenvalues3"][:, 1:].any()      # e3 / e2 = 0 / 0: a NaN quotient fails
    assert not got["saliency"].any() and got["n_keypoints"] == 0
    _, _, oblique = run("oblique_line")
    e = oblique["eigenvalues3"]
    assert (np.abs(e[:, 1:]) <= 1e-14 * e[:, :1]).all()                                         # rank one up to the sweeps' rounding


def test_a_coincident_cloud_has_no_keypoints():
    cloud, args, got = run("coincident")
    assert (got["n_salient"] == 9).all() and not got["scatter6"].any() and not got["eigenvalues3"].any()
    assert not got["saliency"].any() and got["n_keypoints"] == 0


def test_the_corner_of_three_faces_is_the_keypoint():
    cloud, args, got = run("corner")
    assert cloud[0, :3].tolist() == [0, 0, 0]
    assert got["keypoint_index"].tolist() == [0] and np.flatnonzero(got["saliency"] > 0).tolist() == [0]
    assert got["eigenvalues3"][0].round(9).tolist() == [27.0, 12.0, 12.0] and got["n_salient"][0] == 16
    interior = np.flatnonzero(((cloud[:, :3] == 0).sum(axis=1) == 1) & (cloud[:, :3].max(axis=1) <= 3) &
                              (np.sort(cloud[:, :3], axis=1)[:, 1] >= 3))                         # the ball is a disc inside one face
    assert interior.size == 3
    e = got["eigenvalues3"][interior]
    assert (e[:, 2] == 0).all() and (e[:, 1] / e[:, 0] == 1.0).all() and args[2] < 1.0            # they fail gamma_21
    # without the gamma_21 test the edges' points would beat the corner
    loose = R.keypoints(cloud, args[0], args[1], 10.0, args[3], args[4])
    assert (loose["saliency"] > loose["saliency"][0]).any()


def test_exactly_tied_maxima_are_all_kept():
    cloud, args, got = run("ties")
    xyz = cloud[:, :3].astype(int)
    on_boundary = ((xyz == 0) | (xyz == 4)).sum(axis=1)                                          # 0 interior, 1 face, 2 edge, 3 corner
    assert got["saliency"][on_boundary == 0].tolist() == [2.0] * 27
    assert got["saliency"][on_boundary >= 1].tolist() == [1.0] * 98
    # a face's point has an interior neighbour (2 > 1); an edge's and a corner's neighbours all tie with it at 1
    assert got["keypoint_index"].tolist() == np.flatnonzero(on_boundary != 1).tolist() and got["n_keypoints"] == 27 + 36 + 8


def test_ball_sizes_on_both_sides_of_min_neighbors():
    cloud, args, got = run("two_groups")
    assert got["n_salient"].tolist() == [4] * 4 + [5] * 5 and args[4] == 5
    assert not got["scatter6"][:4].any() and not got["eigenvalues3"][:4].any() and not got["saliency"][:4].any()
    assert (got["scatter6"][4:, [0, 3, 5]] > 0).all() and (got["saliency"][4:] > 0).all()
    assert got["keypoint_index"].size >= 1 and (got["keypoint_index"] >= 4).all()
    with_four = R.keypoints(cloud, args[0], args[1], args[2], args[3], 4)
    assert (with_four["saliency"] > 0).all()


def test_a_point_on_the_radius_is_outside():
    cloud, args, got = run("on_the_radius")
    assert float(F32(cloud[1, 0]) * F32(cloud[1, 0])) == float(F32(args[0] * args[0]))          # d2 == r2 exactly
    assert got["n_salient"].tolist() == [1, 1, 2, 2]
    assert not got["scatter6"][:2].any() and (got["scatter6"][2:, 0] > 0).all()


def test_gamma_at_a_points_own_quotient():
    cloud = K.scan(257)
    base = R.keypoints(cloud, 1.5, 1.0, 10.0, 10.0, 5)
    i = int(np.argmax(base["saliency"]))
    e1, e2, e3 = base["eigenvalues3"][i]
    q21, q32 = F64(e2) / F64(e1), F64(e3) / F64(e2)
    assert 0 < q21 < 1 and 0 < q32 < 1 and base["saliency"][i] == e3
    for g21, g32, passes in ((q21, 10.0, False), (np.nextafter(q21, 2.0), 10.0, True), (10.0, q32, False), (10.0, np.nextafter(q32, 2.0), True)):
        got = R.keypoints(cloud, 1.5, 1.0, float(g21), float(g32), 5)
        assert (got["saliency"][i] == e3) == passes and (got["saliency"][i] == 0) == (not passes)
        assert got["eigenvalues3"].tobytes() == base["eigenvalues3"].tobytes()                   # the gammas touch the saliency alone


def test_selection_rule_on_matrices_of_its_own():
    eig = np.array([[3.0, 2.0, -1e-20], [3.0, 2.0, 1.0], [3.0, 2.0, 0.0], [np.inf, 2.0, 1.0], [3.0, np.nan, 1.0], [0.0, 0.0, 0.0],
                    [3.0, 2.0, -0.0]])
    got = R.select(eig, np.full(len(eig), 9), 0.975, 0.975, 5)
    assert got.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and not np.signbit(got[0])
    assert R.select(eig[1:2], [4], 0.975, 0.975, 5).tolist() == [0.0]                            # too few neighbours
    assert R.select(eig[1:2], [9], 0.0, 0.975, 5).tolist() == [0.0] and R.select(eig[1:2], [9], 1.0, 0.5, 5).tolist() == [0.0]
    assert R.sort3([[1.0, 3.0, 2.0], [2.0, 2.0, 5.0], [-1.0, -3.0, 0.0]]).tolist() == [[3.0, 2.0, 1.0], [5.0, 2.0, 2.0], [0.0, -1.0, -3.0]]


def test_nan_rows_are_in_no_ball_and_have_none():
    cloud, args, got = run("nan_rows")
    bad = np.flatnonzero(~S.finite_mask(cloud))
    assert bad.tolist() == [0, 64, 100, 200]
    assert not got["n_salient"][bad].any() and not got["scatter6"][bad].any() and not got["eigenvalues3"][bad].any() and not got["saliency"][bad].any()
    assert not np.isin(got["keypoint_index"], bad).any() and got["n_keypoints"] > 0
    clean = np.delete(cloud, bad, axis=0)                                                        # the same answer as without those rows
    want = R.keypoints(clean, *args)
    keep = np.delete(np.arange(len(cloud)), bad)
    assert np.array_equal(keep[want["keypoint_index"]], got["keypoint_index"])
    assert got["scatter6"][keep].tobytes() == want["scatter6"].tobytes()


def test_non_max_radius_smaller_and_larger_than_the_salient_one():
    _, _, small = run("non_max_smaller")
    _, _, large = run("non_max_larger")
    assert small["n_keypoints"] > large["n_keypoints"] > 0
    cloud, args = CASES["non_max_larger"]
    wider = R.keypoints(cloud, args[0], 2 * args[1], *args[2:])
    assert np.isin(wider["keypoint_index"], large["keypoint_index"]).all() and wider["n_keypoints"] < large["n_keypoints"]


def test_min_neighbors_of_zero_and_one_are_the_same_for_finite_points():
    cloud = K.scan(257)
    a, b = R.keypoints(cloud, 1.0, 1.0, 0.975, 0.975, 0), R.keypoints(cloud, 1.0, 1.0, 0.975, 0.975, 1)
    assert R.same_bits(a, b) == []                                                               # every finite point is in its own ball


def test_empty_and_all_nan_clouds_and_refusals():
    for cloud in (np.empty((0, 4), F32), np.full((7, 4), np.nan, F32)):
        got = R.keypoints(cloud, 1.0, 1.0)
        assert got["n_keypoints"] == 0 and not got["n_salient"].any() and not got["saliency"].any() and got["keypoints"].shape == (0, 4)
    for bad in ((0.0, 1.0, 0.9, 0.9, 5), (1.0, -1.0, 0.9, 0.9, 5), (float("nan"), 1.0, 0.9, 0.9, 5), (1.0, float("inf"), 0.9, 0.9, 5),
                (1.0, 1.0, float("nan"), 0.9, 5), (1.0, 1.0, 0.9, float("inf"), 5), (1.0, 1.0, 0.9, 0.9, -1)):
        with pytest.raises(R.Refused):
            R.keypoints(K.scan(63), *bad)


# ---- the golden fixture and the ABI ------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    got = R.keypoints(g["cloud"], float(g["salient_radius"]), float(g["non_max_radius"]), float(g["gamma_21"]), float(g["gamma_32"]),
                      int(g["min_neighbors"]))
    assert R.same_bits(got, {"n_keypoints": int(g["n_keypoints"]), **{f: g[f] for f in R.FIELDS}}) == []
    assert int(g["n_keypoints"]) > 10 and (g["n_salient"] < int(g["min_neighbors"])).any()
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "rows_f", "gicp_1k5.npz"))   # the largest so far


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in ("icpgpu_iss_keypoints", "icpgpu_iss_fetch", "icpgpu_iss_stats"):
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_iss_keypoints(None, 1.0, 1.0, 0.975, 0.975, 5, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_iss_fetch(None, 0, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_iss_stats(None, None) == _lib.ERR_INVALID_ARG
