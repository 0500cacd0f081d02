"""The boundary estimation's and ISS border estimation's rules on the host (include/icpgpu.h, "boundary estimation" and "ISS
keypoints"): the NumPy restatements (tests/boundary_restated.py, tests/iss_border_restated.py) against the literal loop whose sector
test runs on fractions.Fraction, against PCL's own atan2 / sort / largest-gap rule in float64, against answers known by hand (the
clouds of tests/boundary_cases.py) and against the golden fixtures; and the ABI of the three entry points, which needs no GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import boundary_cases as C
import boundary_restated as B
import iss_border_restated as IB
import iss_cases as K
import iss_restated as R
import normals_restated as N
import search_restated as S
from icpslam_amd import _lib

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rows_f")
CASES = {c[0]: c[1:] for c in C.hand_cases()}
THRESHOLDS = (0.1, 1.0, C.HALF_PI, 2.5, 3.0, math.pi)


def run(name):
    cloud, queries, normals, k, radius, angle = CASES[name]
    return cloud, B.estimate(cloud, queries, normals, k, radius, angle)


# ---- the two restatements ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, radius, angle", [(30, 0.0, C.HALF_PI), (12, 0.0, math.pi), (0, 3.0, 2.5), (0, 1.5, 0.1), (3, 0.0, C.ABOVE_HALF_PI)])
def test_restatement_and_literal_loop_agree_on_a_scan(k, radius, angle):
    cloud = K.scan(600).copy()
    cloud[[7, 300], [1, 0]] = [np.nan, np.inf]
    cloud[50:54] = cloud[400:404]
    normals = N.estimate(cloud, None, 12, 0.0)[0].copy()
    normals[20, :3] = 0.0
    normals[21, 2] = np.nan
    a, b = B.estimate(cloud, None, normals, k, radius, angle), B.estimate_literal(cloud, None, normals, k, radius, angle)
    assert B.same_bits(a, b) == []
    assert a["boundary"][[7, 300, 20, 21]].tolist() == [0, 0, 0, 0] and a["n_directions"][[20, 21]].tolist() == [0, 0]
    if k != 3 and angle > 0.1:
        assert 20 < a["boundary"].sum() < 580                                   # both answers occur


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_and_literal_loop_agree_on_the_hand_clouds(name):
    cloud, queries, normals, k, radius, angle = CASES[name]
    assert B.same_bits(B.estimate(cloud, queries, normals, k, radius, angle), B.estimate_literal(cloud, queries, normals, k, radius, angle)) == []


def test_restatement_and_literal_loop_agree_with_queries_off_the_cloud():
    cloud = K.scan(600)
    queries = cloud[::7].copy()
    queries[:, :3] += F32(0.05)
    normals = N.estimate(cloud, queries, 12, 0.0)[0]
    for k, radius in ((20, 0.0), (0, 2.0)):
        a, b = B.estimate(cloud, queries, normals, k, radius, 2.0), B.estimate_literal(cloud, queries, normals, k, radius, 2.0)
        assert B.same_bits(a, b) == [] and 0 < a["boundary"].sum() < len(queries)


# ---- PCL's own rule ----------------------------------------------------------------------------------------------------------
def pcl_disagreements(directions, angle):
    """(compared, left out, disagreeing) over sets of directions (x, y float32 arrays)."""
    c = math.cos(angle)
    compared = left_out = wrong = 0
    for x, y in directions:
        gap, pcl = B.pcl_rule(x, y, angle)
        if abs(gap - angle) <= 1e-6:
            left_out += 1
            continue
        compared += 1
        wrong += bool(B.survivors(x, y, c).any()) != pcl
    return compared, left_out, wrong


@pytest.mark.parametrize("angle", THRESHOLDS)
def test_the_rule_is_pcls_largest_gap_rule_on_random_direction_sets(angle):
    r = np.random.default_rng(int(angle * 1000))
    sets = []
    for _ in range(4000):
        m = int(r.integers(1, 40))
        a = r.uniform(-math.pi, math.pi, m) if r.random() < 0.5 else r.uniform(0, r.uniform(0.2, 2 * math.pi), m)
        s = 10.0 ** r.uniform(-3, 2, m)
        sets.append(((s * np.cos(a)).astype(F32), (s * np.sin(a)).astype(F32)))
    compared, left_out, wrong = pcl_disagreements(sets, angle)
    assert wrong == 0 and left_out == 0 and compared == 4000


@pytest.mark.parametrize("k, radius", [(30, 0.0), (0, 1.5)])
def test_the_rule_is_pcls_largest_gap_rule_on_a_scan(k, radius):
    cloud = K.scan(2000)
    normals = C.scan_normals(2000)
    start, idx = N.rows(cloud, None, k, radius)
    u, v = B.frame(normals)
    sets = []
    for q in range(len(cloud)):
        row = idx[start[q]:start[q + 1]]
        x, y, keep = B.directions_of_row(cloud[q, :3], u[q], v[q], cloud[row, :3])
        if len(row) >= 3 and keep.any():
            sets.append((x[keep], y[keep]))
    assert len(sets) > 1900
    for angle in THRESHOLDS:
        compared, left_out, wrong = pcl_disagreements(sets, angle)
        assert wrong == 0 and left_out <= 0.01 * len(sets), (angle, compared, left_out, wrong)


# ---- answers known by hand ---------------------------------------------------------------------------------------------------
def test_planar_lattice_under_an_eight_neighbour_radius():
    cloud, got = run("lattice_8")
    xy = cloud[:, :2].astype(int)
    on_rim = ((xy == 0) | (xy == 6)).sum(axis=1)                                  # 0 interior, 1 rim, 2 corner
    assert got["boundary"].tolist() == (on_rim > 0).astype(int).tolist()
    assert got["n_neighbours"][on_rim == 0].tolist() == [9] * 25 and got["n_directions"][on_rim == 0].tolist() == [8] * 25
    assert set(got["n_directions"][on_rim == 1]) == {5} and set(got["n_directions"][on_rim == 2]) == {3}
    assert (got["witness"][on_rim == 0] == -1).all() and (got["witness"][on_rim > 0] >= 0).all()


def test_a_gap_of_exactly_half_pi_on_both_sides_of_the_threshold():
    assert math.cos(C.HALF_PI) > 0 > math.cos(C.ABOVE_HALF_PI)
    cloud, at = run("lattice_4_at")
    _, above = run("lattice_4_above")
    xy = cloud[:, :2].astype(int)
    interior = ((xy > 0) & (xy < 6)).all(axis=1)
    assert at["n_directions"][interior].tolist() == [4] * 25
    assert at["boundary"].all()                                                   # DEVIATION: PCL's float32 comparison says 0 inside
    assert not above["boundary"][interior].any() and above["boundary"][~interior].all()


def test_two_opposite_directions():
    _, at_pi = run("opposite_pi")
    _, at_3 = run("opposite_3")
    assert at_pi["n_directions"].tolist() == [2, 2, 2]
    assert at_pi["boundary"][0] == 0 and at_pi["witness"][0] == -1               # two gaps of exactly pi
    assert at_3["boundary"][0] == 1 and at_3["witness"][0] == 1                  # both survive: the lower index
    assert at_pi["boundary"][1:].tolist() == [1, 1]                              # seen from an end, both neighbours lie one way


def test_a_single_direction_is_a_boundary():
    _, got = run("single_direction")
    assert got["n_neighbours"].tolist() == [3, 3, 3] and got["n_directions"].tolist() == [1, 1, 2]
    assert got["boundary"].tolist() == [1, 1, 1] and got["witness"][:2].tolist() == [2, 2]


def test_rows_of_one_and_two_entries_are_no_boundary():
    _, got = run("rows_of_1_and_2")
    assert got["n_neighbours"].tolist() == [2, 2, 1]
    assert not got["boundary"].any() and (got["witness"] == -1).all() and not got["n_directions"].any()


def test_neighbours_along_the_normal_and_coincident_points_are_no_directions():
    for name in ("along_the_normal", "coincident"):
        _, got = run(name)
        assert (got["n_neighbours"] >= 3).all() and not got["n_directions"].any() and not got["boundary"].any() and (got["witness"] == -1).all()


def test_duplicated_directions_do_not_fill_each_others_sectors():
    _, got = run("duplicated_directions")
    # seen from point 0: +x three times (indices 1, 2, 4) and -x once (3): every +x has -x in its sector at pi, and -x has the +x's
    assert got["n_directions"][0] == 4 and got["boundary"][0] == 0
    cloud, queries, normals, k, radius, _ = CASES["duplicated_directions"]
    tight = B.estimate(cloud, queries, normals, k, radius, 3.0)
    assert tight["boundary"][0] == 1 and tight["witness"][0] == 1                # all four survive below pi: the lowest index


def test_zero_and_nan_normals_give_no_directions():
    for name in ("zero_normal", "nan_normal"):
        _, got = run(name)
        assert (got["n_neighbours"] >= 4).all() and not got["n_directions"].any() and not got["boundary"].any()


def test_both_branches_of_the_frame():
    n = np.array([[0, 0, 1, 0], [1e-6, -1e-6, 1, 0], [1, 0, 0, 0], [1 / 3, 2 / 3, 2 / 3, 0], [0, 1, 0, 0], [2e-5, 0, 1, 0]], F32)
    u, v = B.frame(n)
    assert v[0].tolist() == [0, -1, 0] and u[0].tolist() == [1, 0, 0]              # near: v in the y-z plane
    assert v[1, 0] == 0 and v[5, 2] == 0 and v[2].tolist() == [0, 1, 0] and v[3, 2] == 0
    for i in range(len(n)):
        m = np.stack([u[i], v[i], n[i, :3]]).astype(F64)
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-6) and np.linalg.det(m) < 0   # orthonormal; u = n x v turns from v to u about n
    for name in ("frame_far_branch", "frame_tilted"):
        cloud, got = run(name)
        want = [int(min(i, j) == 0 or max(i, j) == 4) for i in range(5) for j in range(5)]
        assert got["boundary"].tolist() == want and got["n_directions"].reshape(5, 5)[1:4, 1:4].tolist() == [[8] * 3] * 3


def test_the_witness_is_the_lowest_index_among_the_survivors():
    cloud, got = run("witness_ties")
    # the origin is row 0; three directions 120 degrees apart all survive pi / 2
    assert got["n_directions"][0] == 3 and got["boundary"][0] == 1 and got["witness"][0] == 1
    _, full = run("ring_full")
    _, half = run("ring_half")
    assert full["boundary"][0] == 0 and full["n_directions"][0] == 12
    # with n = +z the frame is u = +x, v = -y: sectors open clockwise seen from +z, and the arc's FIRST point looks into the empty half
    assert half["boundary"][0] == 1 and half["witness"][0] == 1


def test_refusals():
    cloud, normals = K.scan(63), C.normals_of(63)
    for angle in (0.0, -1.0, math.nextafter(math.pi, 4.0), float("nan"), float("inf")):
        with pytest.raises(B.Refused):
            B.estimate(cloud, None, normals, 5, 0.0, angle)
    for k, radius in ((0, 0.0), (5, 1.0), (65, 0.0), (-1, 0.0), (0, -1.0), (0, float("nan"))):
        with pytest.raises(B.Refused):
            B.estimate(cloud, None, normals, k, radius)


# ---- ISS with border estimation ----------------------------------------------------------------------------------------------
def test_border_radius_zero_is_the_existing_restatement():
    cloud = K.scan(600)
    args = (1.5, 1.0, 0.975, 0.975, 5)
    got, want = IB.keypoints_border(cloud, *args, border_radius=0.0, angle_threshold=float("nan")), R.keypoints(cloud, *args)
    assert R.same_bits(got, want) == [] and not got["edge"].any() and not got["border"].any()


def test_the_corner_of_three_faces_and_its_rims():
    """The faces' outer rims (a coordinate at 6) are the scan's edge; the cube's own edges and its corner are folds, not rims.  The
    literal loop settles which points are edge points; the corner, 6 away from the rims, stays a keypoint while the border radius is
    below that distance and not above it."""
    cloud = K.three_faces(7)
    xyz = cloud[:, :3].astype(int)
    normals = N.estimate(cloud, None, 0, 1.5)[0]
    def literal_edge(radius):
        lit = B.estimate_literal(cloud, None, normals, 0, radius, C.HALF_PI)
        return lit["boundary"].astype(bool) & (lit["n_neighbours"] >= K.CORNER_ARGS[4])     # the min_neighbors rule

    rim = B.estimate_literal(cloud, None, normals, 0, 1.5, C.HALF_PI)["boundary"].astype(bool)
    on_rim = (xyz == 6).any(axis=1)
    assert rim[on_rim].all() and not rim[(xyz <= 4).all(axis=1)].any() and not rim[0]
    edge = literal_edge(1.5)
    assert edge.sum() == rim.sum() - 3                                            # a face's outer corner has a ball of four points
    near = IB.keypoints_border(cloud, *K.CORNER_ARGS, border_radius=1.5, normal_radius=1.5)
    assert np.array_equal(near["edge"].astype(bool), edge)
    assert near["keypoint_index"].tolist() == [0] and near["border"][on_rim].all() and not near["border"][0]
    d_rim = np.sqrt(((cloud[edge, :3] - cloud[0, :3]) ** 2).sum(axis=1)).min()
    assert 4.9 < d_rim <= 6.0
    for radius, kept in ((float(d_rim) - 0.01, True), (float(d_rim) + 0.01, False)):
        got = IB.keypoints_border(cloud, *K.CORNER_ARGS, border_radius=radius, normals=normals)
        assert np.array_equal(got["edge"].astype(bool), literal_edge(radius))
        assert (got["keypoint_index"].tolist() == [0]) == kept and bool(got["border"][0]) == (not kept)
        if not kept:
            assert got["n_keypoints"] == 0 and not got["scatter6"][0].any() and got["n_salient"][0] == 16


def test_border_points_keep_their_ball_size_and_nothing_else():
    cloud = K.scan(600)
    got = IB.keypoints_border(cloud, 1.5, 1.0, 0.975, 0.975, 5, border_radius=0.7, angle_threshold=math.pi, normal_radius=1.5)
    plain = R.keypoints(cloud, 1.5, 1.0, 0.975, 0.975, 5)
    on = got["border"].astype(bool)
    assert 50 < on.sum() < 550 and (got["edge"] <= got["border"]).all()
    assert np.array_equal(got["n_salient"], plain["n_salient"])
    assert not got["scatter6"][on].any() and not got["eigenvalues3"][on].any() and not got["saliency"][on].any()
    assert got["scatter6"][~on].tobytes() == plain["scatter6"][~on].tobytes() and got["saliency"][~on].tobytes() == plain["saliency"][~on].tobytes()
    assert not np.isin(got["keypoint_index"], np.flatnonzero(on)).any() and 0 < got["n_keypoints"]
    for bad in (dict(border_radius=-1.0), dict(border_radius=float("nan")), dict(border_radius=1.0, angle_threshold=0.0),
                dict(border_radius=1.0, angle_threshold=4.0), dict(border_radius=1.0), dict(border_radius=1.0, normal_radius=-1.0)):
        with pytest.raises(IB.Refused):
            IB.keypoints_border(cloud, 1.5, 1.0, 0.975, 0.975, 5, **bad)


# ---- the golden fixtures and the ABI -----------------------------------------------------------------------------------------
def test_restatements_reproduce_the_golden_fixtures():
    g = np.load(os.path.join(GOLDEN, "boundary_2k.npz"))
    a = B.estimate(g["cloud"], None, g["normals"], int(g["k"]), 0.0, float(g["k_angle"]))
    b = B.estimate(g["cloud"], None, g["normals"], 0, float(g["radius"]), float(g["radius_angle"]))
    assert B.same_bits(a, {f: g[f"k_{f}"] for f in B.FIELDS}) == [] and B.same_bits(b, {f: g[f"radius_{f}"] for f in B.FIELDS}) == []
    assert 100 < g["k_boundary"].sum() < 1900 and 100 < g["radius_boundary"].sum() < 1900
    s = np.load(os.path.join(GOLDEN, "iss_border_2k.npz"))
    got = IB.keypoints_border(s["cloud"], float(s["salient_radius"]), float(s["non_max_radius"]), float(s["gamma_21"]), float(s["gamma_32"]),
                              int(s["min_neighbors"]), float(s["border_radius"]), float(s["angle_threshold"]), s["normals"])
    assert IB.same_bits(got, {"n_keypoints": int(s["n_keypoints"]), **{f: s[f] for f in IB.FIELDS}}) == []
    assert int(s["n_keypoints"]) > 3 and 100 < s["border"].sum() < 1900
    for name in ("boundary_2k.npz", "iss_border_2k.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 128 * 1024


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in ("icpgpu_boundary_estimation", "icpgpu_iss_keypoints_border", "icpgpu_iss_fetch_border"):
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_boundary_estimation(None, None, None, 0, 5, 0.0, 1.0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_iss_keypoints_border(None, 1.0, 1.0, 0.975, 0.975, 5, 0.5, 1.0, None, 0.5, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_iss_fetch_border(None, None, None) == _lib.ERR_INVALID_ARG
