"""Region growing's rules on the host (include/icpgpu.h, "region growing"): the vectorised restatement (tests/region_restated.py)
against the literal loop of the same rule, bit for bit; the relation to PCL 1.8's seed-queue loop transcribed -- the containment that
holds exactly, and the two agreement fractions on scans; answers known by hand (tests/region_cases.py); the golden fixture; and the
ABI of the two entry points, which needs no GPU."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import normals_restated as N
import region_cases as RC
import region_restated as R
import search_restated as S
from icpslam_amd import _lib, synth

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rows_f", "region_2k.npz")
INT_MAX = 2**31 - 1


def assert_same(got, want, what=""):
    for name, g, w in zip(R.NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


def regions(case):
    """(the emitted regions as index lists, labels, region, kind, anchor) of a hand case."""
    start, indices, labels, region, kind, anchor = R.grow(*case)
    return [indices[a:b].tolist() for a, b in zip(start[:-1], start[1:])], labels, region, kind, anchor


@functools.lru_cache(maxsize=None)
def scan_case(seed: int, n: int = 3000, k: int = 30):
    """synth.scan(make_scene(seed), pose z = 1.5, n, seed), its float32 normals (tests/normals_restated.py, the same k) and rows."""
    pose = np.eye(4)
    pose[2, 3] = 1.5
    cloud = synth.scan(synth.make_scene(seed), pose, n, seed)
    normals = N.estimate(cloud, None, k=k)[0]
    rows = R.rows_of(cloud, k)
    for a in (cloud, normals) + tuple(rows):
        a.setflags(write=False)
    return cloud, normals, rows


# ---- the rule, twice --------------------------------------------------------------------------------------------------------
def test_vectorised_rule_and_literal_loop_agree_on_a_scan():
    cloud, normals, _ = scan_case(1, 600, 12)
    normals = normals.copy()
    normals[[5, 77], [1, 3]] = [np.nan, np.inf]
    cloud = cloud.copy()
    cloud[300, 2] = np.nan
    kinds = set()                      # (600 points lie along the sensor's rings: the median curvature at k = 12 is 1.6e-9)
    for k, degrees, threshold, lo, hi in ((12, 30, 1e-8, 1, INT_MAX), (5, 5, 1.0, 2, 40), (30, 10, 1e-9, 3, 3)):
        got = R.grow(cloud, normals, k, RC.cos_of(degrees), threshold, lo, hi)
        assert_same(got, R.grow_literal(cloud, normals, k, RC.cos_of(degrees), threshold, lo, hi), f"k {k}")
        kinds |= set(np.unique(got[4]).tolist())
        # the arrays' own consistency and the order rule
        start, indices, labels, region, kind, anchor = got
        sizes = np.diff(start)
        names = region[indices[start[:-1]]]
        assert (sizes[:-1] >= sizes[1:]).all() and ((sizes[:-1] > sizes[1:]) | (names[:-1] < names[1:])).all()
        assert ((sizes >= lo) & (sizes <= hi)).all() and (labels >= 0).sum() == indices.size
        for r, (a, b) in enumerate(zip(start[:-1], start[1:])):
            assert (np.diff(indices[a:b]) > 0).all() and (labels[indices[a:b]] == r).all() and (region[indices[a:b]] == names[r]).all()
        assert ((kind == -1) == (region == -1)).all() and ((kind == 1) == (anchor >= 0)).all()
        assert (kind[anchor[kind == 1]] == 2).all() and (region[anchor[kind == 1]] == region[kind == 1]).all()
        assert (region[kind == 0] == np.flatnonzero(kind == 0)).all() and (region[kind == 2] <= np.flatnonzero(kind == 2)).all()
    assert kinds == {-1, 0, 1, 2}


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_vectorised_rule_and_literal_loop_agree_on_every_hand_cloud(name):
    assert_same(R.grow(*RC.CASES[name]), R.grow_literal(*RC.CASES[name]), name)


def test_smooth_is_symmetric_bit_for_bit():
    rng = np.random.default_rng(12)
    a = rng.normal(size=(200000, 4)).astype(F32)
    a[:, :3] /= np.linalg.norm(a[:, :3], axis=1, keepdims=True).astype(F32)
    i, j = rng.integers(0, len(a), 400000), rng.integers(0, len(a), 400000)
    dot = lambda p, q: (a[p, 0] * a[q, 0] + a[p, 1] * a[q, 1]) + a[p, 2] * a[q, 2]  # noqa: E731
    assert np.array_equal(dot(i, j).view(np.uint32), dot(j, i).view(np.uint32))


# ---- PCL's loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pcl_regions_from_core_seeds_keep_their_cores_in_one_region(seed):
    """The relation that holds exactly: PCL's propagation edges between cores are edges of the core graph."""
    cloud, normals, rows = scan_case(seed)
    cos = R.smoothness_cos(math.radians(30.0))
    region, kind, _ = R.partition(cloud, normals, 30, cos, 0.05, rows)
    _, seeds, grown = R.pcl_literal(cloud, normals, 30, cos, 0.05, rows=rows)
    assert sorted(p for m in grown for p in m) == np.flatnonzero(kind >= 0).tolist()      # PCL labels every participant once
    checked = 0
    for seed_point, members in zip(seeds, grown):
        if kind[seed_point] != 2:
            continue
        cores = [p for p in members if kind[p] == 2]
        assert len(set(region[cores].tolist())) == 1, (seed_point, len(members))
        checked += len(cores) > 1
    assert checked >= 5


# measured with the project's float32 normals (normals_restated.estimate, k = 30); DESIGN.md section 3 has the same figures
MEASURED = {1: (0.9920, 0.9863), 2: (0.9944, 0.9495), 3: (0.9822, 0.9718)}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_agreement_with_pcl_at_a_minimum_size_of_50(seed):
    """Forward: of the points in PCL regions of 50 or more points, the fraction in their region's majority region under the rule.
    Backward: the same with the roles swapped.  Conditions: forward >= 0.95, backward >= 0.90."""
    cloud, normals, rows = scan_case(seed)
    cos = R.smoothness_cos(math.radians(30.0))
    region, _, _ = R.partition(cloud, normals, 30, cos, 0.05, rows)
    _, _, grown = R.pcl_literal(cloud, normals, 30, cos, 0.05, rows=rows)
    pcl_label = np.full(len(cloud), -1, np.int64)
    for r, members in enumerate(grown):
        pcl_label[members] = r
    ours = [np.flatnonzero(region == name).tolist() for name in np.unique(region[region >= 0])]
    forward, backward = R.agreement(grown, region), R.agreement(ours, pcl_label)
    print(f"seed {seed}: forward {forward:.4f} backward {backward:.4f}")
    assert forward >= 0.95 and backward >= 0.90
    assert (round(forward, 4), round(backward, 4)) == MEASURED[seed]
    assert abs(sum(len(m) >= 50 for m in grown) - sum(len(m) >= 50 for m in ours)) <= 2


# ---- answers known by hand --------------------------------------------------------------------------------------------------
def test_two_planes_are_two_regions_and_the_crease_borders_the_nearer():
    got, labels, region, kind, anchor = regions(RC.CASES["two_planes"])
    crease = np.arange(180, 190)
    assert got == [sorted(list(range(90)) + crease.tolist()), list(range(90, 180))]
    assert (kind[:180] == 2).all() and (kind[crease] == 1).all() and (region[crease] == 0).all()
    assert anchor[crease].tolist() == [9 * x for x in range(10)]                     # A's edge point beside it, 0.9 away (B's: 1.0)
    assert R.pcl_literal(*RC.CASES["two_planes"])[0][0][0] == 0                      # (PCL seeds the lowest index of curvature 0 first)


def test_crease_point_between_two_cores_tie_and_one_ulp():
    c = RC.CASES["crease_tie"]
    assert S.d2_rows(c.cloud[2:3, :3], c.cloud[:2, :3])[0].tolist() == [1.0, 1.0]
    got, _, region, kind, anchor = regions(c)
    assert got == [[0, 2], [1]] and kind.tolist() == [2, 2, 1] and anchor.tolist() == [-1, -1, 0]   # a tie: the lower index
    c = RC.CASES["crease_one_ulp"]
    d2 = S.d2_rows(c.cloud[2:3, :3], c.cloud[:2, :3])[0]
    assert int(d2[0:1].view(np.uint32)[0]) - int(d2[1:2].view(np.uint32)[0]) == 1
    got, _, region, kind, anchor = regions(c)
    assert got == [[1, 2], [0]] and anchor.tolist() == [-1, -1, 1] and region.tolist() == [0, 1, 1]  # one ulp: the nearer
    assert regions(RC.CASES["crease_k_above_n"])[0] == [[0, 2], [1]]


def test_dot_exactly_on_the_threshold():
    c = RC.CASES["dot_on_threshold"]
    n = c.normals
    assert (n[0, 0] * n[1, 0] + n[0, 1] * n[1, 1]) + n[0, 2] * n[1, 2] == F32(0.5) and c.cos == F32(0.5)
    assert regions(c)[0] == [[0, 1]]
    assert regions(RC.CASES["dot_above_threshold"])[0] == [[0], [1]]


def test_curvature_exactly_on_the_threshold_is_core():
    c = RC.CASES["curvature_on_threshold"]
    assert c.normals[0, 3] == c.threshold and c.normals[2, 3] > c.threshold
    got, _, _, kind, anchor = regions(c)
    assert got == [[0, 1, 2]] and kind.tolist() == [2, 2, 1] and anchor.tolist() == [-1, -1, 1]


def test_antiparallel_normals_join():
    assert regions(RC.CASES["antiparallel"])[0] == [[0, 1]]


def test_far_point_that_lists_a_plane_and_is_listed_by_none():
    c = RC.CASES["far_noncore"]
    idx = R.rows_of(c.cloud, c.k)[0]
    assert (idx[25, 1:] < 25).all() and not (idx[:25] == 25).any()
    got, _, region, kind, _ = regions(c)
    assert got == [list(range(25)), [25]] and kind[25] == 0 and region[25] == 25      # not core: single
    c = RC.CASES["far_core"]
    got, _, region, kind, _ = regions(c)
    assert got == [list(range(26))] and kind[25] == 2 and region[25] == 0             # core: it joins through its own row
    assert [sorted(m) for m in R.pcl_literal(*c)[0]] == [list(range(25)), [25]]                            # ... and PCL keeps it apart


def test_a_nan_normal_between_two_halves_does_not_bridge():
    assert regions(RC.CASES["chain"])[0] == [list(range(7))]
    got, labels, region, kind, anchor = regions(RC.CASES["nan_normal"])
    assert got == [[0, 1, 2], [4, 5, 6]]
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and region.tolist() == [0, 0, 0, -1, 4, 4, 4] and kind[3] == -1 and anchor[3] == -1
    assert R.pcl_literal(*RC.CASES["nan_normal"])[0] == [[0, 1, 2], [4, 5, 6]]


def test_duplicated_points():
    c = RC.CASES["duplicates"]
    idx, d2, _ = R.rows_of(c.cloud, c.k)
    assert idx[37, :3].tolist() == [5, 21, 37] and not d2[37, :3].any()                # duplicates in index order, itself last
    got, _, region, kind, anchor = regions(c)
    assert got == [list(range(48))] and (kind[32:] == 1).all() and anchor[32:].tolist() == list(range(16))


def test_k_of_one_leaves_every_participant_alone():
    got, _, region, kind, _ = regions(RC.CASES["two_planes_k1"])
    assert got == [[i] for i in range(190)] and (region == np.arange(190)).all() and (kind[180:] == 0).all()


def test_cylinder_patch_is_one_region_at_30_degrees_and_columns_at_1():
    assert regions(RC.CASES["cylinder_30"])[0] == [list(range(248))]
    got, labels, region, _, _ = regions(RC.CASES["cylinder_1"])
    assert got == [list(range(8 * c, 8 * c + 8)) for c in range(31)]                   # 31 tied sizes: by the lowest name
    assert labels.tolist() == [c for c in range(31) for _ in range(8)]


def test_without_the_curvature_test_and_with_a_cosine_of_zero_or_less():
    got, _, _, kind, _ = regions(RC.CASES["two_planes_no_curvature_test"])
    assert got == [list(range(190))] and (kind == 2).all()                              # the crease, now core, joins both planes
    for name in ("two_planes_cos_zero", "two_planes_cos_negative"):
        got, _, _, kind, _ = regions(RC.CASES[name])
        assert got == [list(range(190))] and (kind[180:] == 1).all()                    # every listed pair joins: dot = 0 too


def test_the_size_window_and_max_below_min():
    got, labels, region, _, _ = regions(RC.CASES["two_planes_window"])
    assert got == [sorted(list(range(90)) + list(range(180, 190)))] and (labels[90:180] == -1).all() and (region[90:180] == 90).all()
    assert len(regions(RC.CASES["cylinder_1_window"])[0]) == 31
    for name in ("cylinder_1_above", "cylinder_1_max_below_min"):
        start, indices, labels, region, _, _ = R.grow(*RC.CASES[name])
        assert start.tolist() == [0] and indices.size == 0 and (labels == -1).all() and (region >= 0).all()
    c = RC.CASES["cylinder_1"]
    for lo, hi in ((1, 0), (0, -1), (INT_MAX, -INT_MAX - 1)):
        assert R.grow(*c._replace(lo=lo, hi=hi))[0].tolist() == [0]
    assert R.grow(*c._replace(lo=-5))[1].size == 248                                    # every value of the two ints is accepted


def test_shapes_built_for_the_device():
    c, order = RC.strip(300, 22)
    assert regions(c)[0] == [list(range(300))]
    got = regions(RC.interleaved_strips(100))[0]
    assert got == [list(range(0, 200, 2)), list(range(1, 200, 2))]
    c, _ = RC.tied_regions(65, 165)
    start, indices, _, _, kind, _ = R.grow(*c)
    assert np.array_equal(start, 2 * np.arange(66)) and (np.diff(indices[0::2]) > 0).all() and (kind == 0).sum() == 40


def test_empty_clouds_no_participant_and_refusals():
    cos = RC.cos_of(30)
    for cloud, normals in ((np.empty((0, 4), F32), np.empty((0, 4), F32)), (np.full((7, 4), np.nan, F32), np.zeros((7, 4), F32)),
                           (np.ones((7, 4), F32), np.full((7, 4), np.nan, F32))):
        start, indices, labels, region, kind, anchor = R.grow(cloud, normals, 5, cos)
        assert start.tolist() == [0] and indices.size == 0
        assert labels.tolist() == region.tolist() == kind.tolist() == anchor.tolist() == [-1] * len(cloud)
    assert R.grow(np.empty((0, 4), F32), None, 5, cos)[0].tolist() == [0]
    c = RC.CASES["chain"]
    for bad in (dict(k=0), dict(k=65), dict(cos=float("nan")), dict(threshold=float("nan")), dict(normals=None)):
        with pytest.raises(R.Refused):
            R.grow(*c._replace(**bad))
    assert R.grow(*c._replace(cos=float("inf")))[0].tolist() == list(range(8))          # nothing is smooth: legal


# ---- the golden fixture and the ABI -----------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    got = R.grow(g["cloud"], g["normals"], int(g["k"]), g["smoothness_cos"], g["curvature_threshold"], int(g["min_size"]), int(g["max_size"]))
    for name, a in zip(R.NAMES, got):
        assert a.dtype == g[name].dtype and a.tobytes() == g[name].tobytes(), name
    assert set(np.unique(g["kind"]).tolist()) == {-1, 0, 1, 2}
    assert os.path.getsize(GOLDEN) <= 2 * os.path.getsize(os.path.join(HERE, "golden", "rows_f", "normals_2k.npz"))


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in ("icpgpu_region_growing", "icpgpu_region_fetch"):
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_region_growing(None, None, 30, 0.5, 0.05, 1, INT_MAX, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_region_fetch(None, 0, 0, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG


def test_pcl_shaped_class_defaults_and_refusals(built):
    from icpslam_amd import IcpGpuError, RegionGrowing
    rg = RegionGrowing.__new__(RegionGrowing)                                           # (no context: no GPU here)
    for call in (lambda: rg.setIndices([0]), lambda: rg.setSmoothModeFlag(False), lambda: rg.setResidualTestFlag(True)):
        with pytest.raises(IcpGpuError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    rg.setSmoothModeFlag(True)
    rg.setResidualTestFlag(False)
