"""ISS keypoints with border estimation on the device (icpgpu_iss_keypoints_border / icpgpu_iss_fetch_border; icp_iss.hip,
icp_boundary.hip) against the NumPy restatement (tests/iss_border_restated.py), bit for bit everywhere: edge and border as int32 beside
every output of icpgpu_iss_keypoints.  There is no tolerance anywhere."""
import functools
import math
import os
import re

import numpy as np
import pytest

import boundary_restated as B
import iss_border_restated as IB
import iss_cases as K
import iss_restated as R
import normals_restated as N
from icpslam_amd import Context, IcpGpuError, ISSKeypoint3D, ISSKeypoint3DBorder, _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "iss_border_2k.npz")
ISS = (1.5, 1.0, 0.975, 0.975, 5)
scan, points = K.scan, K.points
PI = math.pi


@functools.lru_cache(maxsize=None)
def normals_of(n: int, radius: float = 1.5):
    normals = N.estimate(scan(2000)[:n], None, 0, radius)[0]
    normals.setflags(write=False)
    return normals


def assert_same(got, want, what=""):
    assert got["n_keypoints"] == want["n_keypoints"], (what, got["n_keypoints"], want["n_keypoints"])
    for name in IB.FIELDS:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError((what, name, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def check(ctx, cloud, iss, border_radius, angle, normals=None, normal_radius=0.0, what=""):
    got = ctx.iss_keypoints_border(*iss, border_radius, angle, normals, normal_radius)
    assert_same(got, IB.keypoints_border(cloud, *iss, border_radius, angle, normals, normal_radius), f"{what} {iss} {border_radius} {angle}")
    return got


# ---- sizes, normals given and computed, the waits ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 600, 2000])
def test_sizes_with_normals_given_and_computed(ctx, n):
    cloud = scan(2000)[:n]
    ctx.search_set_input(cloud)
    given = check(ctx, cloud, ISS, 1.0, PI, normals_of(n))
    assert ctx.iss_stats() == 2                                                  # the border rows' totals, the count
    computed = check(ctx, cloud, ISS, 1.0, PI, None, 1.5)
    assert ctx.iss_stats() == 3                                                  # ... and the normal rows' totals
    assert all(np.ascontiguousarray(given[f]).tobytes() == np.ascontiguousarray(computed[f]).tobytes() for f in IB.FIELDS)
    device_normals, _ = ctx.normal_estimation(None, 0, 1.5)                      # what the call computed for itself
    assert device_normals.tobytes() == normals_of(n).tobytes()
    if n == 2000:
        assert 100 < given["edge"].sum() < given["border"].sum() < 1900 and given["n_keypoints"] > 10
        plain = ctx.iss_keypoints(*ISS)
        assert ctx.iss_stats() == 1 and plain["n_keypoints"] > 20
        assert np.array_equal(plain["n_salient"], given["n_salient"])


@pytest.mark.parametrize("border_radius, angle, min_neighbors", [(0.6, 2.5, 5), (1.5, PI, 12), (2.5, 1.0, 0), (1.0, PI / 2, 40)])
def test_border_radii_thresholds_and_min_neighbors(ctx, border_radius, angle, min_neighbors):
    cloud = scan(2000).copy()
    cloud[[5, 1000], [0, 2]] = [np.nan, np.inf]
    cloud[50:60] = cloud[400:410]
    normals = normals_of(2000).copy()
    normals[70, :3] = 0.0
    normals[71, 0] = np.nan
    ctx.search_set_input(cloud)
    got = check(ctx, cloud, (1.5, 1.0, 0.975, 0.975, min_neighbors), border_radius, angle, normals)
    assert not got["edge"][[5, 1000, 70, 71]].any() and not got["border"][[5, 1000]].any() and got["edge"].sum() > 0


def test_border_off_is_the_plain_call(ctx):
    cloud = scan(2000)
    ctx.search_set_input(cloud)
    plain = ctx.iss_keypoints(*ISS)
    off = ctx.iss_keypoints_border(*ISS, 0.0, float("nan"), None, -1.0)          # threshold and normals are not looked at
    assert ctx.iss_stats() == 1
    assert off["n_keypoints"] == plain["n_keypoints"] and all(off[f].tobytes() == plain[f].tobytes() for f in R.FIELDS)
    assert off["edge"].dtype == np.int32 and not off["edge"].any() and not off["border"].any()
    ctx.iss_keypoints_border(*ISS, 1.0, PI, None, 1.5)
    assert ctx.iss_fetch_border_raw()[1]["edge"].any()
    ctx.iss_keypoints(*ISS)                                                     # a plain call after a border call: zeros again
    rc, out = ctx.iss_fetch_border_raw()
    assert rc == 0 and not out["edge"].any() and not out["border"].any()
    rc, out = ctx.iss_fetch_border_raw(want=("border",))
    assert rc == 0 and list(out) == ["border"]
    assert ctx._L.icpgpu_iss_fetch_border(ctx._h, None, None) == 0


def test_edge_is_the_boundary_call_on_the_same_rows(ctx):
    cloud = scan(2000)
    normals = normals_of(2000)
    ctx.search_set_input(cloud)
    for border_radius, angle, min_neighbors in ((1.0, PI, 5), (0.7, 2.5, 9)):
        got = ctx.iss_keypoints_border(1.5, 1.0, 0.975, 0.975, min_neighbors, border_radius, angle, normals)
        b = ctx.boundary_estimation(normals, None, 0, border_radius, angle)
        want = (b["boundary"].astype(bool) & (b["n_neighbours"] >= min_neighbors)).astype(np.int32)
        assert np.array_equal(got["edge"], want) and (b["boundary"].sum() > want.sum() or min_neighbors == 5)
        rc, again = ctx.iss_fetch_border_raw()                                   # the result outlives the boundary call
        assert rc == 0 and np.array_equal(again["edge"], got["edge"]) and np.array_equal(again["border"], got["border"])


# ---- the three walks ---------------------------------------------------------------------------------------------------------
def cell_size(ctx, cloud, monkeypatch, capfd):
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(rf"\[icpgpu\] grid n={len(cloud)} .* h=([0-9.]+) ", capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found
    return float(found[-1])


def shells(radius, h):
    return math.ceil(radius / (h * 63 / 64))


def test_cube_walk_and_sweep_give_the_same_bits(ctx, monkeypatch, capfd):
    """n = 385 and a border radius of 8.5 cells (ASSERTED, from the cell size in the library's debug line): more than the 8 shells the
    cube walk takes, so the border rows and the border walk sweep the whole cloud.  Then the same points with eight far ones behind
    them: the cells grow until the border radius takes the cube (ASSERTED).  The first 385 points' answers must be the same bits.
    (385 points and not more: at 8.5 cells a row holds most of the cloud, and the restatement's pair test is quadratic in it.)"""
    cloud = scan(385)
    h = cell_size(ctx, cloud, monkeypatch, capfd)
    border = 8.5 * h
    assert shells(border, h) > 8 and border < 300
    iss = (2.0 * h, 2.0 * h, 0.975, 0.975, 5)
    normals = N.estimate(cloud, None, 12, 0.0)[0]
    swept = check(ctx, cloud, iss, border, PI, normals, what="sweep")
    far = points([[sx * 5000.0, sy * 5000.0, sz * 5000.0] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    both = np.concatenate([cloud, far])
    h2 = cell_size(ctx, both, monkeypatch, capfd)
    assert shells(border, h2) <= 8
    cubed = check(ctx, both, iss, border, PI, np.concatenate([normals, np.zeros((8, 4), F32)]), what="cube")
    assert swept["edge"].any() and swept["border"].sum() > swept["edge"].sum()
    for name in ("edge", "border", "n_salient", "scatter6", "saliency"):
        assert cubed[name][:385].tobytes() == swept[name].tobytes(), name


def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """5 000 points, 4 600 of them in one flat group 20 cm across inside a 400 m box: one cell holds more than 4 096 points and the
    grid refuses the cloud (ASSERTED, from the library's debug line).  Every walk and every row then sweeps the whole cloud."""
    r = np.random.default_rng(41)
    group = points((r.uniform(-30, 30, 3) + r.normal(0, 0.03, (4600, 3)) * [1, 1, 0.05]).astype(F32))
    cloud = np.concatenate([group, points(r.uniform(-200, 200, (400, 3)).astype(F32))])
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=5000 .* max=(\d+) ", capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found and int(found[-1]) > 4096
    normals = np.zeros((5000, 4), F32)
    normals[:, 2] = 1.0
    got = check(ctx, cloud, (0.012, 0.012, 0.975, 0.975, 5), 0.008, PI, normals, what="refused")
    assert 0 < got["edge"].sum() < got["border"].sum() < 4600 and got["n_salient"][7] == 0


# ---- the hand scene, refusals, repeatability, the fixture, the class ----------------------------------------------------------
def test_the_corner_of_three_faces(ctx):
    cloud = K.three_faces(7)
    ctx.search_set_input(cloud)
    near = check(ctx, cloud, K.CORNER_ARGS, 1.5, PI / 2, None, 1.5)
    on_rim = (cloud[:, :3] == 6).any(axis=1)
    assert near["keypoint_index"].tolist() == [0] and near["border"][on_rim].all() and not near["edge"][~on_rim].any()
    normals = N.estimate(cloud, None, 0, 1.5)[0]
    far = check(ctx, cloud, K.CORNER_ARGS, 6.01, PI / 2, normals)
    assert far["n_keypoints"] == 0 and far["border"][0] == 1 and far["n_salient"][0] == 16 and not far["scatter6"][0].any()


def refused(call):
    with pytest.raises(IcpGpuError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID_ARG


def test_refusals():
    inf, nan = float("inf"), float("nan")
    with Context(0) as c:
        refused(lambda: c.iss_keypoints_border(*ISS, 1.0, 1.0, None, 1.0))        # no search cloud
        assert c.iss_fetch_border_raw()[0] == _lib.ERR_INVALID_ARG               # ... and no result
        c.search_set_input(scan(257))
        assert c.iss_fetch_border_raw()[0] == _lib.ERR_INVALID_ARG
        for border_radius in (-1.0, nan, inf, -inf):
            refused(lambda: c.iss_keypoints_border(*ISS, border_radius, 1.0, None, 1.0))
        for angle in (0.0, -1.0, math.nextafter(PI, 4.0), nan, inf):
            refused(lambda: c.iss_keypoints_border(*ISS, 1.0, angle, None, 1.0))
        for normal_radius in (0.0, -1.0, nan, inf):
            refused(lambda: c.iss_keypoints_border(*ISS, 1.0, 1.0, None, normal_radius))   # null normals and nothing to compute them from
        refused(lambda: c.iss_keypoints_border(0.0, 1.0, 0.9, 0.9, 5, 1.0, 1.0, None, 1.0))  # the plain call's refusals hold
        assert c._L.icpgpu_iss_keypoints_border(c._h, 1.0, 1.0, 0.9, 0.9, 5, 1.0, 1.0, None, 1.0, None) == _lib.ERR_INVALID_ARG
        rc, m = c.iss_keypoints_border_raw(*ISS, 1.0, PI, None, 1.5)
        assert rc == 0 and c.iss_stats() == 3 and c.iss_fetch_border_raw()[0] == 0
        refused(lambda: c.iss_keypoints_border(*ISS, -1.0, 1.0, None, 1.0))       # a refused call leaves no result behind
        assert c.iss_fetch_border_raw()[0] == _lib.ERR_INVALID_ARG and c.iss_fetch_raw(m)[0] == _lib.ERR_INVALID_ARG
        assert c.iss_keypoints_border_raw(*ISS, 1.0, PI, None, 1.5) == (0, m)
        c.search_set_input(scan(63))                                             # the search cloud replaced: the result is gone
        assert c.iss_fetch_border_raw()[0] == _lib.ERR_INVALID_ARG


def test_empty_and_all_nan_clouds(ctx):
    for cloud in (np.full((130, 4), np.nan, F32), np.empty((0, 4), F32)):
        ctx.search_set_input(cloud)
        got = check(ctx, cloud, ISS, 1.0, PI, None, 1.5)
        assert got["n_keypoints"] == 0 and not got["edge"].any() and not got["border"].any()


def test_five_calls_give_identical_bytes(ctx):
    cloud = scan(2000)
    ctx.search_set_input(cloud)
    runs = set()
    for _ in range(5):
        got = ctx.iss_keypoints_border(*ISS, 1.0, PI, None, 1.5)
        runs.add(b"".join(np.ascontiguousarray(got[f]).tobytes() for f in IB.FIELDS))
    assert len(runs) == 1


def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    got = ctx.iss_keypoints_border(float(g["salient_radius"]), float(g["non_max_radius"]), float(g["gamma_21"]), float(g["gamma_32"]),
                                   int(g["min_neighbors"]), float(g["border_radius"]), float(g["angle_threshold"]), g["normals"])
    assert_same(got, {"n_keypoints": int(g["n_keypoints"]), **{f: g[f] for f in IB.FIELDS}})


def test_pcl_shaped_class():
    cloud = scan(2000)
    want = IB.keypoints_border(cloud, *ISS, 1.0, PI, None, 1.5)
    iss = ISSKeypoint3DBorder()
    assert isinstance(iss, ISSKeypoint3D)
    iss.setInputCloud(cloud)
    iss.setSalientRadius(ISS[0])
    iss.setNonMaxRadius(ISS[1])
    iss.setBorderRadius(1.0)
    iss.setAngleThreshold(PI)
    with pytest.raises(IcpGpuError):
        iss.compute()                                                           # no normals and no normal radius
    iss.setNormalRadius(1.5)
    got = iss.compute()
    assert got.tobytes() == want["keypoints"].tobytes() and np.array_equal(iss.getKeypointsIndices(), want["keypoint_index"])
    assert np.array_equal(iss.getEdgePoints(), np.flatnonzero(want["edge"])) and np.array_equal(iss.getBorderPoints(), np.flatnonzero(want["border"]))
    iss.setNormalRadius(0.0)
    iss.setNormals(normals_of(2000))
    assert iss.compute().tobytes() == want["keypoints"].tobytes()
    iss.setBorderRadius(0.0)
    assert np.array_equal(iss.compute(), R.keypoints(cloud, *ISS)["keypoints"]) and iss.getEdgePoints().size == 0
    plain = ISSKeypoint3D()
    with pytest.raises(IcpGpuError, match="not provided"):
        plain.setBorderRadius(0.5)                                              # the class the earlier tests pin stays as it was
