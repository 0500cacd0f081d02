"""ISS keypoints on the device (icpgpu_iss_keypoints / icpgpu_iss_fetch / icpgpu_iss_stats; icp_iss.hip) against the NumPy restatement
(tests/iss_restated.py), bit for bit everywhere: n_salient and the keypoint indices as int32, scatter6, eigenvalues3 and saliency as
float64, the keypoint cloud as float32, and the count.  There is no tolerance anywhere."""
import math
import os
import re

import numpy as np
import pytest

import iss_cases as K
import iss_restated as R
from icpslam_amd import Context, IcpGpuError, ISSKeypoint3D, _lib

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "iss_2k.npz")
DEFAULT = (1.5, 1.0, 0.975, 0.975, 5)
scan, points = K.scan, K.points

_REF = {}


def ref(key, cloud, args):
    """The restatement's answer, computed once per (cloud, arguments) and left unchanged; key = None: not worth keeping."""
    if key is None:
        return R.keypoints(cloud, *args)
    k = (key, tuple(float(a) for a in args))
    if k not in _REF:
        _REF[k] = R.keypoints(cloud, *args)
        for a in _REF[k].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[k]


def assert_same(got, want, what=""):
    assert got["n_keypoints"] == want["n_keypoints"], (what, got["n_keypoints"], want["n_keypoints"])
    for name in R.FIELDS:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bits = g.view(np.uint32 if g.itemsize == 4 else np.uint64), w.view(np.uint32 if w.itemsize == 4 else np.uint64)
            bad = np.argwhere(bits[0] != bits[1])
            raise AssertionError((what, name, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def check(ctx, key, cloud, args, what=""):
    """One ISS call on the search cloud in place against the restatement."""
    got = ctx.iss_keypoints(*args)
    want = ref(key, cloud, args)
    assert_same(got, want, f"{what} {args}")
    return got


# ---- sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [DEFAULT, (0.8, 1.6, 0.9, 0.6, 3)])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 2000])
def test_sizes(ctx, n, args):
    cloud = scan(2000)[:n]
    ctx.search_set_input(cloud)
    got = check(ctx, ("scan", n), cloud, args)
    if n == 2000:
        assert 20 < got["n_keypoints"] < (got["saliency"] > 0).sum()     # some survive, some are suppressed
    if n == 2000 and args == DEFAULT:
        sizes = set(got["n_salient"].tolist())
        assert {1, args[4] - 1, args[4], 63, 64, 65} <= sizes and max(sizes) > 100


# ---- ball sizes --------------------------------------------------------------------------------------------------------------
def blobs(sizes, seed):
    """Tight groups (within 2 cm) of exactly the given numbers of points, 50 m apart: a point's ball of 0.1 .. 1 m is its group."""
    r = np.random.default_rng(seed)
    xyz = [np.array([50.0 * g, 0, 0]) + r.uniform(-0.01, 0.01, (m, 3)) for g, m in enumerate(sizes)]
    return points(np.concatenate(xyz).astype(F32))


@pytest.mark.parametrize("args", [(0.5, 0.2, 10.0, 10.0, 5), (0.2, 0.5, 0.975, 0.975, 64), (0.3, 0.3, 10.0, 10.0, 65)])
def test_balls_of_exactly_these_sizes(ctx, args):
    sizes = (1, 4, 5, 63, 64, 65, 300, 129)
    cloud = blobs(sizes, 31)
    cloud[2, 1] = np.nan                                                     # the group of four becomes one of three: a ball of size 0 too
    ctx.search_set_input(cloud)
    got = check(ctx, "blobs", cloud, args)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert got["n_salient"][starts[1:] - 1].tolist() == [1, 3, 5, 63, 64, 65, 300, 129] and got["n_salient"][2] == 0   # (each group's last point)
    assert not got["saliency"][:starts[2]].any() and (args[2] < 10.0 or (got["saliency"][starts[6]:starts[7]] > 0).all())


@pytest.mark.parametrize("leaf", [0.1, 0.2, 0.3, 0.5, 0.8, 1.2])
def test_voxel_filtered_scans(ctx, leaf):
    """A 2 000-point scan through the voxel filter at six leaf sizes: from 2 000 points to a few hundred, the radii following the
    leaf so that the balls run from a handful to several hundred entries."""
    cloud = ctx.voxel_grid(scan(2000), leaf)
    assert 100 < len(cloud) <= 2000
    ctx.search_set_input(cloud)
    for args in ((3 * leaf, 2 * leaf, 0.975, 0.975, 5), (6.0, 3.0, 0.975, 0.975, 5)):
        got = check(ctx, None, cloud, args, f"leaf {leaf}")
    assert got["n_salient"].max() > (300 if leaf <= 0.3 else 30)


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
    """n = 1025 and a salient radius of 8.5 cells (ASSERTED, from the cell size in the library's debug line): more than the 8 shells the
    cube walk takes, so every point sweeps the whole cloud, while the non-max radius of 2 cells takes the cube.  Then the same points
    with eight far ones behind them: the bounding box, and with it the cells, grow until both radii take the cube (ASSERTED).  The
    far points are in no ball but their own, so the first 1 025 points' answers must be the very same bits on both walks."""
    cloud = scan(1025)
    h = cell_size(ctx, cloud, monkeypatch, capfd)
    salient, non_max = 8.5 * h, 2.0 * h
    assert shells(salient, h) > 8 >= shells(non_max, h) and salient < 300
    args = (salient, non_max, 0.975, 0.975, 5)
    swept = check(ctx, None, cloud, args, "sweep")
    far = points([[sx * 5000.0, sy * 5000.0, sz * 5000.0] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    both = np.concatenate([cloud, far])
    h2 = cell_size(ctx, both, monkeypatch, capfd)
    assert shells(salient, h2) <= 8 and shells(non_max, h2) <= 8
    cubed = check(ctx, None, both, args, "cube")
    assert (cubed["n_salient"][1025:] == 1).all() and cubed["n_keypoints"] == swept["n_keypoints"]
    for name in ("n_salient", "scatter6", "eigenvalues3", "saliency"):
        assert cubed[name][:1025].tobytes() == swept[name].tobytes(), name
    assert cubed["keypoint_index"].tobytes() == swept["keypoint_index"].tobytes() and cubed["keypoints"].tobytes() == swept["keypoints"].tobytes()


def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """5 000 points, 4 600 of them in one group 20 cm across inside a 400 m box: one cell holds more than 4 096 points and the grid
    refuses the cloud (ASSERTED, from the library's debug line; no smaller cloud can be refused that way).  Every point then sweeps the
    whole cloud.  Without the far points the same group has a grid: its answers must be the same bits."""
    r = np.random.default_rng(41)
    group = points((r.uniform(-30, 30, 3) + r.normal(0, 0.03, (4600, 3))).astype(F32))
    cloud = np.concatenate([group, points(r.uniform(-200, 200, (400, 3)).astype(F32))])
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=5000 .* max=(\d+) ", capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found and int(found[-1]) > 4096
    args = (0.02, 0.012, 0.975, 0.975, 5)
    swept = check(ctx, "refused", cloud, args)
    assert swept["n_keypoints"] > 10 and swept["n_salient"][7] == 0 and 100 < swept["n_salient"].max()
    ctx.search_set_input(cloud[:4600])
    gridded = check(ctx, "refused-group", cloud[:4600], args)
    if (swept["n_salient"][4600:] == 1).all():                               # (no far point fell into the group)
        for name in ("n_salient", "scatter6", "eigenvalues3", "saliency"):
            assert gridded[name].tobytes() == swept[name][:4600].tobytes(), name


# ---- min_neighbors, the hand cases, degenerate inputs ------------------------------------------------------------------------
@pytest.mark.parametrize("min_neighbors", [0, 1])
def test_min_neighbors_of_zero_and_one(ctx, min_neighbors):
    cloud = scan(257).copy()
    cloud[100, 0] = np.nan
    ctx.search_set_input(cloud)
    got = check(ctx, "scan257nan", cloud, (1.0, 1.0, 0.975, 0.975, min_neighbors))
    assert got["n_salient"][100] == 0 and not got["eigenvalues3"][100].any() and got["n_keypoints"] > 0
    check(ctx, "scan257nan", cloud, (1e-30, 1e-30, 10.0, 10.0, min_neighbors))   # r2 rounds to 0: every ball is empty


@pytest.mark.parametrize("name", [case[0] for case in K.hand_cases()])
def test_hand_cases(ctx, name):
    cloud, args = {c[0]: c[1:] for c in K.hand_cases()}[name]
    ctx.search_set_input(cloud)
    got = check(ctx, ("hand", name), cloud, args, name)
    if name == "ties":
        assert got["n_keypoints"] == 71
    if name == "corner":
        assert got["keypoint_index"].tolist() == [0]
    if name in ("planar_lattice", "line", "coincident"):
        assert got["n_keypoints"] == 0


def test_duplicated_points(ctx):
    cloud = scan(600).copy()
    cloud[50:80] = cloud[400:430]
    cloud[300:310] = cloud[299]
    ctx.search_set_input(cloud)
    got = check(ctx, None, cloud, DEFAULT)
    assert got["saliency"][50:80].tobytes() == got["saliency"][400:430].tobytes()   # coincident points tie exactly and share their fate
    assert np.array_equal(np.isin(np.arange(50, 80), got["keypoint_index"]), np.isin(np.arange(400, 430), got["keypoint_index"]))


def test_all_nan_and_empty_clouds(ctx):
    for cloud in (np.full((130, 4), np.nan, F32), np.empty((0, 4), F32)):
        ctx.search_set_input(cloud)
        got = check(ctx, None, cloud, DEFAULT)
        assert got["n_keypoints"] == 0 and got["keypoints"].shape == (0, 4) and not got["n_salient"].any() and not got["saliency"].any()
        assert ctx.iss_stats() == 1


# ---- thresholds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gammas", [(0.0, 0.0), (1.0, 1.0), (10.0, 10.0), (0.0, 10.0), (10.0, 0.0), (-1.0, 0.5)])
def test_gammas(ctx, gammas):
    cloud = scan(600)
    ctx.search_set_input(cloud)
    got = check(ctx, "scan600", cloud, (1.5, 1.0, *gammas, 5))
    assert (got["n_keypoints"] == 0) == (min(gammas) <= 0.0)


def test_gamma_at_a_points_own_quotient(ctx):
    cloud = scan(257)
    ctx.search_set_input(cloud)
    base = check(ctx, "scan257", cloud, (1.5, 1.0, 10.0, 10.0, 5))
    i = int(np.argmax(base["saliency"]))
    e1, e2, e3 = base["eigenvalues3"][i]
    q21, q32 = F64(e2) / F64(e1), F64(e3) / F64(e2)
    for g21, g32, passes in ((q21, 10.0, False), (np.nextafter(q21, 2.0), 10.0, True), (10.0, q32, False), (10.0, np.nextafter(q32, 2.0), True)):
        got = check(ctx, "scan257", cloud, (1.5, 1.0, float(g21), float(g32), 5))
        assert (got["saliency"][i] == e3) == passes and (got["saliency"][i] == 0) == (not passes)


# ---- the fold's order, and the device's own radius rows ----------------------------------------------------------------------
def test_fold_order_on_terms_of_fourteen_decades(ctx):
    """A ball of 300 neighbours at 1e-5 .. 100 m from its centre: the products span 1e-10 .. 1e4 m^2, and the six sums over lanes and
    batches must still be math.fsum's."""
    r = np.random.default_rng(51)
    d = r.normal(size=(300, 3))
    d *= (10.0 ** r.uniform(-5, 2, 300) / np.linalg.norm(d, axis=1))[:, None]
    cloud = points(np.concatenate([[[0, 0, 0]], d]).astype(F32))
    ctx.search_set_input(cloud)
    got = check(ctx, None, cloud, (150.0, 150.0, 10.0, 10.0, 5))
    assert got["n_salient"][0] == 301
    terms = (cloud[1:, 0].astype(F64)) ** 2
    assert terms.min() < 1e-9 and terms.max() > 1e3 and got["scatter6"][0, 0] == math.fsum(terms.tolist())
    assert got["scatter6"][0, 0] != float(np.sum(terms.astype(F32)))         # (a float32 sum would not do)


@pytest.mark.parametrize("radius", [0.7, 1.5])
def test_ball_sizes_are_the_radius_searchs_own_rows(ctx, radius):
    cloud = scan(2000).copy()
    cloud[[5, 1000], [0, 2]] = [np.nan, np.inf]
    ctx.search_set_input(cloud)
    row_start, _, _ = ctx.search_radius(None, radius)
    rc, m = ctx.iss_keypoints_raw(radius, radius)
    assert rc == 0
    rc, out = ctx.iss_fetch_raw(0, want=("n_salient",))
    assert rc == 0 and np.array_equal(out["n_salient"], np.diff(row_start).astype(np.int32))


# ---- refusals, the fetch, the waits ------------------------------------------------------------------------------------------
def refused(call):
    with pytest.raises(IcpGpuError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID_ARG


def test_refusals():
    inf, nan = float("inf"), float("nan")
    with Context(0) as c:
        refused(lambda: c.iss_keypoints(1.0, 1.0))                               # no search cloud
        assert c.iss_fetch_raw(0)[0] == _lib.ERR_INVALID_ARG                     # ... and no result
        assert c._L.icpgpu_iss_stats(c._h, None) == _lib.ERR_INVALID_ARG
        c.search_set_input(scan(257))
        assert c.iss_fetch_raw(300)[0] == _lib.ERR_INVALID_ARG                   # a cloud, no result yet
        for bad in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, -0.5), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, inf)):
            refused(lambda: c.iss_keypoints(*bad))
        for bad in ((nan, 0.9), (0.9, nan), (inf, 0.9), (0.9, -inf)):
            refused(lambda: c.iss_keypoints(1.0, 1.0, *bad))
        refused(lambda: c.iss_keypoints(1.0, 1.0, 0.9, 0.9, -1))
        assert c._L.icpgpu_iss_keypoints(c._h, 1.0, 1.0, 0.9, 0.9, 5, None) == _lib.ERR_INVALID_ARG   # null n_keypoints
        rc, m = c.iss_keypoints_raw(1.0, 1.0)
        assert rc == 0 and m > 0 and c.iss_stats() == 1
        refused(lambda: c.iss_keypoints(nan, 1.0))                               # a refused call leaves no result behind
        assert c.iss_fetch_raw(m)[0] == _lib.ERR_INVALID_ARG and c._L.icpgpu_iss_stats(c._h, None) == _lib.ERR_INVALID_ARG
        assert c.iss_keypoints_raw(1.0, 1.0) == (0, m) and c.iss_fetch_raw(m)[0] == 0
        c.search_set_input(scan(63))                                             # the search cloud replaced: the result is gone
        assert c.iss_fetch_raw(m)[0] == _lib.ERR_INVALID_ARG


def test_fetch_capacities_and_null_subsets(ctx):
    cloud = scan(600)
    ctx.search_set_input(cloud)
    want = ref("scan600", cloud, DEFAULT)
    rc, m = ctx.iss_keypoints_raw(*DEFAULT)
    assert (rc, m) == (0, want["n_keypoints"]) and m > 2
    for cap in (m - 1, 0):
        rc, out = ctx.iss_fetch_raw(cap)
        assert rc == _lib.ERR_INVALID_ARG and all((a == -2).all() for a in out.values())   # nothing was written
        rc, out = ctx.iss_fetch_raw(cap, want=("keypoints", "saliency"))
        assert rc == _lib.ERR_INVALID_ARG and all((a == -2).all() for a in out.values())
    rc, out = ctx.iss_fetch_raw(0, want=("n_salient", "scatter6", "eigenvalues3", "saliency"))   # no keypoint output: no capacity needed
    assert rc == 0 and all(out[f].tobytes() == want[f].tobytes() for f in out)
    for _ in range(2):
        rc, out = ctx.iss_fetch_raw(m)
        assert rc == 0
        assert_same({**out, "n_keypoints": m}, want)
    rc, out = ctx.iss_fetch_raw(m + 7, want=("keypoint_index", "keypoints"))                     # room to spare
    assert rc == 0 and np.array_equal(out["keypoint_index"][:m], want["keypoint_index"]) and (out["keypoint_index"][m:] == -2).all()
    assert out["keypoints"][:m].tobytes() == want["keypoints"].tobytes() and (out["keypoints"][m:] == -2).all()
    for single in R.FIELDS:
        rc, out = ctx.iss_fetch_raw(m, want=(single,))
        assert rc == 0 and list(out) == [single] and out[single].tobytes() == np.ascontiguousarray(want[single]).tobytes()
    assert ctx._L.icpgpu_iss_fetch(ctx._h, 0, None, None, None, None, None, None) == 0           # every pointer NULL
    assert ctx.iss_stats() == 1


def test_five_calls_give_identical_bytes(ctx):
    cloud = scan(2000)
    ctx.search_set_input(cloud)
    for args in (DEFAULT, (2.5, 2.5, 10.0, 10.0, 0)):
        runs = []
        for _ in range(5):
            got = ctx.iss_keypoints(*args)
            runs.append(b"".join(np.ascontiguousarray(got[f]).tobytes() for f in R.FIELDS))
        assert len(set(runs)) == 1


# ---- the golden fixture and the PCL-shaped class -----------------------------------------------------------------------------
def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    got = ctx.iss_keypoints(float(g["salient_radius"]), float(g["non_max_radius"]), float(g["gamma_21"]), float(g["gamma_32"]),
                            int(g["min_neighbors"]))
    assert_same(got, {"n_keypoints": int(g["n_keypoints"]), **{f: g[f] for f in R.FIELDS}})


def test_pcl_shaped_class():
    cloud = scan(600)
    want = ref("scan600", cloud, DEFAULT)
    iss = ISSKeypoint3D()
    iss.setInputCloud(cloud)
    iss.setSearchMethod(None)
    with pytest.raises(IcpGpuError):
        iss.compute()                                                           # PCL's default radii are 0
    iss.setSalientRadius(DEFAULT[0])
    with pytest.raises(IcpGpuError):
        iss.compute()
    iss.setNonMaxRadius(DEFAULT[1])
    iss.setNormalRadius(0.3)
    iss.setNumberOfThreads(4)
    iss.setBorderRadius(0.0)
    with pytest.raises(IcpGpuError, match="not provided"):
        iss.setBorderRadius(0.5)
    got = iss.compute()                                                         # gammas 0.975 and 5 neighbours: PCL's defaults
    assert got.dtype == F32 and got.tobytes() == want["keypoints"].tobytes()
    assert np.array_equal(iss.getKeypointsIndices(), want["keypoint_index"]) and iss.getKeypointsIndices().dtype == np.int32
    iss.setThreshold21(0.9)
    iss.setThreshold32(0.6)
    iss.setMinNeighbors(3)
    iss.compute()
    assert np.array_equal(iss.getKeypointsIndices(), R.keypoints(cloud, DEFAULT[0], DEFAULT[1], 0.9, 0.6, 3)["keypoint_index"])
    with pytest.raises(IcpGpuError):
        ISSKeypoint3D().compute()
