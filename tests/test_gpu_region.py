"""Region growing on the device (icpgpu_region_growing / icpgpu_region_fetch; icp_region.hip) against the NumPy restatement
(tests/region_restated.py), bit for bit everywhere: region_start as int64; indices, labels, region, kind and anchor as int32; both
counts.  The answer is a partition of integers: there is no tolerance anywhere."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import normals_restated as N
import region_cases as RC
import region_restated as R
from icpslam_amd import Context, IcpGpuError, RegionGrowing, _lib, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
INT_MAX = 2**31 - 1
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2000)
KS = (1, 2, 29, 30, 31, 32, 33, 63, 64)
WINDOWS = ((1, INT_MAX), (2, 50), (5, 5))
COS30 = RC.cos_of(30)
THR = 1e-4   # between the scan's ring-collinear neighbourhoods (curvature ~1e-10) and its surfaces' (~1e-4 .. 1e-2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "region_2k.npz")


@functools.lru_cache(maxsize=None)
def scan():
    """A 2 000-point scan and its normals at k = 12 from the restatement: about a fifth of the points single, a sixth border, the rest core at THR."""
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 5)
    normals = N.estimate(cloud, None, k=12)[0]
    cloud.setflags(write=False)
    normals.setflags(write=False)
    return cloud, normals


_ROWS = {}


def ref_rows(key, cloud, k):
    """The restatement's k-nearest rows, computed once per (cloud, k) and left unchanged; key = None: not worth keeping."""
    if key is None:
        return R.rows_of(np.asarray(cloud, F32), k)
    if (key, k) not in _ROWS:
        _ROWS[key, k] = R.rows_of(np.asarray(cloud, F32), k)
    return _ROWS[key, k]


def assert_same(got, want, what=""):
    for name, g, w in zip(R.NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


def check(ctx, key, cloud, normals, k, cos, threshold, lo=1, hi=INT_MAX):
    """One call on the search cloud in place against the restatement: the two counts, then the six arrays."""
    want = R.grow(cloud, normals, k, cos, threshold, lo, hi, rows=ref_rows(key, cloud, k))
    rc, n_regions, n_in = ctx.region_growing_raw(normals, k, cos, threshold, lo, hi)
    assert (rc, n_regions, n_in) == (0, want[0].size - 1, want[1].size), (k, lo, hi)
    rc, *got = ctx.region_fetch_raw(n_regions, n_in)
    assert rc == 0
    assert_same(got, want, f"k {k} cos {cos} threshold {threshold} window {lo} .. {hi}")
    return got


def check_case(ctx, case, key=None):
    ctx.search_set_input(case.cloud)
    return check(ctx, key, case.cloud, case.normals, case.k, case.cos, case.threshold, case.lo, case.hi)


# ---- sizes and k ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    cloud, normals = scan()[0][:n], scan()[1][:n]
    ctx.search_set_input(cloud)
    for lo, hi in WINDOWS:
        start, indices, labels, region, kind, anchor = check(ctx, ("scan", n), cloud, normals, 12, COS30, THR, lo, hi)
        assert start[0] == 0 and start[-1] == indices.size == (labels >= 0).sum()
    if n == 2000:  # (what makes the case worth its time: every kind of point, hundreds of regions, a window that cuts on both sides)
        assert [int((kind == v).sum()) for v in (-1, 0, 1, 2)] == [0, 406, 338, 1256]
        assert np.unique(region).size == 460
    check(ctx, ("scan", n), cloud, normals, 12, RC.cos_of(5), math.inf)


@pytest.mark.parametrize("k", KS)
def test_ks(ctx, k):
    for n in (300, 40):                                   # (40: k above n for the larger ones)
        cloud, normals = scan()[0][:n], scan()[1][:n]
        ctx.search_set_input(cloud)
        check(ctx, ("scan", n), cloud, normals, k, COS30, THR)
        check(ctx, ("scan", n), cloud, normals, k, RC.cos_of(10), 1e-5, 2, 30)


# ---- every hand cloud -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_hand_clouds(ctx, name):
    check_case(ctx, RC.CASES[name])


# ---- shapes whose diameter is their size, and the ordering's wave and tile boundaries ---------------------------------------
def test_strip_against_the_restatement(ctx):
    case, _ = RC.strip(3000, 21)
    start, indices, labels, region, kind, anchor = check_case(ctx, case)
    assert start.tolist() == [0, 3000] and not region.any() and (kind == 2).all()


def test_long_strip_is_one_region_named_zero(ctx):
    """20 000 cores in a line, the indices shuffled: a core graph of diameter ~10 000.  The answer is known by construction.  That
    this finishes in the time every test gets is the check that the number of launches does not grow with the diameter."""
    n = 20000
    case, _ = RC.strip(n, 22)
    ctx.search_set_input(case.cloud)
    start, indices, labels, region, kind, anchor = ctx.region_growing(case.normals, case.k, smoothness_cos=case.cos)
    assert start.dtype == np.int64 and start.tolist() == [0, n]
    assert indices.dtype == np.int32 and np.array_equal(indices, np.arange(n))
    assert labels.dtype == region.dtype == np.int32 and not labels.any() and not region.any()
    assert (kind == 2).all() and (anchor == -1).all()


def test_interleaved_strips_with_opposed_smoothness_stay_two(ctx):
    m = 1000
    start, indices, labels, region, kind, anchor = check_case(ctx, RC.interleaved_strips(m))
    assert start.tolist() == [0, m, 2 * m] and np.array_equal(region, np.arange(2 * m) % 2)
    assert np.array_equal(indices[:m], np.arange(0, 2 * m, 2)) and np.array_equal(indices[m:], np.arange(1, 2 * m, 2))


@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257])
def test_exactly_m_emitted_regions(ctx, m):
    case, _ = RC.tied_regions(m, 100 + m)
    start, indices, labels, region, kind, anchor = check_case(ctx, case)
    assert np.array_equal(start, 2 * np.arange(m + 1)) and (np.diff(indices[0::2]) > 0).all()
    start = check_case(ctx, case._replace(lo=1, hi=INT_MAX))[0]
    assert start.size - 1 == m + 40


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------
def test_nan_rows_and_nan_normals(ctx):
    cloud, normals = scan()[0][:1025].copy(), scan()[1][:1025].copy()
    cloud[[0, 7, 64, 700, 1024], [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
    normals[[1, 65, 300, 999], [0, 1, 2, 3]] = [np.nan, np.inf, np.nan, np.nan]
    out = [0, 7, 64, 700, 1024, 1, 65, 300, 999]
    ctx.search_set_input(cloud)
    for k, threshold in ((12, THR), (30, math.inf)):
        for lo, hi in WINDOWS:
            _, _, labels, region, kind, anchor = check(ctx, "nonfinite", cloud, normals, k, COS30, threshold, lo, hi)
            assert (kind[out] == -1).all() and (region[out] == -1).all() and (labels[out] == -1).all() and (anchor[out] == -1).all()
    assert (kind >= 0).sum() == 1025 - len(out)


def test_no_participant_and_empty_clouds(ctx):
    ones = np.ones((130, 4), F32)
    for cloud, normals in ((np.full((130, 4), np.nan, F32), ones), (ones, np.full((130, 4), np.nan, F32)), (np.empty((0, 4), F32), np.empty((0, 4), F32))):
        ctx.search_set_input(cloud)
        start, indices, labels, region, kind, anchor = check(ctx, None, cloud, normals, 5, COS30, 0.05)
        assert start.tolist() == [0] and indices.size == 0
        assert labels.tolist() == region.tolist() == kind.tolist() == anchor.tolist() == [-1] * len(cloud)
    assert ctx.region_growing_raw(None, 5, COS30, 0.05, 1, INT_MAX) == (0, 0, 0)                 # an empty cloud needs no normals


def test_all_points_coincident(ctx):
    cloud = np.tile(np.array([[3.0, -2.0, 0.5, 1.0]], F32), (300, 1))
    normals = np.tile(np.array([[0.0, 0.0, 1.0, 0.0]], F32), (300, 1))
    normals[100:, 3] = 1.0
    ctx.search_set_input(cloud)
    start, indices, labels, region, kind, anchor = check(ctx, None, cloud, normals, 8, COS30, 0.05)
    # every row is points 0 .. 7: the cores behind them list them and join, but no core's row has a point that is not core
    assert start[:3].tolist() == [0, 100, 101] and start.size - 1 == 201 and (kind[100:] == 0).all() and not region[:100].any()


def clustered(n, seed):
    """The cloud test_sor_cloud_the_grid_refuses builds: tight clusters (4 centres, sigma 0.3) in a wide sparse volume."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-50, 50, (4, 3))
    c = np.ones((n, 4), F32)
    c[:, :3] = (centres[r.integers(0, 4, n)] + r.normal(0, 0.3, (n, 3))).astype(F32)
    c[::11, :3] = r.uniform(-200, 200, (len(c[::11]), 3)).astype(F32)
    return c


def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """22 000 points, ~5 000 in each cluster of ~2 m across, in a 400 m box: the densest cell holds more than 4 096 points and the
    grid refuses the cloud (ASSERTED, from the library's debug line).  The rows then come from the search's whole-cloud kernel."""
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    r = np.random.default_rng(2)
    normals = r.normal(size=(22000, 4)).astype(F32)
    normals[:, :3] /= np.linalg.norm(normals[:, :3], axis=1, keepdims=True).astype(F32)
    normals[:, 3] = r.uniform(0, 0.1, 22000).astype(F32)
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    assert found and int(found[-1]) > 4096
    start, indices, labels, region, kind, anchor = check(ctx, "refused", cloud, normals, 10, RC.cos_of(60), 0.05)
    assert start.size - 1 > 100 and kind[7] == -1 and set(np.unique(kind).tolist()) == {-1, 0, 1, 2}
    check(ctx, "refused", cloud, normals, 10, RC.cos_of(60), 0.05, 3, 40)


@pytest.mark.parametrize("leaf", [0.4, 0.8])
def test_voxel_filtered_scan_with_the_devices_own_normals(ctx, leaf):
    """The chain a user runs: VoxelGrid, NormalEstimation, RegionGrowing, the device's normals fed straight back."""
    raw = synth.scan(synth.make_scene(3), np.eye(4), 20000, 7)
    cloud = ctx.voxel_grid(raw, leaf)
    assert 1000 < len(cloud) < 20000
    ctx.search_set_input(cloud)
    normals, _ = ctx.normal_estimation(None, k=30)
    for k in (30, 10):
        start, indices, labels, region, kind, anchor = check(ctx, ("voxel", leaf), cloud, normals, k, COS30, 0.05, 50, INT_MAX)
        print(f"leaf {leaf} k {k}: {len(cloud)} points, {start.size - 1} regions of 50 or more, kinds {[int((kind == v).sum()) for v in (-1, 0, 1, 2)]}")
        assert start.size - 1 >= 1 and (kind == 2).sum() > len(cloud) // 2


# ---- the device's own rows --------------------------------------------------------------------------------------------------
def host_regions(normals, kind, idx, d2, cos):
    """region (n,) int32 by a host union-find over the given rows and kinds: the rule's last three paragraphs."""
    n = len(kind)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    best = {}
    for i in np.flatnonzero(kind == 2).tolist():
        js = idx[i]
        ok = (js >= 0) & (js != i)
        ok[ok] &= kind[js[ok]] >= 0
        ok[ok] &= R.smooth_pairs(normals, np.full(int(ok.sum()), i), js[ok].astype(np.int64), cos)
        for s in np.flatnonzero(ok).tolist():
            j = int(js[s])
            if kind[j] == 2:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            else:
                key = (int(d2[i, s:s + 1].view(np.uint32)[0]) << 32) | i
                best[j] = min(best.get(j, key), key)
    region = np.full(n, -1, np.int32)
    for p in range(n):
        if kind[p] == 2:
            region[p] = find(p)
        elif kind[p] >= 0:
            region[p] = find(best[p] & 0xFFFFFFFF) if p in best else p
    return region


@pytest.mark.parametrize("k", [12, 30])
def test_host_union_find_over_the_devices_knn_rows(ctx, k):
    cloud, normals = scan()
    ctx.search_set_input(cloud)
    idx, d2, _ = ctx.search_knn(None, k)
    _, _, _, region, kind, anchor = ctx.region_growing(normals, k, curvature_threshold=THR)
    assert np.array_equal(region, host_regions(normals, kind, idx, np.ascontiguousarray(d2), COS30))
    assert ((kind == 1) == (anchor >= 0)).all() and (kind == 1).sum() > 100 and (kind == 0).sum() > 100


# ---- refusals and the fetch -------------------------------------------------------------------------------------------------
def refused(call):
    with pytest.raises(IcpGpuError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID_ARG


def test_refusals():
    cloud, normals = scan()[0][:257], scan()[1][:257]
    with Context(0) as c:
        refused(lambda: c.region_growing(normals, 12))                                            # no search cloud
        assert c.region_fetch_raw(0, 0)[0] == _lib.ERR_INVALID_ARG                                # ... and no result
        c.search_set_input(cloud)
        assert c.region_fetch_raw(300, 300)[0] == _lib.ERR_INVALID_ARG                            # a cloud, no result yet
        good = (0, *c.region_growing_raw(normals, 12, COS30, THR, 1, INT_MAX)[1:])
        assert good[1] > 1 and good[2] == 257
        bad_calls = [lambda: c.region_growing_raw(None, 12, COS30, THR, 1, INT_MAX),              # null normals with n > 0
                     lambda: c.region_growing_raw(normals, 0, COS30, THR, 1, INT_MAX),            # k outside 1 .. 64
                     lambda: c.region_growing_raw(normals, 65, COS30, THR, 1, INT_MAX),
                     lambda: c.region_growing_raw(normals, -3, COS30, THR, 1, INT_MAX),
                     lambda: c.region_growing_raw(normals, 12, float("nan"), THR, 1, INT_MAX),    # NaN arguments
                     lambda: c.region_growing_raw(normals, 12, COS30, float("nan"), 1, INT_MAX)]
        n = C.c_size_t(7)
        for a, b in ((None, C.byref(n)), (C.byref(n), None), (None, None)):                       # null count pointers
            bad_calls.append(lambda a=a, b=b: (c._L.icpgpu_region_growing(c._h, normals.ctypes.data_as(C.POINTER(C.c_float)), 12, float(COS30), THR, 1,
                                                                          INT_MAX, a, b), 0, 0))
        for call in bad_calls:
            assert c.region_growing_raw(normals, 12, COS30, THR, 1, INT_MAX) == good
            assert call() == (_lib.ERR_INVALID_ARG, 0, 0)
            assert c.region_fetch_raw(good[1], good[2])[0] == _lib.ERR_INVALID_ARG                # a refused call leaves no result behind
        for cos, threshold in ((math.inf, THR), (-math.inf, THR), (COS30, -math.inf)):          # infinities are legal
            assert c.region_growing_raw(normals, 12, cos, threshold, 1, INT_MAX)[0] == 0
        assert c.region_growing_raw(normals, 12, COS30, THR, 1, INT_MAX) == good
        assert c._L.icpgpu_region_fetch(c._h, good[1], good[2], None, None, None, None, None, None) == _lib.ERR_INVALID_ARG  # null region_start
        assert c.region_fetch_raw(good[1], good[2])[0] == 0
        c.search_set_input(cloud)                                                                 # the search cloud replaced: the result is gone
        assert c.region_fetch_raw(good[1], good[2])[0] == _lib.ERR_INVALID_ARG


def test_fetch_twice_capacities_one_too_small_and_null_subsets(ctx):
    cloud, normals = scan()[0][:1025], scan()[1][:1025]
    ctx.search_set_input(cloud)
    want = R.grow(cloud, normals, 12, COS30, THR, 2, 50, rows=ref_rows(("scan", 1025), cloud, 12))
    rc, n_regions, n_in = ctx.region_growing_raw(normals, 12, COS30, THR, 2, 50)
    assert (rc, n_regions, n_in) == (0, want[0].size - 1, want[1].size) and n_regions > 1
    for cap_r, cap_i in ((n_regions - 1, n_in), (n_regions, n_in - 1), (0, 0)):
        rc, *arrays = ctx.region_fetch_raw(cap_r, cap_i)
        assert rc == _lib.ERR_INVALID_ARG and all((a == -2).all() for a in arrays)                # nothing was written
    for _ in range(2):
        rc, *arrays = ctx.region_fetch_raw(n_regions, n_in)
        assert rc == 0
        assert_same(arrays, want)
    per_point = ("labels", "region", "kind", "anchor")
    for subset in ((), ("kind",), ("labels", "anchor"), ("region",)):
        rc, start, indices, *rest = ctx.region_fetch_raw(n_regions + 5, n_in + 9, want=subset)     # room to spare
        assert rc == 0
        assert np.array_equal(start[:n_regions + 1], want[0]) and (start[n_regions + 1:] == -2).all()
        assert np.array_equal(indices[:n_in], want[1]) and (indices[n_in:] == -2).all()
        for name, got, w in zip(per_point, rest, want[2:]):
            assert (got is None) if name not in subset else np.array_equal(got, w)


def test_one_host_wait(ctx, monkeypatch, capfd):
    """The library's own account of the call, from its debug line: the rows are queued, the counts are waited for once."""
    cloud, normals = scan()
    ctx.search_set_input(cloud)
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    rc, n_regions, n_in = ctx.region_growing_raw(normals, 30, COS30, THR, 1, INT_MAX)
    found = re.findall(r"\[icpgpu\] region n=2000 k=30 regions=(\d+) in_regions=(\d+) waits=(\d+)", capfd.readouterr().err)
    assert rc == 0 and found == [(str(n_regions), str(n_in), "1")]


def test_five_calls_give_identical_bytes(ctx):
    cloud, normals = scan()
    ctx.search_set_input(cloud)
    for k, threshold, lo, hi in ((12, THR, 1, INT_MAX), (30, 1e-5, 2, 50)):
        runs = [b"".join(a.tobytes() for a in ctx.region_growing(normals, k, curvature_threshold=threshold, min_size=lo, max_size=hi)) for _ in range(5)]
        assert len(set(runs)) == 1


# ---- the golden fixture and the PCL-shaped class ----------------------------------------------------------------------------
def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    got = ctx.region_growing(g["normals"], int(g["k"]), smoothness_cos=g["smoothness_cos"], curvature_threshold=g["curvature_threshold"],
                             min_size=int(g["min_size"]), max_size=int(g["max_size"]))
    assert_same(got, [g[name] for name in R.NAMES])


def test_pcl_shaped_class(ctx):
    cloud, normals = scan()[0][:1025], scan()[1][:1025]
    rg = RegionGrowing()
    assert (rg.getNumberOfNeighbours(), rg.getCurvatureThreshold(), rg.getMinClusterSize(), rg.getMaxClusterSize()) == (30, 0.05, 1, INT_MAX)
    assert rg.getSmoothnessThreshold() == 30.0 / 180.0 * math.pi and rg.getCurvatureTestFlag()
    rg.setInputCloud(cloud)
    rg.setInputNormals(normals)
    rg.setSearchMethod(None)
    rg.setNumberOfNeighbours(12)
    rg.setSmoothnessThreshold(math.radians(10.0))
    rg.setCurvatureThreshold(THR)
    rg.setMinClusterSize(2)
    rg.setMaxClusterSize(50)
    want = R.grow(cloud, normals, 12, R.smoothness_cos(math.radians(10.0)), THR, 2, 50)
    got = rg.extract()
    assert len(got) == want[0].size - 1 and all(c.dtype == np.int32 for c in got)
    assert np.array_equal(np.concatenate(got), want[1]) and [len(c) for c in got] == np.diff(want[0]).tolist()
    assert np.array_equal(rg.getLabels(), want[2])
    inside, outside = int(want[1][3]), int(np.flatnonzero(want[2] < 0)[0])
    assert np.array_equal(rg.getSegmentFromPoint(inside), got[want[2][inside]]) and rg.getSegmentFromPoint(outside).size == 0
    rg.setCurvatureTestFlag(False)
    assert np.array_equal(np.concatenate(rg.extract()), R.grow(cloud, normals, 12, R.smoothness_cos(math.radians(10.0)), math.inf, 2, 50)[1])
    with pytest.raises(IcpGpuError):
        RegionGrowing().extract()
    for call in (lambda: rg.setIndices([0]), lambda: rg.setSmoothModeFlag(False), lambda: rg.setResidualTestFlag(True)):
        with pytest.raises(IcpGpuError):
            call()
