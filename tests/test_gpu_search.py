"""The neighbour search on the device (icpgpu_search_set_input / _knn / _radius; icp_search.hip) against the NumPy restatement
(tests/search_restated.py), bit for bit everywhere: idx as int32, d2 as uint32, row_start as int64.  No tolerance anywhere."""
import functools
import math
import re

import numpy as np
import pytest

import search_restated as R
from icpslam_amd import Context, IcpGpuError, KdTree, _lib, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 2, "k-1", "k", "k+1", 63, 64, 65, 255, 256, 257, 1025, 3000)
KS = (1, 2, 8, 20, 63, 64)


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


_REF = {}


def ref(kind, key, cloud, queries, *args):
    """The restatement's answer, computed once per (cloud, queries, arguments); key = None: not worth keeping."""
    fn = R.knn if kind == "knn" else R.radius
    if key is None:
        return fn(cloud, queries, *args)
    k = (kind, key) + args
    if k not in _REF:
        _REF[k] = fn(cloud, queries, *args)
    return _REF[k]


def assert_same(got, want, what=""):
    for name, g, w in zip(("first", "idx", "d2"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, (what, name, bad[:8], g.reshape(-1)[bad[:8]], w.reshape(-1)[bad[:8]])


def check_knn(ctx, key, cloud, queries, k):
    idx, d2, n_found = ctx.search_knn(queries, k)
    widx, wd2, wn = ref("knn", key, cloud, queries, k)
    assert_same((n_found, idx, d2), (wn, widx, wd2), f"knn k={k}")
    return idx, d2, n_found


def check_radius(ctx, key, cloud, queries, radius, max_nn=0):
    got = ctx.search_radius(queries, radius, max_nn)
    want = ref("radius", key, cloud, queries, radius, max_nn)
    assert_same(got, want, f"radius {radius} max_nn={max_nn}")
    return got


def size_of(n, k):
    return {"k-1": k - 1, "k": k, "k+1": k + 1}.get(n, n)


# ---- sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_knn_sizes(ctx, n, k):
    n = size_of(n, k)
    cloud = scan(3000)[:n]
    ctx.search_set_input(cloud)
    assert ctx.search_size() == (n, n)
    idx, d2, n_found = check_knn(ctx, ("scan", n), cloud, None, k)
    assert (n_found == min(k, n)).all()
    if n:
        assert np.array_equal(idx[:, 0], np.arange(n)) and not d2[:, 0].any()  # a cloud point finds itself first


@pytest.mark.parametrize("n_q", [1, 3, 4, 5, 255, 256, 257])
def test_query_counts(ctx, n_q):
    cloud, queries = scan(1025), scan(300, 9)[:n_q]
    ctx.search_set_input(cloud)
    for k in (1, 20):
        check_knn(ctx, ("q", n_q), cloud, queries, k)
    for radius, max_nn in ((0.5, 0), (3.0, 0), (3.0, 70)):
        check_radius(ctx, ("q", n_q), cloud, queries, radius, max_nn)


def test_self_queries_equal_the_cloud_passed_explicitly(ctx):
    cloud = scan(1025).copy()
    cloud[[7, 700], 1] = np.nan
    ctx.search_set_input(cloud)
    assert ctx.search_size() == (1025, 1023)
    assert_same(ctx.search_knn(None, 20), ctx.search_knn(cloud, 20))
    assert_same(ctx.search_radius(None, 0.5), ctx.search_radius(cloud, 0.5))
    assert_same(ctx.search_radius(None, 5.0, 100), ctx.search_radius(cloud, 5.0, 100))
    check_knn(ctx, "self-nan", cloud, None, 20)


# ---- ties ----------------------------------------------------------------------------------------------------------------
def lattice(m):
    g = np.arange(m, dtype=F32)
    c = np.ones((m ** 3, 4), F32)
    c[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return c


def test_lattice_ties(ctx):
    """9 x 9 x 9 integer lattice: queried at its points, whole shells of candidates share one d2 (6 at 1, 12 at 2, 8 at 3, ...);
    queried at cell centres the 8 corners tie at 0.75.  The order inside every group of equals is the index order, and a list cut
    inside a group keeps its lowest indices.  The whole-key batch skip test meets exact ties with the kept worst here.  The strict
    form of the shell certificate (kept worst d2 < bound, not <=) needs no pin: an unseen point lies more than rho cells from the
    query's cell on some axis, and the float binning is exact to about 2^-9 of a cell, so it is farther than (rho - 2^-8) h -- a
    kept worst equal to (rho h 63/64)^2 cannot tie with it, and `<=` would certify the same answers.  (The certificate's two sides
    are pinned on clouds built on the grid itself: tests/test_gpu_grid_adversary.py.)"""
    cloud = lattice(9)
    rng = np.random.default_rng(3)
    cloud = cloud[rng.permutation(len(cloud))]  # (index order is not spatial order)
    centres = cloud[:200].copy()
    centres[:, :3] += F32(0.5)
    ctx.search_set_input(cloud)
    for k in (1, 2, 8, 20, 63, 64):
        check_knn(ctx, "lattice-self", cloud, None, k)
        check_knn(ctx, "lattice-centres", cloud, centres, k)
    inner = np.flatnonzero((np.abs(cloud[:, :3] - 4).max(axis=1) <= 3))[0]
    idx, d2, _ = ctx.search_knn(cloud[inner:inner + 1], 27)  # by hand, for an inner point
    assert d2[0].tolist() == [0.0] + [1.0] * 6 + [2.0] * 12 + [3.0] * 8
    for lo, hi in ((1, 7), (7, 19), (19, 27)):
        assert (np.diff(idx[0, lo:hi]) > 0).all()
    for radius, max_nn in ((1.0, 0), (math.sqrt(2.0), 0), (1.5, 0), (1.5, 4), (3.0, 0), (3.0, 65)):
        check_radius(ctx, "lattice-self", cloud, None, radius, max_nn)
        check_radius(ctx, "lattice-centres", cloud, centres, radius, max_nn)
    assert (np.diff(ctx.search_radius(None, 1.0)[0]) == 1).all()  # d2 == r2 is not a neighbour


@pytest.mark.parametrize("copies", [2, 70])
def test_duplicated_points(ctx, copies):
    """Every point `copies` times -- 70: more equal keys' distances than the list has lanes.  The lowest indices win."""
    base = scan(400 if copies == 2 else 40)
    for name, cloud in (("rep", np.repeat(base, copies, axis=0)), ("tile", np.tile(base, (copies, 1)))):
        ctx.search_set_input(cloud)
        for k in (1, 8, 63, 64):
            idx, d2, _ = check_knn(ctx, (name, copies), cloud, None, k)
            m = min(k, copies)
            assert not d2[:, :m].any()
        check_radius(ctx, (name, copies), cloud, None, 0.3)
        check_radius(ctx, (name, copies), cloud, None, 0.3, 64)
        check_radius(ctx, (name, copies), cloud, None, 2.0, 65)
    one = np.tile(F32([4.0, 5.0, -6.0, 1.0]), (70, 1))
    ctx.search_set_input(one)
    idx, d2, n_found = check_knn(ctx, "one-point", one, None, 64)
    assert (idx == np.arange(64)).all() and not d2.any()
    row_start, ridx, _ = check_radius(ctx, "one-point", one, None, 0.1, 0)
    assert (np.diff(row_start) == 70).all() and (ridx.reshape(70, 70) == np.arange(70)).all()


# ---- queries and points in odd places ------------------------------------------------------------------------------------
def test_queries_outside_the_box(ctx):
    cloud = scan(1025)
    lo, hi = cloud[:, :3].min(axis=0), cloud[:, :3].max(axis=0)
    mid = (lo + hi) / 2
    q = []
    for a in range(3):
        for side, off in ((lo, -0.01), (hi, 0.01), (lo, -1.5), (hi, 1.5)):
            p = mid.copy()
            p[a] = side[a] + off
            q.append(p)
    q += [hi + 0.5, lo - 0.5, hi + 30.0, mid + np.array([1000.0, 0, 0]), mid - np.array([0, 700.0, 700.0]), np.array([1e6, -1e6, 1e6])]
    queries = np.ones((len(q), 4), F32)
    queries[:, :3] = np.array(q, F32)
    ctx.search_set_input(cloud)
    for k in (1, 20, 64):
        check_knn(ctx, "outside", cloud, queries, k)
    for radius in (0.5, 2.0, 40.0, 1100.0):
        check_radius(ctx, "outside", cloud, queries, radius)
    check_radius(ctx, "outside", cloud, queries, 1100.0, 100)


def test_isolated_cloud_points(ctx):
    """Returns at 300 to 1 000 m: their own neighbours lie beyond the shells, and so do they for nobody: the far list."""
    cloud = scan(2000).copy()
    far = np.ones((5, 4), F32)
    far[:, :3] = F32([[300, 0, 0], [-450, 200, 5], [0, 700, -3], [600, -600, 40], [1000, 10, 0]])
    cloud = np.concatenate([cloud[:1000], far[:2], cloud[1000:], far[2:]])
    ctx.search_set_input(cloud)
    idx, d2, _ = check_knn(ctx, "isolated", cloud, None, 20)
    assert set(np.flatnonzero(d2[:, 1] > 1e4)) == {1000, 1001, 2002, 2003, 2004}
    check_radius(ctx, "isolated", cloud, None, 0.5)
    check_radius(ctx, "isolated", cloud, cloud[[1000, 2004, 5]], 500.0)


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
    grid refuses the cloud (ASSERTED, from the library's debug line).  Every query then sweeps the whole cloud.  The queries are
    128 explicit points, so that the restatement stays small."""
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    assert found and int(found[-1]) > 4096
    assert ctx.search_size() == (22000, 21999)
    queries = np.concatenate([cloud[:100], clustered(28, 2)])
    for k in (1, 20, 64):
        check_knn(ctx, "refused", cloud, queries, k)
    check_radius(ctx, "refused", cloud, queries, 0.3)
    check_radius(ctx, "refused", cloud, queries, 0.3, 8)
    check_radius(ctx, "refused", cloud, queries, 1.0, 100)


def test_non_finite_rows(ctx):
    """NaN / inf rows at the first, last and wave-boundary indices of the cloud never appear in any row; among the queries they find
    nothing."""
    cloud = scan(1025).copy()
    rows = [0, 63, 64, 65, 255, 256, 1024]
    for j, i in enumerate(rows):
        cloud[i, j % 3] = [np.nan, np.inf, -np.inf][j % 3]
    queries = scan(300, 9).copy()
    qrows = [0, 3, 4, 63, 64, 299]
    queries[qrows, 2] = np.nan
    ctx.search_set_input(cloud)
    assert ctx.search_size() == (1025, 1025 - len(rows))
    for q, key in ((None, "nan-self"), (queries, "nan-q")):
        for k in (8, 64):
            idx, d2, n_found = check_knn(ctx, key, cloud, q, k)
            assert not np.isin(idx, rows).any()
        for radius, max_nn in ((0.5, 0), (1e4, 0), (1e4, 1000)):
            row_start, ridx, _ = check_radius(ctx, key, cloud, q, radius, max_nn)
            assert not np.isin(ridx, rows).any()
    idx, d2, n_found = ctx.search_knn(queries, 8)
    assert not n_found[qrows].any() and (idx[qrows] == -1).all() and np.isinf(d2[qrows]).all()
    row_start = ctx.search_radius(queries, 1e4)[0]
    assert not np.diff(row_start)[qrows].any()


# ---- radius --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.0, 0.3, 0.5])
def test_radius_lidar_radii(ctx, radius):
    cloud = scan(3000)
    ctx.search_set_input(cloud)
    row_start, idx, d2 = check_radius(ctx, ("scan", 3000), cloud, None, radius)
    assert (row_start[-1] == 0) == (radius == 0.0)


@pytest.mark.parametrize("max_nn", [0, 1, 8, 64, 65, 1000])
def test_radius_max_nn(ctx, max_nn):
    """A radius that holds the whole cloud (every row is n_finite entries, sorted: the long-row path) and a LIDAR radius, cut at
    max_nn on either side of the 64-entry boundary."""
    cloud = scan(1025).copy()
    cloud[[5, 900], 0] = np.nan
    ctx.search_set_input(cloud)
    row_start, idx, d2 = check_radius(ctx, "whole", cloud, None, 1e4, max_nn)
    lens = np.diff(row_start)
    assert (lens[[5, 900]] == 0).all() and (np.delete(lens, [5, 900]) == (min(max_nn, 1023) if max_nn else 1023)).all()
    for radius in (0.5, 2.0):
        check_radius(ctx, "whole", cloud, None, radius, max_nn)


def test_radius_two_call_protocol(ctx):
    cloud = scan(1025)
    ctx.search_set_input(cloud)
    want = ref("radius", ("own", 1025), cloud, None, 0.5, 0)
    total = len(want[1])
    assert total > 1025
    for capacity in (0, total - 1):
        rc, row_start, idx, d2, n_total = ctx.search_radius_raw(None, 0.5, 0, capacity)
        assert rc == _lib.ERR_INVALID_ARG and n_total == total
        assert np.array_equal(row_start, want[0])           # row_start and n_total are written ...
        assert (idx == -2).all() and np.isnan(d2).all()     # ... and nothing else
    rc, row_start, idx, d2, n_total = ctx.search_radius_raw(None, 0.5, 0, total)  # capacity exactly n_total
    assert rc == 0 and n_total == total
    assert_same((row_start, idx, d2), want)
    rc, row_start, idx, d2, n_total = ctx.search_radius_raw(None, 0.5, 0, total + 5)
    assert rc == 0 and (idx[total:] == -2).all()
    assert_same((row_start, idx[:total], d2[:total]), want)
    rc, row_start, idx, d2, n_total = ctx.search_radius_raw(None, 0.0, 0, 0)  # nothing to deliver
    assert rc == 0 and n_total == 0 and not row_start.any()


# ---- cross-checks against what the library already has -------------------------------------------------------------------
def test_k1_equals_icpgpu_nn(ctx):
    cloud, queries = scan(3000), scan(1025, 9).copy()
    queries[17, 0] = np.nan
    ctx.set_source(queries)
    ctx.set_target(cloud)
    nn_idx, nn_d2 = ctx.nn(np.eye(4))
    ctx.search_set_input(cloud)
    idx, d2, _ = ctx.search_knn(queries, 1)
    answered = nn_idx >= 0
    assert answered.sum() > 100 and not answered[17]
    assert np.array_equal(idx[answered, 0], nn_idx[answered])
    assert np.array_equal(d2[answered, 0].view(np.uint32), nn_d2[answered].view(np.uint32))
    assert idx[17, 0] == -1


@pytest.mark.parametrize("mean_k", [1, 19, 63])
def test_statistical_filter_measure_from_knn(ctx, mean_k):
    """icpgpu.h's mean-distance formula applied to search_knn(NULL, mean_k + 1)'s d2."""
    cloud = scan(3000)
    ctx.statistical_outlier_removal(cloud, mean_k, 1.0)
    measure = ctx.outlier_fetch()["measure"]
    ctx.search_set_input(cloud)
    _, d2, _ = ctx.search_knn(None, mean_k + 1)
    roots = np.sqrt(d2[:, 1:])  # (float32 in, float32 out: correctly rounded)
    want = np.empty(len(cloud), F32)
    for i, row in enumerate(roots.tolist()):
        s = 0.0
        for v in row:
            s += v
        want[i] = F32(s / float(mean_k))
    assert np.array_equal(measure.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("radius", [0.3, 2.0])
def test_radius_filter_counts_are_the_row_lengths(ctx, radius):
    cloud = scan(3000).copy()
    cloud[[0, 77], 2] = np.inf
    ctx.radius_outlier_removal(cloud, radius, 5)
    k = ctx.outlier_fetch()["measure"]
    ctx.search_set_input(cloud)
    row_start = ctx.search_radius(None, radius, 0)[0]
    assert np.array_equal(np.diff(row_start).astype(F32), k)


# ---- the mirror class, refusals ------------------------------------------------------------------------------------------
def test_kdtree_class(ctx):
    cloud = scan(1025)
    tree = KdTree()
    tree.setInputCloud(cloud)
    widx, wd2, _ = ref("knn", ("own", 1025), cloud, None, 8)
    idx, d2 = tree.nearestKSearch(cloud[40, :3], 8)
    assert np.array_equal(idx, widx[40]) and np.array_equal(d2, wd2[40])
    idx, d2 = tree.nearestKSearch(40, 8)  # by index
    assert np.array_equal(idx, widx[40]) and np.array_equal(d2, wd2[40])
    want = ref("radius", ("own", 1025), cloud, None, 0.5, 0)
    idx, d2 = tree.radiusSearch(40, 0.5)
    a, b = want[0][40], want[0][41]
    assert np.array_equal(idx, want[1][a:b]) and np.array_equal(d2, want[2][a:b])
    idx, d2 = tree.radiusSearch(cloud[40], 0.5, 3)
    assert np.array_equal(idx, want[1][a:a + 3])
    assert_same(tree.radiusSearchBatch(None, 0.5), want)
    assert_same(tree.nearestKSearchBatch(None, 8), (widx, wd2, np.full(1025, 8, np.int32)))
    short = KdTree()
    short.setInputCloud(cloud[:3])
    assert len(short.nearestKSearch(0, 10)[0]) == 3  # fewer than k: a short list, as in PCL


def test_empty_cloud_and_no_queries(ctx):
    ctx.search_set_input(np.empty((0, 4), F32))
    assert ctx.search_size() == (0, 0)
    idx, d2, n_found = ctx.search_knn(scan(64), 5)
    assert (idx == -1).all() and np.isinf(d2).all() and not n_found.any()
    assert not ctx.search_radius(scan(64), 10.0)[0].any()
    assert ctx.search_knn(None, 5)[0].shape == (0, 5)  # n_q = 0
    ctx.search_set_input(scan(64))
    assert ctx.search_knn(np.empty((0, 4), F32), 5)[0].shape == (0, 5)
    assert ctx.search_radius(np.empty((0, 4), F32), 1.0)[0].tolist() == [0]


def test_refusals_leave_the_search_cloud_usable():
    cloud = scan(255)
    with Context(0) as c:
        for call in (lambda: c.search_knn(cloud, 1), lambda: c.search_radius(cloud, 1.0), lambda: c.search_size()):  # no search cloud
            with pytest.raises(IcpGpuError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARG
        c.search_set_input(cloud)
        calls = [lambda: c.search_knn(None, 0), lambda: c.search_knn(None, 65), lambda: c.search_knn(cloud, -3),
                 lambda: c.search_radius(None, -0.1), lambda: c.search_radius(None, float("nan")), lambda: c.search_radius(None, float("inf")),
                 lambda: c.search_radius(None, 0.3, -1), lambda: c.search_knn(None, 5, n_q=254), lambda: c.search_knn(None, 5, n_q=256),
                 lambda: c.search_radius(None, 0.3, 0, n_q=7)]
        for call in calls:
            with pytest.raises(IcpGpuError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARG
            check_knn(c, ("own", 255), cloud, None, 8)  # the search cloud is still there and answers as before
        check_radius(c, ("own", 255), cloud, None, 0.3)
