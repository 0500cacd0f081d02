"""Euclidean clustering on the device (icpgpu_euclidean_cluster_extraction / icpgpu_cluster_fetch; icp_cluster.hip) against the NumPy
restatement (tests/cluster_restated.py), bit for bit everywhere: cluster_start as int64, indices, labels and component as int32.  The
answer is a partition of integers: there is no tolerance anywhere."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import cluster_restated as R
from icpslam_amd import Context, EuclideanClusterExtraction, IcpGpuError, _lib, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
INT_MAX = 2**31 - 1
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 3000)
TOLERANCES = (0.25, 0.5, 1.0, 2.0)
WINDOWS = ((1, INT_MAX), (2, 50), (5, 5))
NAMES = ("cluster_start", "indices", "labels", "component")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "cluster_2k.npz")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def points(xyz) -> np.ndarray:
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = np.asarray(xyz, np.float64).reshape(-1, 3).astype(F32)
    return c


def shuffled(cloud, seed):
    """(the cloud with its indices shuffled by a fixed seed, order): order[k] = the new index of point k."""
    order = np.random.default_rng(seed).permutation(len(cloud))
    out = np.empty_like(cloud)
    out[order] = cloud
    return out, order


_REF = {}


def ref_components(key, cloud, tolerance):
    """The restatement's components, computed once per (cloud, tolerance) and left unchanged; key = None: not worth keeping."""
    if key is None:
        return R.components(cloud, tolerance)
    k = (key, tolerance)
    if k not in _REF:
        _REF[k] = R.components(cloud, tolerance)
        _REF[k].setflags(write=False)
    return _REF[k]


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


def check(ctx, key, cloud, tolerance, lo=1, hi=INT_MAX):
    """One clustering call on the search cloud in place against the restatement."""
    got = ctx.euclidean_cluster_extraction(tolerance, lo, hi)
    want = R.from_components(ref_components(key, cloud, tolerance), lo, hi)
    assert_same(got, want, f"tolerance {tolerance} window {lo} .. {hi}")
    return got


# ---- sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tolerance", TOLERANCES)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n, tolerance):
    cloud = scan(3000)[:n]
    ctx.search_set_input(cloud)
    for lo, hi in WINDOWS:
        start, indices, labels, component = check(ctx, ("scan", n), cloud, tolerance, lo, hi)
        assert start[0] == 0 and start[-1] == indices.size == (labels >= 0).sum()
    if n == 3000:  # (what makes these cases worth their time: hundreds of tied components, a window that cuts on both sides)
        sizes = np.unique(component, return_counts=True)[1]
        assert (sizes.size, int(sizes.max())) == {0.25: (931, 38), 0.5: (332, 1454), 1.0: (94, 2595), 2.0: (31, 2856)}[tolerance]


# ---- shapes whose diameter is their size -----------------------------------------------------------------------------------
def chain(n, tolerance, y=0.0):
    return points(np.stack([np.arange(n) * (0.9 * tolerance), np.full(n, y), np.zeros(n)], -1))


def test_chain_against_the_restatement(ctx):
    cloud, _ = shuffled(chain(3000, 0.5), 21)
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, 0.5)
    assert start.tolist() == [0, 3000] and not component.any()
    check(ctx, None, cloud, 0.44)  # below the spacing: 3000 singletons, in index order


def test_long_chain_is_one_component_named_zero(ctx):
    """20 000 points in a line, 0.45 m apart, the indices shuffled: a graph of diameter 19 999.  The answer is known by construction.
    That this finishes in the time every test gets is the check that the number of launches does not grow with the diameter."""
    n = 20000
    cloud, _ = shuffled(chain(n, 0.5), 22)
    ctx.search_set_input(cloud)
    start, indices, labels, component = ctx.euclidean_cluster_extraction(0.5)
    assert start.dtype == np.int64 and start.tolist() == [0, n]
    assert indices.dtype == np.int32 and np.array_equal(indices, np.arange(n))
    assert labels.dtype == component.dtype == np.int32 and not labels.any() and not component.any()


def test_two_parallel_chains_with_interleaved_indices_stay_two(ctx):
    """Even indices on one line, odd ones on a line 1.01 tolerances beside it: every point's index neighbours are in the other chain."""
    m, tol = 1000, 0.5
    cloud = np.empty((2 * m, 4), F32)
    order = np.random.default_rng(23).permutation(m)
    cloud[0::2] = chain(m, tol)[order]
    cloud[1::2] = chain(m, tol, 1.01 * tol)[order[::-1]]
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, tol)
    assert start.tolist() == [0, m, 2 * m] and np.array_equal(component, np.arange(2 * m) % 2)
    assert np.array_equal(indices[:m], np.arange(0, 2 * m, 2)) and np.array_equal(indices[m:], np.arange(1, 2 * m, 2))


def test_comb(ctx):
    """Many short teeth joined by one spine, and a second comb whose spine has a gap: 1 + 2 components, each tooth reached through
    the spine alone."""
    tol, step = 0.5, 0.45
    xyz = []
    for x0, gap in ((0.0, None), (1000.0, 150)):
        for k in range(300):
            if k == gap:
                continue
            xyz.append([x0 + k * step, 0, 0])
            if k % 3 == 0:
                xyz += [[x0 + k * step, t * step, 0] for t in range(1, 6)]
    cloud, order = shuffled(points(xyz), 24)
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, tol)
    assert start.size - 1 == 3 and start[-1] == len(cloud)
    assert component[order[0]] == component[order[799]] and len(set(component.tolist())) == 3


# ---- wave and tile boundaries of the ordering ------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257])
def test_exactly_m_emitted_clusters(ctx, m):
    """m isolated pairs and 40 single points: with the window 2 .. 2 exactly m clusters come out, all tied, by lowest index."""
    xyz = [[10.0 * k, 0, 0] for k in range(m)] + [[10.0 * k + 0.1, 0, 0] for k in range(m)] + [[10.0 * k, 50, 0] for k in range(40)]
    cloud, _ = shuffled(points(xyz), 100 + m)
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, 0.5, 2, 2)
    assert np.array_equal(start, 2 * np.arange(m + 1)) and (np.diff(indices[0::2]) > 0).all()
    start, _, _, _ = check(ctx, None, cloud, 0.5)
    assert start.size - 1 == m + 40


def test_clusters_of_exactly_64_and_65_points(ctx):
    xyz = [[0.1 * k, 0, 0] for k in range(64)] + [[100 + 0.1 * k, 0, 0] for k in range(65)] + [[0.1 * k, 80, 0] for k in range(63)]
    xyz += [[10.0 * k, -50, 0] for k in range(30)]
    cloud, order = shuffled(points(xyz), 25)
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, 0.5)
    assert start[:4].tolist() == [0, 65, 129, 192] and start.size - 1 == 33
    assert labels[order[64]] == 0 and labels[order[0]] == 1 and labels[order[129]] == 2
    start, _, _, _ = check(ctx, None, cloud, 0.5, 64, 64)
    assert start.tolist() == [0, 64]


# ---- without the grid ------------------------------------------------------------------------------------------------------
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
    grid refuses the cloud (ASSERTED, from the library's debug line).  Every point then sweeps the whole cloud."""
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    assert found and int(found[-1]) > 4096
    start, indices, labels, component = check(ctx, "refused", cloud, 0.05)
    assert start.size - 1 > 2000 and start[1] - start[0] > 100 and component[7] == -1
    check(ctx, "refused", cloud, 0.05, 3, 40)


def test_tolerance_of_more_cells_than_the_cube_walk_takes(ctx, monkeypatch, capfd):
    """n = 1025 in three groups 400 m apart and a tolerance of 9.5 cells (ASSERTED, from the cell size in the library's debug line):
    more than the 8 shells the radius walk takes, so every point sweeps the whole cloud."""
    cloud = scan(1025).copy()
    cloud[:100, 0] += F32(400)
    cloud[100:150, 1] -= F32(400)
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=1025 .* h=([0-9.]+) ", capfd.readouterr().err)
    assert found
    tolerance = 9.5 * float(found[-1])
    assert math.ceil(tolerance / (float(found[-1]) * 63 / 64)) > 8 and tolerance < 300
    start, _, _, component = check(ctx, None, cloud, tolerance)
    assert start.size - 1 >= 3 and len({int(component[0]), int(component[100]), int(component[150])}) == 3


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------
def test_non_finite_rows(ctx):
    cloud = scan(1025).copy()
    cloud[[0, 7, 64, 700, 1024], [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
    ctx.search_set_input(cloud)
    for tolerance in (0.5, 2.0):
        for lo, hi in WINDOWS:
            _, _, labels, component = check(ctx, "nonfinite", cloud, tolerance, lo, hi)
            assert (component[[0, 7, 64, 700, 1024]] == -1).all() and (labels[[0, 7, 64, 700, 1024]] == -1).all()
    assert (component >= 0).sum() == 1020 and component[1] == 1  # the lowest FINITE index names the first component


def test_a_nan_point_does_not_bridge(ctx):
    cloud = points([[0, 0, 0], [0.4, 0, 0], [0.8, 0, 0], [1.2, 0, 0], [1.6, 0, 0]])
    cloud[2, 1] = np.nan
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, 0.5)
    assert start.tolist() == [0, 2, 4] and indices.tolist() == [0, 1, 3, 4] and component.tolist() == [0, 0, -1, 3, 3]


def test_all_points_coincident(ctx):
    cloud = np.tile(np.array([[3.0, -2.0, 0.5, 1.0]], F32), (300, 1))
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, 1e-6)
    assert start.tolist() == [0, 300] and not component.any()
    start, _, _, _ = check(ctx, None, cloud, 0.0)  # tolerance 0: r2 = 0 and d2 = 0 is not below it
    assert start.tolist() == list(range(301))


def test_all_nan_and_empty_clouds(ctx):
    for cloud in (np.full((130, 4), np.nan, F32), np.empty((0, 4), F32)):
        ctx.search_set_input(cloud)
        start, indices, labels, component = check(ctx, None, cloud, 0.5)
        assert start.tolist() == [0] and indices.size == 0 and labels.tolist() == component.tolist() == [-1] * len(cloud)


def test_tolerance_zero_makes_every_finite_point_its_own_cluster(ctx):
    cloud = scan(257).copy()
    cloud[100, 0] = np.nan
    ctx.search_set_input(cloud)
    start, indices, labels, component = check(ctx, None, cloud, 0.0)
    assert start.size - 1 == 256 and np.array_equal(indices, np.delete(np.arange(257), 100))
    assert check(ctx, None, cloud, 0.0, 2, INT_MAX)[0].tolist() == [0]


def test_the_lattice_at_and_just_above_the_tolerance(ctx):
    g = np.arange(4, dtype=F32) * F32(0.5)
    cloud = points(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    ctx.search_set_input(cloud)
    assert check(ctx, None, cloud, 0.5)[0].tolist() == list(range(65))  # d2 == r2: strict, 64 singletons
    assert check(ctx, None, cloud, float(np.nextafter(F32(0.5), F32(1))))[0].tolist() == [0, 64]


# ---- the device's own radius rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tolerance", [0.5, 1.0])
def test_host_union_find_over_the_devices_radius_rows(ctx, tolerance):
    cloud = scan(3000)
    ctx.search_set_input(cloud)
    row_start, idx, _ = ctx.search_radius(None, tolerance)
    component = ctx.euclidean_cluster_extraction(tolerance)[3]
    assert np.array_equal(component, R.components(cloud, tolerance, rows=(cloud, row_start, idx)))


# ---- refusals and the fetch ------------------------------------------------------------------------------------------------
def refused(call):
    with pytest.raises(IcpGpuError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID_ARG


def test_refusals():
    with Context(0) as c:
        refused(lambda: c.euclidean_cluster_extraction(0.5))                      # no search cloud
        assert c.cluster_fetch_raw(0, 0)[0] == _lib.ERR_INVALID_ARG               # ... and no result
        c.search_set_input(scan(257))
        assert c.cluster_fetch_raw(300, 300)[0] == _lib.ERR_INVALID_ARG           # a cloud, no result yet
        for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
            refused(lambda: c.euclidean_cluster_extraction(bad))
        n = C.c_size_t(7)
        for a, b in ((None, C.byref(n)), (C.byref(n), None), (None, None)):       # null count pointers
            assert c._L.icpgpu_euclidean_cluster_extraction(c._h, 0.5, 1, INT_MAX, a, b) == _lib.ERR_INVALID_ARG
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 1, INT_MAX)
        assert rc == 0 and n_clusters > 1 and n_clustered == 257
        refused(lambda: c.euclidean_cluster_extraction(float("nan")))             # a refused call leaves no result behind
        assert c.cluster_fetch_raw(n_clusters, n_clustered)[0] == _lib.ERR_INVALID_ARG
        assert c.cluster_extract_raw(0.5, 1, INT_MAX) == (0, n_clusters, n_clustered)
        assert c._L.icpgpu_cluster_fetch(c._h, n_clusters, n_clustered, None, None, None, None) == _lib.ERR_INVALID_ARG  # null cluster_start
        assert c.cluster_fetch_raw(n_clusters, n_clustered)[0] == 0


def test_fetch_twice_and_capacities_one_too_small(ctx):
    cloud = scan(1025)
    ctx.search_set_input(cloud)
    want = R.from_components(ref_components("scan1025", cloud, 0.5), 2, 50)
    rc, n_clusters, n_clustered = ctx.cluster_extract_raw(0.5, 2, 50)
    assert (rc, n_clusters, n_clustered) == (0, want[0].size - 1, want[1].size) and n_clusters > 1
    for cap_c, cap_i in ((n_clusters - 1, n_clustered), (n_clusters, n_clustered - 1), (0, 0)):
        rc, *arrays = ctx.cluster_fetch_raw(cap_c, cap_i)
        assert rc == _lib.ERR_INVALID_ARG and all((a == -2).all() for a in arrays)  # nothing was written
    for _ in range(2):
        rc, *arrays = ctx.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0
        assert_same(arrays, want)
    rc, start, indices, labels, component = ctx.cluster_fetch_raw(n_clusters + 5, n_clustered + 9, want_labels=False, want_component=False)
    assert rc == 0 and labels is None and component is None                       # room to spare, the optional arrays left out
    assert np.array_equal(start[:n_clusters + 1], want[0]) and (start[n_clusters + 1:] == -2).all()
    assert np.array_equal(indices[:n_clustered], want[1]) and (indices[n_clustered:] == -2).all()


def test_five_calls_give_identical_bytes(ctx):
    cloud = scan(3000)
    ctx.search_set_input(cloud)
    for tolerance, lo, hi in ((0.5, 1, INT_MAX), (0.25, 2, 50)):
        runs = [b"".join(a.tobytes() for a in ctx.euclidean_cluster_extraction(tolerance, lo, hi)) for _ in range(5)]
        assert len(set(runs)) == 1


# ---- the golden fixture and the PCL-shaped class ---------------------------------------------------------------------------
def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    got = ctx.euclidean_cluster_extraction(float(g["tolerance"]), int(g["min_size"]), int(g["max_size"]))
    assert_same(got, [g[name] for name in NAMES])


def test_pcl_shaped_class(ctx):
    cloud = scan(1025)
    want = R.from_components(ref_components("scan1025", cloud, 0.5), 2, 50)
    ec = EuclideanClusterExtraction()
    assert (ec.getClusterTolerance(), ec.getMinClusterSize(), ec.getMaxClusterSize()) == (0.0, 1, INT_MAX)
    ec.setInputCloud(cloud)
    ec.setSearchMethod(None)
    ec.setClusterTolerance(0.5)
    ec.setMinClusterSize(2)
    ec.setMaxClusterSize(50)
    assert (ec.getClusterTolerance(), ec.getMinClusterSize(), ec.getMaxClusterSize()) == (0.5, 2, 50)
    got = ec.extract()
    assert len(got) == want[0].size - 1 and all(c.dtype == np.int32 for c in got)
    assert np.array_equal(np.concatenate(got), want[1]) and [len(c) for c in got] == np.diff(want[0]).tolist()
    assert np.array_equal(ec.getLabels(), want[2])
    with pytest.raises(IcpGpuError):
        EuclideanClusterExtraction().extract()
