"""The fast point feature histograms on the device (icpgpu_fpfh_estimation; icp_fpfh.hip over icp_search.hip's rows) against the
NumPy restatement (tests/fpfh_restated.py), bit for bit everywhere: FPFH and SPFH as uint32, counts as int32.  No tolerance
anywhere."""
import functools
import os
import re

import numpy as np
import pytest

import fpfh_restated as R
import normals_restated as N
from icpslam_amd import FPFH_BINS, Context, FPFHEstimation, IcpGpuError, _lib, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 3, 63, 64, 65, 257, 2000)
KS = (2, 3, 10, 33, 64)


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def scan_normals(n: int, seed: int = 5) -> np.ndarray:
    """The restatement's k = 10 normals of scan(2000)[:n] (NaN where fewer than three points exist)."""
    nrm = N.estimate(scan(2000, seed)[:n], None, k=10)[0]
    nrm.setflags(write=False)
    return nrm


def random_normals(n: int, seed: int) -> np.ndarray:
    v = np.random.default_rng(seed).normal(size=(n, 4)).astype(F32)
    v[:, :3] /= np.linalg.norm(v[:, :3], axis=1, keepdims=True).astype(F32)
    return v


_REF = {}


def ref(key, cloud, normals, queries, mode):
    """The restatement's answer, computed once per (cloud, normals, queries, arguments); key = None: not worth keeping."""
    if key is None:
        return R.estimate(cloud, normals, queries, **mode)
    k = (key,) + tuple(sorted(mode.items()))
    if k not in _REF:
        _REF[k] = R.estimate(cloud, normals, queries, **mode)
    return _REF[k]


def assert_same(got, want, what=""):
    for name, g, w in zip(("fpfh", "counts", "spfh"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if g.size else np.zeros(0, int)
        assert bad.size == 0, (what, name, bad.size, bad[:6], g[bad[:2]], w[bad[:2]])


def check(ctx, key, cloud, normals, queries, **mode):
    got = ctx.fpfh_estimation(normals, queries, want_spfh=True, **mode)
    assert_same(got, ref(key, cloud, normals, queries, mode), f"{key} {mode}")
    return got


def grid_cell(err: str) -> float:
    found = re.findall(r"\[icpgpu\] grid n=\d+ .* h=([0-9.]+) ", err)
    assert found
    return float(found[-1])


# ---- sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_k_sizes(ctx, n, k):
    cloud, normals = scan(2000)[:n], (scan_normals(n) if n >= 3 else random_normals(n, n))
    ctx.search_set_input(cloud)
    fpfh, counts, spfh = check(ctx, ("scan", n), cloud, normals, None, k=k)
    m = min(k, n)
    assert (counts == m).all() and fpfh.shape == (n, FPFH_BINS)
    if n == 1:
        assert not fpfh.any() and not spfh.any()
    if n >= 63:
        assert np.isfinite(fpfh).all() and fpfh.any(axis=1).all()


# ---- radius ---------------------------------------------------------------------------------------------------------------
def test_radius_rows_of_every_length(ctx, monkeypatch, capfd):
    """A strip of 400 collinear points 1 cm apart plus far points, with queries on and off it: radius rows of exactly 0, 1, 63, 64 and
    65 entries (asserted), rows of several hundred, longer than a wave's pass of 64 in each kernel -- the cloud's own rows feed the
    SPFH kernel, the queries' the FPFH kernel -- from the grid's cube, and from the sweep without the grid (more than 8 shells)."""
    strip = np.ones((400, 4), F32)
    strip[:, 0] = np.arange(400, dtype=F32) * F32(0.01)
    strip[:, 1] = F32(0.002) * (np.arange(400) % 3).astype(F32)  # (not exactly collinear: v is not zero everywhere)
    far = np.ones((40, 4), F32)
    far[:, :3] = F32([50, 50, 50]) + F32(1.2) * np.arange(40, dtype=F32)[:, None]
    cloud = np.concatenate([strip, far, scan(600)])
    cloud[:400, 2] += F32(30.0)
    normals = random_normals(len(cloud), 7)
    lone = cloud[400:402].copy()
    lone[1, 2] += F32(1000.0)  # a query with nothing around it
    queries = np.concatenate([cloud[:400:7], lone, cloud[440:500]])
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    h = grid_cell(capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    want = set()
    for r in (0.3155, 0.3205, 0.3255):  # 31.5, 32, 32.5 spacings either side: 63 / 64 / 65 entries in the strip's middle
        _, counts, _ = check(ctx, "strip-q", cloud, normals, queries, radius=r)
        own = check(ctx, "strip-own", cloud, normals, None, radius=r)[1]
        want |= set(counts.tolist()) | set(own.tolist())
    assert {0, 1, 63, 64, 65} <= want, sorted(want)
    big = max(2.5, round(8.5 * h, 2))
    assert np.ceil(0.3255 / (h * 63 / 64)) <= 8 < np.ceil(big / (h * 63 / 64)), h
    _, counts, _ = check(ctx, "strip-q", cloud, normals, queries, radius=big)
    own = check(ctx, "strip-own", cloud, normals, None, radius=big)[1]
    assert counts.max() > 300 and own.max() > 300
    _, counts, _ = check(ctx, "strip-q", cloud, normals, queries, radius=1.0)
    assert 128 < counts.max() and np.ceil(1.0 / (h * 63 / 64)) <= 8


# ---- queries ---------------------------------------------------------------------------------------------------------------
def test_queries_equal_disjoint_and_coincident(ctx):
    cloud, normals = scan(2000), scan_normals(2000)
    ctx.search_set_input(cloud)
    disjoint = scan(300, 9)
    mixed = np.concatenate([cloud[5:40], disjoint[:40], cloud[1990:]])  # some coincide with cloud points: their d2 = 0 entry is skipped
    for mode in (dict(k=10), dict(k=64), dict(radius=0.5)):
        own = check(ctx, "q-own", cloud, normals, None, **mode)
        same = check(ctx, "q-same", cloud, normals, cloud, **mode)
        assert_same(own, same)
        check(ctx, "q-disjoint", cloud, normals, disjoint, **mode)
        check(ctx, "q-mixed", cloud, normals, mixed, **mode)


@pytest.mark.parametrize("copies", [2, 70])
def test_duplicated_points(ctx, copies):
    base = scan(300 if copies == 2 else 30)
    for name, cloud in (("rep", np.repeat(base, copies, axis=0)), ("tile", np.tile(base, (copies, 1)))):
        normals = random_normals(len(cloud), copies)
        ctx.search_set_input(cloud)
        for mode in (dict(k=8), dict(k=64), dict(radius=0.3), dict(radius=2.0))[:4 if copies == 2 else 3]:
            fpfh, _, _ = check(ctx, (name, copies), cloud, normals, None, **mode)
            assert np.isfinite(fpfh).all()
    one = np.tile(F32([4.0, 5.0, -6.0, 1.0]), (70, 1))  # rows of only coincident entries: zeros
    ctx.search_set_input(one)
    for mode in (dict(k=10), dict(radius=0.1)):
        fpfh, counts, spfh = check(ctx, "one-point", one, random_normals(70, 1), None, **mode)
        assert not fpfh.any() and not spfh.any() and (counts == (10 if "k" in mode else 70)).all()


def lattice(m):
    g = np.arange(m, dtype=F32)
    c = np.ones((m ** 3, 4), F32)
    c[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return c


def test_lattice_ties(ctx):
    """9 x 9 x 9 integer lattice in a shuffled order: whole shells of neighbours share one d2, so the rows' order -- and with it
    the order of the float32 sums -- is the index order.  Axis normals put pairs exactly on bin edges and on |a1| == |a2|."""
    cloud = lattice(9)
    cloud = cloud[np.random.default_rng(3).permutation(len(cloud))]
    centres = cloud[:200].copy()
    centres[:, :3] += F32(0.5)
    axis = np.zeros((len(cloud), 4), F32)
    axis[np.arange(len(cloud)), np.random.default_rng(4).integers(0, 3, len(cloud))] = 1
    axis[::2] *= -1
    ctx.search_set_input(cloud)
    for name, normals in (("lattice-axis", axis), ("lattice-rand", random_normals(len(cloud), 5))):
        for mode in (dict(k=7), dict(k=27), dict(k=64), dict(radius=1.0), dict(radius=1.5), dict(radius=3.0)):
            check(ctx, name + "-self", cloud, normals, None, **mode)
            check(ctx, name + "-centres", cloud, normals, centres, **mode)
    plane = cloud[cloud[:, 2] == 4].copy()
    up = np.tile(F32([0, 0, 1, 0]), (len(plane), 1))
    ctx.search_set_input(plane)
    fpfh, _, spfh = check(ctx, "lattice-plane", plane, up, None, k=9)
    hand = np.zeros(FPFH_BINS, F32)
    hand[[5, 16, 27]] = 100
    assert np.array_equal(fpfh, np.tile(hand, (len(plane), 1))) and np.array_equal(spfh, np.tile(hand, (len(plane), 1)))


# ---- non-finite input -----------------------------------------------------------------------------------------------------
def test_nan_rows_queries_and_normals(ctx):
    cloud = scan(2000).copy()
    rows = [0, 63, 64, 65, 255, 256, 1999]
    for j, i in enumerate(rows):
        cloud[i, j % 3] = [np.nan, np.inf, -np.inf][j % 3]
    normals = scan_normals(2000).copy()
    nrows = [1, 62, 66, 700, 1998]
    for j, i in enumerate(nrows):
        normals[i, j % 3] = [np.nan, np.inf, -np.inf][j % 3]
    queries = scan(300, 9).copy()
    qrows = [0, 3, 4, 63, 64, 299]
    queries[qrows, 2] = np.nan
    queries[12, :3] = F32([1e6, -1e6, 1e6])
    ctx.search_set_input(cloud)
    for mode in (dict(k=8), dict(k=64), dict(radius=0.5)):
        fpfh, counts, spfh = check(ctx, "nan-q", cloud, normals, queries, **mode)
        assert not counts[qrows].any() and np.isnan(fpfh[qrows]).all() and np.isfinite(np.delete(fpfh, qrows, axis=0)).all()
        assert not spfh[rows].any() and not spfh[nrows].any()
        fpfh, counts, _ = check(ctx, "nan-own", cloud, normals, None, **mode)
        assert not counts[rows].any() and np.isnan(fpfh[rows]).all()
    all_nan = np.full_like(normals, np.nan)
    fpfh, _, spfh = check(ctx, "nan-all", cloud, all_nan, queries, k=8)
    assert not spfh.any() and not np.delete(fpfh, qrows, axis=0).any()


def test_subnormal_d2(ctx):
    """Two points 1e-20 apart: d2 = 1e-40 is subnormal, 1 / d2 is +inf, inf * 0 is NaN -- nothing is special-cased, and the
    restatement yields the same bits.  A second pair 1e-19 apart (d2 = 1e-38, normal) stays finite."""
    cloud = scan(257).copy()
    cloud[1] = cloud[0]
    cloud[1, 0] = cloud[0, 0] = F32(0)
    cloud[1, 1] = cloud[0, 1] = F32(0)
    cloud[0, 2], cloud[1, 2] = F32(0), F32(1e-20)
    cloud[3] = F32([5, 0, 0, 1])
    cloud[2] = F32([5, 0, 2e-19, 1])
    normals = random_normals(257, 3)
    ctx.search_set_input(cloud)
    d2 = ctx.search_knn(cloud[:1], 2)[1][0, 1]
    assert 0 < d2 < np.finfo(F32).tiny
    for mode in (dict(k=5), dict(radius=0.5)):
        fpfh, _, _ = check(ctx, "subnormal", cloud, normals, None, **mode)
        assert np.isnan(fpfh[0]).any() and np.isfinite(fpfh[4:]).all()


def test_fewer_than_two_finite_points_and_an_empty_cloud(ctx):
    cloud = scan(64)[:5].copy()
    cloud[[1, 3, 4], 0] = np.nan
    normals = random_normals(5, 1)
    ctx.search_set_input(cloud)
    for mode in (dict(k=20), dict(radius=100.0)):
        fpfh, counts, spfh = check(ctx, "two-finite", cloud, normals, None, **mode)
        assert counts.tolist() == [2, 0, 2, 0, 0] and spfh[[0, 2]].any(axis=1).all()
        check(ctx, "two-finite-q", cloud, normals, scan(64, 9), **mode)
    cloud[2, 1] = np.inf
    ctx.search_set_input(cloud)
    fpfh, counts, spfh = check(ctx, "one-finite", cloud, normals, None, k=2)
    assert counts.tolist() == [1, 0, 0, 0, 0] and not spfh.any() and not fpfh[0].any()
    ctx.search_set_input(np.empty((0, 4), F32))
    for mode in (dict(k=5), dict(radius=5.0)):
        fpfh, counts, spfh = ctx.fpfh_estimation(None, scan(64), want_spfh=True, **mode)
        assert not counts.any() and not fpfh.any() and spfh.shape == (0, FPFH_BINS)


# ---- a cloud the grid refuses ---------------------------------------------------------------------------------------------
def clustered(n, seed):
    """The cloud tests/test_gpu_search.py builds for it: tight clusters (4 centres, sigma 0.3) in a wide sparse volume."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-50, 50, (4, 3))
    c = np.ones((n, 4), F32)
    c[:, :3] = (centres[r.integers(0, 4, n)] + r.normal(0, 0.3, (n, 3))).astype(F32)
    c[::11, :3] = r.uniform(-200, 200, (len(c[::11]), 3)).astype(F32)
    return c


def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    normals = random_normals(len(cloud), 2)
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found and int(found[-1]) > 4096
    queries = np.concatenate([cloud[:100], clustered(28, 2)])
    monkeypatch.setattr(R.S, "TREE_ABOVE", float("inf"))  # 22 000 x 22 000 rows for the SPFH: this test's reference stays the brute form
    for mode in (dict(k=20), dict(radius=0.1)):
        check(ctx, "refused", cloud, normals, queries, **mode)


# ---- the golden fixture, the device's own normals ---------------------------------------------------------------------------
def test_golden_fixture(ctx):
    g = np.load(os.path.join(HERE, "golden", "rows_f", "fpfh_512.npz"))
    ctx.search_set_input(g["cloud"])
    for name, mode in (("k", dict(k=int(g["k"]))), ("r", dict(radius=float(g["radius"])))):
        got = ctx.fpfh_estimation(g["normals"], None, want_spfh=True, **mode)
        assert_same(got, (g[f"{name}_fpfh"], g[f"{name}_counts"], g[f"{name}_spfh"]), name)


def test_normals_from_the_device_fed_straight_back(ctx):
    cloud = scan(2000).copy()
    cloud[[10, 1999], :3] = F32([[300, 0, 0], [0, -700, 4]])
    ctx.search_set_input(cloud)
    normals, _ = ctx.normal_estimation(None, k=12, viewpoint=(0.5, -0.25, 1.0))
    assert_same((normals,), (N.estimate(cloud, None, k=12, viewpoint=(0.5, -0.25, 1.0))[0],))
    for mode in (dict(k=10), dict(radius=0.6)):
        check(ctx, "device-normals", cloud, normals, None, **mode)
        check(ctx, "device-normals-q", cloud, normals, scan(300, 9), **mode)


def test_five_identical_runs(ctx):
    cloud, normals, queries = scan(2000), scan_normals(2000), scan(300, 9)
    ctx.search_set_input(cloud)
    for q in (None, queries):
        for mode in (dict(k=33), dict(radius=0.7)):
            first = ctx.fpfh_estimation(normals, q, want_spfh=True, **mode)
            for _ in range(4):
                assert_same(ctx.fpfh_estimation(normals, q, want_spfh=True, **mode), first)


def test_optional_outputs_change_nothing_and_counts_are_the_search_rows(ctx):
    cloud, normals, queries = scan(2000), scan_normals(2000), scan(300, 9)
    ctx.search_set_input(cloud)
    L, ip = ctx._L, _lib.C.POINTER(_lib.C.c_int32)
    fp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))  # noqa: E731
    for q in (None, queries):
        n_q = len(cloud) if q is None else len(q)
        for mode in (dict(k=20), dict(radius=0.5)):
            fpfh, counts, spfh = ctx.fpfh_estimation(normals, q, want_spfh=True, **mode)
            if "k" in mode:
                assert np.array_equal(counts, ctx.search_knn(q, 20)[2])
            else:
                assert np.array_equal(counts, np.diff(ctx.search_radius(q, 0.5)[0]).astype(np.int32))
            for want_counts, want_spfh in ((False, False), (True, False), (False, True)):
                out, cnt, sp = np.full((n_q, FPFH_BINS), 7, F32), np.full(n_q, -5, np.int32), np.full((len(cloud), FPFH_BINS), 7, F32)
                rc = L.icpgpu_fpfh_estimation(ctx._h, fp(normals), None if q is None else fp(q), n_q, mode.get("k", 0), mode.get("radius", 0.0), fp(out),
                                              cnt.ctypes.data_as(ip) if want_counts else None, fp(sp) if want_spfh else None)
                assert rc == 0
                assert_same((out,), (fpfh,))
                assert np.array_equal(cnt, counts) if want_counts else (cnt == -5).all()
                assert np.array_equal(sp.view(np.uint32), spfh.view(np.uint32)) if want_spfh else (sp == 7).all()


def test_mirror_class(ctx):
    cloud, surface = scan(257), scan(2000)
    fe = FPFHEstimation()
    fe.setInputCloud(cloud)
    fe.setInputNormals(scan_normals(257))
    fe.setKSearch(8)
    fe.setSearchMethod(None)
    assert fe.getKSearch() == 8
    assert_same((fe.compute(), fe.getNeighbourCounts()), ref("mirror-own", cloud, scan_normals(257), None, dict(k=8))[:2])
    fe.setSearchSurface(surface)
    with pytest.raises(IcpGpuError):  # the normals are the surface's
        fe.compute()
    fe.setInputNormals(scan_normals(2000))
    fe.setKSearch(0)
    fe.setRadiusSearch(0.6)
    assert_same((fe.compute(), fe.getNeighbourCounts()), ref("mirror-surface", surface, scan_normals(2000), cloud, dict(radius=0.6))[:2])
    fe.setKSearch(5)  # both set: refused
    with pytest.raises(IcpGpuError) as e:
        fe.compute()
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_search_cloud_usable():
    cloud, normals = scan(257), scan_normals(257)
    nan, inf = float("nan"), float("inf")
    empty = np.empty((0, 4), F32)
    with Context(0) as c:
        with pytest.raises(IcpGpuError) as e:  # no search cloud
            c.fpfh_estimation(normals, cloud, k=5)
        assert e.value.code == _lib.ERR_INVALID_ARG
        c.search_set_input(cloud)
        calls = [lambda: c.fpfh_estimation(normals, None), lambda: c.fpfh_estimation(normals, None, k=5, radius=0.3),
                 lambda: c.fpfh_estimation(normals, None, k=65), lambda: c.fpfh_estimation(normals, None, k=1),
                 lambda: c.fpfh_estimation(normals, None, k=-3), lambda: c.fpfh_estimation(normals, None, radius=-0.1),
                 lambda: c.fpfh_estimation(normals, None, radius=nan), lambda: c.fpfh_estimation(normals, None, radius=inf),
                 lambda: c.fpfh_estimation(normals, None, k=5, n_q=256), lambda: c.fpfh_estimation(normals, None, radius=0.3, n_q=258),
                 lambda: c.fpfh_estimation(None, None, k=5), lambda: c.fpfh_estimation(None, cloud[:4], radius=0.3),
                 # n_q = 0 changes none of the argument checks
                 lambda: c.fpfh_estimation(normals, empty), lambda: c.fpfh_estimation(normals, empty, k=5, radius=1.0),
                 lambda: c.fpfh_estimation(normals, empty, k=1), lambda: c.fpfh_estimation(None, empty, k=5)]
        for call in calls:
            with pytest.raises(IcpGpuError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARG
            check(c, ("own", 257), cloud, normals, None, k=8)  # the search cloud is still there and answers as before
        fp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))  # noqa: E731
        assert c._L.icpgpu_fpfh_estimation(c._h, fp(normals), fp(cloud), 257, 5, 0.0, None, None, None) == _lib.ERR_INVALID_ARG  # null output
        assert c._L.icpgpu_fpfh_estimation(c._h, fp(normals), fp(cloud), 0, 5, 0.0, None, None, None) == 0                       # n_q = 0 is OK
        assert c._L.icpgpu_fpfh_estimation(c._h, fp(normals), None, 0, 0, 0.5, None, None, None) == 0
        assert c.fpfh_estimation(normals, empty, radius=0.5)[0].shape == (0, FPFH_BINS)
        check(c, ("own", 257), cloud, normals, None, radius=0.3)


def test_radius_total_beyond_int32(ctx):
    """47 000 coincident points within the radius of one another: 2.2e9 neighbours in all.  The count pass alone runs; nothing is
    filled."""
    cloud = np.tile(F32([1.0, 2.0, 3.0, 1.0]), (47000, 1))
    normals = np.tile(F32([0, 0, 1, 0]), (47000, 1))
    ctx.search_set_input(cloud)
    with pytest.raises(IcpGpuError) as e:
        ctx.fpfh_estimation(normals, None, radius=0.5)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    fpfh, counts = ctx.fpfh_estimation(normals, cloud[:3], k=4)  # the search cloud still answers
    assert (counts == 4).all() and not fpfh.any()
