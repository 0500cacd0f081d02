"""The normal estimation on the device (icpgpu_normal_estimation; icp_normals.hip over icp_search.hip's rows) against the NumPy
restatement (tests/normals_restated.py), bit for bit everywhere: normals and curvature as uint32, counts as int32, moments as
uint32.  No tolerance anywhere."""
import functools
import os
import re

import numpy as np
import pytest

import normals_restated as R
from icpslam_amd import P2PLANE, Context, IcpGpuError, NormalEstimation, _lib, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 3, 4, 63, 64, 65, 257, 3000)
KS = (1, 2, 3, 8, 20, 64)
EYE = (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


_REF = {}


def ref(key, cloud, queries, viewpoint, mode):
    """The restatement's answer, computed once per (cloud, queries, arguments); key = None: not worth keeping."""
    if key is None:
        return R.estimate(cloud, queries, viewpoint=viewpoint, **mode)
    k = (key, tuple(viewpoint)) + tuple(sorted(mode.items()))
    if k not in _REF:
        _REF[k] = R.estimate(cloud, queries, viewpoint=viewpoint, **mode)
    return _REF[k]


def assert_same(got, want, what=""):
    for name, g, w in zip(("normals", "counts", "moments"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if g.size else np.zeros(0, int)
        assert bad.size == 0, (what, name, bad.size, bad[:6], g[bad[:3]], w[bad[:3]])


def check(ctx, key, cloud, queries, viewpoint=EYE, **mode):
    got = ctx.normal_estimation(queries, viewpoint=viewpoint, want_moments=True, **mode)
    want = ref(key, cloud, queries, viewpoint, mode)
    assert_same(got, want, f"{key} {mode} {viewpoint}")
    return got


def grid_cell(err: str) -> float:
    """The cell size of the grid the library kept for the last search cloud (its debug line's last attempt)."""
    found = re.findall(r"\[icpgpu\] grid n=\d+ .* h=([0-9.]+) ", err)
    assert found
    return float(found[-1])


# ---- sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_k_sizes(ctx, n, k):
    cloud = scan(3000)[:n]
    ctx.search_set_input(cloud)
    normals, counts, moments = check(ctx, ("scan", n), cloud, None, k=k)
    m = min(k, n)
    assert (counts == m).all()
    assert np.isnan(normals).all() == (m < 3) and np.isnan(moments).all() == (m < 3)
    if m >= 3:
        assert np.isfinite(normals).all() and np.isfinite(moments).all()


# ---- radius ---------------------------------------------------------------------------------------------------------------
def test_radius_rows_of_every_kind(ctx, monkeypatch, capfd):
    """The 3000-point scan and 50 queries lifted 50 m off it at 0.12 m: rows of 0, 1, 2 and 3 entries among others, from the grid's
    cube.  256 of its points and the lifted ones at 6 m (or 8.5 cells of the grid, if that is more): rows of more than 64
    entries -- the long-row path -- found by the sweep without the grid (more than 8 shells).  Each of these facts is asserted,
    from the restatement or from the library's debug line, so the test cannot quietly lose its edge."""
    cloud = scan(3000)
    lifted = cloud[:50].copy()
    lifted[:, 2] += F32(50.0)
    queries = np.concatenate([cloud, lifted])
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    h = grid_cell(capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    small, big = 0.12, max(6.0, round(8.5 * h, 2))
    assert np.ceil(small / (h * 63 / 64)) <= 8 < np.ceil(big / (h * 63 / 64)), h
    _, counts, _ = check(ctx, "radius-mixed", cloud, queries, radius=small)
    assert set(range(4)) <= set(counts.tolist()), sorted(set(counts.tolist()))[:8]
    queries = np.concatenate([cloud[:256], lifted])
    normals, counts, _ = check(ctx, "radius-sweep", cloud, queries, radius=big)
    assert counts.max() > 64 and not counts[256:].any()
    assert np.isnan(normals[256:]).all() and np.isfinite(normals[counts >= 3]).all()
    _, counts, _ = check(ctx, ("scan", 3000), cloud, None, radius=1.0)  # long rows from the grid's cube as well
    assert counts.max() > 64 and np.ceil(1.0 / (h * 63 / 64)) <= 8


# ---- ties -----------------------------------------------------------------------------------------------------------------
def lattice(m):
    g = np.arange(m, dtype=F32)
    c = np.ones((m ** 3, 4), F32)
    c[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return c


def test_lattice_ties_and_viewpoints(ctx):
    """9 x 9 x 9 integer lattice in a shuffled order: whole shells of neighbours share one d2, so the order of the float32 sums is
    the index order.  Viewpoints: the origin, a point inside the cloud, and one in the lattice plane z = 4.  cos == 0 itself is
    pinned by hand below: one lattice plane as the cloud, the viewpoint in it."""
    cloud = lattice(9)
    cloud = cloud[np.random.default_rng(3).permutation(len(cloud))]
    centres = cloud[:200].copy()
    centres[:, :3] += F32(0.5)
    ctx.search_set_input(cloud)
    for vp in (EYE, (4.25, 3.5, 4.75), (4.5, 4.5, 4.0)):
        for mode in (dict(k=7), dict(k=20), dict(k=64), dict(radius=1.0), dict(radius=1.5), dict(radius=3.0)):
            check(ctx, "lattice-self", cloud, None, vp, **mode)
            check(ctx, "lattice-centres", cloud, centres, vp, **mode)
    # every normal is (0, 0, 1) and v = viewpoint - p has no z: cos == 0 exactly, the sign stays the eigenvector's
    plane = cloud[cloud[:, 2] == 4].copy()
    ctx.search_set_input(plane)
    normals, _, _ = check(ctx, "lattice-plane", plane, None, (40.0, -3.0, 4.0), k=9)
    assert np.array_equal(normals, np.tile(F32([0, 0, 1, 0]), (81, 1)))
    below, _, _ = check(ctx, "lattice-plane", plane, None, (4.0, 4.0, -1.0), radius=1.5)
    assert np.array_equal(below[:, :3], np.tile(F32([0, 0, -1]), (81, 1)))


@pytest.mark.parametrize("copies", [2, 70])
def test_duplicated_points(ctx, copies):
    base = scan(400 if copies == 2 else 40)
    for name, cloud in (("rep", np.repeat(base, copies, axis=0)), ("tile", np.tile(base, (copies, 1)))):
        ctx.search_set_input(cloud)
        for mode in (dict(k=8), dict(k=64), dict(radius=0.3), dict(radius=2.0)):
            check(ctx, (name, copies), cloud, None, **mode)


# ---- degenerate clouds --------------------------------------------------------------------------------------------------
def test_coincident_and_collinear_clouds(ctx):
    one = np.tile(F32([4.0, 5.0, -6.0, 1.0]), (70, 1))
    ctx.search_set_input(one)
    normals, counts, moments = check(ctx, "one-point", one, None, k=10)
    assert np.array_equal(normals, np.tile(F32([-1, 0, 0, 0]), (70, 1)))  # (1, 0, 0) turned towards the origin
    normals, counts, _ = check(ctx, "one-point", one, None, (10.0, 0.0, 0.0), radius=0.1)
    assert (counts == 70).all() and np.array_equal(normals, np.tile(F32([1, 0, 0, 0]), (70, 1)))
    line = np.ones((300, 4), F32)
    line[:, :3] = np.arange(300, dtype=F32)[:, None] * F32([0.25, 0, 0]) + F32([0, 0, 3])
    ctx.search_set_input(line)
    normals, _, _ = check(ctx, "line-x", line, None, (0.0, 9.0, 3.0), k=5)
    assert np.array_equal(normals, np.tile(F32([0, 1, 0, 0]), (300, 1)))
    skew = line.copy()
    skew[:, 1] = skew[:, 0] * F32(0.7)
    skew[:, 2] = skew[:, 0] * F32(-1.3)
    ctx.search_set_input(skew)
    for mode in (dict(k=3), dict(k=20), dict(radius=1.0), dict(radius=30.0)):
        check(ctx, "line-skew", skew, None, **mode)


# ---- queries that are not cloud points ------------------------------------------------------------------------------------
def test_search_surface_and_odd_queries(ctx, monkeypatch, capfd):
    """The queries are another cloud (setSearchSurface); some lie more than 64 cells outside the surface's box (asserted from the
    grid's cell size), some are non-finite; the surface has non-finite rows at the first, last and wave-boundary indices."""
    cloud = scan(3000).copy()
    rows = [0, 63, 64, 65, 255, 256, 2999]
    for j, i in enumerate(rows):
        cloud[i, j % 3] = [np.nan, np.inf, -np.inf][j % 3]
    queries = scan(300, 9).copy()
    qrows = [0, 3, 4, 63, 64, 299]
    queries[qrows, 2] = np.nan
    mid = np.nanmean(np.where(np.isfinite(cloud[:, :3]), cloud[:, :3], np.nan), axis=0)
    queries[10, :3] = mid + F32([4000.0, 0, 0])
    queries[11, :3] = mid - F32([0, 2500.0, 2500.0])
    queries[12, :3] = F32([1e6, -1e6, 1e6])
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    h = grid_cell(capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    extent = float(np.nanmax(np.abs(np.where(np.isfinite(cloud[:, :3]), cloud[:, :3], np.nan) - mid)))
    assert (2500.0 - extent) / h > 64
    for vp in (EYE, (1.0, -2.0, 0.5)):
        for mode in (dict(k=8), dict(k=64), dict(radius=0.5), dict(radius=5000.0)):
            if mode == dict(radius=5000.0) and vp != EYE:
                continue
            q = queries if "k" in mode or mode["radius"] < 1 else queries[:16]  # (whole-cloud rows: a few queries are enough)
            normals, counts, moments = check(ctx, ("surface", len(q)), cloud, q, vp, **mode)
            bad = [r for r in qrows if r < len(q)]
            assert not counts[bad].any() and np.isnan(normals[bad]).all() and np.isnan(moments[bad]).all()
    assert_same(ctx.normal_estimation(None, k=20, want_moments=True), ctx.normal_estimation(cloud, k=20, want_moments=True))
    normals, counts = ctx.normal_estimation(None, k=20)
    assert not counts[rows].any() and np.isnan(normals[rows]).all() and (np.delete(counts, rows) == 20).all()


def test_fewer_than_three_finite_points(ctx):
    cloud = scan(64)[:5].copy()
    cloud[[1, 3, 4], 0] = np.nan
    ctx.search_set_input(cloud)
    for mode in (dict(k=20), dict(radius=100.0)):
        normals, counts, moments = check(ctx, "two-finite", cloud, None, **mode)
        assert counts.tolist() == [2, 0, 2, 0, 0] and np.isnan(normals).all() and np.isnan(moments).all()
        normals, counts, _ = check(ctx, "two-finite-q", cloud, scan(64, 9), **mode)
        assert (counts == 2).all() and np.isnan(normals).all()
    ctx.search_set_input(np.empty((0, 4), F32))
    normals, counts = ctx.normal_estimation(scan(64), k=5)
    assert not counts.any() and np.isnan(normals).all()
    normals, counts = ctx.normal_estimation(scan(64), radius=5.0)
    assert not counts.any() and np.isnan(normals).all()


def test_non_finite_covariance_entry(ctx):
    huge = np.ones((5, 4), F32)
    huge[:, 0] = F32([0, 3e19, -3e19, 1e19, 2e19])
    ctx.search_set_input(huge)
    normals, counts, moments = check(ctx, "huge", huge, None, k=5)
    assert (counts == 5).all() and np.isnan(normals).all() and not np.isfinite(moments[:, 0]).any() and np.isfinite(moments[:, 3:6]).all()


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
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found and int(found[-1]) > 4096
    queries = np.concatenate([cloud[:100], clustered(28, 2)])
    for mode in (dict(k=3), dict(k=20), dict(k=64), dict(radius=0.1), dict(radius=0.3)):
        check(ctx, "refused", cloud, queries, **mode)


# ---- the golden fixture ---------------------------------------------------------------------------------------------------
def test_golden_fixture(ctx):
    g = np.load(os.path.join(HERE, "golden", "rows_f", "normals_2k.npz"))
    cloud = g["cloud"]
    ctx.search_set_input(cloud)
    for name, mode in (("k", dict(k=int(g["k"]))), ("r", dict(radius=float(g["radius"])))):
        normals, counts, moments = ctx.normal_estimation(None, viewpoint=g["viewpoint"], want_moments=True, **mode)
        assert_same((normals[::2], counts, moments[::8]), (g[f"{name}_normals"], g[f"{name}_counts"], g[f"{name}_moments"]), name)


# ---- consistency ----------------------------------------------------------------------------------------------------------
def test_counts_are_the_search_rows_and_optional_outputs_change_nothing(ctx):
    cloud, queries = scan(3000).copy(), scan(300, 9).copy()
    cloud[[5, 900], 0] = np.nan
    queries[17, 1] = np.inf
    ctx.search_set_input(cloud)
    L, ip = ctx._L, _lib.C.POINTER(_lib.C.c_int32)
    fp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))  # noqa: E731
    for q in (None, queries):
        n_q = len(cloud) if q is None else len(q)
        for mode in (dict(k=20), dict(radius=0.5)):
            normals, counts, moments = ctx.normal_estimation(q, want_moments=True, **mode)
            if "k" in mode:
                assert np.array_equal(counts, ctx.search_knn(q, 20)[2])
            else:
                assert np.array_equal(counts, np.diff(ctx.search_radius(q, 0.5)[0]).astype(np.int32))
            for want_counts, want_moments in ((False, False), (True, False), (False, True)):
                out = np.full((n_q, 4), 7, F32)
                cnt, mom = np.full(n_q, -5, np.int32), np.full((n_q, 9), 7, F32)
                rc = L.icpgpu_normal_estimation(ctx._h, None if q is None else fp(q), n_q, mode.get("k", 0), mode.get("radius", 0.0), None, fp(out),
                                                cnt.ctypes.data_as(ip) if want_counts else None, fp(mom) if want_moments else None)
                assert rc == 0
                assert_same((out,), (normals,))  # (a NULL viewpoint is the origin)
                assert np.array_equal(cnt, counts) if want_counts else (cnt == -5).all()
                assert np.array_equal(mom.view(np.uint32), moments.view(np.uint32)) if want_moments else (mom == 7).all()


def test_mirror_class(ctx):
    cloud, surface = scan(257), scan(3000)
    ne = NormalEstimation()
    ne.setInputCloud(cloud)
    ne.setKSearch(8)
    ne.setSearchMethod(None)
    ne.setViewPoint(1.0, 2.0, 3.0)
    assert ne.getViewPoint() == (1.0, 2.0, 3.0) and ne.getKSearch() == 8
    assert_same((ne.compute(), ne.getNeighbourCounts()), ref("mirror-own", cloud, None, (1.0, 2.0, 3.0), dict(k=8))[:2])
    ne.setSearchSurface(surface)
    ne.setKSearch(0)
    ne.setRadiusSearch(0.6)
    assert_same((ne.compute(), ne.getNeighbourCounts()), ref("mirror-surface", surface, cloud, (1.0, 2.0, 3.0), dict(radius=0.6))[:2])
    ne.setKSearch(5)  # both set: refused, as in PCL
    with pytest.raises(IcpGpuError) as e:
        ne.compute()
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_search_cloud_usable():
    cloud = scan(255)
    nan, inf = float("nan"), float("inf")
    with Context(0) as c:
        with pytest.raises(IcpGpuError) as e:  # no search cloud
            c.normal_estimation(cloud, k=5)
        assert e.value.code == _lib.ERR_INVALID_ARG
        c.search_set_input(cloud)
        calls = [lambda: c.normal_estimation(None), lambda: c.normal_estimation(None, k=5, radius=0.3), lambda: c.normal_estimation(None, k=65),
                 lambda: c.normal_estimation(None, k=-3), lambda: c.normal_estimation(None, radius=-0.1), lambda: c.normal_estimation(None, radius=nan),
                 lambda: c.normal_estimation(None, radius=inf), lambda: c.normal_estimation(None, k=5, viewpoint=(0.0, nan, 0.0)),
                 lambda: c.normal_estimation(None, radius=0.3, viewpoint=(inf, 0.0, 0.0)), lambda: c.normal_estimation(None, k=5, n_q=254),
                 lambda: c.normal_estimation(None, radius=0.3, n_q=256),
                 # n_q = 0 changes none of the argument checks
                 lambda: c.normal_estimation(np.empty((0, 4), F32)), lambda: c.normal_estimation(np.empty((0, 4), F32), k=5, radius=1.0),
                 lambda: c.normal_estimation(np.empty((0, 4), F32), k=65), lambda: c.normal_estimation(np.empty((0, 4), F32), k=5, viewpoint=(nan, 0, 0))]
        for call in calls:
            with pytest.raises(IcpGpuError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARG
            check(c, ("own", 255), cloud, None, k=8)  # the search cloud is still there and answers as before
        fp = cloud.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
        assert c._L.icpgpu_normal_estimation(c._h, fp, 255, 5, 0.0, None, None, None, None) == _lib.ERR_INVALID_ARG  # null output
        assert c._L.icpgpu_normal_estimation(c._h, fp, 0, 5, 0.0, None, None, None, None) == 0                       # n_q = 0 is OK
        assert c.normal_estimation(np.empty((0, 4), F32), radius=0.5)[0].shape == (0, 4)
        check(c, ("own", 255), cloud, None, radius=0.3)


def test_radius_total_beyond_int32(ctx):
    """47 000 coincident points within the radius of one another: 2.2e9 neighbours in all.  The count pass alone runs (a wave per
    query over one cell of 47 000 points -- the grid refuses the cloud, so the sweep); nothing is filled."""
    cloud = np.tile(F32([1.0, 2.0, 3.0, 1.0]), (47000, 1))
    ctx.search_set_input(cloud)
    with pytest.raises(IcpGpuError) as e:
        ctx.normal_estimation(None, radius=0.5)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    normals, counts = ctx.normal_estimation(cloud[:3], k=4)  # the search cloud still answers
    assert (counts == 4).all() and np.array_equal(normals, np.tile(F32([-1, 0, 0, 0]), (3, 1)))


# ---- isolation ------------------------------------------------------------------------------------------------------------
def same(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def estimates(c, cloud, queries):
    c.search_set_input(cloud)
    return (c.normal_estimation(None, k=20, want_moments=True) + c.normal_estimation(queries, radius=0.5, viewpoint=(1.0, 2.0, 3.0), want_moments=True)
            + c.normal_estimation(queries, k=64, want_moments=True) + c.normal_estimation(None, radius=0.3, want_moments=True))


def p2plane_round(c, src, tgt, user_normals, between=None):
    """One finished P2PLANE alignment, then (optionally) `between`, then what must not have moved."""
    c.set_params(method=P2PLANE, max_iterations=6)
    c.set_source(src)
    c.set_target(tgt)
    if user_normals is not None:
        c.set_target_normals(user_normals)
    first = c.align(want_cloud=True, want_fitness=True)
    if between:
        between(c)
    nrm_t, nrm_s = c.normals(True), c.normals(False)
    second = c.align(want_cloud=True, want_fitness=True)
    return first, nrm_t, nrm_s, second


@pytest.mark.parametrize("user_normals", [False, True])
def test_isolation(user_normals):
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    cloud, queries = scan(3000), scan(300, 9)
    given = None
    if user_normals:
        given = ref("isolation-target", tgt, None, EYE, dict(k=12))[0].copy()
    with Context(0) as fresh:
        want_est = estimates(fresh, cloud, queries)
        want_rows = fresh.search_knn(None, 20) + fresh.search_radius(queries, 3.0, 70)
    with Context(0) as plain:
        want = p2plane_round(plain, src, tgt, given)
    got_est = []
    with Context(0) as c:
        got = p2plane_round(c, src, tgt, given, between=lambda c: got_est.append(estimates(c, cloud, queries)))
        rows = c.search_knn(None, 20) + c.search_radius(queries, 3.0, 70)  # (the last estimate left cloud as the search cloud)
        again = estimates(c, cloud, queries)
    for a, b in zip(got, want):
        if isinstance(a, dict):
            for k in ("T", "cloud"):
                assert a[k].tobytes() == b[k].tobytes(), k
            for k in ("iterations", "n_corr", "converged", "fitness", "mse"):
                assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
        else:
            assert a.tobytes() == b.tobytes()
    assert same(rows, want_rows)
    assert same(got_est[0], want_est) and same(again, want_est)
    assert_same(want_est[0:3], ref(("scan", 3000), cloud, None, EYE, dict(k=20)))


# ---- the other kernel -----------------------------------------------------------------------------------------------------
def test_wave_per_query_variant_gives_the_same_bits(built, dev_flavour, monkeypatch):
    """ICPGPU_NORMALS_WAVE=1 (development flavour only): a wave per query summing through lane reads -- the alternative EXPERIMENTS.md
    records beside the lane-per-query kernel.  Same rows, same order, same bits, on either side of its 64-entry batches."""
    if dev_flavour.delegated:
        return
    monkeypatch.setenv("ICPGPU_NORMALS_WAVE", "1")
    cloud, queries = scan(3000).copy(), scan(300, 9).copy()
    cloud[[0, 64, 2999], 1] = np.nan
    queries[[0, 63, 299], 2] = np.inf
    with Context(0) as c:
        c.search_set_input(cloud)
        for mode in (dict(k=2), dict(k=3), dict(k=20), dict(k=63), dict(k=64), dict(radius=0.12), dict(radius=1.0), dict(radius=4.0)):
            check(c, "variant-self", cloud, None, (1.0, 2.0, 3.0), **mode)
            check(c, "variant-queries", cloud, queries, **mode)
