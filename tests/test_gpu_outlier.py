"""The outlier filters on the device (icpgpu_statistical_outlier_removal, icpgpu_radius_outlier_removal; icp_outlier.hip) against
the NumPy restatement (tests/outlier_restated.py), bit for bit everywhere: measure, kept indices, output cloud, the statistics as
uint64.  No tolerance anywhere."""
import functools
import re

import numpy as np
import pytest

import outlier_restated as R
from icpslam_amd import GICP, Context, IcpGpuError, RadiusOutlierRemoval, StatisticalOutlierRemoval, _lib, synth

pytestmark = pytest.mark.gpu

SIZES = ("k+1", "k+2", 63, 64, 65, 255, 256, 257, 1025, 3000)
MEAN_KS = (1, 2, 8, 19, 50, 63)


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _ref_dist(key, mean_k):
    return R.sor_distances(_CLOUDS[key], mean_k)


_CLOUDS = {}


def ref_sor(key, cloud, mean_k, mult, negative=False):
    """The restatement's answer, its distances computed once per (cloud, mean_k)."""
    _CLOUDS.setdefault(key, cloud)
    dist = _ref_dist(key, mean_k)
    st = R.sor_stats(dist, int(R.finite_mask(cloud).sum()), mult)
    d64 = dist.astype(np.float64)
    with np.errstate(invalid="ignore"):
        removed = (d64 <= st["threshold"]) if negative else (d64 > st["threshold"])
    idx = np.arange(len(cloud), dtype=np.int32)
    return dict(st, measure=dist, kept=idx[~removed], removed=idx[removed], cloud=cloud[~removed])


def bits(x):
    return np.float64(x).view(np.uint64)


def check_sor(ctx, key, cloud, mean_k, mult, negative=False):
    ref = ref_sor(key, cloud, mean_k, mult, negative)
    out = ctx.statistical_outlier_removal(cloud, mean_k, mult, negative)
    got, st = ctx.outlier_fetch(), ctx.outlier_stats()
    bad = np.flatnonzero(got["measure"].view(np.uint32) != ref["measure"].view(np.uint32))
    assert bad.size == 0, (bad[:8], got["measure"][bad[:8]], ref["measure"][bad[:8]])
    for k in ("mean", "stddev", "threshold"):
        assert bits(st[k]) == bits(ref[k]), (k, st[k], ref[k])
    assert st["n_valid"] == ref["n_valid"]
    assert np.array_equal(got["kept"], ref["kept"]) and np.array_equal(got["removed"], ref["removed"])
    assert out.tobytes() == ref["cloud"].tobytes()
    return ref


def check_ror(ctx, cloud, radius, min_pts, negative=False, ref_k=None):
    k = R.ror_counts(cloud, radius) if ref_k is None else ref_k
    removed = (k > min_pts) if negative else (k <= min_pts)
    out = ctx.radius_outlier_removal(cloud, radius, min_pts, negative)
    got = ctx.outlier_fetch()
    assert np.array_equal(got["measure"], k.astype(np.float32)), np.flatnonzero(got["measure"] != k)[:8]
    assert np.array_equal(got["kept"], np.flatnonzero(~removed)) and np.array_equal(got["removed"], np.flatnonzero(removed))
    assert out.tobytes() == cloud[~removed].tobytes()
    return k


def size_of(n, mean_k):
    return mean_k + 1 if n == "k+1" else mean_k + 2 if n == "k+2" else n


# ---- SOR -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_k", MEAN_KS)
@pytest.mark.parametrize("n", SIZES)
def test_sor_sizes(ctx, n, mean_k):
    n = size_of(n, mean_k)
    cloud = scan(3000)[:n] if n < 3000 else scan(3000)
    if n < mean_k + 1:
        with pytest.raises(IcpGpuError) as e:
            ctx.statistical_outlier_removal(cloud, mean_k, 1.0)
        assert e.value.code == _lib.ERR_INVALID_ARG
        return
    ref = check_sor(ctx, ("scan", n), cloud, mean_k, 1.0)
    assert len(ref["kept"]) + len(ref["removed"]) == n


def test_sor_raw_scan_20k(ctx):
    """Near-field density and far-field sparsity in one grid."""
    ref = check_sor(ctx, ("raw", 20000), scan(20000, 6), 50, 1.0)
    assert 0 < len(ref["removed"]) < 20000


@pytest.mark.parametrize("mult", [-1.0, 0.0, 1.0, 1e9])
@pytest.mark.parametrize("negative", [False, True])
def test_sor_multipliers_and_negative(ctx, mult, negative):
    ref = check_sor(ctx, ("scan", 3000), scan(3000), 8, mult, negative)
    if mult == 1e9:
        assert len(ref["removed"]) == (3000 if negative else 0)


def test_sor_coincident_points(ctx):
    rng = np.random.default_rng(12)
    cloud = np.ones((300, 4), np.float32)
    cloud[:200, :3] = np.float32([1.5, -2.25, 0.75])
    cloud[200:, :3] = rng.uniform(-3, 3, (100, 3)).astype(np.float32)
    cloud = cloud[rng.permutation(300)]
    ref = check_sor(ctx, "coincident", cloud, 50, 1.0)
    assert (ref["measure"] == 0).sum() == 200


@pytest.mark.parametrize("negative", [False, True])
def test_sor_cloud_that_is_one_point(ctx, negative):
    cloud = np.tile(np.float32([4.0, 5.0, -6.0, 1.0]), (70, 1))
    ref = check_sor(ctx, "one-point", cloud, 63, 1.0, negative)
    assert not ref["measure"].any() and ref["threshold"] == 0.0
    assert len(ref["removed"]) == (70 if negative else 0)


@pytest.mark.parametrize("negative", [False, True])
def test_sor_pairs_pin_greater_than(ctx, negative):
    """Every dist is 0.5 = the mean = the threshold exactly: `dist > threshold` removes nothing, `>=` would remove everything."""
    cloud = np.ones((80, 4), np.float32)
    cloud[:, 1:3] = 0
    cloud[0::2, 0] = 100.0 * np.arange(40)
    cloud[1::2, 0] = 100.0 * np.arange(40) + 0.5
    ref = check_sor(ctx, "pairs", cloud, 1, 0.0, negative)
    assert (ref["measure"] == 0.5).all() and ref["mean"] == 0.5 and ref["threshold"] == 0.5
    assert len(ref["removed"]) == (80 if negative else 0)


def test_sor_isolated_points(ctx):
    """Returns at 300 to 1 000 m: the certification across empty shells, and the far list."""
    cloud = scan(2000).copy()
    far = np.ones((5, 4), np.float32)
    far[:, :3] = np.float32([[300, 0, 0], [-450, 200, 5], [0, 700, -3], [600, -600, 40], [1000, 10, 0]])
    cloud = np.concatenate([cloud[:1000], far[:2], cloud[1000:], far[2:]])
    ref = check_sor(ctx, "isolated", cloud, 19, 1.0)
    assert set(np.flatnonzero(ref["measure"] > 100)) == {1000, 1001, 2002, 2003, 2004}


def clustered(n, seed):
    """The cloud test_gicp_on_a_cloud_the_knn_grid_refuses builds: tight clusters (4 centres, sigma 0.3) in a wide sparse volume."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-50, 50, (4, 3))
    c = np.ones((n, 4), np.float32)
    c[:, :3] = (centres[r.integers(0, 4, n)] + r.normal(0, 0.3, (n, 3))).astype(np.float32)
    c[::11, :3] = r.uniform(-200, 200, (len(c[::11]), 3)).astype(np.float32)
    return c


def densest_cell(err: str, n: int) -> int:
    """The densest cell's population of the last grid built over an n-point cloud, from the library's ICPGPU_DEBUG line."""
    found = re.findall(rf"\[icpgpu\] grid n={n} .* max=(\d+) ", err)
    assert found, err[-500:]
    return int(found[-1])


def test_sor_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """22 000 points (the smallest round size at which the refusal has a margin; the restatement is quadratic), ~5 000 in each
    cluster of ~2 m across, in a 400 m box.  The grid starts from cells of 45 m (the box filled evenly), and its one correction stops
    at 3.7 m, so a cluster falls into one cell or a few: the densest holds ~5 000 points, and above 4 096 the grid refuses the cloud.
    That it did is ASSERTED, from the library's debug line: every point then goes through the whole-cloud kernel.  (The radius
    filter's count without a grid: test_ror_radius_larger_than_the_cloud, where the radius alone rules the grid out.)"""
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    check_sor(ctx, "clustered", cloud, 19, 1.0)
    assert densest_cell(capfd.readouterr().err, 22000) > 4096


@pytest.mark.parametrize("mean_k", [8, 63])
def test_sor_non_finite_rows(ctx, mean_k):
    """NaN / inf rows at the first, last and wave-boundary indices: kept with dist 0, nobody's neighbour, not in n_valid."""
    cloud = scan(1025).copy()
    rows = [0, 63, 64, 65, 255, 256, 1024]
    for j, i in enumerate(rows):
        cloud[i, j % 3] = [np.nan, np.inf, -np.inf][j % 3]
    ref = check_sor(ctx, ("nan", 1025), cloud, mean_k, 1.0)
    assert not ref["measure"][rows].any() and ref["n_valid"] == 1025 - len(rows)
    assert set(rows) <= set(ref["kept"])


# ---- ROR -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 1025, 3000])
def test_ror_sizes(ctx, n):
    cloud = scan(3000)[:n]
    for radius in (0.0, 0.05, 0.3, 2.0):
        k = R.ror_counts(cloud, radius)
        for min_pts in (0, 1, 5, 40):
            check_ror(ctx, cloud, radius, min_pts, negative=(min_pts == 5), ref_k=k)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_ror_sizes_around_the_compactions_tile(ctx, n):
    """The compaction's scan works in tiles of 4096 flags (icp_scan.hip): a tile less one flag, one tile, a tile and one flag -- the
    last point is kept by exactly one of the two calls."""
    cloud = scan(4097)[:n]
    k = R.ror_counts(cloud, 0.3)
    kept = 0
    for negative in (False, True):
        check_ror(ctx, cloud, 0.3, 5, negative, ref_k=k)
        got = ctx.outlier_fetch()
        assert 1000 < got["kept"].size < n - 1000 and got["kept"].size + got["removed"].size == n
        kept += got["kept"].size
    assert kept == n


def test_ror_lattice_pins_strict_less(ctx):
    """Spacing exactly 0.25, radius 0.25: d2 == r2 is not a neighbour."""
    g = np.arange(8, dtype=np.float32) * np.float32(0.25)
    cloud = np.ones((512, 4), np.float32)
    cloud[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    k = check_ror(ctx, cloud, 0.25, 1)
    assert (k == 1).all()
    k = check_ror(ctx, cloud, 0.2500001, 1)
    assert k.max() == 7 and k.min() == 4


def test_ror_radius_larger_than_the_cloud(ctx):
    cloud = scan(1025).copy()
    cloud[[0, 500], 2] = np.nan
    k = check_ror(ctx, cloud, 1e4, 5)
    fin = R.finite_mask(cloud)
    assert (k[fin] == fin.sum()).all() and not k[~fin].any()
    check_ror(ctx, cloud, 1e8, 5, negative=True, ref_k=k)


def test_ror_non_finite_rows(ctx):
    cloud = scan(1025).copy()
    rows = [0, 63, 64, 65, 255, 256, 1024]
    cloud[rows, 1] = np.inf
    for negative in (False, True):
        k = check_ror(ctx, cloud, 0.3, 5, negative)
    assert not k[rows].any()


# ---- entry points, history, refusals -------------------------------------------------------------------------------------
def test_entry_points_agree(ctx):
    cloud = scan(3000)
    a = ctx.statistical_outlier_removal(cloud, 19, 1.0)
    b = ctx.statistical_outlier_removal(cloud, 19, 1.0, view=True)
    again = ctx.statistical_outlier_removal(cloud, 19, 1.0)
    f = StatisticalOutlierRemoval()
    f.setInputCloud(cloud)
    f.setMeanK(19)
    f.setStddevMulThresh(1.0)
    c = f.filter()
    assert a.tobytes() == b.tobytes() == again.tobytes() == c.tobytes() and 0 < len(a) < 3000
    assert np.array_equal(f.getRemovedIndices(), ref_sor(("scan", 3000), cloud, 19, 1.0)["removed"])
    a = ctx.radius_outlier_removal(cloud, 0.3, 5)
    b = ctx.radius_outlier_removal(cloud, 0.3, 5, view=True)
    again = ctx.radius_outlier_removal(cloud, 0.3, 5)
    g = RadiusOutlierRemoval()
    g.setInputCloud(cloud)
    g.setRadiusSearch(0.3)
    g.setMinNeighborsInRadius(5)
    c = g.filter()
    assert a.tobytes() == b.tobytes() == again.tobytes() == c.tobytes() and 0 < len(a) < 3000
    assert len(g.getRemovedIndices()) == 3000 - len(a)
    f.setMeanK(0)
    assert f.filter().shape == (0, 4)  # a refused call leaves the output empty
    assert ctx.statistical_outlier_removal(np.empty((0, 4), np.float32), 5, 1.0).shape == (0, 4)
    assert ctx.outlier_fetch()["measure"].shape == (0,)


def test_filters_leave_the_context_as_it_was():
    src, tgt, _ = synth.make_pair(4000, 4000, seed=3)
    raw = scan(20000, 6)
    with Context(0) as c:
        c.set_params(method=GICP, max_iterations=8)
        c.set_source(src)
        c.set_target(tgt)
        first = c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.radius_outlier_removal(raw, 0.3, 5)
        second = c.align(want_cloud=True, want_fitness=True)
        for k in ("T", "cloud"):
            assert first[k].tobytes() == second[k].tobytes()
        for k in ("iterations", "n_corr", "converged", "fitness", "mse"):
            assert first[k] == second[k], k

        def chain(cc):
            cc.set_params(method=GICP, max_iterations=8)
            cc.set_target(tgt)
            vox = cc.voxel_grid(raw, 0.4)
            filtered = cc.statistical_outlier_removal(vox, 8, 1.0)
            cc.set_source(filtered)
            return filtered, cc.align(want_cloud=True)

        f1, r1 = chain(c)
    with Context(0) as fresh:
        f2, r2 = chain(fresh)
    assert f1.tobytes() == f2.tobytes() and 0 < len(f1)
    assert r1["T"].tobytes() == r2["T"].tobytes() and r1["cloud"].tobytes() == r2["cloud"].tobytes()
    assert r1["iterations"] == r2["iterations"]


def test_refusals_leave_the_context_usable(ctx):
    cloud = scan(255).copy()
    cloud[20:, 0] = np.nan  # 20 finite points
    calls = [lambda: ctx.statistical_outlier_removal(cloud, 0, 1.0), lambda: ctx.statistical_outlier_removal(cloud, 64, 1.0),
             lambda: ctx.statistical_outlier_removal(cloud, 20, 1.0), lambda: ctx.radius_outlier_removal(cloud, -0.1, 1),
             lambda: ctx.radius_outlier_removal(cloud, float("nan"), 1), lambda: ctx.radius_outlier_removal(cloud, float("inf"), 1),
             lambda: ctx.radius_outlier_removal(cloud, 0.3, -1)]
    for call in calls:
        with pytest.raises(IcpGpuError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(IcpGpuError):
            ctx.outlier_fetch()  # a refused call leaves nothing to observe
    check_sor(ctx, ("nan20", 255), cloud, 19, 1.0)  # n_finite = mean_k + 1 is enough
    check_ror(ctx, cloud, 0.3, 1)
    with pytest.raises(IcpGpuError):
        ctx.outlier_stats()  # the last filter was the radius one
