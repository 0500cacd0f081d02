"""The neighbour search at the sizes where its code changes path (icp_search.hip, icp_scan.hip, icpgpu_search.cpp's deliver), against
the NumPy restatement bit for bit: the bench scan voxel-filtered at 0.2 m (the size DESIGN.md quotes its timings for), more than
4 096 listed queries, more than one scan tile, more than 65 536 queries, results above the staging buffer, and the 65 536-point limit
of a cloud the grid refuses.  The reference is tests/search_restated.py's tree-narrowed form (exact: test_search_host.py); its share of
rows left to the whole-cloud sweep is asserted here too, per reference, on the device's own filtered scan.  No tolerance anywhere."""
import contextlib
import re

import numpy as np
import pytest

import search_restated as R
from icpslam_amd import Context, IcpGpuError, _lib
from test_gpu_search import assert_same, check_knn, check_radius, clustered, ref, scan

pytestmark = pytest.mark.gpu

F32 = np.float32
STAGE_MAX_BYTES = 8 << 20   # icp_ctx.h: kStageMaxBytes
SCAN_TILE = 4096            # icp_scan.hip: one tile of launch_exclusive_scan
FAR_GRID = 4096             # icp_search.hip: search_far_kernel's grid is min(n_q, 4096) workgroups
TOTALS_LANES = 256 * 256    # icp_search.hip: search_totals_kernel's grid is capped at 256 workgroups of 256 lanes

_F = []


def filtered(ctx) -> np.ndarray:
    """F: the 200 000-point bench scan through the device's voxel filter at 0.2 m (about 17 500 points)."""
    if not _F:
        f = ctx.voxel_grid(scan(200000, 6), 0.2)
        f.setflags(write=False)
        _F.append(f)
    assert len(_F[0]) > 16384
    return _F[0]


@contextlib.contextmanager
def few_rows_swept():
    """Of the rows the tree-narrowed forms decide inside the block -- one test's references, where they are computed and not taken
    from the cache or from the brute forms -- fewer than 1 % fall back to the whole-cloud sweep."""
    before = dict(R.tree_stats)
    yield
    rows, swept = R.tree_stats["rows"] - before["rows"], R.tree_stats["swept"] - before["swept"]
    assert swept * 100 < rows or rows == 0, (swept, rows)


def prefix_knn(want, n_q):
    return tuple(a[:n_q] for a in want)


def prefix_radius(want, n_q):
    row_start, idx, d2 = want
    return row_start[:n_q + 1], idx[:row_start[n_q]], d2[:row_start[n_q]]


# ---- scan size, self-queries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 20, 64])
def test_scan_size_knn(ctx, k):
    """search_knn_kernel over the filtered scan's own points.  k = 64 is the first search test of deliver()'s direct path: idx and d2
    together exceed kStageMaxBytes (ASSERTED from the byte count) and are copied straight into the caller's arrays."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    assert ctx.search_size() == (len(F), len(F))
    if k == 64:
        assert len(F) * 64 * 8 > STAGE_MAX_BYTES
    with few_rows_swept():
        idx, d2, n_found = check_knn(ctx, "F", F, None, k)
    assert (n_found == k).all() and np.array_equal(idx[:, 0], np.arange(len(F))) and not d2[:, 0].any()


@pytest.mark.parametrize("radius, max_nn", [(0.5, 0), (1.0, 0), (1.0, 8), (1.0, 65)])
def test_scan_size_radius(ctx, radius, max_nn):
    """Radius rows over the filtered scan's own points: at 0.5 m every row is filled and sorted in the lanes, at 1.0 m thousands of
    rows take the ranked scratch path (search_radius_fill_kernel's second half) and lie in every tile of both scans; idx + d2 then
    exceed kStageMaxBytes: the first radius search delivered on deliver()'s direct path (ASSERTED from the byte count).  max_nn = 8
    cuts every long row back into the lanes, 65 leaves the cut rows on the ranked path."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        row_start, idx, d2 = check_radius(ctx, "F", F, None, radius, max_nn)
    lens = np.diff(row_start)
    assert row_start[-1] == len(idx) == len(d2) and lens.min() >= 1
    if radius == 0.5:
        assert lens.max() <= 64
    elif max_nn == 0:
        long_rows = np.flatnonzero(lens > 64)
        assert len(long_rows) > 1000 and len(set((long_rows // SCAN_TILE).tolist())) == -(-len(F) // SCAN_TILE)
        assert (len(idx) + len(d2)) * 4 > STAGE_MAX_BYTES
    else:
        assert lens.max() == max_nn and (lens == max_nn).sum() > 1000


# ---- the scans' tiles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1.0, 0.5])
@pytest.mark.parametrize("n_q", [4095, 4096, 4097, 8191, 8192, 8193])
def test_query_counts_around_the_scan_tiles(ctx, n_q, radius):
    """The first search tests of launch_exclusive_scan (icp_scan.hip) beyond one tile: row_start and scratch_start are scans of
    n_q + 1 entries in tiles of 4 096, so 4 095 queries fill one tile exactly, 4 096 put only the total into a second, 8 192 only the
    total into a third (scan_tiles_kernel's offsets, scan_apply_tiles_kernel's + tile_sums[blockIdx.x]).  At 1.0 m rows of more than
    64 entries sit in the later tiles, so scratch_start's offsets there are used, not only computed (asserted where a later tile
    holds more than its first row)."""
    F = filtered(ctx)
    queries = scan(8193, 9)
    ctx.search_set_input(F)
    with few_rows_swept():
        want = prefix_radius(ref("radius", ("F", "q8193"), F, queries, radius, 0), n_q)
    got = ctx.search_radius(queries[:n_q], radius)
    assert_same(got, want, f"radius {radius} n_q={n_q}")
    lens = np.diff(got[0])
    assert -(-(n_q + 1) // SCAN_TILE) == {4095: 1, 4096: 2, 4097: 2, 8191: 2, 8192: 3, 8193: 3}[n_q]
    if radius == 1.0:
        assert (lens[:SCAN_TILE] > 64).any()
        if n_q >= 8191:
            assert (lens[SCAN_TILE:n_q] > 64).sum() > 100
    else:
        assert lens.max() <= 64 and lens[-1] > 0


# ---- more than 65 536 queries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [65535, 65536, 65537, 131073])
def test_more_queries_than_the_totals_grid_has_lanes(ctx, n_q):
    """The first test of search_totals_kernel's grid-stride loop (256 workgroups of 256 lanes: a second round from 65 537 queries;
    the query count is the evidence).  Its sum sizes idx / d2 on its own, the scan makes row_start: n_total == row_start[-1] == the
    restatement's total.  Also search_knn_kernel / search_radius_*_kernel with more than 2^14 workgroups."""
    F = filtered(ctx)
    queries = scan(n_q, 9)
    assert (n_q > TOTALS_LANES) == (n_q >= 65537)
    ctx.search_set_input(F)
    with few_rows_swept():
        want = ref("radius", ("F", "scan9", n_q), F, queries, 0.3, 0)
    rc, row_start, _, _, n_total = ctx.search_radius_raw(queries, 0.3, 0, 0)
    assert rc == _lib.ERR_INVALID_ARG and n_total == row_start[-1] == want[0][-1] == len(want[1]) > n_q // 2
    rc, row_start, idx, d2, n_total = ctx.search_radius_raw(queries, 0.3, 0, n_total)
    assert rc == 0 and n_total == len(want[1])
    assert_same((row_start, idx, d2), want, f"radius 0.3 n_q={n_q}")
    with few_rows_swept():
        check_knn(ctx, ("F", "scan9", n_q), F, queries, 8)


def test_a_total_that_rests_on_the_last_queries(ctx):
    """131 073 queries of which all but the last 40 are moved 1 000 m up and find nothing: the whole total comes from the lanes of
    search_totals_kernel's second round, and every row in front of the tail is empty in every tile of the scan."""
    F = filtered(ctx)
    n_q = 131073
    queries = scan(n_q, 9).copy()
    queries[:-40, 2] += F32(1000.0)
    ctx.search_set_input(F)
    with few_rows_swept():
        want = ref("radius", ("F", "scan9-moved"), F, queries, 0.3, 0)
    assert want[0][n_q - 40] == 0 and want[0][-1] > 0
    rc, row_start, _, _, n_total = ctx.search_radius_raw(queries, 0.3, 0, 0)
    assert rc == _lib.ERR_INVALID_ARG and n_total == row_start[-1] == want[0][-1]
    assert_same(ctx.search_radius(queries, 0.3), want, "radius 0.3, moved")


# ---- more than 4 096 listed queries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("n_q", [4095, 4096, 4097, 8193, 12289])
def test_more_listed_queries_than_the_far_kernel_has_workgroups(ctx, n_q, k):
    """The first test of search_far_kernel's loop over listed queries (for (e = blockIdx.x; e < m; e += gridDim.x), 4 096 workgroups
    at most): 4 097 listed queries give one workgroup a second round, 8 193 and 12 289 a third and a fourth.  EVERY query is listed
    by construction: each lies 1e5 m outside the cloud's box, the grid spans that box with at least three cells an axis, so a cell is
    no larger than the box and the query is more than kSearchOutside = 64 cells outside (asserted as arithmetic on the box)."""
    cloud = scan(1025)
    queries = scan(12289, 9).copy()
    queries[:, 0] += F32(1e5)
    lo, hi = cloud[:, :3].min(axis=0), cloud[:, :3].max(axis=0)
    assert (queries[:, 0].min() - hi[0]) > 65 * float((hi - lo).max())
    assert (n_q > FAR_GRID) == (n_q >= 4097)
    ctx.search_set_input(cloud)
    want = prefix_knn(ref("knn", "far-outside", cloud, queries, k), n_q)
    idx, d2, n_found = ctx.search_knn(queries[:n_q], k)
    assert_same((n_found, idx, d2), (want[2], want[0], want[1]), f"knn k={k} n_q={n_q}")
    assert (n_found == k).all()


def test_every_query_of_a_refused_cloud_is_listed(ctx, monkeypatch, capfd):
    """test_gpu_search.py's 22 000-point cloud that the grid refuses (ASSERTED from the debug line), asked for all its own points:
    22 000 listed queries, six rounds of search_far_kernel's 4 096 workgroups over a cloud of many sweep batches; then 4 097 of them
    at k = 64 and, without a grid, search_radius_count / _fill_kernel's sweeps with rows of hundreds of entries."""
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    assert found and int(found[-1]) > 4096
    assert ctx.search_size() == (22000, 21999)
    with few_rows_swept():
        idx, d2, n_found = check_knn(ctx, "refused-self", cloud, None, 20)
    assert n_found[7] == 0 and (np.delete(n_found, 7) == 20).all()
    with few_rows_swept():
        check_knn(ctx, "refused-4097", cloud, cloud[:4097], 64)
    with few_rows_swept():
        row_start = check_radius(ctx, "refused-4097", cloud, cloud[:4097], 0.3)[0]
    assert np.diff(row_start).max() > 64


# ---- the 65 536-point limit of a cloud without a grid --------------------------------------------------------------------------
def piled(n):
    """scan(n - 5000) and 5 000 more copies of one of its points: smaller cells cannot split equal points, so one cell holds more
    than kMaxCellPopulation = 4 096 of them and the grid refuses the cloud."""
    base = scan(n - 5000)
    return np.concatenate([base, np.repeat(base[100:101], 5000, axis=0)])


def test_refused_cloud_of_exactly_65536_points(ctx, monkeypatch, capfd):
    """The first test of icpgpu.h's "a cloud the grid cannot index is searched without it up to 65536 points", at the limit itself:
    the cloud is refused by the grid (ASSERTED from the debug line), accepted by the search, and answers by sweeps."""
    cloud = piled(65536)
    assert len(cloud) == 65536
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=65536 .* max=(\d+) ", capfd.readouterr().err)
    assert found and int(found[-1]) > 4096
    assert ctx.search_size() == (65536, 65536)
    queries = np.concatenate([cloud[:60], cloud[-20:], scan(48, 9)])  # (the 20: inside the pile)
    assert len(queries) == 128
    for k in (20, 64):
        idx, d2, _ = check_knn(ctx, "piled", cloud, queries, k)
        assert not d2[60:80].any() and (idx[60:80] == [100] + list(range(60536, 60536 + k - 1))).all()
    row_start = check_radius(ctx, "piled", cloud, queries, 0.3)[0]
    assert (np.diff(row_start)[60:80] > 5000).all()


def test_refused_cloud_of_65537_points_is_unsupported():
    """... and one point beyond it: ICPGPU_ERR_UNSUPPORTED, the context then has no search cloud (every search call: INVALID_ARG), and
    the next search cloud answers as in a fresh context."""
    cloud, small = piled(65537), scan(255)
    assert len(cloud) == 65537
    with Context(0) as c:
        c.search_set_input(small)
        with pytest.raises(IcpGpuError) as e:
            c.search_set_input(cloud)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        for call in (lambda: c.search_size(), lambda: c.search_knn(small, 1), lambda: c.search_radius(small, 1.0)):
            with pytest.raises(IcpGpuError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARG
        c.search_set_input(small)
        assert c.search_size() == (255, 255)
        check_knn(c, ("own", 255), small, None, 8)
        check_radius(c, ("own", 255), small, None, 0.3)
