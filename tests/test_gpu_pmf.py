"""The ground filter on the device (icpgpu_morphological_operator / icpgpu_progressive_morphological_filter / icpgpu_pmf_fetch /
icpgpu_pmf_extract; icp_morph.hip) against the NumPy restatement (tests/pmf_restated.py), bit for bit: the four operators' z, the
schedule, the ground, its size after every pass and removed_at."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import pmf_cases as K
import pmf_restated as R
from icpslam_amd import Context, IcpGpuError, ProgressiveMorphologicalFilter, _lib, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "pmf_2k.npz")
OPS = (R.ERODE, R.DILATE, R.OPEN, R.CLOSE)
NAMES = ("ground", "windows", "thresholds", "ground_after", "removed_at")
AXIS_CELLS, CELLS_PER_WINDOW = 512, 8        # icp_kernels.h: kMorphAxisCells, kMorphCellsPerWindow


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def device(ctx, **kw) -> dict:
    """One filter call over the search cloud in place and its fetch, shaped like the restatement's answer."""
    rc, n_ground, n_passes = ctx.pmf_filter_raw(**kw)
    assert rc == 0, ctx._L.icpgpu_last_error(ctx._h)
    rc, f = ctx.pmf_fetch_raw(n_ground, n_passes)
    assert rc == 0
    return f


def assert_same(got: dict, want: dict, what=""):
    for name in NAMES:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, g[:8], w[:8])


def check(ctx, cloud, windows=(), want=None, **kw) -> dict:
    """The search cloud set, the operators at `windows` and the filter against the restatement; the host waits."""
    ctx.search_set_input(cloud)
    for w in windows:
        for op in OPS:
            got = ctx.morphological_operator(w, op)
            assert got.dtype == F32 and got.tobytes() == R.operator(cloud, w, op).tobytes(), (len(cloud), w, op)
            assert ctx.pmf_stats()[0] == (1 if len(cloud) else 0)
    got = device(ctx, **kw)
    want = R.run(cloud, **kw) if want is None else want
    assert_same(got, want, f"n {len(cloud)} {kw}")
    assert (np.diff(got["ground"]) > 0).all()
    assert ctx.pmf_stats()[0] == (1 if len(cloud) and len(want["windows"]) else 0)
    return got


# ---- sizes and box populations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2000])
def test_sizes(ctx, n):
    got = check(ctx, scan(2000)[:n], windows=(2.0,))
    assert n < 1000 or 0 < got["ground"].size < n


def test_box_populations_on_a_line(ctx):
    """1 000 points a metre apart: a window's box holds the point alone (0.5), exactly 2 at the line's ends (2), 63, 64 at the ends (126),
    65, 129, 401 and the whole cloud."""
    rng = np.random.default_rng(3)
    cloud = K.points(np.stack([np.arange(1000.0), np.zeros(1000), rng.normal(0, 1, 1000)], axis=1))
    ctx.search_set_input(cloud)
    for w, interior, at_end in ((0.5, 1, 1), (2.0, 3, 2), (62.0, 63, 32), (126.0, 127, 64), (64.0, 65, 33), (128.0, 129, 65), (400.0, 401, 201),
                                (1e4, 1000, 1000)):
        rows = R.boxes(cloud, np.arange(1000), w, rows=np.array([500, 0])).sum(axis=1)
        assert rows.tolist() == [interior, at_end]
        for op in OPS:
            assert ctx.morphological_operator(w, op).tobytes() == R.operator(cloud, w, op).tobytes(), (w, op)


def test_box_populations_in_the_plane(ctx):
    cloud = scan(2000)
    ctx.search_set_input(cloud)
    finite = np.arange(2000)
    for w in (1e-4, 1.0, 7.0, 40.0, 1e4):
        sizes = R.boxes(cloud, finite, w).sum(axis=1)
        assert sizes.min() >= 1 and (w < 1e4 or sizes.min() == 2000) and (w > 1e-4 or np.median(sizes) == 1)
        for op in OPS:
            assert ctx.morphological_operator(w, op).tobytes() == R.operator(cloud, w, op).tobytes(), (w, op)
    assert 300 < R.boxes(cloud, finite, 40.0).sum(axis=1).max()


# ---- the cell table's edges ----------------------------------------------------------------------------------------------------
def test_two_far_points_make_the_cell_cap_bite_and_change_nothing(ctx):
    """Two points 10 km away: the finite box is 20 km wide, window / 8 would need far more than 512 cells an axis, the cells are coarsened
    to 39 m and nearly every box becomes rim -- the answers on the rest are the ones without the two."""
    base = scan(1000)
    cloud = np.concatenate([base, K.points([[1e4, 1e4, 3.0], [-1e4, -1e4, -2.0]])])
    assert 2e4 / (3.0 / CELLS_PER_WINDOW) > AXIS_CELLS
    got = check(ctx, cloud, windows=(3.0, 33.0))
    alone = R.run(base)
    assert got["removed_at"][:1000].tobytes() == alone["removed_at"].tobytes() and got["removed_at"][1000:].tolist() == [-1, -1]
    ctx.search_set_input(cloud)
    assert ctx.morphological_operator(9.0, R.OPEN)[:1000].tobytes() == R.operator(base, 9.0, R.OPEN).tobytes()


def test_a_cloud_inside_one_cell_and_a_vertical_line(ctx):
    tiny = scan(300).copy()
    tiny[:, :2] *= F32(1e-3)                                  # a few centimetres across: one cell at every window
    check(ctx, tiny, windows=(3.0, 0.02))
    cloud, kw, windows = K.CASES["vertical_line"]
    got = check(ctx, cloud, windows=windows, **kw)
    assert got["ground"].size == 1                            # every box is everything: only the lowest point is within 0.15 of the opening
    huge = scan(300).copy()
    huge[:, :2] *= F32(1e30)                                  # an extent whose cell side overflows nothing but is coarsened to 1e28
    huge[0, 0], huge[1, 0] = F32(3e38), F32(-3e38)            # ... and one whose extent is not finite: one cell
    check(ctx, huge, windows=(3.0,))


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_hand_clouds(ctx, name):
    cloud, kw, windows = K.CASES[name]
    check(ctx, cloud, windows=windows, **kw)


def test_nan_only_and_empty_clouds(ctx):
    for cloud in (np.empty((0, 4), F32), np.full((70, 4), np.nan, F32)):
        got = check(ctx, cloud, windows=(3.0,) if len(cloud) else ())
        assert got["ground"].size == 0 and got["ground_after"].tolist() == [0] * 5
    ctx.search_set_input(np.empty((0, 4), F32))
    assert ctx.morphological_operator(3.0, R.OPEN).size == 0 and ctx.pmf_stats()[0] == 0
    assert ctx.pmf_filter_raw() == (0, 0, 5) and ctx.pmf_stats()[0] == 0
    assert ctx.pmf_extract(False).shape == ctx.pmf_extract(True, view=True).shape == (0, 4)


@pytest.mark.parametrize("leaf", [0.3, 0.6, 1.2])
def test_voxel_filtered_scans(ctx, leaf):
    cloud = ctx.voxel_grid(scan(5000, 6), leaf)
    assert 300 < len(cloud) < 5000
    got = check(ctx, cloud, windows=(2.0 * leaf,))
    assert 0 < got["ground"].size < len(cloud)


def clustered(n, seed):
    """The cloud test_gpu_cluster.py's test_cloud_the_grid_refuses builds: tight clusters (4 centres, sigma 0.3) in a wide sparse volume."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-50, 50, (4, 3))
    c = np.ones((n, 4), F32)
    c[:, :3] = (centres[r.integers(0, 4, n)] + r.normal(0, 0.3, (n, 3))).astype(F32)
    c[::11, :3] = r.uniform(-200, 200, (len(c[::11]), 3)).astype(F32)
    return c


def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """The 3-D grid refuses this cloud (ASSERTED, from the library's debug line); the ground filter needs no 3-D grid and works there.
    22 000 points are too many for the restatement's n x n matrix, so the stages are checked one on the other: ERODE and DILATE on 1 500
    sampled rows against the restatement, OPEN on those rows against the maximum of the DEVICE's erosion over the restatement's boxes, and
    the one-pass filter against z - OPEN < threshold on every point."""
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    assert found and int(found[-1]) > 4096
    finite = np.flatnonzero(R.finite_rows(cloud))
    rows = np.random.default_rng(2).choice(finite.size, 1500, replace=False)
    M = R.boxes(cloud, finite, 3.0, rows=rows)
    assert M.sum(axis=1).max() > 3000
    eroded, dilated, opened = (ctx.morphological_operator(3.0, op) for op in (R.ERODE, R.DILATE, R.OPEN))
    z = cloud[finite, 2]
    assert eroded[finite[rows]].tobytes() == R.extremum(M, z, False).tobytes() and dilated[finite[rows]].tobytes() == R.extremum(M, z, True).tobytes()
    assert opened[finite[rows]].tobytes() == R.extremum(M, eroded[finite], True).tobytes()
    assert eroded[7] == cloud[7, 2] and opened[7] == cloud[7, 2]
    got = device(ctx, max_window_size=3)
    stays = (cloud[:, 2] - opened) < F32(0.15)
    want = np.where(stays, -1, 0).astype(np.int32)
    want[7] = -2
    assert got["removed_at"].tobytes() == want.tobytes() and np.array_equal(got["ground"], np.flatnonzero(want == -1))
    assert got["ground_after"].tolist() == [got["ground"].size] and ctx.pmf_stats()[0] == 1


# ---- schedules -----------------------------------------------------------------------------------------------------------------
def test_schedules_of_0_1_5_and_32_passes_and_one_more(ctx):
    cloud = scan(500)
    thirty_two = dict(max_window_size=10, exponential=False, base=0.3, cell_size=0.5)
    for kw, passes in ((dict(max_window_size=0), 0), (dict(max_window_size=3), 1), ({}, 5), (thirty_two, 32)):
        got = check(ctx, cloud, **kw)
        assert got["windows"].size == passes <= _lib.PMF_MAX_PASSES
        if passes == 0:
            assert got["ground"].tolist() == list(range(500)) and (got["removed_at"] == -1).all()
            assert np.array_equal(ctx.pmf_extract(False), cloud) and ctx.pmf_extract(True).shape == (0, 4)
    rc, n_ground, n_passes = ctx.pmf_filter_raw(**{**thirty_two, "max_window_size": 11})        # 10.1 < 11: a 33rd pass
    assert (rc, n_ground, n_passes) == (_lib.ERR_INVALID_ARG, 0, 0) and b"32" in ctx._L.icpgpu_last_error(ctx._h)
    assert ctx.pmf_fetch_raw(500, 40)[0] == _lib.ERR_INVALID_ARG
    with pytest.raises(R.Refused):
        R.schedule(**{**thirty_two, "max_window_size": 11})


# ---- calls ---------------------------------------------------------------------------------------------------------------------
REFUSED = [dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=math.nan), dict(cell_size=1e-46), dict(slope=-0.1), dict(slope=math.inf),
           dict(initial_distance=-1e-3), dict(initial_distance=math.nan), dict(max_distance=-1.0), dict(max_distance=math.inf), dict(max_distance=1e39),
           dict(base=1.0), dict(base=0.5), dict(base=math.nan), dict(exponential=False, base=0.0), dict(exponential=False, base=-2.0),
           dict(max_window_size=2**30, exponential=False, base=1.0), dict(max_window_size=2**31 - 1, cell_size=1e-3),
           dict(max_window_size=100, exponential=False, base=1e-30), dict(max_window_size=2**31 - 1, base=3e38, cell_size=3e38)]


def test_every_refusal_drops_the_previous_result(ctx):
    cloud = scan(63)
    ctx.search_set_input(cloud)
    for kw in REFUSED:
        with pytest.raises(R.Refused):
            R.schedule(**kw)
        assert ctx.pmf_filter_raw()[0] == 0 and ctx.pmf_fetch_raw(63, 5)[0] == 0
        assert ctx.pmf_filter_raw(**kw) == (_lib.ERR_INVALID_ARG, 0, 0), kw
        assert ctx.pmf_fetch_raw(63, 5)[0] == _lib.ERR_INVALID_ARG, kw
        with pytest.raises(IcpGpuError):
            ctx.pmf_extract(False)
    L, h = ctx._L, ctx._h
    n_ground, n_passes = C.c_size_t(), C.c_int32()
    assert ctx.pmf_filter_raw()[0] == 0
    assert L.icpgpu_progressive_morphological_filter(h, 33, 0.7, 0.15, 10.0, 1.0, 2.0, 1, None, C.byref(n_passes)) == _lib.ERR_INVALID_ARG
    assert ctx.pmf_fetch_raw(63, 5)[0] == _lib.ERR_INVALID_ARG
    assert L.icpgpu_progressive_morphological_filter(h, 33, 0.7, 0.15, 10.0, 1.0, 2.0, 1, C.byref(n_ground), None) == _lib.ERR_INVALID_ARG
    for w, op in ((0.0, R.OPEN), (-1.0, R.OPEN), (math.nan, R.ERODE), (math.inf, R.ERODE), (1.0, 4), (1.0, -1), (1e-46, R.CLOSE)):
        with pytest.raises(R.Refused):
            R.operator(cloud, w, op)
        rc, out = ctx.morphological_operator_raw(w, op)
        assert rc == _lib.ERR_INVALID_ARG and (out == -2).all()
    assert L.icpgpu_morphological_operator(h, 1.0, 0, None) == _lib.ERR_INVALID_ARG
    rc, n_ground, n_passes = ctx.pmf_filter_raw()             # a refused OPERATOR call leaves a filter result alone, and so does a good one
    assert rc == 0
    ctx.morphological_operator_raw(math.nan, 0)
    ctx.morphological_operator(5.0, R.CLOSE)
    rc, f = ctx.pmf_fetch_raw(n_ground, n_passes)
    assert rc == 0
    assert_same(f, R.run(cloud))
    with Context(0) as fresh:                                 # no search cloud
        assert fresh.pmf_filter_raw()[0] == _lib.ERR_INVALID_ARG and fresh._L.icpgpu_morphological_operator(fresh._h, 1.0, 0, None) == _lib.ERR_INVALID_ARG
        assert fresh._L.icpgpu_pmf_stats(fresh._h, None, None) == _lib.ERR_INVALID_ARG
        n_out = C.c_size_t()
        assert fresh._L.icpgpu_pmf_extract(fresh._h, 0, None, C.byref(n_out)) == _lib.ERR_INVALID_ARG


def test_fetch_capacities_and_null_subsets(ctx):
    cloud = scan(300)
    ctx.search_set_input(cloud)
    want = R.run(cloud)
    rc, n_ground, n_passes = ctx.pmf_filter_raw()
    assert (rc, n_ground, n_passes) == (0, want["ground"].size, 5)
    for cap_g, cap_p in ((n_ground - 1, 5), (n_ground, 4), (0, 0)):
        rc, f = ctx.pmf_fetch_raw(cap_g, cap_p)
        assert rc == _lib.ERR_INVALID_ARG and all((f[name] == -2).all() for name in NAMES)
    rc, f = ctx.pmf_fetch_raw(n_ground + 7, 9)               # room to spare: the tails stay as they were
    assert rc == 0 and (f["ground"][n_ground:] == -2).all() and (f["windows"][5:] == -2).all() and (f["ground_after"][5:] == -2).all()
    assert f["ground"][:n_ground].tobytes() == want["ground"].tobytes() and f["thresholds"][:5].tobytes() == want["thresholds"].tobytes()
    for subset in (("ground",), ("removed_at",), ("windows", "ground_after"), ()):
        rc, f = ctx.pmf_fetch_raw(n_ground, 5, want=subset)
        assert rc == 0
        for name in NAMES:
            assert f[name].tobytes() == want[name].tobytes() if name in subset else (f[name] == -2).all(), (subset, name)
    assert ctx.pmf_fetch_raw(n_ground - 1, 5, want=())[0] == _lib.ERR_INVALID_ARG    # the capacities count whatever is asked for


def test_extract_both_ways_and_the_view(ctx):
    cloud = scan(1000).copy()
    cloud[::50, 0] = np.nan
    ctx.search_set_input(cloud)
    want = R.run(cloud)
    mask = np.zeros(1000, bool)
    mask[want["ground"]] = True
    assert 0 < mask.sum() < 980
    ctx.pmf_filter_raw()
    for view in (False, True):
        assert ctx.pmf_extract(False, view=view).tobytes() == cloud[mask].tobytes()
        assert ctx.pmf_extract(True, view=view).tobytes() == cloud[~mask].tobytes()          # the NaN rows are "not ground": kept
    assert ctx.pmf_extract(False).tobytes() == R.extract(cloud, want["ground"], False).tobytes()
    n_out = C.c_size_t(99)
    assert ctx._L.icpgpu_pmf_extract(ctx._h, 0, None, C.byref(n_out)) == 0 and n_out.value == mask.sum()   # the count alone
    assert ctx._L.icpgpu_pmf_extract(ctx._h, 0, None, None) == _lib.ERR_INVALID_ARG
    assert ctx._L.icpgpu_pmf_extract_view(ctx._h, 0, None, C.byref(n_out)) == _lib.ERR_INVALID_ARG
    rc, f = ctx.pmf_fetch_raw(int(mask.sum()), 5)             # the result outlives its extracts
    assert rc == 0
    assert_same(f, want)


def test_one_host_wait_whatever_the_passes_and_five_identical_runs(ctx):
    cloud = scan(2000)
    ctx.search_set_input(cloud)
    for kw, passes in ((dict(max_window_size=3), 1), ({}, 5)):
        r = ctx.progressive_morphological_filter(**kw)
        assert r["windows"].size == passes and r["host_waits"] == 1
    waits, tests = ctx.pmf_stats()
    assert waits == 1 and 0 < tests < 5 * 2 * 2000 * 2000     # two sweeps a pass, fewer exact tests than every pair
    runs = [[a.tobytes() for a in device(ctx).values()] + [ctx.morphological_operator(9.0, R.OPEN).tobytes()] for _ in range(5)]
    assert all(run == runs[0] for run in runs[1:])
    assert ctx.progressive_morphological_filter(max_window_size=0)["host_waits"] == 0


def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    assert ctx.morphological_operator(float(g["open_window"]), R.OPEN).tobytes() == g["opened"].tobytes()
    got = device(ctx)
    assert_same(got, {name: g[name] for name in NAMES})


def test_the_operators_open_is_the_filters_first_pass(ctx):
    cloud = scan(1500)
    ctx.search_set_input(cloud)
    for kw, w in ((dict(max_window_size=3), 3.0), (dict(max_window_size=7, cell_size=3.0), 9.0)):
        got = device(ctx, **kw)
        assert got["windows"].tolist() == [w]
        opened = ctx.morphological_operator(float(got["windows"][0]), R.OPEN)
        stays = (cloud[:, 2] - opened) < got["thresholds"][0]
        assert np.array_equal(got["removed_at"] == -1, stays) and 0 < stays.sum() < 1500


def test_pcl_shaped_front_end():
    cloud = scan(800)
    pmf = ProgressiveMorphologicalFilter()
    with pytest.raises(IcpGpuError):
        pmf.extract()
    pmf.setInputCloud(cloud)
    assert pmf.extract().tobytes() == R.run(cloud)["ground"].tobytes()
    pmf.setMaxWindowSize(9)
    pmf.setSlope(1.0)
    pmf.setInitialDistance(0.3)
    pmf.setMaxDistance(2.5)
    pmf.setCellSize(0.5)
    pmf.setBase(3.0)
    want = R.run(cloud, max_window_size=9, slope=1.0, initial_distance=0.3, max_distance=2.5, cell_size=0.5, base=3.0)
    ground = pmf.extract()
    assert ground.tobytes() == want["ground"].tobytes() and pmf.last["thresholds"].tobytes() == want["thresholds"].tobytes()
    assert pmf.extractCloud(True).tobytes() == R.extract(cloud, ground, True).tobytes()
    pmf.setExponential(False)
    assert pmf.extract().tobytes() == R.run(cloud, max_window_size=9, slope=1.0, initial_distance=0.3, max_distance=2.5, cell_size=0.5, base=3.0,
                                            exponential=False)["ground"].tobytes()
