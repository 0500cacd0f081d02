"""The cropping and sampling filters on the device (icpgpu_pass_through, icpgpu_crop_box, icpgpu_uniform_sampling,
icpgpu_farthest_point_sampling and their observers) against the NumPy restatement (tests/sampling_restated.py): the kept and removed
indices, the measures and the output rows, bit for bit, at every size at which a kernel or the compaction changes its shape."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from icpslam_amd import IcpGpuError, _lib

import sampling_cases as SC
import sampling_restated as R
import voxel_edge_cases as vx

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "sampling_2k.npz")
ONE_MAX = R.FPS_ONE_WORKGROUP_MAX
KIND = {"pass": _lib.SUBSET_PASS_THROUGH, "crop": _lib.SUBSET_CROP_BOX, "uniform": _lib.SUBSET_UNIFORM_SAMPLING, "fps": _lib.SUBSET_FARTHEST_POINT_SAMPLING}
LAUNCHES = {"pass": 5, "crop": 5, "uniform": 8}   # fixed, whatever the cloud
T_POSE = R.crop_box_matrix(None, (0.4, -0.2, 0.1), (0.02, -0.03, 0.3))
BOX = ((-8.0, -6.0, -2.0), (10.0, 6.0, 1.0))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def expected(kind, cloud, args):
    if kind == "pass":
        kept = R.pass_through(cloud, *args)
    elif kind == "crop":
        kept = R.crop_box(cloud, *args)
    elif kind == "uniform":
        return R.uniform_sampling(cloud, *args)
    else:
        return R.farthest_point_sampling(cloud, *args)
    return kept, np.zeros(len(kept), F32)


def call(ctx, kind, cloud, args, view):
    fn = {"pass": ctx.pass_through, "crop": ctx.crop_box, "uniform": ctx.uniform_sampling, "fps": ctx.farthest_point_sampling}[kind]
    return fn(cloud, *args, view=view)


def check(ctx, kind, cloud, args, view=False, want=None):
    """One call against the restatement: output rows, kept, measure, removed, sizes and statistics."""
    kept, measure = want if want is not None else expected(kind, cloud, args)
    out = call(ctx, kind, cloud, args, view)
    f, st = ctx.subset_fetch(), ctx.subset_stats()
    what = (kind, len(cloud), args, view)
    assert same(f["kept"], kept), what
    assert same(f["measure"], measure), what
    assert same(out, np.asarray(cloud, F32)[kept]), what                     # the rows themselves, w carried through
    assert same(f["removed"], R.removed_of(len(cloud), kept)), what
    assert f["n_in"] == len(cloud) and st["kind"] == KIND[kind], what
    assert st["host_waits"] == 1 if len(kept) else st["host_waits"] in (0, 1), what   # (0: nothing was launched -- no row, no finite row, no sample)
    if len(kept) and kind != "fps":
        assert st["launches"] == LAUNCHES[kind] and st["path"] == 0, what
    return f, st


def bad_scan(n, seed=5):
    return SC.with_bad_rows(SC.scan(n, seed), SC.one_wave_of_bad_rows(n)) if n > 3 else SC.scan(n, seed)


# ---- all four filters ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.SIZES)
def test_all_four_at_every_size(ctx, n):
    for cloud in (SC.scan(n), bad_scan(n)):
        n_finite = int(R.finite_rows(cloud).sum())
        for negative in (False, True):
            check(ctx, "pass", cloud, (2, -1.2, 2.0, negative), view=negative)
            check(ctx, "crop", cloud, (*BOX, None, negative), view=not negative)
            check(ctx, "crop", cloud, (*BOX, T_POSE, negative), view=negative)
        check(ctx, "pass", cloud, (-1, 0.0, 0.0, True))
        for view in (False, True):
            check(ctx, "uniform", cloud, (1.0,), view=view)
            check(ctx, "fps", cloud, (min(5, n_finite), -1), view=view)
        check(ctx, "fps", cloud, (min(70, n_finite), -1))


def test_all_nan_and_empty_clouds(ctx):
    empty = np.empty((0, 4), F32)
    nan = SC.scan(300).copy()
    nan[:, 1] = np.nan
    for cloud in (empty, nan):
        for view in (False, True):
            for kind, args in (("pass", (2, -1.0, 1.0, False)), ("pass", (2, -1.0, 1.0, True)), ("pass", (-1, 0.0, 0.0, False)),
                               ("crop", (*BOX, None, True)), ("crop", (*BOX, T_POSE, False)), ("uniform", (0.5,)), ("fps", (0, -1))):
                f, st = check(ctx, kind, cloud, args, view=view)
                assert len(f["kept"]) == 0 and len(f["removed"]) == len(cloud)
        with pytest.raises(IcpGpuError):
            ctx.farthest_point_sampling(cloud, 1)                                  # more samples than finite rows


def test_fetch_capacities_and_null_outputs(ctx):
    cloud = bad_scan(1000)
    kept, measure = R.uniform_sampling(cloud, 2.0)
    n_out = C.c_size_t()
    L, h = ctx._L, ctx._h
    fp = cloud.ctypes.data_as(C.POINTER(C.c_float))
    assert L.icpgpu_uniform_sampling(h, fp, len(cloud), C.c_float(2.0), None, C.byref(n_out)) == 0       # out_xyzw NULL: the count alone
    assert n_out.value == len(kept)
    k = len(kept)
    rc, got_k, got_m, n_in, n_kept = ctx.subset_fetch_raw(0, want=())
    assert (rc, got_k, got_m, n_in, n_kept) == (0, None, None, 1000, k)                                   # both NULL: the sizes, whatever the capacity
    rc, got_k, got_m, n_in, n_kept = ctx.subset_fetch_raw(k - 1)
    assert rc == _lib.ERR_INVALID_ARG and (n_in, n_kept) == (1000, k)
    assert (got_k == -1).all() and (got_m == -1).all()                                                    # nothing written
    rc, got_k, got_m, _, _ = ctx.subset_fetch_raw(k + 3, want=("kept",))
    assert rc == 0 and got_m is None and same(got_k[:k], kept) and (got_k[k:] == -1).all()
    rc, got_k, got_m, _, _ = ctx.subset_fetch_raw(k, want=("measure",))
    assert rc == 0 and got_k is None and same(got_m, measure)
    rc, rem, n_rem = ctx.subset_removed_raw(0, want=False)
    assert (rc, rem, n_rem) == (0, None, 1000 - k)
    rc, rem, n_rem = ctx.subset_removed_raw(1000 - k - 1)
    assert rc == _lib.ERR_INVALID_ARG and n_rem == 1000 - k and (rem == -1).all()
    rc, rem, n_rem = ctx.subset_removed_raw(1000)
    assert rc == 0 and same(rem[:n_rem], R.removed_of(1000, kept)) and (rem[n_rem:] == -1).all()
    assert same(ctx.subset_fetch()["kept"], kept)                                                         # the result outlives its observers


def refused(ctx, fn, *args, code=_lib.ERR_INVALID_ARG):
    with pytest.raises(IcpGpuError) as e:
        fn(*args)
    assert e.value.code == code, (args[1:], e.value)
    rc, _, _, n_in, n_kept = ctx.subset_fetch_raw(0, want=())
    assert rc == _lib.ERR_INVALID_ARG and (n_in, n_kept) == (0, 0)                                        # nothing left to fetch
    assert ctx.subset_removed_raw(0, want=False)[0] == _lib.ERR_INVALID_ARG
    with pytest.raises(IcpGpuError):
        ctx.subset_stats()


def test_every_refusal_leaves_nothing_to_fetch(ctx):
    cloud = SC.with_bad_rows(SC.scan(300), [0, 5, 64, 299])
    n_finite = int(R.finite_rows(cloud).sum())

    def both(kind, args):
        """The validator refuses what the library refuses, after a call that left something to fetch."""
        check(ctx, "pass", cloud, (2, -1.0, 1.0, False))
        with pytest.raises((R.Refused, R.Unsupported)) as e:
            expected(kind, cloud, args)
        code = _lib.ERR_UNSUPPORTED if e.type is R.Unsupported else _lib.ERR_INVALID_ARG
        for view in (False, True):
            refused(ctx, lambda *a: call(ctx, kind, a[0], a[1], view), cloud, args, code=code)

    for args in ((3, 0.0, 1.0, False), (-2, 0.0, 1.0, False), (0, math.nan, 1.0, False), (1, 0.0, math.nan, True)):
        both("pass", args)
    for args in (((math.nan, 0, 0), (1, 1, 1), None, False), ((0, 0, 0), (1, math.nan, 1), T_POSE, True)):
        both("crop", args)
    for leaf in (0.0, -1.0, math.inf, math.nan):
        both("uniform", (leaf,))
    for args in ((n_finite + 1, -1), (1, -2), (1, 300), (1, 0), (1, 299), (0, 300)):
        both("fps", args)
    # a NULL cloud with rows, and a cloud beyond the size limit (refused before it is read)
    L, h, n_out = ctx._L, ctx._h, C.c_size_t()
    fp = cloud.ctypes.data_as(C.POINTER(C.c_float))
    assert L.icpgpu_pass_through(h, None, 5, 2, C.c_float(0), C.c_float(1), 0, None, C.byref(n_out)) == _lib.ERR_INVALID_ARG
    for fn, args in ((L.icpgpu_pass_through, (2, C.c_float(0), C.c_float(1), 0)), (L.icpgpu_uniform_sampling, (C.c_float(1.0),)),
                     (L.icpgpu_farthest_point_sampling, (1, -1))):
        assert fn(h, fp, 2**31 - 4096, *args, None, C.byref(n_out)) == _lib.ERR_INVALID_ARG and n_out.value == 0
        assert ctx.subset_fetch_raw(0, want=())[0] == _lib.ERR_INVALID_ARG
    assert L.icpgpu_pass_through(h, fp, 300, 2, C.c_float(0), C.c_float(1), 0, None, None) == _lib.ERR_INVALID_ARG


def test_both_refused_verdicts_of_the_plan(ctx):
    """UniformSampling refuses what PCL's VoxelGrid passes through and what wraps its index (boxes: tests/voxel_edge_cases.py)."""
    seen = set()
    for name, lo, hi, leaf, want in vx.boundary_boxes():
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and math.isfinite(leaf) and leaf > 0):
            continue
        cloud = SC.rows([lo, hi, lo, hi])
        if want == vx.PASS_THROUGH:
            refused(ctx, ctx.uniform_sampling, cloud, leaf, code=_lib.ERR_UNSUPPORTED)
        elif want == vx.DIRECT:
            check(ctx, "uniform", cloud, (leaf,))
        seen.add(want)
    assert {vx.PASS_THROUGH, vx.DIRECT} <= seen
    rng = np.random.default_rng(9000 + 2864)                                     # (tests/test_voxel_plan_host.py: the wrapped index)
    n = int(rng.integers(1, 120000))
    leaf = float(rng.choice([0.03, 0.1, 0.2, 0.35, 0.77, 2.0, 5.0]))
    c = np.ones((n, 4), F32)
    c[:, :3] = rng.normal(0, float(rng.choice([2.0, 30.0, 300.0])), (n, 3)).astype(F32)
    lo, hi = vx.bbox(c)
    assert vx.plan_exact(lo, hi, leaf)[0] == vx.WRAP
    refused(ctx, ctx.uniform_sampling, SC.rows([lo, hi]), leaf, code=_lib.ERR_UNSUPPORTED)


def test_five_identical_runs(ctx):
    cloud = SC.duplicated(5000)
    big = SC.rows(np.random.default_rng(8).normal(0, 20, (ONE_MAX + 3000, 3)))
    for kind, c, args in (("pass", cloud, (0, -5.0, 9.0, True)), ("crop", cloud, (*BOX, T_POSE, False)), ("uniform", cloud, (0.7,)),
                          ("uniform", cloud, (25.0,)), ("fps", cloud, (200, 17)), ("fps", big, (40, -1))):
        want = expected(kind, c, args)
        for run in range(5):
            check(ctx, kind, c, args, view=bool(run % 2), want=want)


def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    c = g["cloud"]
    z = [float(v) for v in g["z_limits"]]
    for neg in (0, 1):
        check(ctx, "pass", c, (2, *z, bool(neg)), want=(g[f"pass{neg}_kept"], np.zeros(len(g[f"pass{neg}_kept"]), F32)))
        check(ctx, "crop", c, (g["crop_min"], g["crop_max"], None, bool(neg)), want=(g[f"crop{neg}_kept"], np.zeros(len(g[f"crop{neg}_kept"]), F32)))
        check(ctx, "crop", c, (g["crop_min"], g["crop_max"], g["crop_T"], bool(neg)),
              want=(g[f"cropT{neg}_kept"], np.zeros(len(g[f"cropT{neg}_kept"]), F32)))
    for i, leaf in enumerate(g["leaves"]):
        check(ctx, "uniform", c, (float(leaf),), want=(g[f"uniform{i}_kept"], g[f"uniform{i}_measure"]))
    for i, (k, first) in enumerate(g["fps_cases"]):
        check(ctx, "fps", c, (int(k), int(first)), want=(g[f"fps{i}_kept"], g[f"fps{i}_measure"]))


# ---- the crops -----------------------------------------------------------------------------------------------------------------------
def test_pass_through_fields_and_limits(ctx):
    cloud = bad_scan(3000)
    for negative in (False, True):
        for field in (0, 1, 2):
            v = float(cloud[1234, field])
            for lo, hi in ((-3.0, 4.5), (v, v), (v, math.inf), (-math.inf, v), (-math.inf, math.inf), (4.5, -3.0), (R.FLT_MIN, R.FLT_MAX)):
                check(ctx, "pass", cloud, (field, lo, hi, negative))
        check(ctx, "pass", cloud, (-1, 4.5, -3.0, negative))
    f, _ = check(ctx, "pass", cloud, (-1, 0.0, 0.0, True))
    assert same(f["kept"], np.flatnonzero(R.finite_rows(cloud)).astype(np.int32))
    assert len(check(ctx, "pass", cloud, (2, 1.0, -1.0, False))[0]["kept"]) == 0                          # lo > hi keeps nothing
    exact = SC.rows([(0, 0, -1.0), (0, 0, -0.5), (0, 0, 0.25), (0, 0, 2.0), (np.nan, 0, 0.0)])
    assert check(ctx, "pass", exact, (2, -0.5, 2.0, False))[0]["kept"].tolist() == [1, 2, 3]
    assert check(ctx, "pass", exact, (2, -0.5, 2.0, True))[0]["kept"].tolist() == [0]


def test_crop_box_faces_transforms_and_extremes(ctx):
    f = SC.faces()
    on, off = [0] + list(range(1, 13, 2)), list(range(2, 13, 2))
    assert check(ctx, "crop", f, (SC.EGO_MIN, SC.EGO_MAX, None, False))[0]["kept"].tolist() == on         # all six faces are inside
    assert check(ctx, "crop", f, (SC.EGO_MIN, SC.EGO_MAX, None, True))[0]["kept"].tolist() == off
    assert check(ctx, "crop", f, (SC.EGO_MIN, SC.EGO_MAX, np.eye(4), False))[0]["kept"].tolist() == on    # ... through the identity's fma chains too
    cloud = bad_scan(3000)
    n_finite = int(R.finite_rows(cloud).sum())
    for negative in (False, True):
        for T in (None, T_POSE, R.crop_box_matrix(T_POSE, (30, 2, 0), (0, 0, 3.0))):
            check(ctx, "crop", cloud, (*BOX, T, negative))
            nothing = check(ctx, "crop", cloud, ((500, 500, 500), (501, 501, 501), T, negative))[0]
            everything = check(ctx, "crop", cloud, ((-math.inf,) * 3, (math.inf,) * 3, T, negative))[0]
            assert len(nothing["kept"]) == (n_finite if negative else 0) and len(everything["kept"]) == (0 if negative else n_finite)
    Tinf = np.eye(4, dtype=F32)
    Tinf[0, 0] = np.inf                                                                                    # 0 * inf: a NaN image is inside
    c = SC.rows([(0.0, 50.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
    box = ((-1, -100, -1), (1, 100, 1))
    assert check(ctx, "crop", c, (*box, Tinf, False))[0]["kept"].tolist() == [0, 2]
    assert check(ctx, "crop", c, (*box, Tinf, True))[0]["kept"].tolist() == [1]


# ---- uniform sampling -----------------------------------------------------------------------------------------------------------------
def cells_with(k, n_cells, seed=2):
    """n_cells cells of side 1 along a 3-D diagonal-free lattice, k rows in each, shuffled."""
    r = np.random.default_rng(seed + k)
    origin = np.stack(np.unravel_index(np.arange(n_cells) * 7 % 343, (7, 7, 7)), axis=1) * 3 - 9
    pts = (origin[:, None, :] + r.uniform(0.02, 0.98, (n_cells, k, 3))).reshape(-1, 3)
    return SC.rows(r.permutation(pts))


@pytest.mark.parametrize("k", [1, 2, 64, 65, 400])
def test_uniform_sampling_rows_per_cell(ctx, k):
    cloud = cells_with(k, 40)
    f, _ = check(ctx, "uniform", cloud, (1.0,))
    assert len(f["kept"]) == 40
    check(ctx, "uniform", cloud, (1.0,), view=True)
    check(ctx, "uniform", SC.with_bad_rows(cloud, [0, len(cloud) - 1]), (0.37,))


def test_uniform_sampling_shapes_of_clouds(ctx):
    one_cell = SC.rows(np.random.default_rng(3).uniform(0.1, 0.9, (3000, 3)))
    assert len(check(ctx, "uniform", one_cell, (1.0,))[0]["kept"]) == 1                                   # all rows in one cell
    lat = SC.lattice444()
    assert check(ctx, "uniform", lat, (1.0,))[0]["kept"].tolist() == list(range(64))                     # one row per cell
    assert check(ctx, "uniform", lat, (2.0,))[0]["kept"].tolist() == [21, 23, 29, 31, 53, 55, 61, 63]
    f, _ = check(ctx, "uniform", SC.tie_cells(), (1.0,))
    assert f["kept"].tolist() == [0, 3, 4] and f["measure"].tolist() == [0.0625, 0.25, 0.0625]           # ties: the lowest index
    for leaf in (0.05, 0.5, 4.0):
        check(ctx, "uniform", SC.duplicated(3000), (leaf,))                                              # duplicated rows: the first copy
        check(ctx, "uniform", SC.far_away(3000), (leaf,))                                                # 3 km from the origin
    big = SC.scan(200000, 7)
    for leaf in (0.5, 1.0):
        check(ctx, "uniform", big, (leaf,), view=True)


# ---- farthest point sampling ------------------------------------------------------------------------------------------------------------
def test_farthest_point_sampling_counts_and_first_rows(ctx):
    cloud = SC.duplicated(3000)
    for k in (0, 1, 2, 63, 64, 65):
        for first in (-1, 0, 2999):
            _, st = check(ctx, "fps", cloud, (k, first))
            assert st["path"] == (_lib.FPS_PATH_ONE if k else 0)
    f, st = check(ctx, "fps", cloud, (3000, -1))                                                         # every row, duplicates last
    assert sorted(f["kept"].tolist()) == list(range(3000)) and st["launches"] == 2
    zeros = int((f["measure"] == 0).sum())
    assert zeros >= 900 and (f["measure"][-zeros:] == 0).all() and (np.diff(f["kept"][-zeros:]) > 0).all()
    bad = SC.with_bad_rows(cloud, [0, 1, 64, 2999])
    check(ctx, "fps", bad, (int(R.finite_rows(bad).sum()), -1))
    check(ctx, "fps", bad, (65, 2998))


def test_farthest_point_sampling_lattice_ties(ctx):
    f, _ = check(ctx, "fps", SC.lattice444(), (8, 0))
    assert f["kept"].tolist() == [0, 63, 7, 28, 49, 14, 35, 56] and f["measure"][:3].tolist() == [math.inf, 27.0, 10.0]
    check(ctx, "fps", SC.lattice444(), (64, -1))
    base = [(0, 0, 0), (5, 0, 0), (0, 7, 0)]
    f, _ = check(ctx, "fps", SC.rows(base + base[::-1] + [(1, 1, 1)]), (7, -1))
    assert f["kept"].tolist() == [0, 2, 1, 6, 3, 4, 5]


def test_farthest_point_sampling_both_shapes_at_their_edge(ctx):
    """n = ICPGPU_FPS_ONE_WORKGROUP_MAX - 1, the constant, + 1: the path on each side, and the two shapes' answers equal on a cloud just
    above the edge whose rows past its prefix just below are not finite."""
    r = np.random.default_rng(12)
    full = SC.rows(r.normal(0, 15, (ONE_MAX + 1, 3)))
    full[1::1000, :3] = full[0, :3]                                                                       # duplicates of the first point
    for n, path in ((ONE_MAX - 1, _lib.FPS_PATH_ONE), (ONE_MAX, _lib.FPS_PATH_ONE), (ONE_MAX + 1, _lib.FPS_PATH_MANY)):
        for k in (5, 70):
            _, st = check(ctx, "fps", full[:n], (k, -1))
            assert st["path"] == path and st["launches"] == (2 if path == _lib.FPS_PATH_ONE else k + 2)
        check(ctx, "fps", full[:n], (5, n - 1), view=True)
    above = full.copy()
    above[ONE_MAX - 1:, 0] = np.nan                                                                       # the same finite rows as the prefix
    below = above[:ONE_MAX - 1]
    want = R.farthest_point_sampling(below, 70, -1)
    f1, s1 = check(ctx, "fps", below, (70, -1), want=want)
    f2, s2 = check(ctx, "fps", above, (70, -1), want=want)
    assert (s1["path"], s2["path"]) == (_lib.FPS_PATH_ONE, _lib.FPS_PATH_MANY)
    assert same(f1["kept"], f2["kept"]) and same(f1["measure"], f2["measure"])


def test_farthest_point_sampling_many_workgroups(ctx):
    cloud = SC.with_bad_rows(SC.scan(40000, 9), [0, 1023, 1024, 39999])
    _, st = check(ctx, "fps", cloud, (300, -1), view=True)
    assert st["path"] == _lib.FPS_PATH_MANY and st["launches"] == 302 and st["host_waits"] == 1


@pytest.mark.parametrize("n", [2**20 - 1, 2**20, 2**20 + 1])
def test_farthest_point_sampling_around_the_grid_cap(ctx, n):
    """The many-workgroup shape's grid is capped at 1024 workgroups of 1024 rows: one row short of a second trip, the cap, one row past it.
    (The other kernels of this section have no cap: DESIGN.md section 5.)"""
    r = np.random.default_rng(31)
    cloud = SC.rows(r.normal(0, 40, (2**20 + 1, 3)))[:n]
    cloud[n - 1, :3] = (900.0, -900.0, 50.0)                                                              # the last row is the second sample
    f, st = check(ctx, "fps", cloud, (3, 0), view=True)
    assert f["kept"][1] == n - 1 and st["path"] == _lib.FPS_PATH_MANY
    check(ctx, "pass", cloud, (0, -10.0, 25.0, True), view=True)
