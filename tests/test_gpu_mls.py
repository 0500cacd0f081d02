"""Moving least squares on the device (icpgpu_moving_least_squares / icpgpu_mls_fetch / icpgpu_mls_stats; icp_mls.hip) against the
NumPy restatement (tests/mls_restated.py), bit for bit everywhere: the kept points and normals as float32, the indices, status and
n_neighbours as int32, plane7 and coeff10 as float64 compared as uint64, and the count.  There is no tolerance anywhere, with one
allowance: where both sides hold a NaN its sign and payload -- the processor's, not the rule's -- are not compared."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mls_cases as K
import mls_restated as R
import normals_restated as NR
from icpslam_amd import Context, IcpGpuError, _lib

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "mls_1k.npz")
CASES = {c[0]: c[1:] for c in K.hand_cases()}
scan, points = K.scan, K.points

_REF = {}


def ref(key, cloud, queries, radius, order, s=0.0):
    """The restatement's answer, computed once per (key, arguments) and left unchanged; key = None: not worth keeping."""
    if key is None:
        return R.project(cloud, queries, radius, order, s)
    k = (key, float(radius), int(order), float(s))
    if k not in _REF:
        _REF[k] = R.project(cloud, queries, radius, order, s)
        for a in _REF[k].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[k]


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = np.uint32 if a.itemsize == 4 else np.uint64
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def device(ctx, queries, radius, order, s=0.0, want_normals=True):
    """One call and one fetch: the restatement's dict, and that nothing was written past n_out."""
    rc, m, pts, nrm, index = ctx.moving_least_squares_raw(queries, radius, order, s, want_normals=want_normals)
    assert rc == 0, ctx.last_error() if hasattr(ctx, "last_error") else rc
    assert (pts[m:] == -2).all() and (index[m:] == -2).all() and (nrm is None or (nrm[m:] == -2).all())
    rc, rec = ctx.mls_fetch_raw(len(index))
    assert rc == 0
    return {"n_out": m, "points": pts[:m], "normals": None if nrm is None else nrm[:m], "index": index[:m], **rec}


def assert_same(got, want, what=""):
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for name in R.FIELDS:
        if got[name] is None:
            continue
        if not same_bits(got[name], want[name]):
            g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w)))) if g.dtype.kind == "f" else np.argwhere(g != w)
            raise AssertionError((what, name, len(bad), bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def check(ctx, key, cloud, queries, radius, order, s=0.0, what=""):
    got = device(ctx, queries, radius, order, s)
    assert_same(got, ref(key, cloud, queries, radius, order, s), f"{what} r={radius} order={order} s={s}")
    return got


# ---- sizes and rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 2000])
def test_sizes(ctx, n):
    cloud = scan(2000)[:n]
    ctx.search_set_input(cloud)
    for order in (2, 3):
        got = check(ctx, ("scan", n), cloud, None, 1.5, order)
    if n == 2000:
        assert set(np.unique(got["status"]).tolist()) >= {0, 1, 2} and got["n_neighbours"].max() > 100 and 0 < got["n_out"] < n


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_rows_of_exactly_these_lengths(ctx, order):
    """Rows of 0 (a non-finite point), 1, 2, 3, 5, 6, 7, 9, 10, 11, 63, 64, 65, 128, 129 and 300 entries: the status boundaries of
    both orders, and one, two, three and five passes of a wave over a row."""
    cloud = K.blobs().copy()
    starts = np.concatenate([[0], np.cumsum(K.BLOB_SIZES)])
    cloud = np.concatenate([cloud, np.full((1, 4), np.nan, F32)])
    ctx.search_set_input(cloud)
    got = check(ctx, "blobs+nan", cloud, None, K.BLOB_RADIUS, order)
    assert got["n_neighbours"][starts[1:] - 1].tolist() == list(K.BLOB_SIZES) and got["n_neighbours"][-1] == 0
    nc = R.n_coefficients(order)
    want_status = [0 if m < 3 else 1 if order < 2 or m < nc else 2 for m in K.BLOB_SIZES]
    assert got["status"][starts[1:] - 1].tolist() == want_status and got["status"][-1] == 0


@pytest.mark.parametrize("leaf", [0.2, 0.5, 1.0])
def test_voxel_filtered_scans(ctx, leaf):
    cloud = ctx.voxel_grid(scan(2000), leaf)
    assert 100 < len(cloud) <= 2000
    ctx.search_set_input(cloud)
    for order, radius in ((2, 3 * leaf), (3, 5 * leaf)):
        got = check(ctx, None, cloud, None, radius, order, what=f"leaf {leaf}")
    assert (got["status"] == 2).sum() > 50


# ---- the walks ---------------------------------------------------------------------------------------------------------------------
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
    """n = 1025 and a radius of 8.5 cells (ASSERTED, from the cell size in the library's debug line): more than the 8 shells the cube
    walk takes, so every row is found by a sweep.  Then the same points with eight far ones behind them: the cells grow until the
    radius takes the cube (ASSERTED).  The far points are in no row but their own, so the first 1 025 queries' answers must be the
    very same bits on both walks."""
    cloud = scan(1025)
    h = cell_size(ctx, cloud, monkeypatch, capfd)
    radius = 8.5 * h
    assert shells(radius, h) > 8 and radius < 300
    swept = check(ctx, None, cloud, None, radius, 2, what="sweep")
    far = points([[sx * 5000.0, sy * 5000.0, sz * 5000.0] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    both = np.concatenate([cloud, far])
    h2 = cell_size(ctx, both, monkeypatch, capfd)
    assert shells(radius, h2) <= 8
    cubed = check(ctx, None, both, None, radius, 2, what="cube")
    assert (cubed["n_neighbours"][1025:] == 1).all() and cubed["n_out"] == swept["n_out"]
    for name in ("status", "n_neighbours", "plane7", "coeff10"):
        assert same_bits(cubed[name][:1025], swept[name]), name
    assert same_bits(cubed["points"], swept["points"]) and same_bits(cubed["normals"], swept["normals"])


def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """5 000 points, 4 600 of them in one group 20 cm across inside a 400 m box: one cell holds more than 4 096 points and the grid
    refuses the cloud (ASSERTED, from the library's debug line).  Every row is then found by a sweep of the whole cloud; 150 of the
    group's points are the queries."""
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
    queries = np.concatenate([cloud[:150], cloud[4990:]])
    got = check(ctx, "refused", cloud, queries, 0.02, 2)
    assert got["status"][7] == 0 and got["n_neighbours"].max() > 100 and (got["status"] == 2).sum() > 100


# ---- queries, duplicates, ties, the hand cases, degenerate inputs ------------------------------------------------------------------
def test_queries_equal_to_disjoint_from_and_coincident_with_the_cloud(ctx):
    cloud = K.hemisphere(2)
    ctx.search_set_input(cloud)
    own = check(ctx, "hemi2", cloud, None, 0.45, 2)
    given = device(ctx, cloud.copy(), 0.45, 2)                                            # the same points, handed in
    assert_same(given, own)
    r = np.random.default_rng(3)
    lifted = cloud[::5].copy()
    lifted[:, :3] += r.normal(0, 0.03, (len(lifted), 3)).astype(F32)
    got = check(ctx, "hemi2-lifted", cloud, lifted, 0.45, 2)
    assert got["n_out"] == len(lifted) and K.radial_rms(got["points"]) < 0.5 * K.radial_rms(lifted)
    one = np.repeat(cloud[17:18], 70, axis=0)                                            # seventy queries on one cloud point
    got = check(ctx, "hemi2-one", cloud, one, 0.45, 3)
    assert len({got["points"][i].tobytes() for i in range(70)}) == 1
    far = points(r.uniform(50, 60, (5, 3)).astype(F32))
    assert check(ctx, "hemi2-far", cloud, far, 0.45, 2)["n_out"] == 0


def test_duplicated_points_and_lattice_ties(ctx):
    cloud = scan(600).copy()
    cloud[50:80] = cloud[400:430]
    cloud[300:310] = cloud[299]
    ctx.search_set_input(cloud)
    got = check(ctx, None, cloud, None, 1.5, 2)
    assert same_bits(got["coeff10"][50:80], got["coeff10"][400:430]) and same_bits(got["plane7"][50:80], got["plane7"][400:430])
    cube = K.lattice(6, 6, 6)                                                               # every distance tied many times over
    ctx.search_set_input(cube)
    for order in (2, 3):
        check(ctx, "cube", cube, None, 1.8, order)


@pytest.mark.parametrize("name", list(CASES))
def test_hand_cases(ctx, name):
    cloud, queries, radius, s = CASES[name]
    ctx.search_set_input(cloud)
    for order in (0, 2, 3):
        got = check(ctx, ("hand", name), cloud, queries, radius, order, s, what=name)
    if name in ("planar_lattice", "plane_x", "explicit_s"):
        assert got["points"].tobytes() == cloud.tobytes()
    if name in ("line", "coincident", "tiny_s"):
        assert (device(ctx, queries, radius, 2, s)["status"] == 3).all()
    if name == "far_from_origin":
        assert np.abs(cloud[:, :3]).min() > 115 and (got["status"] == 2).sum() > 500


def test_explicit_default_and_null_normals(ctx):
    cloud, _, radius, _ = CASES["paraboloid"]
    ctx.search_set_input(cloud)
    default = device(ctx, None, radius, 2, 0.0)
    explicit = device(ctx, None, radius, 2, radius * radius)
    assert_same(explicit, default)
    other = device(ctx, None, radius, 2, 0.05)
    assert not same_bits(other["coeff10"], default["coeff10"])
    bare = device(ctx, None, radius, 2, 0.0, want_normals=False)                           # out_nxyzc NULL
    assert bare["normals"] is None
    assert_same(bare, default)


def test_all_nan_and_empty_clouds(ctx):
    for cloud in (np.full((130, 4), np.nan, F32), np.empty((0, 4), F32)):
        ctx.search_set_input(cloud)
        got = check(ctx, None, cloud, None, 1.0, 2)
        assert got["n_out"] == 0 and got["points"].shape == (0, 4) and not got["status"].any()
        given = check(ctx, None, cloud, scan(63), 1.0, 3)                                 # finite queries over a cloud without a finite point
        assert given["n_out"] == 0 and not given["n_neighbours"].any()
    assert ctx.mls_stats() == 2
    ctx.search_set_input(np.empty((0, 4), F32))
    assert ctx.moving_least_squares_raw(None, 1.0)[:2] == (0, 0) and ctx.mls_stats() == 0  # n_q = 0: nothing to wait for
    assert ctx.mls_fetch_raw(0)[0] == 0


# ---- refusals, the fetch, the waits ------------------------------------------------------------------------------------------------
def test_refusals():
    inf, nan = float("inf"), float("nan")
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    with Context(0) as c:
        assert c.moving_least_squares_raw(scan(63), 1.0)[0] == _lib.ERR_INVALID_ARG         # no search cloud
        assert c.mls_fetch_raw(0)[0] == _lib.ERR_INVALID_ARG                               # ... and no result
        assert c._L.icpgpu_mls_stats(c._h, None) == _lib.ERR_INVALID_ARG
        cloud = scan(257)
        c.search_set_input(cloud)
        assert c.mls_fetch_raw(300)[0] == _lib.ERR_INVALID_ARG                             # a cloud, no result yet
        for radius in (0.0, -1.0, nan, inf):
            assert c.moving_least_squares_raw(None, radius)[0] == _lib.ERR_INVALID_ARG
        for order in (-1, 4, 100):
            assert c.moving_least_squares_raw(None, 1.0, order)[0] == _lib.ERR_INVALID_ARG
        for s in (-1.0, nan, inf, -0.5):
            assert c.moving_least_squares_raw(None, 1.0, 2, s)[0] == _lib.ERR_INVALID_ARG
        for n_q in (1, 256, 258):                                                          # null queries mean all n points, or none
            assert c.moving_least_squares_raw(None, 1.0, n_q=n_q)[0] == _lib.ERR_INVALID_ARG
        pts, nrm, index = np.zeros((257, 4), F32), np.zeros((257, 4), F32), np.zeros(257, np.int32)
        n_out = C.c_size_t(99)
        args = (c._h, None, 257, 1.0, 2, 0.0)
        P, N, I = pts.ctypes.data_as(fp), nrm.ctypes.data_as(fp), index.ctypes.data_as(ip)
        assert c._L.icpgpu_moving_least_squares(*args, None, N, I, C.byref(n_out)) == _lib.ERR_INVALID_ARG and n_out.value == 0
        assert c._L.icpgpu_moving_least_squares(*args, P, N, None, C.byref(n_out)) == _lib.ERR_INVALID_ARG
        assert c._L.icpgpu_moving_least_squares(*args, P, N, I, None) == _lib.ERR_INVALID_ARG
        rc, m, *_ = c.moving_least_squares_raw(None, 1.5)
        assert rc == 0 and m > 0 and c.mls_stats() == 2
        assert c.moving_least_squares_raw(None, nan)[0] == _lib.ERR_INVALID_ARG            # a refused call leaves no result behind
        assert c.mls_fetch_raw(257)[0] == _lib.ERR_INVALID_ARG and c._L.icpgpu_mls_stats(c._h, None) == _lib.ERR_INVALID_ARG
        assert c.moving_least_squares_raw(None, 1.5)[:2] == (0, m) and c.mls_fetch_raw(257)[0] == 0
        assert c.moving_least_squares_raw(None, 1.0, n_q=0)[:2] == (0, 0) and c.mls_fetch_raw(0)[0] == 0   # n_q = 0 with a cloud: an empty result
        c.search_set_input(scan(63))                                                       # the search cloud replaced: the result is gone
        assert c.mls_fetch_raw(257)[0] == _lib.ERR_INVALID_ARG
        with pytest.raises(IcpGpuError):
            c.moving_least_squares(-1.0)


def test_fetch_capacities_and_null_subsets(ctx):
    cloud = scan(600)
    ctx.search_set_input(cloud)
    want = ref("scan600", cloud, None, 1.5, 2)
    rc, m, *_ = ctx.moving_least_squares_raw(None, 1.5, 2)
    assert (rc, m) == (0, want["n_out"])
    for cap in (599, 0):
        rc, out = ctx.mls_fetch_raw(cap)
        assert rc == _lib.ERR_INVALID_ARG and all((a == -2).all() for a in out.values())   # nothing was written
    for _ in range(2):
        rc, out = ctx.mls_fetch_raw(600)
        assert rc == 0 and all(same_bits(out[f], want[f]) for f in out)
    rc, out = ctx.mls_fetch_raw(607)                                                        # room to spare
    assert rc == 0 and all(same_bits(out[f][:600], want[f]) and (out[f][600:] == -2).all() for f in out)
    for single in ("status", "n_neighbours", "plane7", "coeff10"):
        rc, out = ctx.mls_fetch_raw(600, want=(single,))
        assert rc == 0 and list(out) == [single] and same_bits(out[single], want[single])
    assert ctx._L.icpgpu_mls_fetch(ctx._h, 600, None, None, None, None) == 0               # every pointer NULL
    assert ctx.mls_stats() == 2


def test_two_host_waits_whatever_the_call(ctx):
    """The totals that size the rows, then the results with the kept count: two, for every order, with and without queries, whether
    anything is kept or not."""
    cloud = scan(600)
    ctx.search_set_input(cloud)
    for queries, radius, order in ((None, 1.5, 0), (None, 1.5, 3), (cloud[:40].copy(), 0.7, 2), (None, 1e-30, 2), (points([[900, 900, 900]]), 1.0, 2)):
        rc, m, *_ = ctx.moving_least_squares_raw(queries, radius, order)
        assert rc == 0 and ctx.mls_stats() == 2
    assert m == 0


def test_five_calls_give_identical_bytes(ctx):
    cloud = scan(2000)
    ctx.search_set_input(cloud)
    for order in (2, 3):
        runs = []
        for _ in range(5):
            got = device(ctx, None, 1.5, order)
            runs.append(b"".join(np.ascontiguousarray(got[f]).tobytes() for f in R.FIELDS))
        assert len(set(runs)) == 1


# ---- the golden fixture, the search's own rows, normal estimation, the chain -------------------------------------------------------
def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    for order in (2, 3):
        got = device(ctx, None, float(g["radius"]), order, float(g["sqr_gauss_param"]))
        assert_same(got, {"n_out": int(g[f"n_out_{order}"]), **{f: g[f"{f}_{order}"] for f in R.FIELDS}}, f"order {order}")


@pytest.mark.parametrize("radius", [0.7, 1.5])
def test_rows_are_the_radius_searchs_own(ctx, radius):
    cloud = scan(2000).copy()
    cloud[[5, 1000], [0, 2]] = [np.nan, np.inf]
    ctx.search_set_input(cloud)
    row_start, idx, _ = ctx.search_radius(None, radius)
    got = device(ctx, None, radius, 0)
    assert np.array_equal(got["n_neighbours"], np.diff(row_start).astype(np.int32))
    assert np.array_equal(got["index"], np.flatnonzero(np.diff(row_start) >= 3).astype(np.int32))


def test_plane_normals_agree_with_normal_estimation(ctx):
    """Orders 0 and 1 return the plane's normal: icpgpu_normal_estimation's at the same radius, up to sign and up to the two rules'
    arithmetic -- float32 moments there, float64 here.  MEASURED on the CPU between the two restatements on this cloud (scan(600),
    radius 1.5 m, the 578 rows of three or more entries): at most 3.33e-4 rad, at a row of six entries; the median is 1e-7 rad.
    Ten times the worst is asserted, for every row both sides keep."""
    cloud = scan(600)
    ctx.search_set_input(cloud)
    normals, counts = ctx.normal_estimation(None, radius=1.5)[:2]
    ref_n = NR.estimate(cloud, None, 0, 1.5)[0]
    want = ref("scan600", cloud, None, 1.5, 0)
    both = np.flatnonzero((want["status"] != 0) & np.isfinite(ref_n[:, 0]))

    def angles(mls_normals, index, ne):
        full = np.full((len(cloud), 3), np.nan)
        full[index] = mls_normals[:, :3]
        a, b = full[both], ne[both, :3].astype(F64)
        return np.arcsin(np.clip(np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)), 0, 1))

    measured = angles(want["normals"], want["index"], ref_n)
    print("plane normals against normal estimation (CPU, rad): worst", measured.max(), "median", np.median(measured), "rows", len(both))
    for order in (0, 1):
        got = device(ctx, None, 1.5, order)
        assert np.array_equal(got["n_neighbours"], counts)
        worst = angles(got["normals"], got["index"], normals).max()
        print("order", order, "device worst", worst)
        assert len(both) > 500 and worst <= 10 * 3.33e-4


def test_chain_smooths_the_normals_on_the_device(ctx):
    """MLS, then search_set_input(smoothed), then normal_estimation: on the noisy hemisphere the normals are closer to radial at the
    median than normal_estimation's on the raw points.  Two device results, no threshold beyond 'smaller'."""
    cloud = K.hemisphere(0)
    ctx.search_set_input(cloud)
    raw = ctx.normal_estimation(None, radius=0.3)[0]
    pts, nrm, index = ctx.moving_least_squares(0.45, 2)
    assert len(index) == len(cloud) and K.radial_rms(pts) <= 0.7 * K.radial_rms(cloud)
    assert np.median(K.radial_angle_deg(pts, nrm)) <= 5.0
    ctx.search_set_input(pts)
    smooth = ctx.normal_estimation(None, radius=0.3)[0]
    ok_raw, ok_smooth = np.isfinite(raw[:, 0]), np.isfinite(smooth[:, 0])
    before = np.median(K.radial_angle_deg(cloud[ok_raw], raw[ok_raw]))
    after = np.median(K.radial_angle_deg(pts[ok_smooth], smooth[ok_smooth]))
    print("chain: median angle to radial, degrees: raw", before, "after MLS", after)
    assert after < before


def test_record_on_request(ctx):
    cloud = K.hemisphere(1)
    ctx.search_set_input(cloud)
    pts, nrm, index, rec = ctx.moving_least_squares(0.45, 2, want_record=True)
    want = ref("hemi1", cloud, None, 0.45, 2)
    assert_same({"n_out": len(index), "points": pts, "normals": nrm, "index": index, **rec}, want)
