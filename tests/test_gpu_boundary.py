"""Boundary estimation on the device (icpgpu_boundary_estimation; icp_boundary.hip) against the NumPy restatement
(tests/boundary_restated.py), bit for bit everywhere: boundary as bytes, n_neighbours, n_directions and witness as int32.  There is no
tolerance anywhere."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import boundary_cases as C
import boundary_restated as B
import normals_restated as N
from icpslam_amd import BoundaryEstimation, Context, IcpGpuError, _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "boundary_2k.npz")
scan, points = C.scan, C.points
PI, HALF_PI, ABOVE = math.pi, C.HALF_PI, C.ABOVE_HALF_PI


@functools.lru_cache(maxsize=None)
def scan_part(n: int):
    """(the first n points of the 2 000-point scan, their restated normals from 10 neighbours -- NaN below three points)."""
    cloud = scan(2000)[:n]
    normals = N.estimate(cloud, None, 10, 0.0)[0]
    normals.setflags(write=False)
    return cloud, normals


def assert_same(got, want, what=""):
    for name in B.FIELDS:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g != w)
            raise AssertionError((what, name, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist()))


def check(ctx, cloud, queries, normals, k, radius, angle, what=""):
    """One call on the search cloud in place against the restatement."""
    got = ctx.boundary_estimation(normals, queries, k, radius, angle)
    assert_same(got, B.estimate(cloud, queries, normals, k, radius, angle), f"{what} k={k} r={radius} angle={angle}")
    return got


# ---- sizes, k, thresholds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129, 2000])
def test_sizes(ctx, n):
    cloud, normals = scan_part(n)
    ctx.search_set_input(cloud)
    a = check(ctx, cloud, None, normals, 30, 0.0, HALF_PI)
    b = check(ctx, cloud, None, normals, 0, 1.5, 2.5)
    if n == 2000:
        for got in (a, b):
            assert 200 < got["boundary"].sum() < 1800                            # both answers occur
        assert b["n_neighbours"].max() > 128 and {1, 2, 3} <= set(b["n_neighbours"].tolist())


@pytest.mark.parametrize("k", [1, 2, 3, 4, 63, 64])
def test_k(ctx, k):
    cloud, normals = scan_part(600)
    ctx.search_set_input(cloud)
    got = check(ctx, cloud, None, normals, k, 0.0, PI)
    assert bool(got["boundary"].any()) == (k >= 3)


@pytest.mark.parametrize("angle", [0.1, HALF_PI, ABOVE, PI])
def test_thresholds(ctx, angle):
    cloud, normals = scan_part(2000)
    ctx.search_set_input(cloud)
    got = check(ctx, cloud, None, normals, 30, 0.0, angle)
    assert 50 < got["boundary"].sum()
    lattice = C.lattice(9, 9, 1)
    ctx.search_set_input(lattice)
    got = check(ctx, lattice, None, C.normals_of(81), 0, 1.1, angle)
    assert got["boundary"][40] == (1 if angle <= HALF_PI else 0)                 # the centre's four gaps are exactly pi / 2


# ---- rows and direction counts of exactly these sizes ------------------------------------------------------------------------
def blobs(sizes, seed):
    """Tight flat groups (within 2 cm, 2 mm thick) of exactly the given numbers of points, 50 m apart."""
    r = np.random.default_rng(seed)
    xyz = [np.array([50.0 * g, 0, 0]) + r.uniform(-0.01, 0.01, (m, 3)) * [1, 1, 0.1] for g, m in enumerate(sizes)]
    return points(np.concatenate(xyz).astype(F32))


@pytest.mark.parametrize("angle", [HALF_PI, 2.5])
def test_radius_rows_of_exactly_these_sizes(ctx, angle):
    sizes = (1, 2, 3, 63, 64, 65, 128, 129, 400, 4)
    cloud = blobs(sizes, 17)
    cloud[-1, 1] = np.nan                                                        # a row of 0 entries; its group becomes one of three
    ctx.search_set_input(cloud)
    got = check(ctx, cloud, None, C.normals_of(len(cloud)), 0, 0.5, angle)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert got["n_neighbours"][starts[:-1]].tolist() == [1, 2, 3, 63, 64, 65, 128, 129, 400, 3] and got["n_neighbours"][-1] == 0
    big = slice(starts[8], starts[9])
    assert 0 < got["boundary"][big].sum() < 400                                  # the group's rim, not its middle


def fan(n_directions, arc, extra_same=3, extra_normal=2):
    """A centre, copies of it, points straight along the normal, and exactly n_directions points spread over `arc` radians around it
    at radii of their own: the centre's row has 1 + extra_same + extra_normal + n_directions entries and n_directions directions."""
    t = 0.1 + arc * np.arange(n_directions) / n_directions
    rad = 0.2 + 0.5 * ((np.arange(n_directions) * 7) % 11) / 11.0
    pts = [[0, 0, 0]] * (1 + extra_same) + [[0, 0, 0.1 * (s + 1)] for s in range(extra_normal)]
    pts += [[r * math.cos(a), r * math.sin(a), 0] for r, a in zip(rad, t)]
    return points(np.array(pts)[np.random.default_rng(n_directions).permutation(len(pts))])


@pytest.mark.parametrize("arc", [2 * PI, PI])
@pytest.mark.parametrize("n_directions", [63, 64, 65, 127, 128, 129])
def test_rows_with_exactly_this_many_directions(ctx, n_directions, arc):
    cloud = fan(n_directions, arc)
    centre = int(np.flatnonzero((cloud[:, :3] == 0).all(axis=1))[0])
    ctx.search_set_input(cloud)
    got = check(ctx, cloud, None, C.normals_of(len(cloud)), 0, 5.0, HALF_PI)
    assert got["n_neighbours"][centre] == n_directions + 6 and got["n_directions"][centre] == n_directions
    assert got["boundary"][centre] == (0 if arc > 4 else 1)


def test_k_rows_with_sixty_four_directions(ctx):
    cloud = fan(64, PI, extra_same=0, extra_normal=0)                            # 65 points: the centre's row of k = 64 has 63 directions
    ctx.search_set_input(cloud)
    got = check(ctx, cloud, None, C.normals_of(65), 64, 0.0, HALF_PI)
    assert got["n_directions"].max() == 63
    queries = points([[0.01, 0.01, 0]])                                          # off the cloud: all 64 of a row are directions
    got = check(ctx, cloud, queries, C.normals_of(1), 64, 0.0, HALF_PI)
    assert got["n_directions"].tolist() == [64]


# ---- queries -----------------------------------------------------------------------------------------------------------------
def test_queries_equal_to_disjoint_from_and_coincident_with_the_cloud(ctx):
    cloud, normals = scan_part(2000)
    ctx.search_set_input(cloud)
    own = check(ctx, cloud, None, normals, 20, 0.0, 2.5)
    same = check(ctx, cloud, cloud.copy(), normals, 20, 0.0, 2.5, "equal")
    assert all(own[f].tobytes() == same[f].tobytes() for f in B.FIELDS)
    shifted = cloud[::5].copy()
    shifted[:, :3] += F32(0.07)
    for k, radius in ((20, 0.0), (0, 1.5)):
        got = check(ctx, cloud, shifted, normals[::5], k, radius, 2.0, "disjoint")
        assert 0 < got["boundary"].sum() < len(shifted)
    one = np.repeat(cloud[700:701], 70, axis=0)
    got = check(ctx, cloud, one, np.repeat(normals[700:701], 70, axis=0), 0, 1.5, 2.0, "coincident queries")
    assert len(set(got["witness"].tolist())) == 1 and got["n_neighbours"][0] >= 3


def test_duplicated_points_and_a_coincident_cloud(ctx):
    cloud, normals = scan_part(600)
    cloud = cloud.copy()
    cloud[50:80] = cloud[400:430]
    cloud[300:310] = cloud[299]
    ctx.search_set_input(cloud)
    for k, radius in ((12, 0.0), (0, 2.0)):
        check(ctx, cloud, None, normals, k, radius, 2.5)
    same = points([[3, -2, 7]] * 70)
    ctx.search_set_input(same)
    got = check(ctx, same, None, C.normals_of(70), 0, 0.5, HALF_PI)
    assert (got["n_neighbours"] == 70).all() and not got["n_directions"].any() and not got["boundary"].any()


def test_nan_rows_queries_and_normals_and_a_zero_normal(ctx):
    cloud, normals = scan_part(600)
    cloud, normals = cloud.copy(), normals.copy()
    cloud[[0, 64, 200], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    cloud[100] = np.nan
    normals[[10, 11, 12], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    normals[13, :3] = 0.0
    normals[14] = np.nan
    ctx.search_set_input(cloud)
    for k, radius in ((15, 0.0), (0, 2.0)):
        got = check(ctx, cloud, None, normals, k, radius, 2.5)
        bad = [0, 64, 100, 200]
        assert not got["n_neighbours"][bad].any() and not got["boundary"][bad].any() and (got["witness"][bad] == -1).all()
        assert not got["n_directions"][10:15].any() and not got["boundary"][10:15].any() and (got["n_neighbours"][11:15] >= 3).all()
    queries = cloud[90:110].copy()
    queries[3, 2] = np.nan
    check(ctx, cloud, queries, normals[90:110], 0, 2.0, 2.5, "nan queries")
    nothing = np.full((130, 4), np.nan, F32)
    ctx.search_set_input(nothing)
    got = check(ctx, nothing, None, C.normals_of(130), 5, 0.0, HALF_PI)
    assert not got["n_neighbours"].any()


@pytest.mark.parametrize("name", [case[0] for case in C.hand_cases()])
def test_hand_cases(ctx, name):
    cloud, queries, normals, k, radius, angle = {c[0]: c[1:] for c in C.hand_cases()}[name]
    ctx.search_set_input(cloud)
    check(ctx, cloud, queries, normals, k, radius, angle, name)


# ---- a cloud without a grid --------------------------------------------------------------------------------------------------
def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """5 000 points, 4 600 of them in one group 20 cm across inside a 400 m box: one cell holds more than 4 096 points and the grid
    refuses the cloud (ASSERTED, from the library's debug line).  Every query then sweeps the whole cloud."""
    r = np.random.default_rng(41)
    group = points((r.uniform(-30, 30, 3) + r.normal(0, 0.03, (4600, 3)) * [1, 1, 0.05]).astype(F32))
    cloud = np.concatenate([group, points(r.uniform(-200, 200, (400, 3)).astype(F32))])
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=5000 .* max=(\d+) ", capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found and int(found[-1]) > 4096
    queries = cloud[::8].copy()
    normals = C.normals_of(len(queries))
    for k, radius in ((12, 0.0), (0, 0.02)):
        got = check(ctx, cloud, queries, normals, k, radius, 2.5, "refused")
        assert 0 < got["boundary"].sum() < len(queries) and got["n_neighbours"][0] > 3
    own = ctx.boundary_estimation(C.normals_of(5000), None, 8, 0.0, 2.5)        # the cloud's own points, sampled
    want = B.estimate(cloud, queries, normals, 8, 0.0, 2.5)
    assert all(own[f][::8].tobytes() == want[f].tobytes() for f in B.FIELDS)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def refused(call, code=_lib.ERR_INVALID_ARG):
    with pytest.raises(IcpGpuError) as e:
        call()
    assert e.value.code == code


def test_refusals():
    inf, nan = float("inf"), float("nan")
    cloud, normals = scan_part(257)
    with Context(0) as c:
        refused(lambda: c.boundary_estimation(normals, cloud, 5))                # no search cloud
        c.search_set_input(cloud)
        for k, radius in ((0, 0.0), (5, 1.0), (0, -1.0), (0, nan), (0, inf), (-1, 0.0), (65, 0.0)):
            refused(lambda: c.boundary_estimation(normals, None, k, radius))
        for angle in (0.0, -0.5, math.nextafter(PI, 4.0), nan, inf):
            refused(lambda: c.boundary_estimation(normals, None, 5, 0.0, angle))
        refused(lambda: c.boundary_estimation(None, None, 5))                    # null normals
        refused(lambda: c.boundary_estimation(normals, None, 5, n_q=100))        # n_q against null queries
        rc = c._L.icpgpu_boundary_estimation(c._h, normals.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, 257, 5, 0.0, 1.0, None, None, None, None)
        assert rc == _lib.ERR_INVALID_ARG                                        # a null boundary
        assert c._L.icpgpu_boundary_estimation(c._h, None, None, 0, 5, 0.0, 1.0, None, None, None, None) == 0   # n_q = 0 writes nothing
        rc, out = c.boundary_estimation_raw(normals, None, 5, 0.0, 1.0, want=())  # the three optional outputs may be NULL
        assert rc == 0 and list(out) == ["boundary"] and out["boundary"].tobytes() == B.estimate(cloud, None, normals, 5, 0.0, 1.0)["boundary"].tobytes()
        rc, out = c.boundary_estimation_raw(normals, None, 5, 0.0, nan)
        assert rc == _lib.ERR_INVALID_ARG and (out["boundary"] == 0xFE).all() and (out["witness"] == -2).all()   # nothing was written


# ---- repeatability, the fixture, the device's own normals, the class ---------------------------------------------------------
def test_five_calls_give_identical_bytes(ctx):
    cloud, normals = scan_part(2000)
    ctx.search_set_input(cloud)
    for k, radius in ((30, 0.0), (0, 1.5)):
        runs = set()
        for _ in range(5):
            got = ctx.boundary_estimation(normals, None, k, radius, 2.5)
            runs.add(b"".join(np.ascontiguousarray(got[f]).tobytes() for f in B.FIELDS))
        assert len(runs) == 1


def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    assert_same(ctx.boundary_estimation(g["normals"], None, int(g["k"]), 0.0, float(g["k_angle"])), {f: g[f"k_{f}"] for f in B.FIELDS}, "k")
    assert_same(ctx.boundary_estimation(g["normals"], None, 0, float(g["radius"]), float(g["radius_angle"])),
                {f: g[f"radius_{f}"] for f in B.FIELDS}, "radius")


def test_the_devices_own_normals_fed_straight_back(ctx):
    cloud = scan(2000)
    ctx.search_set_input(cloud)
    for k, radius in ((30, 0.0), (0, 1.5)):
        normals, counts = ctx.normal_estimation(None, k, radius)
        got = check(ctx, cloud, None, normals, k, radius, HALF_PI)
        assert np.array_equal(got["n_neighbours"], counts) and 100 < got["boundary"].sum() < 1900
        assert not got["boundary"][np.isnan(normals[:, 0])].any()


def test_pcl_shaped_class():
    cloud, normals = scan_part(600)
    be = BoundaryEstimation()
    with pytest.raises(IcpGpuError):
        be.compute()
    be.setInputCloud(cloud)
    be.setInputNormals(normals)
    be.setSearchMethod(None)
    with pytest.raises(IcpGpuError):
        be.compute()                                                            # neither k nor a radius
    be.setKSearch(20)
    assert be.getAngleThreshold() == HALF_PI
    got = be.compute()
    assert got.dtype == np.uint8 and got.tobytes() == B.estimate(cloud, None, normals, 20, 0.0, HALF_PI)["boundary"].tobytes()
    be.setKSearch(0)
    be.setRadiusSearch(1.5)
    be.setAngleThreshold(2.5)
    queries = cloud[::3].copy()
    be.setSearchSurface(cloud)
    be.setInputCloud(queries)
    be.setInputNormals(normals[::3])
    assert be.compute().tobytes() == B.estimate(cloud, queries, normals[::3], 0, 1.5, 2.5)["boundary"].tobytes()
    assert_same(be.getLastResult(), B.estimate(cloud, queries, normals[::3], 0, 1.5, 2.5))
    be.setInputNormals(normals)
    with pytest.raises(IcpGpuError):
        be.compute()                                                            # 600 normals for 200 input points
