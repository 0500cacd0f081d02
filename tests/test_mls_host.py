"""CPU tests of the moving least squares projection (pcl::MovingLeastSquares, added under C-ABI 1.2): the restatement
(tests/mls_restated.py) against a literal loop in exact rationals, against answers known by hand (tests/mls_cases.py), on the
end-to-end hemisphere and against the golden fixture; exp_neg and wsum on their own; the host build of the kernels' shared
definitions (tests/cpp/mls_host_check.cpp: icp_exp.h, icp_jacobi3.h, icp_mls.h) against the restatement, bit for bit; and the ABI of
the three entry points, which needs no GPU."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import mls_cases as K
import mls_restated as R
import search_restated as S
from icpslam_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "rows_f", "mls_1k.npz")
F32, F64 = np.float32, np.float64
CASES = {c[0]: c[1:] for c in K.hand_cases()}
SYMBOLS = ("icpgpu_moving_least_squares", "icpgpu_mls_fetch", "icpgpu_mls_stats")


def run(name, order):
    cloud, queries, radius, s = CASES[name]
    return cloud, R.project(cloud, queries, radius, order, s)


def same_bits(a, b) -> bool:
    """Equal bit for bit, a NaN matching any NaN (a NaN's sign and payload are the processor's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = np.uint32 if a.itemsize == 4 else np.uint64
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


# ---- exp_neg and wsum ----------------------------------------------------------------------------------------------------------
def ulps(got, want):
    return np.abs(got - want) / np.spacing(want)


def test_exp_neg_is_within_two_ulp_of_libm():
    """Measured: at most 1.0 ulp from math.exp on these 100 000 arguments (and on 1.2 million more)."""
    r = np.random.default_rng(7)
    a = np.concatenate([-r.uniform(0, 708, 60000), -10.0 ** r.uniform(-12, 0, 20000), -r.uniform(0, 40, 20000)])
    got = R.exp_neg(a)
    want = np.array([math.exp(v) for v in a])
    worst = float(ulps(got, want).max())
    print("exp_neg: worst ulp", worst)
    assert worst <= 2.0
    assert R.exp_neg(0.0) == 1.0 and R.exp_neg(-0.0) == 1.0
    assert ulps(R.exp_neg(-708.0), math.exp(-708.0)) <= 2.0 and R.exp_neg(-708.0) > 2.2250738585072014e-308      # still a normal number
    assert R.exp_neg(np.nextafter(-708.0, -1000.0)) == 0.0 and R.exp_neg(-1e300) == 0.0 and R.exp_neg(-np.inf) == 0.0
    assert np.isnan(R.exp_neg(np.nan))
    assert [c.hex() for c in R.EXP_C[:4]] == ["0x1.0000000000000p+0", "0x1.0000000000000p+0", "0x1.0000000000000p-1", "0x1.5555555555555p-3"]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 129])
def test_wsum_against_fsum(m):
    """A term passes through at most ceil(m / 64) additions in its partial and six in the fold: the issue's bound of 64 + 6 additions
    of relative error 2^-53 each, on the sum of the magnitudes, holds with room."""
    r = np.random.default_rng(m)
    terms = r.normal(size=m) * 10.0 ** r.uniform(-6, 6, m)
    got, want = R.wsum(terms), math.fsum(terms.tolist())
    assert abs(got - want) <= 70 * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
    ints = r.integers(-2 ** 40, 2 ** 40, m).astype(F64)
    assert R.wsum(ints) == math.fsum(ints.tolist())
    both = R.wsum(np.stack([terms, ints], 1))
    assert both[0] == got and both[1] == math.fsum(ints.tolist())                       # several sums at once: the same bits


def test_wsum_takes_the_lanes_order():
    """Entries 0, 64 and 128 share partial 0: 1e16 + 1 + 1 loses both ones there, where entries 0, 1 and 2 -- three partials -- meet as
    (1e16 + 1) + 1 too (the fold pairs 0 with 2 before 1), but entries 0, 1 and 3 meet as 1e16 + (1 + 1)."""
    terms = np.zeros(130)
    terms[0], terms[64], terms[128] = 1e16, 1.0, 1.0
    assert R.wsum(terms) == 1e16 != math.fsum(terms.tolist()) == 1e16 + 2.0
    assert R.wsum(np.array([1e16, 1.0, 1.0])) == 1e16 and R.wsum(np.array([1e16, 1.0, 0.0, 1.0])) == 1e16 + 2.0
    assert R.wsum(np.zeros(0)) == 0.0 and math.copysign(1.0, R.wsum(np.array([-0.0]))) == 1.0   # the partials start at +0.0


# ---- the restatement against the exact loop --------------------------------------------------------------------------------------
WELL_CONDITIONED = 1e-4


def test_restatement_against_the_exact_loop_on_the_hemisphere():
    """Order 2, radius 0.45 m, every fourth query of the hemisphere (seed 0): the restatement's float64 rule against exact sums, an
    exact solve and numpy's eigh.  MEASURED on the 143 well-conditioned status-2 queries (reciprocal condition number of A above
    1e-4; 8.3 % of the 156 fall below): the plane normals differ by at most 8.7e-16 rad, the coefficients by at most 2.9e-18 in
    max |c - c_exact| / max |c_exact| x rcond(A) -- a relative error of at most 5.6e-15.  Ten times those are asserted."""
    cloud = K.hemisphere(0)
    want = R.project(cloud, None, 0.45, 2)
    only = range(0, len(cloud), 4)
    exact = R.project_exact(cloud, None, 0.45, 2, align_with=want["plane7"][:, :3], only=only)
    rows = np.array(list(only))
    assert np.array_equal(exact["status"][rows], want["status"][rows]) and np.array_equal(exact["n_neighbours"], want["n_neighbours"])
    fitted = rows[want["status"][rows] == 2]
    well = fitted[exact["rcond"][fitted] > WELL_CONDITIONED]
    share_below = 1.0 - len(well) / len(fitted)
    angle = np.linalg.norm(np.cross(exact["normal"][rows], want["plane7"][rows, :3]), axis=1)
    dev = np.abs(exact["coeff"][well, :6] - want["coeff10"][well, :6]).max(1) / np.abs(exact["coeff"][well, :6]).max(1)
    print("exact loop: queries", len(fitted), "below the threshold", share_below, "normal angle", angle.max(), "coefficients x rcond",
          (dev * exact["rcond"][well]).max(), "relative", dev.max())
    assert len(fitted) > 100 and share_below <= 0.10
    assert angle.max() <= 8.7e-15
    assert (dev * exact["rcond"][well]).max() <= 2.9e-17
    assert np.abs(exact["centroid"][rows] - want["plane7"][rows, 3:6]).max() <= 1e-14 * 8.0        # (coordinates of up to 8 m)


def test_order_three_against_the_exact_loop():
    """Order 3, radius 0.6 m, every sixteenth query: the ten-coefficient systems are worse conditioned (median rcond 6e-5), so
    the bound is the same product with the condition number: MEASURED 2.2e-18 at most, ten times that asserted."""
    cloud = K.hemisphere(0)
    want = R.project(cloud, None, 0.6, 3)
    rows = np.arange(0, len(cloud), 16)
    exact = R.project_exact(cloud, None, 0.6, 3, align_with=want["plane7"][:, :3], only=rows)
    assert np.array_equal(exact["status"][rows], want["status"][rows])
    fitted = rows[want["status"][rows] == 2]
    dev = np.abs(exact["coeff"][fitted] - want["coeff10"][fitted]).max(1) / np.abs(exact["coeff"][fitted]).max(1)
    print("order 3: queries", len(fitted), "coefficients x rcond", (dev * exact["rcond"][fitted]).max())
    assert len(fitted) > 30 and (dev * exact["rcond"][fitted]).max() <= 2.2e-17
    assert np.isnan(want["coeff10"][want["status"] == 1]).all()


# ---- answers known by hand -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, axis", [("planar_lattice", 2), ("plane_x", 0)])
@pytest.mark.parametrize("order", [0, 2, 3])
def test_a_planar_lattice_stays_where_it_is(name, axis, order):
    """Every point kept and unmoved, the normal along the axis exactly -- along z the frame takes its second branch, along x its first
    --, curvature 0 and every coefficient 0."""
    cloud, got = run(name, order)
    assert got["n_out"] == len(cloud) and np.array_equal(got["index"], np.arange(len(cloud)))
    assert got["points"].tobytes() == cloud.tobytes()
    want_n = np.zeros(3)
    want_n[axis] = 1
    assert np.array_equal(np.abs(got["plane7"][:, :3]), np.broadcast_to(want_n, (len(cloud), 3))) and not got["plane7"][:, 6].any()
    assert np.array_equal(np.abs(got["normals"][:, :3]), np.broadcast_to(want_n.astype(F32), (len(cloud), 3))) and not got["normals"][:, 3].any()
    if order >= 2:
        ran = got["n_neighbours"] >= R.n_coefficients(order)
        assert set(got["status"][ran].tolist()) <= {2, 3} and (got["status"][~ran] == 1).all() and (got["status"] == 2).sum() > 50
        nc = R.n_coefficients(order)
        assert not got["coeff10"][got["status"] == 2, :nc].any() and np.isnan(got["coeff10"][:, nc:]).all()
    else:
        assert (got["status"] == 1).all() and np.isnan(got["coeff10"]).all()
    U, V = R.frame_of(got["plane7"][:1, :3])
    assert (V[0, 0] == 0 and abs(V[0, 1]) == 1) if axis == 2 else (abs(V[0, 1]) == 1 and V[0, 2] == 0)
    assert abs(U[0, (axis + 1) % 3 if axis == 2 else 2]) == 1


def test_paraboloid_coefficients_at_the_apex():
    """z = a x^2 + b y^2: at the apex the plane is z = const, N = (0, 0, +-1), U = +-x, V = +-y, and the fit reproduces the surface:
    c = (-f(Q), 0, b, 0, 0, a) times N's sign -- the issue's (0, 0, b, 0, 0, a) with the plane's offset from the apex in c_0 -- within
    1e-9, and the projected point is the apex again."""
    a, b = K.PARABOLOID
    cloud, got = run("paraboloid", 2)
    apex = len(cloud) // 2
    assert not cloud[apex, :3].any() and got["status"][apex] == 2 and got["n_neighbours"][apex] > 12
    N, c = got["plane7"][apex, :3], got["coeff10"][apex]
    sign = 1.0 if N[2] > 0 else -1.0
    assert abs(abs(N[2]) - 1) < 1e-12
    plane_z = got["plane7"][apex, 5]                                             # the centroid's height: the plane's
    assert np.abs(c[:6] - sign * np.array([-plane_z, 0, b, 0, 0, a])).max() < 1e-9
    where = list(got["index"]).index(apex)
    assert np.abs(got["points"][where, :3]).max() < 1e-7 and got["points"][where, 3] == 1
    n = got["normals"][where, :3]
    assert abs(abs(n[2]) - 1) < 1e-6 and np.abs(n[:2]).max() < 1e-6


def test_collinear_and_coincident_clouds():
    """A row on a line along y: the covariance has one entry, N = (1, 0, 0) -- the lowest index among the two zero eigenvalues --, u is
    0 for every entry, the fourth pivot is 0 and the solve yields NaN: status 3 in the restatement and a zero pivot in the exact
    loop alike; the plane's projection is kept.  A coincident cloud: covariance 0, N = (1, 0, 0), status 3."""
    cloud, queries, radius, s = CASES["line"]
    got = R.project(cloud, None, 1.6, 2)
    exact = R.project_exact(cloud, None, 1.6, 2)
    assert (got["status"] == 3).all() and (exact["status"] == 3).all() and exact["singular"].all()
    assert got["n_out"] == 40 and got["points"].tobytes() == cloud.tobytes()
    assert np.array_equal(got["plane7"][:, :3], np.broadcast_to([1.0, 0, 0], (40, 3))) and np.isnan(got["coeff10"][:, 0]).all()
    cloud, got = run("coincident", 2)
    assert (got["status"] == 3).all() and got["points"].tobytes() == cloud.tobytes() and (got["n_neighbours"] == 9).all()
    assert np.array_equal(got["plane7"], np.broadcast_to([1.0, 0, 0, 3, -2, 7, 0], (9, 7))) and not got["normals"][:, 3].any()
    assert R.project_exact(cloud, None, 0.5, 2)["singular"].all()
    for order in (0, 1):
        assert (run("coincident", order)[1]["status"] == 1).all()


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_rows_at_the_status_boundaries(order):
    """Rows of exactly 1, 2, 3, 5, 6, 7, 9, 10, 11, ... entries: dropped below 3, plane only below nc, the fit from nc on."""
    cloud, got = run("blobs", order)
    starts = np.concatenate([[0], np.cumsum(K.BLOB_SIZES)])
    last = starts[1:] - 1                                                         # each group's last point
    assert got["n_neighbours"][last].tolist() == list(K.BLOB_SIZES)
    nc = R.n_coefficients(order)
    for m, st in zip(K.BLOB_SIZES, got["status"][last]):
        assert st == (0 if m < 3 else 1 if order < 2 or m < nc else 2), (m, st)
    ran = got["status"] >= 2
    assert np.isnan(got["coeff10"][~ran]).all() and np.isfinite(got["coeff10"][ran, :nc]).all() and np.isnan(got["coeff10"][:, nc:]).all()
    assert np.isnan(got["plane7"][got["status"] == 0]).all() and np.isfinite(got["plane7"][got["status"] != 0]).all()
    assert got["n_out"] == (got["status"] != 0).sum() == len(cloud) - 3 and np.array_equal(got["index"], np.flatnonzero(got["status"]))


def test_sqr_gauss_param_default_explicit_and_tiny():
    cloud, default = run("planar_lattice", 2)
    _, explicit = run("explicit_s", 2)
    assert all(same_bits(default[f], explicit[f]) for f in R.FIELDS)                # 0 means radius * radius, in double
    para, radius = CASES["paraboloid"][0], CASES["paraboloid"][2]
    assert not all(same_bits(R.project(para, None, radius, 2, 0.05)[f], R.project(para, None, radius, 2)[f]) for f in R.FIELDS)
    for name in ("tiny_s", "small_s"):                                              # the neighbours' weights underflow: A is singular
        cloud, got = run(name, 2)
        plane = R.project(cloud, None, CASES[name][2], 0)
        assert (got["status"] == 3).all() and got["points"].tobytes() == plane["points"].tobytes()
        assert got["normals"].tobytes() == plane["normals"].tobytes()
    assert R.exp_neg(-(0.125 ** 2) / 1e-7) == 0.0 and 0.0 < R.exp_neg(-(0.125 ** 2) / 2.5e-5) < 1e-270


def test_nan_rows_and_nan_queries():
    cloud, got = run("nan_rows", 2)
    bad = ~np.isfinite(cloud[:, :3]).all(1)
    assert bad.sum() == 4 and (got["status"][bad] == 0).all() and (got["n_neighbours"][bad] == 0).all() and not np.isin(np.flatnonzero(bad), got["index"]).any()
    assert np.isfinite(got["points"]).all() and (got["status"] == 2).sum() > 100
    clean = R.project(cloud[~bad], None, CASES["nan_rows"][2], 2)                    # non-finite points are in no row
    assert clean["points"].tobytes() == got["points"].tobytes() and clean["normals"].tobytes() == got["normals"].tobytes()
    cloud, got = run("nan_queries", 2)
    assert (got["status"][[3, 17, 30]] == 0).all() and got["n_out"] == 40 - 3 - (got["n_neighbours"][np.isfinite(K.nan_queries()).all(1)] < 3).sum()


def test_queries_off_the_cloud_are_projected_onto_it():
    cloud = K.hemisphere(2)
    r = np.random.default_rng(3)
    lifted = cloud[::7].copy()
    lifted[:, :3] += (0.05 * (lifted[:, :3] - K.HEMISPHERE_CENTRE.astype(F32)) / 2.0).astype(F32)      # 5 cm off the surface, radially
    got = R.project(cloud, lifted, 0.45, 2)
    assert got["n_out"] == len(lifted) and K.radial_rms(lifted) > 0.045 and K.radial_rms(got["points"]) < 0.012
    far = K.points(r.uniform(50, 60, (5, 3)))
    assert R.project(cloud, far, 0.45, 2)["n_out"] == 0


def test_empty_and_all_nan_clouds_and_refusals():
    for cloud in (np.empty((0, 4), F32), np.full((7, 4), np.nan, F32)):
        got = R.project(cloud, None, 1.0, 2)
        assert got["n_out"] == 0 and got["points"].shape == (0, 4) and not got["status"].any() and np.isnan(got["plane7"]).all()
    for bad in ((0.0, 2, 0.0), (-1.0, 2, 0.0), (float("nan"), 2, 0.0), (float("inf"), 2, 0.0), (1.0, -1, 0.0), (1.0, 4, 0.0), (1.0, 2, -1.0),
                (1.0, 2, float("nan")), (1.0, 2, float("inf"))):
        with pytest.raises(R.Refused):
            R.project(K.scan(63), None, *bad)


# ---- the end-to-end scene ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hemisphere_is_smoothed(seed):
    """Order 2, radius 0.45 m on 1 cm of radial noise: the radial rms falls from 9.7-10.1 mm to 5.0-5.1 mm (MEASURED: ratios 0.520,
    0.506, 0.515), the normals' median angle to the radial direction is 1.0-1.1 degrees."""
    cloud = K.hemisphere(seed)
    got = R.project(cloud, None, 0.45, 2)
    before, after = K.radial_rms(cloud), K.radial_rms(got["points"])
    angle = float(np.median(K.radial_angle_deg(got["points"], got["normals"])))
    print("hemisphere", seed, len(cloud), before, after, after / before, angle)
    assert 550 < len(cloud) < 650 and 0.009 < before < 0.011 and got["n_out"] == len(cloud)
    assert after <= 0.7 * before
    assert angle <= 5.0


# ---- the kernels' shared definitions, built for the host ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mls") / "mls_host_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "icpslam_amd", "csrc"),
                           os.path.join(HERE, "cpp", "mls_host_check.cpp"), "-o", exe])
    return exe


def host_rows(exe, tmp_path, cloud, queries, radius, order, s):
    cloud = np.ascontiguousarray(cloud, F32)
    q = cloud if queries is None else np.ascontiguousarray(queries, F32)
    start, idx, _ = S.radius(cloud, queries, radius, 0)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<4id", len(cloud), len(q), order, len(idx), radius * radius if s == 0 else s))
        for a in (cloud, q, start.astype(np.int32), idx.astype(np.int32)):
            f.write(a.tobytes())
    subprocess.check_call([exe, "rows", str(src), str(dst)])
    raw, n, at = dst.read_bytes(), len(q), 0
    out = {}
    for name, dtype, width in (("status", np.int32, 1), ("plane7", F64, 7), ("coeff10", F64, 10), ("points", F32, 4), ("normals", F32, 4)):
        out[name] = np.frombuffer(raw, dtype, n * width, at).reshape((n, width) if width > 1 else (n,))
        at += out[name].nbytes
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_shared_definitions_on_the_host_give_the_restatements_bits(host_check, tmp_path, name):
    """icp_exp.h, icp_jacobi3.h and icp_mls.h -- what the kernels call -- compiled for the host and driven over the hand cases' rows."""
    cloud, queries, radius, s = CASES[name]
    for order in (0, 2, 3):
        want = R.project(cloud, queries, radius, order, s)
        got = host_rows(host_check, tmp_path, cloud, queries, radius, order, s)
        kept = want["index"]
        assert np.array_equal(got["status"], want["status"]), (name, order)
        assert same_bits(got["plane7"], want["plane7"]) and same_bits(got["coeff10"], want["coeff10"]), (name, order)
        assert same_bits(got["points"][kept], want["points"]) and same_bits(got["normals"][kept], want["normals"]), (name, order)


def test_exp_neg_on_the_host_gives_the_restatements_bits(host_check):
    r = np.random.default_rng(11)
    a = np.concatenate([-r.uniform(0, 708, 20000), -10.0 ** r.uniform(-300, 3, 5000), [0.0, -0.0, -708.0, np.nextafter(-708.0, -1e3), -1e300, -np.inf]])
    text = "\n".join(f"{b:016x}" for b in a.view(np.uint64))
    out = subprocess.run([host_check, "exp"], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = np.array([int(w, 16) for w in out], np.uint64)
    assert got.tobytes() == np.ascontiguousarray(R.exp_neg(a)).view(np.uint64).tobytes()


# ---- the golden fixture and the ABI ------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    assert 800 < len(g["cloud"]) < 1300 and os.path.getsize(GOLDEN) < 400 * 1024
    for order in (2, 3):
        got = R.project(g["cloud"], None, float(g["radius"]), order, float(g["sqr_gauss_param"]))
        assert got["n_out"] == int(g[f"n_out_{order}"])
        for f in R.FIELDS:
            assert same_bits(got[f], g[f"{f}_{order}"]), (order, f)
        assert set(np.unique(got["status"]).tolist()) >= {1, 2}


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "icpgpu.h")).read()
    for symbol in SYMBOLS:
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS
    assert "#define ICPGPU_MLS_MAX_ORDER 3\n" in header


def test_header_compiles_as_c_with_the_prototypes(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){\n'
                   '  int (*f1)(icpgpu_ctx*, const float*, size_t, double, int, double, float*, float*, int32_t*, size_t*) = icpgpu_moving_least_squares;\n'
                   '  int (*f2)(icpgpu_ctx*, size_t, int32_t*, int32_t*, double*, double*) = icpgpu_mls_fetch;\n'
                   '  int (*f3)(const icpgpu_ctx*, int32_t*) = icpgpu_mls_stats;\n'
                   '  size_t n_out = 7;\n'
                   '  printf("%d %d %d %d %d\\n", ICPGPU_MLS_MAX_ORDER, ICPGPU_HEADER_VERSION, f1(NULL, NULL, 0, 1.0, 2, 0.0, NULL, NULL, NULL, &n_out),\n'
                   '         f2(NULL, 0, NULL, NULL, NULL, NULL), f3(NULL, NULL));\n'
                   '  return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    order, version, rc1, rc2, rc3 = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert (order, version) == (3, 1002) and rc1 == rc2 == rc3 == _lib.ERR_INVALID_ARG       # a null context is refused: no GPU is needed


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_moving_least_squares(None, None, 0, 1.0, 2, 0.0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_mls_fetch(None, 0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_mls_stats(None, None) == _lib.ERR_INVALID_ARG
