"""CPU tests of the segment moments' rule (include/icpgpu.h, "segment moments"): the vectorised restatement against the literal loop
with Fraction sums, bit for bit; what the hand clouds must give; every refusal against a Python validator; the golden fixture; the
shared definitions of icp_segment.h compiled for the host (tests/cpp/segment_host_check.cpp) against the restatement, bit for bit; and
the ABI of the two entry points, which needs no GPU."""
import ctypes as C
import functools
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cluster_restated as CR
import segment_cases as K
import segment_restated as R
from icpslam_amd import _lib, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "rows_f", "segment_2k.npz")
F32, F64 = np.float32, np.float64
SYMBOLS = ("icpgpu_segment_moments", "icpgpu_segment_stats")
EPS = 2.0 ** -52


def of(case):
    start, idx = R.csr(case.segments)
    return R.records(case.cloud, start, idx)


@functools.lru_cache(maxsize=None)
def scan_clusters():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 3000, 5)
    start, idx, _, _ = CR.extract(cloud, 0.6, 1)
    return cloud, start, idx


# ---- the two restatements -------------------------------------------------------------------------------------------------------
def test_vectorised_rule_and_literal_loop_agree_on_a_scans_clusters():
    cloud, start, idx = scan_clusters()
    sizes = np.diff(start)
    assert sizes.size > 100 and sizes.max() > 200 and sizes.min() == 1          # very unequal rows
    assert R.same_records(R.records(cloud, start, idx), R.records_literal(cloud, start, idx)) == []


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_vectorised_rule_and_literal_loop_agree_on_every_hand_cloud(name):
    case = K.CASES[name]
    start, idx = R.csr(case.segments)
    assert R.same_records(R.records(case.cloud, start, idx), R.records_literal(case.cloud, start, idx)) == []
    assert R.RECORD.itemsize == 400


# ---- by hand ------------------------------------------------------------------------------------------------------------------------
def test_axis_parallel_box_lattice():
    """Spacings 2 x 3 x 5 with four points per axis: variances 5, 11.25, 31.25.  The axes are z, y and z x y = -x exactly; the dims
    are exact; the oriented box is the axis-aligned one."""
    r = of(K.box_lattice())[0]
    assert (r["count"], r["status"], r["first"]) == (64, R.OK, 0)
    assert r["eigenvalues"].tolist() == [31.25, 11.25, 5.0]
    assert r["axes"].tolist() == [0, 0, 1, 0, 1, 0, -1, 0, 0]
    assert r["obb_dims"].tolist() == [15.0, 9.0, 6.0]
    assert r["obb_position"].tolist() == r["centroid"].tolist() == list(K.BOX_CENTRE)
    assert r["aabb_min"].tolist() == [1.0, -2.0, 0.5] and r["aabb_max"].tolist() == [7.0, 7.0, 15.5]
    assert ((r["aabb_max"] + r["aabb_min"]) / 2).tolist() == r["obb_position"].tolist()
    assert sorted((r["aabb_max"] - r["aabb_min"]).tolist()) == sorted(r["obb_dims"].tolist())
    assert r["cov"].tolist() == [5.0, 0, 0, 11.25, 0, 31.25]


def test_box_lattice_yawed_by_30_degrees():
    """The coordinates are float32 roundings of the rotated lattice (2^-21 at magnitude 8..16), so the dims hold within a few of
    those and the position is the centre within one."""
    r = of(K.box_yawed())[0]
    step = 2.0 ** -20
    assert np.abs(r["obb_dims"] - [15.0, 9.0, 6.0]).max() < 4 * step
    assert np.abs(r["obb_position"] - K.BOX_CENTRE).max() < 2 * step
    assert np.abs(r["centroid"] - K.BOX_CENTRE).max() < step
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    want = np.array([[0, 0, 1], [-s, c, 0], [-c, -s, 0]])      # major z; middle: the lattice's y, largest component positive; minor = z x y'
    assert np.abs(r["axes"].reshape(3, 3) - want).max() < 1e-6


def test_cube_lattice_three_tied_eigenvalues():
    """The covariance is diagonal with three equal entries: no rotation runs, no column moves, no sign changes -- the identity."""
    r = of(K.cube_lattice())[0]
    assert r["eigenvalues"][0] == r["eigenvalues"][1] == r["eigenvalues"][2] == 45.0 / 27.0 - 1.0   # (S_xx / m - mean_x^2 about K = the corner)
    assert r["axes"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert r["obb_dims"].tolist() == [2.0, 2.0, 2.0] and r["obb_position"].tolist() == [1.0, 1.0, 1.0]


def test_two_tied_eigenvalues_keep_the_lower_column_first():
    """x and y tied above z: x stays major.  y and z tied above x: y is major, z middle, and the minor axis is y x z = +x."""
    pts = np.array([[i, j, 0.5 * k] for i in range(3) for j in range(3) for k in range(3)], F64)
    r = of(K.whole(pts))[0]
    assert r["axes"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and r["eigenvalues"][0] == r["eigenvalues"][1] > r["eigenvalues"][2]
    r = of(K.whole(pts[:, [2, 0, 1]]))[0]
    assert r["axes"].tolist() == [0, 1, 0, 0, 0, 1, 1, 0, 0]


def test_sign_rule_follows_the_component_of_largest_magnitude():
    r = of(K.whole([[-t, 0.5 * t, 0.0] for t in range(5)] + [[0.1, 0.2, 0.0]]))[0]
    major = r["axes"][:3]
    assert abs(major[0]) > abs(major[1]) and major[0] > 0 > major[1]


def test_planar_segments():
    r = of(K.plane_axis_parallel())[0]
    assert r["eigenvalues"][2] == 0.0 and r["obb_dims"].tolist() == [4.0, 1.5, 0.0] and r["axes"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    r = of(K.plane_tilted())[0]
    assert abs(r["eigenvalues"][2]) < 16 * EPS * r["eigenvalues"][0] and r["obb_dims"][2] < 4e-7   # (float32 z: 2^-23 of 1.9, twice, along the normal)
    n = np.array([0.37, -0.21, -1.0]) / np.linalg.norm([0.37, -0.21, -1.0])
    assert abs(abs(r["axes"][6:] @ n) - 1.0) < 1e-6


def test_collinear_coincident_and_single():
    r = of(K.collinear())[0]
    d = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    assert np.abs(r["axes"][:3] - d).max() < 4 * EPS and abs(r["eigenvalues"][1]) < 64 * EPS and abs(r["eigenvalues"][2]) < 64 * EPS
    assert abs(r["obb_dims"][0] - 2.0 * math.sqrt(14.0)) < 16 * EPS and r["obb_dims"][1] < 1e-14 and r["obb_dims"][2] < 1e-14
    for case, count, at in ((K.coincident(), 5, [1.5, -2.25, 3.0]), (K.single_point(), 1, [7.0, -8.0, 9.5])):
        r = of(case)[0]
        assert r["count"] == count and r["status"] == R.OK
        assert not r["moments"].any() and not r["cov"].any() and not r["eigenvalues"].any() and not r["obb_dims"].any()
        assert r["axes"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
        assert r["centroid"].tolist() == r["obb_position"].tolist() == r["K"].tolist() == at
        assert r["aabb_min"].tolist() == r["aabb_max"].tolist() == at
    assert of(K.single_point())[0]["first"] == 1


def test_nan_rows_empty_segments_and_k():
    rec = of(K.nan_segments())
    assert rec["status"].tolist() == [R.EMPTY, R.OK, R.OK, R.EMPTY, R.OK] and rec["count"].tolist() == [0, 3, 4, 0, 1]
    for r in rec[[0, 3]]:
        assert r.tobytes() == np.zeros(1, R.RECORD)[0].tobytes()[:8] + struct.pack("<i", R.EMPTY) + bytes(R.RECORD.itemsize - 12)
    assert rec["first"].tolist() == [0, 3, 3, 0, 7]                      # (a NaN first entry: K is the next finite one)
    assert rec[1]["K"].tolist() == [1.0, 0.0, 0.0] and rec[1]["centroid"].tolist() == [2.0, 1.0 / 3.0, 1.0 / 3.0]
    assert rec[2]["aabb_max"].tolist() == [4.0, 2.0, 2.0]


def test_repeats_overlaps_and_order():
    case = K.repeated_and_overlapping()
    rec = of(case)
    assert rec["count"].tolist() == [7, 12, 12, 18, 18]
    pts = case.cloud[case.segments[0], :3].astype(F64)
    assert np.abs(rec[0]["centroid"] - pts.mean(axis=0)).max() < 4 * EPS    # (index 5 three times, index 0 twice)
    both = of(K.Case(case.cloud, [case.segments[1]]))[0], of(K.Case(case.cloud, [case.segments[2]]))[0]
    assert both[0].tobytes() == rec[1].tobytes() and both[1].tobytes() == rec[2].tobytes()   # (a segment's record is its own)
    unsorted, ordered = rec[3], rec[4]
    assert unsorted["first"] != ordered["first"] and unsorted["K"].tolist() != ordered["K"].tolist()
    assert np.abs(unsorted["centroid"] - ordered["centroid"]).max() <= 4 * EPS
    assert np.abs(unsorted["cov"] - ordered["cov"]).max() <= 16 * EPS
    assert unsorted["aabb_min"].tobytes() == ordered["aabb_min"].tobytes() and unsorted["aabb_max"].tobytes() == ordered["aabb_max"].tobytes()


def test_negative_zero_orders_below_positive_zero():
    rec = of(K.signed_zeros())
    sign = lambda a: np.signbit(a).tolist()   # noqa: E731
    for r in rec:                            # x holds both zeros whatever the list order; y only -0; z only +0
        assert sign(r["aabb_min"]) == [True, True, False] and sign(r["aabb_max"]) == [False, True, False]
    assert R.ordered_extremes(np.array([0.0, -0.0]))[0].tobytes() == np.array(-0.0).tobytes()
    assert R.ordered_extremes(np.array([-0.0, 0.0]))[1].tobytes() == np.array(0.0).tobytes()


def test_segment_three_kilometres_from_the_origin():
    """The centroid about K agrees with the exact mean of the float32 coordinates within 1 ulp of double.  The textbook form, float64
    sums about the origin, is measured beside it and printed.  Measured on this cloud: the centroid 0.36 ulp either way (400 addends
    of 3000 m lose nothing a double cannot hold); cov_xx 1.8 ulp by the rule against 4.9e6 ulp for E[x x] - E[x] E[x] about the
    origin, which is where the digits go."""
    case = K.far_from_origin()
    r = of(case)[0]
    pts = case.cloud[:, :3].astype(F64)
    exact_mean = [Fraction(0)] * 3
    for p in pts:
        exact_mean = [m + Fraction(float(x)) for m, x in zip(exact_mean, p)]
    exact_mean = [m / len(pts) for m in exact_mean]
    ulp = np.spacing(np.abs(r["centroid"]))
    ours = max(abs(float(Fraction(float(c)) - m)) / u for c, m, u in zip(r["centroid"], exact_mean, ulp))
    naive_mean = pts.sum(axis=0) / len(pts)
    naive = max(abs(float(Fraction(float(c)) - m)) / u for c, m, u in zip(naive_mean, exact_mean, ulp))
    exact_xx = sum((Fraction(float(p[0])) - exact_mean[0]) ** 2 for p in pts) / len(pts)
    naive_xx = (pts[:, 0] * pts[:, 0]).sum() / len(pts) - naive_mean[0] * naive_mean[0]
    cov_ulp = float(np.spacing(float(exact_xx)))
    ours_cov, naive_cov = abs(float(Fraction(float(r["cov"][0])) - exact_xx)) / cov_ulp, abs(float(Fraction(float(naive_xx)) - exact_xx)) / cov_ulp
    print(f"centroid: {ours:.2f} ulp (about K) against {naive:.2f} ulp (about the origin); cov_xx: {ours_cov:.1f} ulp against {naive_cov:.3g} ulp")
    assert ours <= 1.0
    assert naive_cov > 1e3 * max(ours_cov, 1.0)          # (the loss the difference from K is there to avoid)


def test_one_sum_whose_terms_span_fourteen_decades():
    case = K.wide_sum()
    r = of(case)[0]
    x = case.cloud[:, 0].astype(F64)
    terms = x * x
    assert terms[terms > 0].min() < 1.1e-10 and terms.max() == 1e4
    assert r["moments"][0] == math.fsum(terms.tolist()) == float(sum(Fraction(float(t)) for t in terms))
    assert r["moments"][0] != float(np.sum(terms[::-1].astype(F32)))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def refusal_cases(n=8):
    """(name, arguments of R.validate, refused): shared with tests/test_gpu_segment.py."""
    good = dict(n=n, source=0, n_segments=2, segment_start=[0, 3, 5], indices=[0, 1, 2, 7, 7])
    yield "good", good, False
    yield "no search cloud", dict(good, search_set=False), True
    yield "unknown source", dict(good, source=3), True
    yield "negative source", dict(good, source=-1), True
    yield "null segment_start", dict(good, segment_start=None), True
    yield "segment_start not from 0", dict(good, segment_start=[1, 3, 5]), True
    yield "segment_start decreasing", dict(good, segment_start=[0, 4, 3]), True
    yield "null indices", dict(good, indices=None), True
    yield "null indices, zero total", dict(good, segment_start=[0, 0, 0], indices=None), False
    yield "index n", dict(good, indices=[0, 1, 2, 7, n]), True
    yield "index -1", dict(good, indices=[-1, 1, 2, 7, 7]), True
    yield "index beyond the total is not read", dict(good, indices=[0, 1, 2, 7, 7, 99]), False
    yield "null out", dict(good, null_out=True), True
    yield "null out, no segment", dict(good, n_segments=0, segment_start=[0], indices=None, null_out=True), False
    yield "short record", dict(good, sizeof_record=R.RECORD.itemsize - 8), True
    yield "long record", dict(good, sizeof_record=R.RECORD.itemsize + 8), True
    yield "clusters without a result", dict(n=n, source=1, n_segments=2, segment_start=None, indices=None), True
    yield "regions without a result", dict(n=n, source=2, n_segments=2, segment_start=None, indices=None), True
    yield "clusters, another count", dict(n=n, source=1, n_segments=2, segment_start=None, indices=None, have_clusters=3), True
    yield "clusters with arrays", dict(n=n, source=1, n_segments=2, segment_start=[0, 3, 5], indices=None, have_clusters=2), True
    yield "clusters", dict(n=n, source=1, n_segments=2, segment_start=None, indices=None, have_clusters=2), False
    yield "regions, the clusters' count", dict(n=n, source=2, n_segments=2, segment_start=None, indices=None, have_clusters=2, have_regions=4), True


def test_validator_states_every_refusal():
    seen = {name: R.validate(**args) for name, args, _ in refusal_cases()}
    assert seen == {name: refused for name, _, refused in refusal_cases()}
    assert sum(seen.values()) >= 16


# ---- the golden fixture and the ABI -----------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    got = R.records(g["cloud"], g["segment_start"], g["indices"])
    assert got.dtype == R.RECORD and got.tobytes() == g["records"].tobytes()
    assert set(got["status"].tolist()) == {R.OK, R.EMPTY}
    assert os.path.getsize(GOLDEN) <= 2 * os.path.getsize(os.path.join(HERE, "golden", "rows_f", "normals_2k.npz"))


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "icpgpu.h")).read()
    for symbol in SYMBOLS:
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS
    assert f"#define ICPGPU_SEGMENT_CHUNK {_lib.SEGMENT_CHUNK}\n" in header and _lib.SEGMENT_CHUNK == R.CHUNK


def test_record_layout_matches_the_header(built, tmp_path):
    src = tmp_path / "t.c"
    fields = ("count", "status", "first", "K", "moments", "centroid", "cov", "eigenvalues", "axes", "aabb_min", "aabb_max", "obb_lo", "obb_hi",
              "obb_position", "obb_dims")
    offsets = ", ".join(f"offsetof(icpgpu_segment_record, {f})" for f in fields)
    src.write_text('#include "icpgpu.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){size_t o[] = {' + offsets + ', sizeof(icpgpu_segment_record)};\n'
                   'for (unsigned i = 0; i < sizeof o / sizeof o[0]; ++i) printf("%zu ", o[i]);\nreturn 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    from icpslam_amd import SEGMENT_RECORD
    assert fields == R.FIELDS == SEGMENT_RECORD.names
    assert got == [R.RECORD.fields[f][1] for f in fields] + [R.RECORD.itemsize] == [SEGMENT_RECORD.fields[f][1] for f in fields] + [C.sizeof(_lib.SegmentRecord)]
    assert R.RECORD == SEGMENT_RECORD


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_segment_moments(None, 0, 0, None, None, R.RECORD.itemsize, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_segment_stats(None, None) == _lib.ERR_INVALID_ARG


def test_pcl_shaped_class_refusals(built):
    from icpslam_amd import IcpGpuError, MomentOfInertiaEstimation
    moi = MomentOfInertiaEstimation.__new__(MomentOfInertiaEstimation)                   # (no context: no GPU here)
    moi._input, moi._indices, moi._records = np.ones((3, 4), F32), np.arange(3, dtype=np.int32), None
    for call in (moi.getMomentOfInertia, moi.getEccentricity, lambda: moi.setAngleStep(10.0), lambda: moi.compute_segments([[0], [1]]),
                 lambda: moi.compute_clusters(None)):
        with pytest.raises(IcpGpuError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(IcpGpuError) as e:
        moi.getAABB()
    assert e.value.code == _lib.ERR_NO_INPUT


# ---- icp_segment.h on the host --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("segment") / "segment_host_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "icpslam_amd", "csrc"),
                           os.path.join(HERE, "cpp", "segment_host_check.cpp"), "-o", exe])
    return exe


def host_records(exe, tmp_path, cloud, start, idx):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<3i", len(cloud), len(start) - 1, len(idx)))
        for a in (np.ascontiguousarray(cloud, F32), np.asarray(start, np.int32), np.asarray(idx, np.int32)):
            f.write(a.tobytes())
    subprocess.check_call([exe, str(src), str(dst)])
    return np.frombuffer(dst.read_bytes(), R.RECORD)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_shared_definitions_on_the_host_give_the_restatements_bits(host_check, tmp_path, name):
    """icp_segment.h, icp_jacobi3.h and icp_dd.h -- what the kernels call -- compiled for the host and driven over the hand cases."""
    case = K.CASES[name]
    start, idx = R.csr(case.segments)
    assert R.same_records(host_records(host_check, tmp_path, case.cloud, start, idx), R.records(case.cloud, start, idx)) == []


def test_shared_definitions_on_the_host_over_a_scans_clusters(host_check, tmp_path):
    """Rows from 1 to hundreds of entries that cross the chunk's multiples at every offset."""
    cloud, start, idx = scan_clusters()
    assert R.same_records(host_records(host_check, tmp_path, cloud, start, idx), R.records(cloud, start, idx)) == []
