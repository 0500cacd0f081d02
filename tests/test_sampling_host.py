"""The cropping and sampling filters without a GPU: the NumPy restatement (tests/sampling_restated.py) against its literal per-point
loops and against hand answers, icpgpu_crop_box_matrix (host only) against a double-precision composition, icp_sampling.h compiled for
the host against the restatement, the new symbols' ABI, and the golden fixture.  Every comparison is bit for bit."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import icpslam_amd
from icpslam_amd import _lib

import sampling_cases as SC
import sampling_restated as R

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "rows_f", "sampling_2k.npz")
NEW_SYMBOLS = ["icpgpu_pass_through", "icpgpu_pass_through_view", "icpgpu_crop_box", "icpgpu_crop_box_view", "icpgpu_crop_box_matrix",
               "icpgpu_uniform_sampling", "icpgpu_uniform_sampling_view", "icpgpu_farthest_point_sampling", "icpgpu_farthest_point_sampling_view",
               "icpgpu_subset_fetch", "icpgpu_subset_removed", "icpgpu_subset_stats"]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def small_cloud():
    return SC.with_bad_rows(SC.scan(300, 5), [0, 5, 64, 299])


# ---- the restatement against the literal loops ----------------------------------------------------------------------------------
@pytest.mark.parametrize("negative", [False, True])
def test_crops_equal_their_literal_loops(negative):
    c = small_cloud()
    for field, lo, hi in ((-1, 0.0, 0.0), (0, -3.0, 4.0), (1, -1.0, -1.0), (2, -1.2, 0.5), (2, 1.0, -1.0), (0, -math.inf, 2.0), (1, -2.0, math.inf)):
        assert same(R.pass_through(c, field, lo, hi, negative), R.pass_through_literal(c, field, lo, hi, negative)), (field, lo, hi)
    T = R.crop_box_matrix(None, (0.4, -0.2, 0.1), (0.02, -0.03, 0.3))
    for box in ((SC.EGO_MIN, SC.EGO_MAX), ((-8, -6, -2), (10, 6, 1)), ((-1e9,) * 3, (1e9,) * 3), ((1, 1, 1), (-1, -1, -1))):
        for Tm in (None, T):
            assert same(R.crop_box(c, *box, Tm, negative), R.crop_box_literal(c, *box, Tm, negative)), box


def test_samplers_equal_their_literal_loops():
    for c in (small_cloud(), SC.duplicated(200), SC.far_away(250), SC.tie_cells(), SC.lattice444()):
        for leaf in (0.3, 1.0, 7.0):
            a, b = R.uniform_sampling(c, leaf), R.uniform_sampling_literal(c, leaf)
            assert same(a[0], b[0]) and same(a[1], b[1]), leaf
        for k, first in ((0, -1), (1, -1), (17, -1), (17, len(c) - 1 if np.isfinite(c[-1, :3]).all() else 1)):
            k = min(k, int(R.finite_rows(c).sum()))
            a, b = R.farthest_point_sampling(c, k, first), R.farthest_point_sampling_literal(c, k, first)
            assert same(a[0], b[0]) and same(a[1], b[1]), (k, first)


def test_fused_multiply_add_emulations_agree():
    """The vectorised emulation (symmetric_restated.fma_f32) and the exact rational one of the literal loops, on ordinary and on
    cancelling operands."""
    from symmetric_restated import fma_f32
    r = np.random.default_rng(1)
    a, b = r.normal(0, 30, 400).astype(F32), r.normal(0, 30, 400).astype(F32)
    c = np.where(np.arange(400) % 2 == 0, r.normal(0, 900, 400), -(a.astype(np.float64) * b)).astype(F32)
    want = fma_f32(a, b, c)
    assert same(want, np.array([R.fma_scalar(x, y, z) for x, y, z in zip(a, b, c)], F32))


# ---- hand answers -----------------------------------------------------------------------------------------------------------------
def test_limits_exactly_on_a_points_value():
    c = SC.rows([(0, 0, -1.0), (0, 0, -0.5), (0, 0, 0.25), (0, 0, 2.0), (np.nan, 0, 0.0)])
    assert R.pass_through(c, 2, -0.5, 2.0, False).tolist() == [1, 2, 3]       # both ends inclusive
    assert R.pass_through(c, 2, -0.5, 2.0, True).tolist() == [0]              # ... and so excluded in negative mode
    assert R.pass_through(c, 2, 2.0, -0.5, False).tolist() == []              # lo > hi keeps nothing
    assert R.pass_through(c, 2, 2.0, -0.5, True).tolist() == [0, 1, 2, 3]
    assert R.pass_through(c, -1, 2.0, -0.5, True).tolist() == [0, 1, 2, 3]    # no field: `negative` is ignored
    assert R.pass_through(c, 2, -math.inf, math.inf, False).tolist() == [0, 1, 2, 3]
    f = SC.faces()
    on, off = [0] + list(range(1, 13, 2)), list(range(2, 13, 2))
    assert R.crop_box(f, SC.EGO_MIN, SC.EGO_MAX).tolist() == on               # a row ON a face is inside
    assert R.crop_box(f, SC.EGO_MIN, SC.EGO_MAX, None, True).tolist() == off


def test_a_nan_image_is_inside():
    """An infinite entry of T times a zero coordinate is NaN; no comparison with a NaN holds, so the row is inside (PCL's comparisons)."""
    T = np.eye(4, dtype=F32)
    T[0, 0] = np.inf
    c = SC.rows([(0.0, 50.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
    assert np.isnan(R.xform(T, c)[0, 0]) and np.isinf(R.xform(T, c)[1, 0])
    box = ((-1, -100, -1), (1, 100, 1))
    assert R.crop_box(c, *box, T, False).tolist() == [0, 2] and R.crop_box(c, *box, T, True).tolist() == [1]
    assert same(R.crop_box(c, *box, T, False), R.crop_box_literal(c, *box, T, False))


def test_lattice_ties_and_a_row_on_a_cell_face():
    kept, measure = R.uniform_sampling(SC.tie_cells(), 1.0)
    assert kept.tolist() == [0, 3, 4]                                          # rows 0 / 1 and 4 / 5 tie: the lower index; row 3 is alone in cell (1, 0, 0)
    assert measure.tolist() == [0.0625, 0.25, 0.0625]
    cell, _ = R.uniform_cells(SC.tie_cells(), 1.0)
    assert cell[3].tolist() == [1, 0, 0] and cell[4].tolist() == [-1, -1, -1]
    # one row per cell, and all rows in one cell
    lat = SC.lattice444()
    assert R.uniform_sampling(lat, 1.0)[0].tolist() == list(range(64))
    assert R.uniform_sampling(lat, 4.0)[0].tolist() == [42]                    # the one cell's centre (2, 2, 2) is row 2 + 4 * 2 + 16 * 2 itself
    assert R.uniform_sampling(lat, 2.0)[0].tolist() == [21, 23, 29, 31, 53, 55, 61, 63]   # the centres (1, 1, 1) + 2 k are rows themselves


def test_farthest_points_of_the_lattice_by_hand():
    """From the corner (0, 0, 0): the opposite corner (d2 27); then every row's m is min(d2 to either corner), largest 10 at (3, 1, 0) and its
    like, of which row 7 is the lowest."""
    kept, measure = R.farthest_point_sampling(SC.lattice444(), 8, 0)
    assert kept[:3].tolist() == [0, 63, 7] and measure[:3].tolist() == [math.inf, 27.0, 10.0]
    assert kept.tolist() == [0, 63, 7, 28, 49, 14, 35, 56]                     # the tie order: ascending index among equal m
    all_rows, m = R.farthest_point_sampling(SC.lattice444(), 64, -1)
    assert sorted(all_rows.tolist()) == list(range(64)) and (np.diff(m[1:]) <= 0).all()   # a permutation, m never grows


def test_duplicates_of_selected_points_come_last():
    base = [(0, 0, 0), (5, 0, 0), (0, 7, 0)]
    c = SC.rows(base + base[::-1] + [(1, 1, 1)])
    kept, measure = R.farthest_point_sampling(c, 7, -1)
    assert kept[:4].tolist() == [0, 2, 1, 6] and kept[4:].tolist() == [3, 4, 5]   # the copies: m = 0, lowest index first
    assert measure[4:].tolist() == [0.0, 0.0, 0.0] and measure[3] > 0


def test_the_k_centre_bound_on_a_scan():
    """Gonzalez' theorem: the farthest-point set's cover radius is at most twice the best k-centre radius, hence at most twice ANY
    64-subset's -- here 64 evenly strided rows."""
    c = SC.scan(3000, 5)
    kept, _ = R.farthest_point_sampling(c, 64, -1)
    strided = np.arange(64) * (3000 // 64)
    r_fps, r_strided = R.cover_radius(c, kept), R.cover_radius(c, strided)
    print(f"cover radius: farthest point sampling {r_fps:.4f}, strided {r_strided:.4f}, ratio {r_fps / r_strided:.4f}")
    assert r_fps <= 2.0 * r_strided


# ---- the validators ----------------------------------------------------------------------------------------------------------------
def test_validators_refuse_what_the_header_says():
    c = small_cloud()
    for bad in ((3, 0.0, 1.0), (-2, 0.0, 1.0), (0, math.nan, 1.0), (0, 0.0, math.nan)):
        with pytest.raises(R.Refused):
            R.pass_through(c, *bad)
    for mn, mx in (((math.nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, math.nan, 1))):
        with pytest.raises(R.Refused):
            R.crop_box(c, mn, mx)
    for leaf in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(R.Refused):
            R.uniform_sampling(c, leaf)
    n_finite = int(R.finite_rows(c).sum())
    for k, first in ((n_finite + 1, -1), (1, -2), (1, len(c)), (1, 0), (1, 299)):   # rows 0 and 299 are not finite
        with pytest.raises(R.Refused):
            R.farthest_point_sampling(c, k, first)
    assert len(R.farthest_point_sampling(c, n_finite, -1)[0]) == n_finite
    import voxel_edge_cases as vx
    refused = 0
    for name, lo, hi, leaf, want in vx.boundary_boxes():
        if want == vx.PASS_THROUGH and np.isfinite(lo).all() and np.isfinite(hi).all():
            with pytest.raises(R.Unsupported):
                R.uniform_sampling(SC.rows([lo, hi]), leaf)
            refused += 1
    assert refused > 0


# ---- the host-only entry point -------------------------------------------------------------------------------------------------------
def lib_matrix(transform, translation, rotation):
    return icpslam_amd.crop_box_matrix(transform, translation, rotation)


def test_crop_box_matrix(built):
    r = np.random.default_rng(4)
    for trial in range(200):
        tf = None if trial % 3 == 0 else icpslam_amd.synth.pose_matrix(*r.uniform(-5, 5, 3), *r.uniform(-3, 3, 3)).astype(F32)
        tr, ro = r.uniform(-20, 20, 3).astype(F32), r.uniform(-3.2, 3.2, 3).astype(F32)
        assert same(lib_matrix(tf, tr, ro), R.crop_box_matrix(tf, tr, ro)), trial
    eye = np.eye(4, dtype=F32)
    assert same(lib_matrix(None, (0, 0, 0), (0, 0, 0)), eye)                                   # identity
    want = eye.copy()
    want[:3, 3] = (-1.5, 2.0, -0.25)
    assert same(lib_matrix(None, (1.5, -2.0, 0.25), (0, 0, 0)), want)                          # a pure translation: Tr(-t)
    # a quarter turn about z: R^-1 takes (x, y) to (y, -x), the box onto itself rotated
    quarter = lib_matrix(None, (0, 0, 0), (0, 0, math.pi / 2))
    hand = np.array([[0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    assert np.abs(quarter - hand).max() <= 5e-8                                                # (cos of float32(pi / 2) is 4.4e-8, not 0)
    c = SC.scan(500, 5)
    turned = c.copy()
    turned[:, 0], turned[:, 1] = c[:, 1], -c[:, 0]
    box = ((-6, -9, -2), (6, 9, 1))
    assert same(R.crop_box(c, *box, hand.astype(F32)), R.crop_box(turned, *box))
    # transform and rotation cancelling
    angle = F32(0.7)
    rz = icpslam_amd.synth.pose_matrix(0, 0, 0, 0, 0, float(angle))
    assert np.abs(lib_matrix(rz.astype(F32), (0, 0, 0), (0, 0, angle)) - np.eye(4)).max() <= 1e-7
    L = _lib.load()
    out = np.zeros(16, F32)
    fp = C.POINTER(C.c_float)
    assert L.icpgpu_crop_box_matrix(None, None, out.ctypes.data_as(fp), out.ctypes.data_as(fp)) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_crop_box_matrix(None, out.ctypes.data_as(fp), out.ctypes.data_as(fp), None) == _lib.ERR_INVALID_ARG


def test_seeded_first_row(built, tmp_path):
    c = small_cloud()
    exe = _host_check_exe(tmp_path)
    for seed in (0, 1, 12345, 2**63 + 7, 2**64 - 1):
        assert icpslam_amd.seeded_first_row(c, seed) == R.seeded_first_row(c, seed)
        draw = int(subprocess.run([str(exe), "seed", str(seed), str(len(c))], capture_output=True, text=True, check=True).stdout)
        import sac_restated as SR
        assert draw == SR.sample_int(seed, 0, 0, len(c))
    bad = c.copy()
    bad[:, 0] = np.nan
    assert icpslam_amd.seeded_first_row(bad, 1) == -1 == R.seeded_first_row(bad, 1)
    wrap = c.copy()
    wrap[1:, 1] = np.inf
    wrap[0, :3] = 1.0
    assert icpslam_amd.seeded_first_row(wrap, 5) == 0 == R.seeded_first_row(wrap, 5)            # cyclically: past the end, back to row 0


# ---- the ABI of the new symbols -------------------------------------------------------------------------------------------------------
def test_the_new_symbols_abi(built):
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "icpgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert re.search(rf"\bint {name}\(", header), name
    defines = dict(re.findall(r"^#define (ICPGPU_(?:FPS|SUBSET)_[A-Z_]+) (\d+)$", header, flags=re.M))
    assert int(defines["ICPGPU_FPS_ONE_WORKGROUP_MAX"]) == _lib.FPS_ONE_WORKGROUP_MAX == R.FPS_ONE_WORKGROUP_MAX
    assert [int(defines[f"ICPGPU_SUBSET_{k}"]) for k in ("PASS_THROUGH", "CROP_BOX", "UNIFORM_SAMPLING", "FARTHEST_POINT_SAMPLING")] == \
        [_lib.SUBSET_PASS_THROUGH, _lib.SUBSET_CROP_BOX, _lib.SUBSET_UNIFORM_SAMPLING, _lib.SUBSET_FARTHEST_POINT_SAMPLING]
    assert [int(defines["ICPGPU_FPS_PATH_ONE"]), int(defines["ICPGPU_FPS_PATH_MANY"])] == [_lib.FPS_PATH_ONE, _lib.FPS_PATH_MANY]
    assert "ICPGPU_VERSION_MINOR 2" in header and L.icpgpu_version() == 1002                   # the header version stays 1.2
    # without a context every call is refused, and says so by its code
    n = C.c_size_t(99)
    assert L.icpgpu_pass_through(None, None, 0, 2, 0.0, 1.0, 0, None, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_uniform_sampling(None, None, 0, 0.5, None, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_farthest_point_sampling(None, None, 0, 0, -1, None, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_subset_fetch(None, 0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_subset_removed(None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_subset_stats(None, None, None, None, None) == _lib.ERR_INVALID_ARG
    for name in ("PassThrough", "CropBox", "UniformSampling", "FarthestPointSampling"):
        assert name in icpslam_amd.__all__ and hasattr(icpslam_amd, name)
    for method in ("pass_through", "crop_box", "uniform_sampling", "farthest_point_sampling", "subset_fetch", "subset_stats"):
        assert hasattr(icpslam_amd.Context, method)


# ---- icp_sampling.h compiled for the host -------------------------------------------------------------------------------------------
def _host_check_exe(tmp_path):
    exe = tmp_path / "sampling_host_check"
    if not exe.exists():
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                               os.path.join(HERE, "cpp", "sampling_host_check.cpp"), "-o", str(exe)])
    return exe


def _host_check(tmp_path, mode, records):
    path = tmp_path / f"{mode}.bin"
    np.ascontiguousarray(records, F32).tofile(path)
    out = subprocess.run([str(_host_check_exe(tmp_path)), mode, str(path)], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.strip().split("\n")]


def _bits(a):
    return [f"{v:08x}" for v in np.asarray(a, F32).view(np.uint32).tolist()]


def test_the_shared_header_compiled_for_the_host_equals_the_restatement(tmp_path):
    c = np.concatenate((small_cloud(), SC.faces(), SC.tie_cells(), SC.far_away(100)))
    n = len(c)
    # pass through
    for field, lo, hi, neg in ((-1, 0.0, 0.0, 1), (2, -1.2, 0.5, 0), (2, -1.2, 0.5, 1), (0, 2.5, -1.5, 0), (1, -1.0, 1.0, 1), (0, -math.inf, 2.5, 0)):
        rec = np.concatenate((c[:, :3], np.tile(F32([field, lo, hi, neg]), (n, 1))), axis=1)
        keep = np.array([int(r[0]) for r in _host_check(tmp_path, "pass", rec)])
        assert np.flatnonzero(keep).tolist() == R.pass_through(c, field, lo, hi, bool(neg)).tolist(), (field, lo, hi, neg)
    # crop box, with and without a transform (an infinite entry among them)
    T = R.crop_box_matrix(None, (0.4, -0.2, 0.1), (0.02, -0.03, 0.3))
    Tinf = np.eye(4, dtype=F32)
    Tinf[1, 1] = np.inf
    cz = c.copy()
    cz[10:20, 1] = 0.0
    for Tm, neg in ((None, 0), (None, 1), (T, 0), (T, 1), (Tinf, 0), (Tinf, 1)):
        m12 = np.eye(4, dtype=F32)[:3].reshape(12) if Tm is None else np.asarray(Tm, F32)[:3].reshape(12)
        rec = np.concatenate((np.tile(m12, (n, 1)), cz[:, :3], np.tile(F32(SC.EGO_MIN + SC.EGO_MAX + (neg, Tm is not None)), (n, 1))), axis=1)
        rows = _host_check(tmp_path, "crop", rec)
        assert np.flatnonzero([int(r[0]) for r in rows]).tolist() == R.crop_box(cz, SC.EGO_MIN, SC.EGO_MAX, Tm, bool(neg)).tolist()
        if Tm is not None:
            q = R.xform(Tm, cz)
            fin = R.finite_rows(cz)
            for a in range(3):
                assert [r[1 + a] for r, f in zip(rows, fin) if f] == [b for b, f in zip(_bits(q[:, a]), fin) if f]
    # the cells and their keys
    fin = R.finite_rows(c)
    for leaf in (0.25, 1.0, 7.0):
        rows = _host_check(tmp_path, "cell", np.concatenate((c[:, :3], np.full((n, 1), leaf, F32)), axis=1))
        cell, d2 = R.uniform_cells(c, leaf)
        got_cell = np.array([[int(v) for v in r[:3]] for r in rows])
        assert np.array_equal(got_cell[fin], cell[fin])
        assert [r[3] for r, f in zip(rows, fin) if f] == [b for b, f in zip(_bits(d2), fin) if f]
        keys = [(int(b, 16) << 32) | i for i, b in enumerate(_bits(d2))]
        assert [int(r[4], 16) for r, f in zip(rows, fin) if f] == [k for k, f in zip(keys, fin) if f]
    # the farthest point sampling's d2 and key
    cf = c[fin]
    rec = np.concatenate((cf[:, :3], np.tile(cf[17, :3], (len(cf), 1))), axis=1)
    rows = _host_check(tmp_path, "far", rec)
    d2 = R.d2_rows(cf, 17)
    assert [r[0] for r in rows] == _bits(d2)
    for i, r in enumerate(rows):
        assert int(r[1], 16) == (int(r[0], 16) << 32) | (~i & 0xFFFFFFFF) and int(r[2]) == i and r[3] == r[0]
    order = sorted(range(len(rows)), key=lambda i: -int(rows[i][1], 16))            # the largest key first ...
    assert order == sorted(range(len(rows)), key=lambda i: (-float(d2[i]), i))      # ... is the largest d2, then the lowest index


# ---- the golden fixture ------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_sampling", os.path.join(HERE, "golden", "make_golden_sampling.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    want = np.load(GOLDEN)
    got = maker.fixture()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert same(want[k], np.asarray(got[k])), k
    assert 0 < len(want["pass0_kept"]) < 2000 and 0 < len(want["cropT0_kept"]) < 2000 and len(want["uniform1_kept"]) > 100
