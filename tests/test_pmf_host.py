"""The ground filter's rule on the host (include/icpgpu.h, "ground filter"): the NumPy restatement (tests/pmf_restated.py) against its
literal per-pass, per-point, per-candidate loop, the schedule and answers known by hand, the golden fixture, an end-to-end scene that
says why the feature exists, and the ABI of the new entry points, which needs no GPU."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import pmf_cases as K
import pmf_restated as R
import sac_restated as SR
from icpslam_amd import _lib, synth

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "rows_f", "pmf_2k.npz")
SYMBOLS = ("icpgpu_morphological_operator", "icpgpu_progressive_morphological_filter", "icpgpu_pmf_fetch", "icpgpu_pmf_stats", "icpgpu_pmf_extract",
           "icpgpu_pmf_extract_view")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def same(a: dict, b: dict):
    assert a.keys() == b.keys()
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), key


# ---- the restatement and its literal loop --------------------------------------------------------------------------------------
def test_restatement_equals_the_literal_loop_on_a_scan():
    cloud = scan(600).copy()
    cloud[::97, 1] = np.nan
    same(R.run(cloud), R.run_literal(cloud))
    for op in (R.ERODE, R.DILATE, R.OPEN, R.CLOSE):
        assert R.operator(cloud[:200], 2.5, op).tobytes() == R.operator_literal(cloud[:200], 2.5, op).tobytes()


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_restatement_equals_the_literal_loop_on_the_hand_clouds(name):
    cloud, kw, windows = K.CASES[name]
    same(R.run(cloud, **kw), R.run_literal(cloud, **kw))
    for w in windows:
        for op in (R.ERODE, R.DILATE, R.OPEN, R.CLOSE):
            assert R.operator(cloud, w, op).tobytes() == R.operator_literal(cloud, w, op).tobytes(), (w, op)


def test_erode_then_dilate_is_open_and_dilate_then_erode_is_close():
    """The second half works on the first half's values with the INPUT's boxes: applying the operator to a cloud whose z was replaced."""
    for cloud in (scan(300), K.CASES["duplicates"][0], K.CASES["nan_rows"][0]):
        for w in (1.0, 4.0):
            for first, second, both in ((R.ERODE, R.DILATE, R.OPEN), (R.DILATE, R.ERODE, R.CLOSE)):
                half = cloud.copy()
                half[:, 2] = R.operator(cloud, w, first)
                finite = R.finite_rows(cloud)
                got = R.operator(half, w, second, np.flatnonzero(finite))
                assert got.tobytes() == R.operator(cloud, w, both).tobytes()


# ---- the schedule by hand ------------------------------------------------------------------------------------------------------
def test_the_default_schedule_by_hand():
    windows, thresholds = R.schedule()
    assert windows.dtype == thresholds.dtype == F32
    assert windows.tolist() == [3.0, 5.0, 9.0, 17.0, 33.0]
    slope, initial, cell = F32(0.7), F32(0.15), F32(1.0)
    want = [initial] + [slope * (F32(b) - F32(a)) * cell + initial for a, b in ((3, 5), (5, 9), (9, 17), (17, 33))]
    assert all(type(t) is F32 for t in want)
    want[4] = min(want[4], F32(10.0))                       # 0.7 * 16 + 0.15 = 11.35: the clamp bites in the last pass
    assert want[4] == F32(10.0) and thresholds.tobytes() == np.array(want, F32).tobytes()
    assert float(thresholds[1]) == float(F32(F32(F32(0.7) * F32(2.0)) + F32(0.15)))


def test_linear_clamped_and_short_schedules():
    windows, thresholds = R.schedule(max_window_size=8, exponential=False, base=1.0)
    assert windows.tolist() == [3.0, 5.0, 7.0, 9.0]         # cell * (2 (it + 1) base + 1); the loop appends the first window >= max
    assert thresholds.tobytes() == np.array([F32(0.15)] + [F32(0.7) * F32(2.0) * F32(1.0) + F32(0.15)] * 3, F32).tobytes()
    windows, thresholds = R.schedule(max_window_size=10, exponential=False, base=F32(0.3), cell_size=0.5)
    k = [F32(0.5) * (F32(2) * F32(i + 1) * F32(0.3) + F32(1)) for i in range(len(windows))]
    assert windows.tobytes() == np.array(k, F32).tobytes() and len(windows) == R.MAX_PASSES     # 0.8, 1.1, ... 9.8 < 10 <= 10.1: exactly 32 passes
    windows, thresholds = R.schedule(max_distance=1.0)
    assert thresholds.tolist() == [float(F32(0.15)), 1.0, 1.0, 1.0, 1.0]
    for max_window, want in ((0, []), (-5, []), (1, [3.0]), (3, [3.0]), (4, [3.0, 5.0])):
        assert R.schedule(max_window_size=max_window)[0].tolist() == want
    # a base that is no power of two: B by successive double multiplications of the float32 base
    b = float(F32(1.3))
    assert R.schedule(max_window_size=6, base=1.3)[0].tobytes() == np.array([F32(3.0), F32(2.0 * b + 1.0), F32(2.0 * (b * b) + 1.0),
                                                                            F32(2.0 * (b * b * b) + 1.0), F32(2.0 * (b * b * b * b) + 1.0)], F32).tobytes()


def test_refusals_against_the_validator():
    bad = [dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=math.nan), dict(slope=-0.1), dict(slope=math.inf), dict(initial_distance=-1e-3),
           dict(initial_distance=math.nan), dict(max_distance=-1.0), dict(max_distance=math.inf), dict(max_distance=1e39), dict(base=1.0), dict(base=0.5),
           dict(base=math.nan), dict(exponential=False, base=0.0), dict(exponential=False, base=-2.0), dict(cell_size=1e-46),   # (rounds to 0)
           dict(max_window_size=2**30, exponential=False, base=1.0),                                   # more than 32 passes
           dict(max_window_size=2**31 - 1, cell_size=1e-3),                                            # likewise, exponential (2^32 > 2^31 needs 33)
           dict(max_window_size=100, exponential=False, base=1e-30),                                   # the window never grows
           dict(max_window_size=2**31 - 1, base=3e38, cell_size=3e38)]                                 # a window that is not finite
    for kw in bad:
        with pytest.raises(R.Refused):
            R.schedule(**kw)
    for kw in (dict(base=1.0000002, max_window_size=3), dict(exponential=False, base=1e-3, max_window_size=1), dict(slope=0.0), dict(initial_distance=0.0),
               dict(max_distance=0.0), dict(max_window_size=-1), dict(max_window_size=2**31 - 1)):
        R.schedule(**kw)
    assert len(R.schedule(max_window_size=2**31 - 1)[0]) == 31 and len(R.schedule(max_window_size=2**31 - 1, cell_size=0.5)[0]) == R.MAX_PASSES
    for w, op in ((0.0, R.OPEN), (-1.0, R.OPEN), (math.nan, R.ERODE), (math.inf, R.ERODE), (1.0, 4), (1.0, -1), (1e-46, R.CLOSE)):
        with pytest.raises(R.Refused):
            R.operator(scan(63), w, op)


# ---- answers known by hand -----------------------------------------------------------------------------------------------------
def test_neighbours_exactly_on_the_bounds_are_in():
    cloud = K.edge_lattice()                                 # 9 x 7, spacing 1.5 = h of window 3
    M = R.boxes(cloud, np.arange(len(cloud)), 3.0)
    ix, iy = np.arange(63) % 9, np.arange(63) // 9
    want = (np.abs(ix[:, None] - ix[None, :]) <= 1) & (np.abs(iy[:, None] - iy[None, :]) <= 1)
    assert np.array_equal(M, want) and M[31].sum() == 9 and M[0].sum() == 4
    assert R.boxes(cloud, np.arange(63), 2.999)[31].sum() == 1                  # a little less: the point alone
    e = R.operator(cloud, 3.0, R.ERODE)
    assert e[31] == cloud[want[31], 2].min() and R.operator(cloud, 3.0, R.DILATE)[0] == cloud[want[0], 2].max()


def test_the_box_relation_need_not_be_symmetric():
    """Around 2^24 float32's spacing goes from 1 to 2: 16777215 + 1 is exact and reaches 16777216, 16777216 - 1 = 16777215 is exact too, but
    16777218 - 1 = 16777217 rounds to 16777216 while 16777216 + 1 = 16777217 rounds to 16777216 as well (ties to even)."""
    cloud = K.offset_lattice()
    M = R.boxes(cloud, np.arange(len(cloud)), 2.0)
    assert (M != M.T).any() and M.diagonal().all()
    x = cloud[:12, 0]
    a, b = int(np.flatnonzero(x == 16777218.0)[0]), int(np.flatnonzero(x == 16777216.0)[0])
    assert M[a, b] and not M[b, a]                           # 2^24 is in 16777218's box (lo rounds down to it), not the other way round
    assert (R.boxes(cloud - F32([16777210.0, 0, 0, 0]), np.arange(len(cloud)), 2.0) == R.boxes(cloud - F32([16777210.0, 0, 0, 0]), np.arange(len(cloud)), 2.0).T).all()
    same(R.run(cloud, **K.SMALL), R.run_literal(cloud, **K.SMALL))


def test_a_raised_block_leaves_at_the_first_window_that_exceeds_it():
    cloud = K.block(3)                                       # 3 x 3 points, 2 m across, raised by 2
    r = R.run(cloud, **K.SMALL)                              # windows 3 (threshold 0.15) and 5 (1.55)
    raised = cloud[:, 2] > 0
    assert raised.sum() == 9 and (r["removed_at"][raised] == 1).all() and (r["removed_at"][~raised] == -1).all()
    assert r["ground_after"].tolist() == [441, 432] and np.array_equal(r["ground"], np.flatnonzero(~raised))
    # window 3 reaches 1.5 m: the block's centre sees only the block, its erosion stays up and lifts the opening of all nine
    assert (R.operator(cloud, 3.0, R.OPEN)[raised] == 2.0).all() and (R.operator(cloud, 5.0, R.OPEN)[raised] == 0.0).all()
    wide = K.block(7)                                        # 6 m across: wider than both windows
    r = R.run(wide, **K.SMALL)
    assert (r["removed_at"] == -1).all() and r["ground"].size == 441


def test_signed_zeros_have_defined_bits():
    cloud = K.signed_zeros()
    neg = np.signbit(cloud[:, 2])
    assert 10 < neg.sum() < 54
    M = R.boxes(cloud, np.arange(64), 2.0)
    e, d = R.operator(cloud, 2.0, R.ERODE), R.operator(cloud, 2.0, R.DILATE)
    assert np.array_equal(np.signbit(e), (M & neg[None, :]).any(axis=1))        # -0.0 wins a minimum wherever the box holds one
    assert np.array_equal(np.signbit(d), ~(M & ~neg[None, :]).any(axis=1))      # +0.0 wins a maximum
    assert R.keys(F32([-0.0, 0.0])).tolist() == [0x7FFFFFFF, 0x80000000] and R.unkeys(R.keys(cloud[:, 2])).tobytes() == cloud[:, 2].tobytes()


def test_duplicates_nan_rows_slope_zero_and_initial_zero():
    cloud = K.duplicates()
    r = R.run(cloud, **K.SMALL)
    assert (r["removed_at"][40:60] == 0).all()               # a copy 0.5 m above its twin is off the ground at once (threshold 0.15)
    assert (r["removed_at"][60:] == r["removed_at"][0:40:5]).all()   # exact copies share their twin's fate
    cloud = K.nan_rows()
    r = R.run(cloud, **K.SMALL)
    bad = ~np.isfinite(cloud[:, :3]).all(axis=1)
    assert bad.sum() == 17 and (r["removed_at"][bad] == -2).all() and (r["removed_at"][~bad] != -2).all() and r["removed_at"][50] == 0
    assert not np.isin(np.flatnonzero(bad), r["ground"]).any()
    o = R.operator(cloud, 3.0, R.OPEN)
    assert o[bad].tobytes() == cloud[bad, 2].tobytes()       # they keep their own z, and are nobody's neighbour:
    clean = cloud[~bad]
    assert o[~bad].tobytes() == R.operator(clean, 3.0, R.OPEN).tobytes()
    windows, thresholds = R.schedule(max_window_size=9, slope=0.0)
    assert thresholds.tolist() == [float(F32(0.15))] * 3     # slope 0: every pass has the initial threshold
    r = R.run(K.block(3), max_window_size=9, slope=0.0)
    assert r["ground_after"].tolist() == [441, 432, 432]
    # initial_distance 0: the first threshold is 0, z - o < 0 is false wherever the boxes are symmetric (o <= z there): everything leaves
    r = R.run(K.CASES["initial_zero"][0], max_window_size=3, initial_distance=0.0)
    assert r["thresholds"].tolist() == [0.0] and r["ground"].size == 0 and (r["removed_at"] == 0).all()


def test_empty_and_degenerate_clouds():
    for cloud in (np.empty((0, 4), F32), np.full((9, 4), np.nan, F32)):
        r = R.run(cloud)
        assert r["ground"].size == 0 and r["ground_after"].tolist() == [0] * 5 and (r["removed_at"] == -2).all()
    r = R.run(scan(63), max_window_size=0)
    assert r["ground"].tolist() == list(range(63)) and r["windows"].size == 0 and r["ground_after"].size == 0
    one = K.points([[1, 2, 3]])
    assert R.run(one)["ground"].tolist() == [0] and R.operator(one, 1.0, R.CLOSE).tolist() == [3.0]


# ---- why the feature exists ----------------------------------------------------------------------------------------------------
def test_a_crowned_street_is_ground_for_the_filter_and_not_for_a_plane():
    """A street crowned along x = 0 with a 5 % grade to either side and a 5 cm ripple, five boxes 1 - 2 m high on it, 3 000 points.
    Measured here from the restatement: the filter with PCL's defaults keeps 2 700 of 2 700 true ground points (share 1.0) and none of the
    300 box points; plane RANSAC at the same 0.15 m keeps 1 476 of 2 700 (share 0.547: it misses 45 %, seeds 1 - 3 give 0.543 - 0.547)
    and takes 33 - 60 box points with it.  These bounds test the rule; the kernels are compared with it bit for bit."""
    cloud, is_box = K.graded_scene()
    assert len(cloud) == 3000 and is_box.sum() == 300
    r = R.run(cloud)
    ground = np.zeros(3000, bool)
    ground[r["ground"]] = True
    height = cloud[:, 2] + F32(0.05) * np.abs(cloud[:, 0])
    assert not (ground & is_box & (height > 0.5)).any() and not (ground & is_box).any()
    assert (ground & ~is_box).sum() / (~is_box).sum() >= 0.98
    s = SR.segment(cloud, 0.15, 200, 0.99, 1, True)
    plane = np.zeros(3000, bool)
    plane[s["inliers"]] = True
    assert s["found"] == 1 and (plane & ~is_box).sum() / (~is_box).sum() <= 0.60      # the plane misses at least 40 % of the ground


# ---- the golden fixture and the ABI --------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    r = R.run(g["cloud"])
    for name in ("ground", "windows", "thresholds", "ground_after", "removed_at"):
        assert r[name].dtype == g[name].dtype and r[name].tobytes() == g[name].tobytes(), name
    assert R.operator(g["cloud"], float(g["open_window"]), R.OPEN).tobytes() == g["opened"].tobytes()
    assert 100 < r["ground"].size < 2000 and (r["removed_at"] == -2).sum() == 2 and len(set(r["removed_at"].tolist())) >= 3
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "rows_f", "normals_2k.npz"))


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "icpgpu.h")).read()
    for symbol in SYMBOLS:
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS
    assert "#define ICPGPU_PMF_MAX_PASSES 32\n" in header and _lib.PMF_MAX_PASSES == R.MAX_PASSES == 32
    assert (_lib.MORPH_ERODE, _lib.MORPH_DILATE, _lib.MORPH_OPEN, _lib.MORPH_CLOSE) == (R.ERODE, R.DILATE, R.OPEN, R.CLOSE) == (0, 1, 2, 3)


def test_header_compiles_as_c_with_the_prototypes(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){\n'
                   '  int (*f1)(icpgpu_ctx*, double, int, float*) = icpgpu_morphological_operator;\n'
                   '  int (*f2)(icpgpu_ctx*, int, double, double, double, double, double, int, size_t*, int32_t*) = icpgpu_progressive_morphological_filter;\n'
                   '  int (*f3)(icpgpu_ctx*, size_t, size_t, int32_t*, float*, float*, int32_t*, int32_t*) = icpgpu_pmf_fetch;\n'
                   '  int (*f4)(const icpgpu_ctx*, int32_t*, uint64_t*) = icpgpu_pmf_stats;\n'
                   '  int (*f5)(icpgpu_ctx*, int, float*, size_t*) = icpgpu_pmf_extract;\n'
                   '  int (*f6)(icpgpu_ctx*, int, const float**, size_t*) = icpgpu_pmf_extract_view;\n'
                   '  icpgpu_morph_op op = ICPGPU_MORPH_CLOSE;\n'
                   '  printf("%d %d %d %d %d %d\\n", ICPGPU_MORPH_ERODE, ICPGPU_MORPH_DILATE, ICPGPU_MORPH_OPEN, (int)op, ICPGPU_PMF_MAX_PASSES,\n'
                   '         ICPGPU_HEADER_VERSION);\n'
                   '  printf("%d %d %d %d %d %d\\n", f1(NULL, 1.0, 0, NULL), f2(NULL, 33, 0.7, 0.15, 10.0, 1.0, 2.0, 1, NULL, NULL),\n'
                   '         f3(NULL, 0, 0, NULL, NULL, NULL, NULL, NULL), f4(NULL, NULL, NULL), f5(NULL, 0, NULL, NULL), f6(NULL, 1, NULL, NULL));\n'
                   '  return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[:6] == [0, 1, 2, 3, 32, 1002] and out[6:] == [_lib.ERR_INVALID_ARG] * 6      # a null context is refused: no GPU is needed


def test_front_end_defaults_and_exports():
    import icpslam_amd as pkg
    for name in ("ProgressiveMorphologicalFilter", "MORPH_ERODE", "MORPH_DILATE", "MORPH_OPEN", "MORPH_CLOSE", "PMF_MAX_PASSES"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for method in ("setInputCloud", "setMaxWindowSize", "setSlope", "setMaxDistance", "setInitialDistance", "setCellSize", "setBase", "setExponential",
                   "extract"):
        assert callable(getattr(pkg.ProgressiveMorphologicalFilter, method))
    import inspect
    sig = inspect.signature(pkg.Context.progressive_morphological_filter)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == R.DEFAULTS
