"""Euclidean clustering's rules on the host (include/icpgpu.h, "euclidean clustering"): the NumPy restatement (tests/cluster_restated.py)
against PCL 1.8's seed-queue loop transcribed, against answers known by hand, and against the golden fixture; the symmetry of d2 that
makes the graph undirected; and the ABI of the two entry points, which needs no GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_restated as R
import search_restated as S
from icpslam_amd import _lib, synth

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rows_f", "cluster_2k.npz")
INT_MAX = 2**31 - 1


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def points(xyz) -> np.ndarray:
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = np.asarray(xyz, F32).reshape(-1, 3)
    return c


def lattice(m, spacing) -> np.ndarray:
    g = np.arange(m, dtype=F32) * F32(spacing)
    return points(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def clusters(cloud, tolerance, lo=1, hi=INT_MAX):
    start, indices, labels, component = R.extract(cloud, tolerance, lo, hi)
    return [indices[a:b].tolist() for a, b in zip(start[:-1], start[1:])], labels, component


# ---- the restatement and PCL's loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tolerance", [0.25, 0.5, 1.0, 2.0])
@pytest.mark.parametrize("n", [257, 1025, 3000])
def test_restatement_and_pcl_loop_agree_as_sets(n, tolerance):
    cloud = scan(3000)[:n]
    rows = R.radius_rows(cloud, tolerance)                             # (the adjacency lists, once for the three windows)
    assert all(np.array_equal(a, b) for a, b in zip(R.extract(cloud, tolerance), R.from_components(R.components(cloud, tolerance, rows))))
    for lo, hi in ((1, INT_MAX), (2, 50), (5, 5)):
        start, indices, labels, component = R.from_components(R.components(cloud, tolerance, rows), lo, hi)
        literal = R.pcl_literal(cloud, tolerance, lo, hi, rows)
        assert R.as_sets(start, indices) == {frozenset(c) for c in literal}
        assert len(literal) == start.size - 1 and sum(map(len, literal)) == indices.size
        # the order rule and the arrays' own consistency
        sizes = np.diff(start)
        names = indices[start[:-1]] if sizes.size else np.zeros(0, np.int32)
        assert (sizes[:-1] >= sizes[1:]).all() and ((sizes[:-1] > sizes[1:]) | (names[:-1] < names[1:])).all()
        assert ((sizes >= lo) & (sizes <= hi)).all()
        for r, (a, b) in enumerate(zip(start[:-1], start[1:])):
            assert (np.diff(indices[a:b]) > 0).all() and (labels[indices[a:b]] == r).all() and (component[indices[a:b]] == indices[a]).all()
        assert (labels >= 0).sum() == indices.size


def test_the_scan_really_exercises_ties_and_the_window():
    """What the cases above rest on: at n = 3000 the four tolerances give 931 / 332 / 94 / 31 components, 548 / 164 / 40 / 10 of them
    singletons, the largest of 38 / 1454 / 2595 / 2856 points."""
    want = {0.25: (931, 548, 38), 0.5: (332, 164, 1454), 1.0: (94, 40, 2595), 2.0: (31, 10, 2856)}
    for tolerance, numbers in want.items():
        sizes = np.unique(R.components(scan(3000), tolerance), return_counts=True)[1]
        assert (sizes.size, int((sizes == 1).sum()), int(sizes.max())) == numbers


def test_windowed_rows_of_a_large_cloud_are_the_plain_ones():
    """Above 4096 points the restatement asks search_restated.radius chunk by chunk in x order: the rows must be the very rows of one
    call over the whole cloud (ties, non-finite rows and duplicated points included)."""
    cloud = scan(6000, 7).copy()
    cloud[[5, 4000], [0, 2]] = [np.nan, np.inf]
    cloud[100:110] = cloud[5000:5010]
    for tolerance in (0.0, 0.3, 1.5):
        _, start, idx = R.radius_rows(cloud, tolerance)
        want_start, want_idx, _ = S.radius(cloud, None, tolerance)
        assert start.dtype == want_start.dtype and idx.dtype == want_idx.dtype
        assert np.array_equal(start, want_start) and np.array_equal(idx, want_idx)


# ---- answers known by hand -------------------------------------------------------------------------------------------------
def test_lattice_at_exactly_the_tolerance_is_64_singletons():
    cloud = lattice(4, 0.5)                                            # neighbours at d2 == 0.25 == r2: strict, not joined
    got, labels, component = clusters(cloud, 0.5)
    assert got == [[i] for i in range(64)]
    assert np.array_equal(component, np.arange(64)) and np.array_equal(labels, np.arange(64))


def test_lattice_just_above_the_tolerance_is_one_component():
    got, labels, component = clusters(lattice(4, 0.5), float(np.nextafter(F32(0.5), F32(1))))
    assert got == [list(range(64))] and not labels.any() and not component.any()


def test_duplicated_points_are_joined_for_any_positive_tolerance():
    cloud = points([[0, 0, 0], [5, 0, 0], [0, 0, 0], [5, 0, 0], [0, 0, 0], [9, 9, 9]])
    assert clusters(cloud, 1e-6)[0] == [[0, 2, 4], [1, 3], [5]]
    assert clusters(cloud, 0.0)[0] == [[i] for i in range(6)]          # tolerance 0: r2 = 0, nothing is below it


def test_a_nan_point_between_two_groups_does_not_bridge_them():
    cloud = points([[0, 0, 0], [0.4, 0, 0], [0.8, 0, 0], [1.2, 0, 0], [1.6, 0, 0]])
    assert clusters(cloud, 0.5)[0] == [[0, 1, 2, 3, 4]]
    cloud[2, 1] = np.nan
    got, labels, component = clusters(cloud, 0.5)
    assert got == [[0, 1], [3, 4]]
    assert labels.tolist() == [0, 0, -1, 1, 1] and component.tolist() == [0, 0, -1, 3, 3]
    assert R.pcl_literal(cloud, 0.5) == [[0, 1], [3, 4]]


def test_max_size_drops_a_component_whole():
    cloud = points([[0.3 * i, 0, 0] for i in range(6)] + [[50, 0, 0], [50.3, 0, 0]])
    assert clusters(cloud, 0.5)[0] == [[0, 1, 2, 3, 4, 5], [6, 7]]
    got, labels, component = clusters(cloud, 0.5, 1, 5)
    assert got == [[6, 7]]                                             # never truncated to five points
    assert labels.tolist() == [-1] * 6 + [0, 0] and component.tolist() == [0] * 6 + [6, 6]


def test_max_below_min_emits_nothing():
    for lo, hi in ((3, 2), (1, 0), (0, -1), (INT_MAX, -INT_MAX - 1)):
        start, indices, labels, component = R.extract(scan(257), 0.5, lo, hi)
        assert start.tolist() == [0] and indices.size == 0 and (labels == -1).all() and (component >= 0).all()
    start, indices, _, _ = R.extract(scan(257), 0.5, -5, INT_MAX)      # every value of the two ints is accepted
    assert indices.size == 257


def test_ties_come_out_by_lowest_index():
    pairs = [[100.0 * k, 0, 0] for k in range(5)]
    cloud = points(pairs + [[100.0 * k + 0.1, 0, 0] for k in (4, 3, 2, 1, 0)] + [[300.0, 0.1, 0]])
    got, labels, _ = clusters(cloud, 0.5)
    assert got == [[3, 6, 10], [0, 9], [1, 8], [2, 7], [4, 5]]
    assert labels.tolist() == [1, 2, 3, 0, 4, 4, 0, 3, 2, 1, 0]


def test_empty_and_all_nan_clouds():
    for cloud in (np.empty((0, 4), F32), np.full((7, 4), np.nan, F32)):
        start, indices, labels, component = R.extract(cloud, 0.5)
        assert start.tolist() == [0] and indices.size == 0 and labels.tolist() == component.tolist() == [-1] * len(cloud)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(R.Refused):
            R.extract(scan(63), bad)


# ---- the graph is undirected -----------------------------------------------------------------------------------------------
def test_d2_is_symmetric_bit_for_bit():
    rng = np.random.default_rng(11)
    a = (rng.normal(size=(200000, 3)) * rng.choice([1e-3, 1.0, 80.0, 1e4], (200000, 1))).astype(F32)
    b = (a + rng.normal(size=a.shape) * rng.choice([1e-4, 0.3, 50.0], (200000, 1))).astype(F32)
    ab, ba = S._d2_pairs(a, b), S._d2_pairs(b, a)
    assert np.array_equal(ab.view(np.uint32), ba.view(np.uint32))
    rows = S.d2_rows(scan(257)[:, :3], scan(257)[:, :3])
    assert np.array_equal(rows.view(np.uint32), rows.T.view(np.uint32))


# ---- the golden fixture and the ABI ----------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_fixture():
    g = np.load(GOLDEN)
    got = R.extract(g["cloud"], float(g["tolerance"]), int(g["min_size"]), int(g["max_size"]))
    for name, a in zip(("cluster_start", "indices", "labels", "component"), got):
        assert a.dtype == g[name].dtype and a.tobytes() == g[name].tobytes(), name
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "rows_f", "normals_2k.npz"))


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in ("icpgpu_euclidean_cluster_extraction", "icpgpu_cluster_fetch"):
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_euclidean_cluster_extraction(None, 0.5, 1, INT_MAX, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_cluster_fetch(None, 0, 0, None, None, None, None) == _lib.ERR_INVALID_ARG
