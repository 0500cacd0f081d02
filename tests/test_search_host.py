"""The neighbour search's rules (include/icpgpu.h, "neighbour search") without a device: the NumPy restatement against a literal
per-pair loop, answers known by hand, the tree-narrowed forms against the brute forms, and the C-ABI's new symbols."""
import math
import os
import subprocess
import time
from fractions import Fraction

import numpy as np
import pytest

import oracle
import search_restated as R
from icpslam_amd import _lib, synth
from test_gpu_search import KS, SIZES, clustered, lattice, scan, size_of  # (the clouds the device tests use)

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
NEW_SYMBOLS = ["icpgpu_search_set_input", "icpgpu_search_size", "icpgpu_search_knn", "icpgpu_search_radius"]


def fmaf(a, b, c):
    """fmaf on three float32 scalars through exact rational arithmetic."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    lo = F32(float(exact))  # (float() of a Fraction rounds correctly to float64; narrowing may double-round: fix below)
    cands = [lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(F32(v).view(np.int32)) & 1))


def literal_d2(p, q):
    dx, dy, dz = F32(q[0] - p[0]), F32(q[1] - p[1]), F32(q[2] - p[2])
    return fmaf(dz, dz, fmaf(dy, dy, F32(dx * dx)))


def literal_neighbours(cloud, p):
    """Every finite cloud point as (bits of d2, index, d2), ascending: pair by pair, as the rule is written."""
    if not all(math.isfinite(v) for v in p[:3]):
        return []
    out = []
    for j, q in enumerate(cloud):
        if all(math.isfinite(v) for v in q[:3]):
            d = literal_d2(p, q)
            out.append((int(F32(d).view(np.uint32)), j, d))
    return sorted(out)


def small_cloud(n, seed):
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed).copy()
    c[3, 1] = np.nan
    return c


def same(a, b):
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_restatement_against_a_literal_loop():
    cloud = small_cloud(300, 4)
    cloud[40:44] = cloud[39]  # coincident points: the index decides
    queries = np.concatenate([cloud[:25], small_cloud(12, 9), F32([[np.inf, 0, 0, 1], [500, 500, 500, 1]])])
    lists = [literal_neighbours(cloud, p) for p in queries]
    for k in (1, 5, 20, 64):
        idx, d2, n_found = R.knn(cloud, queries, k)
        for i, full in enumerate(lists):
            want = full[:k]
            assert n_found[i] == len(want)
            assert idx[i, :len(want)].tolist() == [j for _, j, _ in want] and (idx[i, len(want):] == -1).all()
            assert d2[i, :len(want)].tolist() == [float(d) for _, _, d in want] and np.isinf(d2[i, len(want):]).all()
        assert same(R.knn_literal(cloud, queries, k), (idx, d2, n_found))
    for radius, max_nn in ((0.0, 0), (0.3, 0), (3.0, 0), (3.0, 2), (1e3, 70), (1e3, 0)):
        row_start, idx, d2 = R.radius(cloud, queries, radius, max_nn)
        r2 = F32(radius * radius)
        for i, full in enumerate(lists):
            want = [e for e in full if e[2] < r2]
            want = want[:max_nn] if max_nn else want
            a, b = row_start[i], row_start[i + 1]
            assert idx[a:b].tolist() == [j for _, j, _ in want] and d2[a:b].tolist() == [float(d) for _, _, d in want]
        assert row_start[-1] == len(idx) == len(d2)
        assert same(R.radius_literal(cloud, queries, radius, max_nn), (row_start, idx, d2))


def test_narrowing_pass_changes_nothing():
    """The chunked forms against the exact expression on every pair, on clouds with ties: duplicates, a lattice."""
    cloud = small_cloud(700, 8)
    cloud[100:140] = cloud[99]
    g = np.arange(6, dtype=F32) * F32(0.25)
    lattice = np.ones((216, 4), F32)
    lattice[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for c in (cloud, lattice):
        for k in (1, 8, 27, 64):
            assert same(R.knn(c, None, k), R.knn_literal(c, None, k))
        for radius, max_nn in ((0.05, 0), (0.25, 0), (0.2500001, 0), (0.3, 3), (2.0, 0), (2.0, 65)):
            assert same(R.radius(c, None, radius, max_nn), R.radius_literal(c, None, radius, max_nn))


def lattice3():
    g = np.arange(3, dtype=F32)
    c = np.ones((27, 4), F32)
    c[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return c


def test_lattice_by_hand():
    """3 x 3 x 3 integer lattice queried at its centre (index 13): itself, then 6 neighbours at d2 = 1, 12 at 2, 8 at 3, each group in
    index order."""
    c = lattice3()
    idx, d2, n_found = R.knn(c, c[13:14], 27)
    assert n_found.tolist() == [27] and idx[0, 0] == 13 and d2[0].tolist() == [0.0] + [1.0] * 6 + [2.0] * 12 + [3.0] * 8
    manhattan = np.abs(c[:, :3] - 1).sum(axis=1)
    for lo, hi, dist in ((1, 7, 1), (7, 19, 2), (19, 27, 3)):
        assert idx[0, lo:hi].tolist() == np.flatnonzero(manhattan == dist).tolist()
    idx7, d7, _ = R.knn(c, c[13:14], 5)  # a cut inside a group of equals keeps the lowest indices
    assert idx7[0].tolist() == [13, 4, 10, 12, 14]
    row_start, ridx, rd2 = R.radius(c, c[13:14], math.sqrt(2.0))  # float32(2.0) exactly: d2 == r2 does not qualify
    assert row_start.tolist() == [0, 7] and ridx.tolist() == idx[0, :7].tolist()
    row_start, ridx, rd2 = R.radius(c, c[13:14], 1.5, max_nn=4)
    assert row_start.tolist() == [0, 4] and ridx.tolist() == [13, 4, 10, 12] and rd2.tolist() == [0, 1, 1, 1]
    assert R.radius(c, c[13:14], 1.0)[1].tolist() == [13]  # strict at d2 == r2 = 1
    assert R.radius(c, None, 0.0)[0].tolist() == [0] * 28  # radius 0 finds nothing, not even the query itself


def test_coincident_points_and_short_lists():
    c = np.tile(F32([4.0, 5.0, -6.0, 1.0]), (70, 1))
    idx, d2, n_found = R.knn(c, c[:2], 64)
    assert idx[0].tolist() == list(range(64)) and not d2.any() and n_found.tolist() == [64, 64]
    c[5, 0] = np.nan
    idx, d2, n_found = R.knn(c[:10], c[:3], 20)  # k > n_finite: a short list, no error
    assert n_found.tolist() == [9, 9, 9] and idx[0, :9].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9] and (idx[:, 9:] == -1).all() and np.isinf(d2[:, 9:]).all()
    idx, d2, n_found = R.knn(c[:10], c[5:6], 3)  # a non-finite query
    assert n_found.tolist() == [0] and (idx == -1).all() and np.isinf(d2).all()
    assert R.radius(c[:10], c[4:7], 1.0)[0].tolist() == [0, 9, 9, 18]
    empty = np.zeros((0, 4), F32)
    assert R.knn(empty, c[:2], 3)[2].tolist() == [0, 0] and R.radius(empty, c[:2], 1.0)[0].tolist() == [0, 0, 0]
    assert R.knn(c, empty, 3)[0].shape == (0, 3) and R.radius(c, empty, 1.0)[0].tolist() == [0]


def test_refusals():
    c = lattice3()
    for k in (0, 65, -1):
        with pytest.raises(R.Refused):
            R.knn(c, None, k)
    for radius, max_nn in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.3, -1)):
        with pytest.raises(R.Refused):
            R.radius(c, None, radius, max_nn)


def test_restatement_is_cheap_at_the_largest_device_case():
    """3 000 x 3 000 is the largest exact pass any device test asks for: the restatement answers it (seconds on an idle host; the
    time is printed, not asserted: a loaded host says nothing about the code), one row chunk never holds more than 2^21 pairs, and the
    whole-cloud radius returns every pair."""
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 3000, 5)
    assert all((b - a) * 3000 <= 1 << 21 for a, b in R._chunks(3000, 3000))
    t0 = time.perf_counter()
    idx, d2, n_found = R.knn(cloud, None, 64)
    R.radius(cloud, None, 0.5)
    row_start = R.radius(cloud, None, 1e4)[0]
    print(f"restatement, 3000 x 3000: knn 64 + radius 0.5 + whole-cloud radius in {time.perf_counter() - t0:.1f} s")
    assert row_start[-1] == 3000 * 3000 and (n_found == 64).all() and (idx[:, 0] == np.arange(3000)).all()


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for s in NEW_SYMBOLS:
        assert f" T {s}\n" in names, s
        assert f"int {s}(" in header and s in _lib.EXPORTS
    assert "#define ICPGPU_SEARCH_MAX_K 64" in header and _lib.SEARCH_MAX_K == R.SEARCH_MAX_K == 64


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    assert L.icpgpu_search_set_input(None, None, 0) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_search_size(None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_search_knn(None, None, 0, 1, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_search_radius(None, None, 0, 1.0, 0, 0, None, None, None, None) == _lib.ERR_INVALID_ARG


# ---- the tree-narrowed forms (knn_tree / radius_tree) are the brute forms, byte for byte --------------------------------------------
def forms_agree(cloud, queries, ks=(), radii=()):
    for k in ks:
        a, b = R.knn(cloud, queries, k, form="tree"), R.knn(cloud, queries, k, form="brute")
        assert [v.dtype for v in a] == [np.int32, np.float32, np.int32] and same(a, b), ("knn", k)
    for radius, max_nn in radii:
        a, b = R.radius(cloud, queries, radius, max_nn, form="tree"), R.radius(cloud, queries, radius, max_nn, form="brute")
        assert [v.dtype for v in a] == [np.int64, np.int32, np.float32] and same(a, b), ("radius", radius, max_nn)


@pytest.mark.parametrize("n", SIZES)
def test_tree_form_scan_sizes(n):
    """Sizes 1 to 3 000 (k - 1, k, k + 1 among them: k above the finite count, and k + 8 proposals reaching the whole cloud) with two
    NaN rows where the cloud has them."""
    for k in KS:
        cloud = scan(3000)[:size_of(n, k)].copy()
        cloud[[i for i in (7, 700) if i < len(cloud)], 1] = np.nan
        forms_agree(cloud, None, ks=(k,), radii=((0.0, 0), (0.3, 0), (0.5, 0)) if k == 20 else ())


def test_tree_form_ties_fall_back_to_the_sweep():
    """The shuffled 9 x 9 x 9 lattice at its points and at cell centres, every point 2 and 70 times, one point 70 times: rows whose
    decision lies inside a group of equals are answered by the whole-cloud sweep (counted), never by the tree's order."""
    cloud = lattice(9)
    cloud = cloud[np.random.default_rng(3).permutation(len(cloud))]
    centres = cloud[:200].copy()
    centres[:, :3] += F32(0.5)
    radii = ((1.0, 0), (math.sqrt(2.0), 0), (1.5, 0), (1.5, 4), (3.0, 0), (3.0, 65))
    R.tree_stats.update(rows=0, swept=0)
    forms_agree(cloud, None, ks=KS, radii=radii)
    assert R.tree_stats["swept"] > 0
    forms_agree(cloud, centres, ks=KS, radii=radii)
    for copies in (2, 70):
        base = scan(400 if copies == 2 else 40)
        for c in (np.repeat(base, copies, axis=0), np.tile(base, (copies, 1))):
            forms_agree(c, None, ks=(1, 8, 63, 64), radii=((0.3, 0), (0.3, 64), (2.0, 65)))
    one = np.tile(F32([4.0, 5.0, -6.0, 1.0]), (70, 1))
    forms_agree(one, None, ks=(1, 64), radii=((0.1, 0), (0.0, 0)))
    forms_agree(np.tile(one, (3, 1)), one[:5], ks=(1, 64), radii=((0.1, 0), (0.1, 65)))


def test_tree_form_queries_and_points_in_odd_places():
    """Queries outside the box out to 1e6, isolated returns at 300 to 1 000 m, NaN and inf rows in the cloud and among the queries,
    the clustered cloud the grid refuses, an empty cloud, no queries, radius 0, and coordinates of 1e19, whose d2 is +inf."""
    cloud = scan(1025)
    lo, hi = cloud[:, :3].min(axis=0), cloud[:, :3].max(axis=0)
    mid = (lo + hi) / 2
    q = [lo - 0.01, hi + 0.01, lo - 1.5, hi + 1.5, hi + 30.0, mid + np.array([1000.0, 0, 0]), mid - np.array([0, 700.0, 700.0]),
         np.array([1e6, -1e6, 1e6])]
    queries = np.ones((len(q), 4), F32)
    queries[:, :3] = np.array(q, F32)
    forms_agree(cloud, queries, ks=(1, 20, 64), radii=((0.5, 0), (2.0, 0), (40.0, 0), (1100.0, 0), (1100.0, 100)))

    far = np.ones((5, 4), F32)
    far[:, :3] = F32([[300, 0, 0], [-450, 200, 5], [0, 700, -3], [600, -600, 40], [1000, 10, 0]])
    base = scan(2000)
    isolated = np.concatenate([base[:1000], far[:2], base[1000:], far[2:]])
    forms_agree(isolated, None, ks=(20,), radii=((0.5, 0),))
    forms_agree(isolated, isolated[[1000, 2004, 5]], ks=(1, 64), radii=((500.0, 0),))

    holes = scan(1025).copy()
    rows = [0, 63, 64, 65, 255, 256, 1024]
    for j, i in enumerate(rows):
        holes[i, j % 3] = [np.nan, np.inf, -np.inf][j % 3]
    queries = scan(300, 9).copy()
    queries[[0, 3, 4, 63, 64, 299], 2] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    for qq in (None, queries):
        forms_agree(holes, qq, ks=(8, 64), radii=((0.5, 0), (1e4, 0), (1e4, 1000)))
        idx = R.knn(holes, qq, 64, form="tree")[0]
        assert not np.isin(idx, rows).any()

    refused = clustered(22000, 1)
    refused[7, 1] = np.nan
    forms_agree(refused, np.concatenate([refused[:100], clustered(28, 2)]), ks=(1, 20, 64), radii=((0.3, 0), (0.3, 8), (1.0, 100)))

    empty = np.empty((0, 4), F32)
    forms_agree(empty, scan(64), ks=(5,), radii=((10.0, 0),))
    forms_agree(empty, None, ks=(5,), radii=((10.0, 0),))
    forms_agree(scan(64), empty, ks=(5,), radii=((1.0, 0),))
    forms_agree(scan(3000), None, radii=((0.0, 0),))
    assert R.radius(scan(3000), None, 0.0, form="tree")[0].tolist() == [0] * 3001

    huge = scan(300).copy()
    huge[::3, :3] *= F32(1e19)  # d2 between a huge point and any other: +inf; among the others: finite
    huge[1::3, 0] += F32(1e19)
    with np.errstate(over="ignore", invalid="ignore"):  # (the brute forms' float32 products overflow aloud)
        forms_agree(huge, None, ks=(1, 8, 64), radii=((0.5, 0), (1e4, 0), (1e18, 0), (1e19, 70)))
        forms_agree(huge, scan(40, 9), ks=(8, 64), radii=((1e4, 0),))
        assert np.isinf(R.knn(huge, None, 64, form="tree")[1]).any()


@pytest.mark.parametrize("max_nn", [1, 8, 64, 65, 1000])
def test_tree_form_max_nn(max_nn):
    cloud = scan(1025).copy()
    cloud[[5, 900], 0] = np.nan
    forms_agree(cloud, None, radii=((1e4, max_nn), (0.5, max_nn), (2.0, max_nn)))


def test_forms_are_picked_by_size_and_can_be_forced(monkeypatch):
    """Every caller from before the tree forms keeps the brute form: 3 000 and 6 000 points asked for themselves
    (test_gpu_search.py, test_cluster_host.py), cluster_restated's windows of 1 024 queries over 22 000 points."""
    calls = []
    for name in ("knn_brute", "knn_tree", "radius_brute", "radius_tree"):
        monkeypatch.setattr(R, name, lambda *a, _n=name: calls.append(_n))
    small, six, big = scan(3000), np.ones((6000, 4), F32), np.ones((8193, 4), F32)
    assert max(6000 * 6000, 1024 * 22000) < 8192 * 8192 == R.TREE_ABOVE < 8193 * 8193
    R.knn(small, None, 8), R.radius(small, None, 0.5), R.knn(six, None, 8), R.radius(six, None, 1.5)
    R.radius(np.ones((22000, 4), F32), six[:1024], 0.5), R.knn(big[:8192], None, 8)
    assert calls == ["knn_brute", "radius_brute", "knn_brute", "radius_brute", "radius_brute", "knn_brute"]
    del calls[:]
    R.knn(big, None, 8), R.radius(big, None, 0.5, 3), R.knn(small, None, 8, form="tree"), R.radius(big, None, 0.5, form="brute")
    assert calls == ["knn_tree", "radius_tree", "knn_tree", "radius_brute"]
    with pytest.raises(ValueError):
        R.knn(small, None, 8, form="kd")


def test_tree_form_refusals():
    for k in (0, 65):
        with pytest.raises(R.Refused):
            R.knn_tree(lattice3(), None, k)
    for radius, max_nn in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.3, -1)):
        with pytest.raises(R.Refused):
            R.radius_tree(lattice3(), None, radius, max_nn)


def test_scan_size_rows_are_decided_without_the_sweep():
    """A CONDITION of the scan-size device tests (test_gpu_search_scale.py, test_gpu_search_consumers_scale.py), not a measurement:
    on their inputs -- the bench scan voxel-filtered at 0.2 m, here from the oracle's filter; self-queries, scan queries, the
    clustered cloud -- fewer than 1 % of the rows fall back to the whole-cloud sweep.  Otherwise the fast reference is the slow one
    in disguise.  (It is 0 on every one of these.)  One sampled comparison with the brute form at that size closes the loop."""
    F = oracle.voxel_grid(scan(200000, 6), 0.2)
    assert len(F) > 16384
    R.tree_stats.update(rows=0, swept=0)

    def share(what):
        rows, swept = R.tree_stats["rows"], R.tree_stats["swept"]
        R.tree_stats.update(rows=0, swept=0)
        print(f"{what}: {swept} of {rows} rows swept")
        assert rows > 0 and swept < 0.01 * rows, (what, swept, rows)

    for k in (1, 10, 20, 64):
        R.knn(F, None, k)
        share(f"F self k={k}")
    for radius, max_nn in ((0.3, 0), (0.5, 0), (0.8, 0), (1.0, 0), (1.0, 8), (1.0, 65), (1.2, 0)):
        R.radius(F, None, radius, max_nn)
        share(f"F self radius {radius} max_nn={max_nn}")
    q = scan(8193, 9)
    for radius in (0.5, 1.0):
        R.radius(F, q, radius)
        share(f"F, 8193 scan queries, radius {radius}")
    q = scan(131073, 9)
    R.knn(F, q, 8)
    share("F, 131073 scan queries, k=8")
    R.radius(F, q, 0.3)
    share("F, 131073 scan queries, radius 0.3")
    moved = q.copy()
    moved[:-40, 2] += F32(1000.0)
    R.radius(F, moved, 0.3)
    share("F, 131073 queries of which 131033 are 1 000 m up, radius 0.3")
    c = clustered(22000, 1)
    R.knn(c, None, 20)
    share("clustered 22 000 self k=20")
    sample = F[::37]
    assert same(R.knn(F, sample, 64, form="tree"), R.knn(F, sample, 64, form="brute"))
    assert same(R.radius(F, sample, 1.0, 65, form="tree"), R.radius(F, sample, 1.0, 65, form="brute"))
