"""The neighbour search and the rest of a context: the search calls change nothing an alignment reads, a
search's answers depend on nothing the context did before, and a new search cloud never meets the previous one's grid."""
import functools

import numpy as np
import pytest

import search_restated as R
from icpslam_amd import GICP, NDT, P2P_SVD, Context, synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def same(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def searches(c, cloud, queries):
    c.search_set_input(cloud)
    return c.search_knn(None, 20) + c.search_knn(queries, 64) + c.search_radius(None, 0.5) + c.search_radius(queries, 3.0, 70)


@pytest.mark.parametrize("method", [P2P_SVD, GICP, NDT])
def test_an_alignment_returns_the_same_bits_after_searches(method):
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    with Context(0) as c:
        c.set_params(method=method, max_iterations=8)
        c.set_source(src)
        c.set_target(tgt)
        first = c.align(want_cloud=True, want_fitness=True)
        searches(c, scan(3000), scan(300, 9))
        second = c.align(want_cloud=True, want_fitness=True)
        c.search_set_input(tgt)  # the target's own points as a search cloud: another buffer, another grid
        c.search_knn(src, 8)
        third = c.align(want_cloud=True, want_fitness=True)
    for other in (second, third):
        for k in ("T", "cloud"):
            assert first[k].tobytes() == other[k].tobytes(), k
        for k in ("iterations", "n_corr", "converged", "fitness", "mse"):  # (as bits: NDT reports no mse, a NaN)
            assert np.float64(first[k]).tobytes() == np.float64(other[k]).tobytes(), k


def test_a_context_with_history_searches_as_a_new_one():
    cloud, queries = scan(3000), scan(300, 9)
    with Context(0) as fresh:
        want = searches(fresh, cloud, queries)
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw = scan(20000, 6)
    with Context(0) as c:
        for method in (P2P_SVD, GICP, NDT):
            c.set_params(method=method, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.radius_outlier_removal(raw, 0.3, 5)
        c.voxel_grid(raw, 0.4)
        searches(c, raw, scan(1025))  # another, larger search cloud and other queries first
        got = searches(c, cloud, queries)
        assert same(got, want)
        c.statistical_outlier_removal(cloud, 8, 1.0)  # a filter between two searches of the same cloud
        assert same(c.search_knn(None, 20) + c.search_radius(queries, 3.0, 70), want[0:3] + want[9:12])
    assert same(want[0:3], R.knn(cloud, None, 20)) and same(want[9:12], R.radius(cloud, queries, 3.0, 70))


def test_a_second_cloud_never_meets_the_first_ones_grid():
    """Same size, one point moved 40 m: with the first cloud's grid the moved point would be binned where it no longer is."""
    a = scan(1025)
    b = a.copy()
    b[500, :3] += np.float32([40.0, -40.0, 3.0])
    queries = np.concatenate([a[495:505], b[500:501]])
    refs = {id(x): (R.knn(x, queries, 8), R.radius(x, queries, 1.0)) for x in (a, b)}
    assert not same(refs[id(a)][0], refs[id(b)][0])
    with Context(0) as c:
        for cloud in (a, b, a, a, b):
            c.search_set_input(cloud)
            assert same(c.search_knn(queries, 8), refs[id(cloud)][0])
            assert same(c.search_radius(queries, 1.0), refs[id(cloud)][1])
