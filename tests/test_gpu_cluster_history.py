"""Euclidean clustering and the rest of a context: a context with any history clusters as a new one does; a
clustering call changes nothing an alignment, a filter, a search or a normal estimation reads; a result that has not been fetched
outlives later search and normal calls; icpgpu_search_set_input drops it."""
import functools

import numpy as np
import pytest

import cluster_restated as R
import history_model as hm
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def same(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def clusterings(c, cloud):
    c.search_set_input(cloud)
    return c.euclidean_cluster_extraction(0.5) + c.euclidean_cluster_extraction(0.25, 2, 50) + c.euclidean_cluster_extraction(2.0, 5, 5)


@functools.lru_cache(maxsize=None)
def fresh_clusterings():
    with Context(0) as fresh:
        want = clusterings(fresh, scan(3000))
    ref = R.extract(scan(3000), 0.5) + R.extract(scan(3000), 0.25, 2, 50) + R.extract(scan(3000), 2.0, 5, 5)
    assert same(want, ref)
    return want


def test_a_context_with_a_modelled_history_clusters_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with clustering calls over other clouds between the steps: the walk's observations do not move (the model knows nothing of
    clustering), and at the end the context clusters as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                w.ctx.search_set_input(scan(1025, 9 + k % 3))
                w.ctx.euclidean_cluster_extraction(0.5 + 0.25 * (k % 3), 1 + k % 2)   # (unfetched results are left lying, too)
                if k % 8 == 1:
                    w.ctx.cluster_extract_raw(1.0, 1, INT_MAX)
            w.step(op)
        assert w.n_obs > 10
        assert same(clusterings(w.ctx, scan(3000)), fresh_clusterings())


def test_a_context_with_history_clusters_as_a_new_one():
    want = fresh_clusterings()
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw = scan(20000, 6)
    with Context(0) as c:
        for method in (hm.P2P, hm.GICP, hm.NDT):
            c.set_params(method=method, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.radius_outlier_removal(raw, 0.3, 5)
        c.voxel_grid(raw, 0.4)
        c.search_set_input(raw)                       # another, larger search cloud first: searches, normals and a clustering of it
        c.search_knn(scan(300, 9), 20)
        c.search_radius(scan(300, 9), 3.0, 70)
        c.normal_estimation(None, k=20)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        assert same(clusterings(c, scan(3000)), want)
        c.statistical_outlier_removal(scan(3000), 8, 1.0)   # a filter between two clusterings of the same cloud
        assert same(c.euclidean_cluster_extraction(0.5), want[0:4])


def observations(c, src, tgt, raw, cloud, queries):
    """An alignment per method, both filters, the voxel filter, searches and normal estimations: everything as bytes."""
    out = []
    for method in (hm.P2P, hm.GICP, hm.P2PLANE, hm.NDT):
        c.set_params(method=method, max_iterations=6)
        c.set_source(src)
        c.set_target(tgt)
        r = c.align(want_cloud=True, want_fitness=True)
        out += [r["T"], r["cloud"]] + [np.float64(r[k]) for k in ("iterations", "n_corr", "converged", "fitness", "mse")]
    out += [c.statistical_outlier_removal(raw, 19, 1.0), c.outlier_fetch()["measure"], c.radius_outlier_removal(raw, 0.3, 5), c.voxel_grid(raw, 0.4)]
    out += list(c.search_knn(None, 20) + c.search_radius(queries, 3.0, 70) + c.search_radius(None, 0.5))
    out += list(c.normal_estimation(None, k=20, want_moments=True) + c.normal_estimation(queries, radius=0.8))
    return [np.asarray(a).tobytes() for a in out]


def test_everything_else_returns_the_same_bits_after_a_clustering_call():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(3000), scan(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, cloud, queries)
        for tolerance, lo, hi in ((0.5, 1, INT_MAX), (2.0, 2, 50)):      # on the same search cloud: the search state must stay as it is
            assert same(c.euclidean_cluster_extraction(tolerance, lo, hi), R.extract(cloud, tolerance, lo, hi))
        second = observations(c, src, tgt, raw, cloud, queries)
        c.cluster_extract_raw(1.0, 1, INT_MAX)                            # ... and with a result left unfetched
        third = observations(c, src, tgt, raw, cloud, queries)
    assert first == second == third


def test_an_unfetched_result_survives_search_and_normal_calls():
    cloud, queries = scan(3000), scan(300, 9)
    want = R.extract(cloud, 0.5, 2, 50)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert (rc, n_clusters, n_clustered) == (0, want[0].size - 1, want[1].size)
        c.search_knn(None, 64)
        c.search_knn(queries, 20)
        c.search_radius(None, 2.0)                    # (rows far longer than the clustering's arrays: the search scratch grows)
        c.search_radius(queries, 3.0, 70)
        c.normal_estimation(None, k=20, want_moments=True)
        c.normal_estimation(queries, radius=0.8)
        c.statistical_outlier_removal(cloud, 8, 1.0)
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and same(arrays, want)


def test_search_set_input_drops_the_result():
    cloud = scan(1025)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 1, INT_MAX)
        assert rc == 0 and c.cluster_fetch_raw(n_clusters, n_clustered)[0] == 0
        c.search_set_input(cloud)                     # the same cloud again: the result is gone all the same
        assert c.cluster_fetch_raw(n_clusters, n_clustered)[0] == _lib.ERR_INVALID_ARG
        assert c.cluster_extract_raw(0.5, 1, INT_MAX) == (0, n_clusters, n_clustered)
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): whatever it returns
        assert rc == _lib.ERR_INVALID_ARG
        assert c.cluster_fetch_raw(n_clusters, n_clustered)[0] == _lib.ERR_INVALID_ARG
        assert c.cluster_extract_raw(0.5, 1, INT_MAX)[0] == _lib.ERR_INVALID_ARG   # (and there is no search cloud any more)
