"""The plane segmentation and the rest of a context: a context with any history segments as a new one does; a
segmentation (and an extract) changes nothing an alignment, a filter, a search, a normal estimation or a clustering reads; unfetched
clustering and segmentation results survive each other; icpgpu_search_set_input drops the result."""
import functools

import numpy as np
import pytest

import cluster_restated as CR
import history_model as hm
import sac_restated as R
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
CALLS = ((0.2, 50, 0.99, 3, True, None, 0.0), (0.004, 130, 0.99, 9, True, None, 0.0), (0.2, 50, 0.9, 1, False, (0.1, 0.0, 1.0), 0.3))
NAMES = ("counts", "sample", "coeff_unrefined", "moments", "inliers")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def segmentation(c, args):
    """Everything one call and its fetch and extracts hand out, as bytes."""
    rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*args)
    assert rc == 0
    rc, f = c.sac_fetch_raw(n_inliers, iterations)
    assert rc == 0
    out = [coeff, np.int64([n_inliers, iterations, found, f["best_t"], f["n_unrefined"]])] + [f[name] for name in NAMES]
    out += [c.sac_extract(False), c.sac_extract(True, view=True)]
    return [np.asarray(a).tobytes() for a in out]


def restated(cloud, args):
    r = R.segment(cloud, *args)
    out = [r["coeff"], np.int64([r["inliers"].size, r["iterations"], r["found"], r["best_t"], r["n_unrefined"]])] + [r[name] for name in NAMES]
    out += [R.extract(cloud, r["inliers"], False), R.extract(cloud, r["inliers"], True)]
    return [np.ascontiguousarray(a).tobytes() for a in out]


def segmentations(c, cloud):
    c.search_set_input(cloud)
    return [segmentation(c, args) for args in CALLS]


@functools.lru_cache(maxsize=None)
def fresh_segmentations():
    with Context(0) as fresh:
        want = segmentations(fresh, scan(3000))
    assert want == [restated(scan(3000), args) for args in CALLS]
    return want


def test_a_context_with_a_modelled_history_segments_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with segmentations and extracts over other clouds between the steps: the walk's observations do not move (the model knows nothing
    of segmentation), and at the end the context segments as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                w.ctx.search_set_input(scan(1025, 9 + k % 3))
                w.ctx.sac_segment_raw(0.1 + 0.1 * (k % 3), 50 + 40 * (k % 2), 0.99, k)      # (unfetched results are left lying, too)
                if k % 8 == 1:
                    w.ctx.sac_extract(True, view=True)
            w.step(op)
        assert w.n_obs > 10
        assert segmentations(w.ctx, scan(3000)) == fresh_segmentations()


def test_a_context_with_history_segments_as_a_new_one():
    want = fresh_segmentations()
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
        c.search_set_input(raw)                       # another, larger search cloud first: searches, normals, a clustering, a segmentation
        c.search_knn(scan(300, 9), 20)
        c.normal_estimation(None, k=20)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        c.sac_extract(True)
        assert segmentations(c, scan(3000)) == want
        c.statistical_outlier_removal(scan(3000), 8, 1.0)   # a filter and a clustering between two segmentations of the same cloud
        c.euclidean_cluster_extraction(0.5)
        assert segmentation(c, CALLS[0]) == want[0]


def observations(c, src, tgt, raw, cloud, queries):
    """An alignment per method, both filters, the voxel filter, searches, normal estimations and clusterings: everything as bytes."""
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
    out += list(c.euclidean_cluster_extraction(0.5) + c.euclidean_cluster_extraction(0.25, 2, 50))
    return [np.asarray(a).tobytes() for a in out]


def test_everything_else_returns_the_same_bits_after_a_segmentation():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(3000), scan(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, cloud, queries)
        for args in CALLS:                                                # on the same search cloud: the search state must stay as it is
            assert segmentation(c, args) == restated(cloud, args)
        second = observations(c, src, tgt, raw, cloud, queries)
        c.sac_segment_raw(0.3, 200, 0.999, 8)                             # ... and with a result left unfetched
        third = observations(c, src, tgt, raw, cloud, queries)
    assert first == second == third


def test_unfetched_cluster_and_segmentation_results_survive_each_other():
    cloud, queries = scan(3000), scan(300, 9)
    want_clusters = CR.extract(cloud, 0.5, 2, 50)
    want = restated(cloud, CALLS[0])
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert (rc, n_clusters, n_clustered) == (0, want_clusters[0].size - 1, want_clusters[1].size)
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*CALLS[0])       # a segmentation over an unfetched clustering
        assert rc == 0 and found == 1
        c.sac_extract(True, view=True)
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and all(np.asarray(g).dtype == w.dtype and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(arrays, want_clusters))
        c.euclidean_cluster_extraction(2.0, 5, 5)                                    # clusterings, searches, normals and a filter over
        c.cluster_extract_raw(0.25, 1, INT_MAX)                                      # the unfetched segmentation
        c.search_knn(None, 64)
        c.search_radius(None, 2.0)
        c.search_radius(queries, 3.0, 70)
        c.normal_estimation(None, k=20, want_moments=True)
        c.statistical_outlier_removal(cloud, 8, 1.0)
        rc, f = c.sac_fetch_raw(n_inliers, iterations)
        assert rc == 0
        got = [coeff, np.int64([n_inliers, iterations, found, f["best_t"], f["n_unrefined"]])] + [f[name] for name in NAMES]
        got += [c.sac_extract(False), c.sac_extract(True)]
        assert [np.asarray(a).tobytes() for a in got] == want


def test_search_set_input_drops_the_result():
    cloud = scan(1025)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(0.2)
        assert rc == 0 and found == 1 and c.sac_fetch_raw(n_inliers, iterations)[0] == 0
        c.search_set_input(cloud)                     # the same cloud again: the result is gone all the same
        assert c.sac_fetch_raw(n_inliers, iterations)[0] == _lib.ERR_INVALID_ARG
        with pytest.raises(_lib.IcpGpuError):
            c.sac_extract(False)
        again = c.sac_segment_raw(0.2)
        assert again[0] == 0 and again[2:] == (n_inliers, iterations, found) and again[1].tobytes() == coeff.tobytes()
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): whatever it returns
        assert rc == _lib.ERR_INVALID_ARG
        assert c.sac_fetch_raw(n_inliers, iterations)[0] == _lib.ERR_INVALID_ARG
        assert c.sac_segment_raw(0.2)[0] == _lib.ERR_INVALID_ARG                     # (and there is no search cloud any more)
