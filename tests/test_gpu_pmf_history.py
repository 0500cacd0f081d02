"""The ground filter and the rest of a context: a context with any history filters as a new one does; a filter,
an operator call and an extract change nothing an alignment, a filter, a search, a normal estimation, a clustering or a segmentation
reads; unfetched clustering, segmentation, ISS and ground filter results survive each other; icpgpu_search_set_input drops the result."""
import functools

import numpy as np
import pytest

import cluster_restated as CR
import history_model as hm
import pmf_restated as R
import sac_restated as SR
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
CALLS = (dict(), dict(max_window_size=9, slope=1.0, initial_distance=0.3, cell_size=0.5), dict(max_window_size=8, exponential=False, base=1.0))
NAMES = ("ground", "windows", "thresholds", "ground_after", "removed_at")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def filtering(c, kw):
    """Everything one filter call, its fetch, an operator call and the extracts hand out, as bytes."""
    rc, n_ground, n_passes = c.pmf_filter_raw(**kw)
    assert rc == 0
    rc, f = c.pmf_fetch_raw(n_ground, n_passes)
    assert rc == 0
    out = [np.int64([n_ground, n_passes])] + [f[name] for name in NAMES]
    out += [c.morphological_operator(4.0, R.CLOSE), c.pmf_extract(False), c.pmf_extract(True, view=True)]
    return [np.asarray(a).tobytes() for a in out]


def restated(cloud, kw):
    r = R.run(cloud, **kw)
    out = [np.int64([r["ground"].size, r["windows"].size])] + [r[name] for name in NAMES]
    out += [R.operator(cloud, 4.0, R.CLOSE), R.extract(cloud, r["ground"], False), R.extract(cloud, r["ground"], True)]
    return [np.ascontiguousarray(a).tobytes() for a in out]


def filterings(c, cloud):
    c.search_set_input(cloud)
    return [filtering(c, kw) for kw in CALLS]


@functools.lru_cache(maxsize=None)
def fresh_filterings():
    with Context(0) as fresh:
        want = filterings(fresh, scan(2000))
    assert want == [restated(scan(2000), kw) for kw in CALLS]
    return want


def test_a_context_with_a_modelled_history_filters_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with ground filters, operator calls and extracts over other clouds between the steps: the walk's observations do not move (the model
    knows nothing of the ground filter), and at the end the context filters as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                w.ctx.search_set_input(scan(1025, 9 + k % 3))
                w.ctx.pmf_filter_raw(max_window_size=3 + 6 * (k % 3), slope=0.5 + 0.25 * (k % 2))   # (unfetched results are left lying, too)
                if k % 8 == 1:
                    w.ctx.pmf_extract(True, view=True)
                else:
                    w.ctx.morphological_operator(2.0 + k % 3, k % 4)
            w.step(op)
        assert w.n_obs > 10
        assert filterings(w.ctx, scan(2000)) == fresh_filterings()


def test_a_context_with_history_filters_as_a_new_one():
    want = fresh_filterings()
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw = scan(20000, 6)
    with Context(0) as c:
        for method in (hm.P2P, hm.GICP, hm.NDT):
            c.set_params(method=method, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.voxel_grid(raw, 0.4)
        c.search_set_input(raw)                       # another, larger search cloud first: a search, a clustering, a segmentation, a filter
        c.search_knn(scan(300, 9), 20)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        c.progressive_morphological_filter(max_window_size=17)
        c.morphological_operator(50.0, R.DILATE)
        c.pmf_extract(True)
        assert filterings(c, scan(2000)) == want
        c.statistical_outlier_removal(scan(2000), 8, 1.0)   # a filter, a clustering and a segmentation between two filterings of the same cloud
        c.euclidean_cluster_extraction(0.5)
        c.sac_plane_segmentation(0.2)
        assert filtering(c, CALLS[0]) == want[0]


def observations(c, src, tgt, raw, cloud, queries):
    """An alignment per method, both outlier filters, the voxel filter, searches, normal estimations, clusterings, a segmentation and ISS
    keypoints: everything as bytes."""
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
    inliers, coeff, iterations, found = c.sac_plane_segmentation(0.2, 50, 0.99, 3)
    out += [inliers, coeff, np.int64([iterations, found]), c.sac_extract(True)]
    return [np.asarray(a).tobytes() for a in out]


def test_everything_else_returns_the_same_bits_after_a_ground_filter():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(2000), scan(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, cloud, queries)
        for kw in CALLS:                                                  # on the same search cloud: the search state must stay as it is
            assert filtering(c, kw) == restated(cloud, kw)
        second = observations(c, src, tgt, raw, cloud, queries)
        c.pmf_filter_raw(max_window_size=17)                              # ... and with a result left unfetched
        c.morphological_operator(7.0, R.OPEN)
        third = observations(c, src, tgt, raw, cloud, queries)
    assert first == second == third


def test_unfetched_cluster_segmentation_iss_and_ground_filter_results_survive_each_other():
    cloud, queries = scan(2000), scan(300, 9)
    want_clusters = CR.extract(cloud, 0.5, 2, 50)
    want_sac = SR.segment(cloud, 0.2, 50, 0.99, 3, True)
    want = restated(cloud, CALLS[0])
    with Context(0) as c, Context(0) as other:
        other.search_set_input(cloud)
        want_iss = other.iss_keypoints(1.0, 0.8, 0.975, 0.975, 5)
        c.search_set_input(cloud)
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert (rc, n_clusters, n_clustered) == (0, want_clusters[0].size - 1, want_clusters[1].size)
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(0.2, 50, 0.99, 3)
        assert rc == 0 and found == 1
        rc, n_keypoints = c.iss_keypoints_raw(1.0, 0.8, 0.975, 0.975, 5)
        assert rc == 0 and n_keypoints == want_iss["n_keypoints"] > 0
        rc, n_ground, n_passes = c.pmf_filter_raw(**CALLS[0])            # a ground filter over unfetched clustering and segmentation results
        assert rc == 0
        c.morphological_operator(3.0, R.ERODE)
        c.pmf_extract(True, view=True)
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and all(np.asarray(g).dtype == w.dtype and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(arrays, want_clusters))
        rc, f = c.sac_fetch_raw(n_inliers, iterations)
        assert rc == 0 and f["inliers"].tobytes() == want_sac["inliers"].tobytes() and f["counts"].tobytes() == want_sac["counts"].tobytes()
        assert coeff.tobytes() == want_sac["coeff"].tobytes()
        rc, got_iss = c.iss_fetch_raw(n_keypoints)
        assert rc == 0 and all(np.asarray(got_iss[k]).tobytes() == np.asarray(want_iss[k]).tobytes() for k in got_iss)
        c.euclidean_cluster_extraction(2.0, 5, 5)                        # clusterings, a segmentation, keypoints, searches, normals and a
        c.cluster_extract_raw(0.25, 1, 2**31 - 1)                        # filter over the unfetched ground filter result
        c.sac_segment_raw(0.3, 200, 0.999, 8)
        c.sac_extract(True, view=True)
        c.iss_keypoints(1.0, 0.8, 0.975, 0.975, 5)
        c.search_knn(None, 64)
        c.search_radius(queries, 3.0, 70)
        c.normal_estimation(None, k=20, want_moments=True)
        c.statistical_outlier_removal(cloud, 8, 1.0)
        rc, f = c.pmf_fetch_raw(n_ground, n_passes)
        assert rc == 0
        got = [np.int64([n_ground, n_passes])] + [f[name] for name in NAMES]
        got += [c.morphological_operator(4.0, R.CLOSE), c.pmf_extract(False), c.pmf_extract(True)]
        assert [np.asarray(a).tobytes() for a in got] == want


def test_search_set_input_drops_the_result():
    cloud = scan(1025)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_ground, n_passes = c.pmf_filter_raw()
        assert rc == 0 and n_ground > 0 and c.pmf_fetch_raw(n_ground, n_passes)[0] == 0
        c.search_set_input(cloud)                     # the same cloud again: the result is gone all the same
        assert c.pmf_fetch_raw(n_ground, n_passes)[0] == _lib.ERR_INVALID_ARG
        assert c._L.icpgpu_pmf_stats(c._h, None, None) == _lib.ERR_INVALID_ARG
        with pytest.raises(_lib.IcpGpuError):
            c.pmf_extract(False)
        assert c.pmf_filter_raw() == (0, n_ground, n_passes)
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): whatever it returns
        assert rc == _lib.ERR_INVALID_ARG
        assert c.pmf_fetch_raw(n_ground, n_passes)[0] == _lib.ERR_INVALID_ARG
        assert c.pmf_filter_raw()[0] == _lib.ERR_INVALID_ARG                         # (and there is no search cloud any more)
