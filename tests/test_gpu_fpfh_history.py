"""The fast point feature histograms and the rest of a context: a context with any history answers
icpgpu_fpfh_estimation as a new one does; the call changes nothing an alignment, a filter, a search, a normal estimation, a clustering
or a segmentation reads; unfetched clustering and segmentation results survive it."""
import functools

import numpy as np
import pytest

import cluster_restated as CR
import fpfh_restated as R
import history_model as hm
import normals_restated as N
import sac_restated as SR
from icpslam_amd import Context, synth

pytestmark = pytest.mark.gpu
SAC = (0.2, 50, 0.99, 3, True, None, 0.0)
SAC_NAMES = ("counts", "sample", "coeff_unrefined", "moments", "inliers")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def normals_of(n: int, seed: int = 5) -> np.ndarray:
    nrm = N.estimate(scan(n, seed), None, k=10)[0]
    nrm.setflags(write=False)
    return nrm


def histograms(c, cloud, normals, queries):
    """Four calls over one search cloud -- both modes, with and without queries -- as bytes."""
    c.search_set_input(cloud)
    out = (c.fpfh_estimation(normals, None, k=10, want_spfh=True) + c.fpfh_estimation(normals, queries, radius=0.6, want_spfh=True)
           + c.fpfh_estimation(normals, queries, k=64, want_spfh=True) + c.fpfh_estimation(normals, None, radius=0.4, want_spfh=True))
    return [np.asarray(a).tobytes() for a in out]


@functools.lru_cache(maxsize=None)
def fresh_histograms():
    cloud, normals, queries = scan(2000), normals_of(2000), scan(300, 9)
    with Context(0) as fresh:
        want = histograms(fresh, cloud, normals, queries)
    restated = (R.estimate(cloud, normals, None, k=10) + R.estimate(cloud, normals, queries, radius=0.6) + R.estimate(cloud, normals, queries, k=64)
                + R.estimate(cloud, normals, None, radius=0.4))
    assert want == [np.ascontiguousarray(a).tobytes() for a in restated]
    return want


def test_a_context_with_a_modelled_history_answers_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with histograms over other clouds between the steps: the walk's observations do not move (the model knows nothing of the call),
    and at the end the context answers as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                n = (1025, 700, 257)[k % 3]
                w.ctx.search_set_input(scan(n, 9 + k % 3))
                w.ctx.fpfh_estimation(normals_of(n, 9 + k % 3), None if k % 8 == 1 else scan(100, 4), **(dict(k=5 + k % 50) if k % 8 == 1 else dict(radius=0.5)))
            w.step(op)
        assert w.n_obs > 10
        assert histograms(w.ctx, scan(2000), normals_of(2000), scan(300, 9)) == fresh_histograms()


def test_a_context_with_history_answers_as_a_new_one():
    want = fresh_histograms()
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw = scan(20000, 6)
    with Context(0) as c:
        for method in (hm.P2P, hm.GICP, hm.P2PLANE, hm.NDT):
            c.set_params(method=method, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.radius_outlier_removal(raw, 0.3, 5)
        c.voxel_grid(raw, 0.4)
        c.search_set_input(raw)                       # another, larger search cloud first: searches, normals, histograms, a clustering, a segmentation
        c.search_knn(scan(300, 9), 20)
        big_normals, _ = c.normal_estimation(None, k=20)
        c.fpfh_estimation(big_normals, None, k=20)
        c.fpfh_estimation(big_normals, scan(300, 9), radius=0.5)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        assert histograms(c, scan(2000), normals_of(2000), scan(300, 9)) == want
        c.statistical_outlier_removal(scan(2000), 8, 1.0)   # a filter, a clustering and a segmentation between two calls on the same cloud
        c.euclidean_cluster_extraction(0.5)
        c.sac_plane_segmentation(0.2, 50, 0.99, 3)
        got = c.fpfh_estimation(normals_of(2000), None, k=10, want_spfh=True)
        assert [np.asarray(a).tobytes() for a in got] == want[:3]


def observations(c, src, tgt, raw, queries):
    """An alignment per method, both filters, the voxel filter, searches, normal estimations, clusterings and a segmentation: everything
    as bytes."""
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
    rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*SAC)
    assert rc == 0
    out += [coeff, np.int64([n_inliers, iterations, found]), c.sac_extract(False)]
    return [np.asarray(a).tobytes() for a in out]


def test_everything_else_returns_the_same_bits_after_the_call():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(2000), scan(300, 9)
    normals = normals_of(2000)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, queries)
        for q, mode in ((None, dict(k=10)), (queries, dict(radius=0.6)), (queries, dict(k=64)), (None, dict(radius=0.4))):  # on the same search cloud
            got = c.fpfh_estimation(normals, q, want_spfh=True, **mode)
            want = R.estimate(cloud, normals, q, **mode)
            assert [np.asarray(a).tobytes() for a in got] == [np.ascontiguousarray(a).tobytes() for a in want]
        second = observations(c, src, tgt, raw, queries)
    assert first == second


def test_unfetched_cluster_and_segmentation_results_survive_the_call():
    cloud, queries, normals = scan(2000), scan(300, 9), normals_of(2000)
    want_clusters = CR.extract(cloud, 0.5, 2, 50)
    r = SR.segment(cloud, *SAC)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert (rc, n_clusters, n_clustered) == (0, want_clusters[0].size - 1, want_clusters[1].size)
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*SAC)
        assert rc == 0 and found == 1
        c.fpfh_estimation(normals, None, k=20)                                       # histograms in every mode over both unfetched results
        c.fpfh_estimation(normals, queries, radius=0.6)
        c.fpfh_estimation(normals, queries, k=64, want_spfh=True)
        c.fpfh_estimation(normals, None, radius=1.0)
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and all(np.asarray(g).dtype == w.dtype and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(arrays, want_clusters))
        rc, f = c.sac_fetch_raw(n_inliers, iterations)
        assert rc == 0
        got = [coeff, np.int64([n_inliers, iterations, found, f["best_t"], f["n_unrefined"]])] + [f[name] for name in SAC_NAMES]
        got += [c.sac_extract(False), c.sac_extract(True)]
        want = [r["coeff"], np.int64([r["inliers"].size, r["iterations"], r["found"], r["best_t"], r["n_unrefined"]])] + [r[name] for name in SAC_NAMES]
        want += [SR.extract(cloud, r["inliers"], False), SR.extract(cloud, r["inliers"], True)]
        assert [np.asarray(a).tobytes() for a in got] == [np.ascontiguousarray(a).tobytes() for a in want]
