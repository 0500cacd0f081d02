"""The feature-space k-nearest search, the sample-consensus alignment and the rest of a context: a context with
any history answers icpgpu_feature_knn and icpgpu_scp_align as a new one does; the calls change nothing an alignment, a filter, a
search, a normal or FPFH estimation, a clustering or a segmentation reads; unfetched clustering, segmentation and alignment results
survive each other; icpgpu_search_set_input drops the alignment's result."""
import functools

import numpy as np
import pytest

import cluster_restated as CR
import history_model as hm
import normals_restated as N
import sac_restated as SR
import scp_restated as R
import scp_scenes as S
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
SAC = (0.2, 50, 0.99, 3, True, None, 0.0)
SAC_NAMES = ("counts", "sample", "coeff_unrefined", "moments", "inliers")
SCP = dict(nr_samples=3, k_correspondences=2, similarity_threshold=0.9, max_correspondence_distance=0.3, inlier_fraction=0.25, max_iterations=129, seed=7)
SCP_NAMES = ("status", "source_idx", "target_idx", "transforms", "count", "sum", "error", "inliers")


scan = S.scan


@functools.lru_cache(maxsize=None)
def normals_of(n: int, seed: int = 5) -> np.ndarray:
    nrm = N.estimate(scan(n, seed), None, k=10)[0]
    nrm.setflags(write=False)
    return nrm


def alignment(c, scene, **kw):
    """One alignment over the search cloud in place and everything its fetch hands out, as bytes."""
    source, sf, target, tf = scene[:4]
    rc, T, n_in, fit, conv, cloud = c.scp_align_raw(source, sf, tf, **{**SCP, **kw})
    assert rc == 0
    f = c.scp_fetch()
    return [np.asarray(a).tobytes() for a in [T, np.float64([n_in, fit, conv, f["best_t"]]), cloud] + [f[name] for name in SCP_NAMES]]


def answers(c):
    """Feature searches and alignments over two scenes, as bytes."""
    out = []
    for scene, kw in ((S.matched(300, 257), {}), (S.matched(65, 65), dict(nr_samples=4, similarity_threshold=0.5))):
        source, sf, target, tf = scene[:4]
        out += [np.asarray(a).tobytes() for a in c.feature_knn(tf, sf, 5) + c.feature_knn(sf, tf, 64)]
        c.search_set_input(target)
        out += alignment(c, scene, **kw)
    return out


@functools.lru_cache(maxsize=None)
def fresh_answers():
    with Context(0) as fresh:
        want = answers(fresh)
    source, sf, target, tf = S.matched(300, 257)[:4]
    restated = R.feature_knn(tf, sf, 5) + R.feature_knn(sf, tf, 64)
    assert want[:6] == [np.ascontiguousarray(a).tobytes() for a in restated]
    return want


def test_a_context_with_a_modelled_history_answers_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with feature searches and alignments over other clouds between the steps: the walk's observations do not move (the model knows
    nothing of the calls), and at the end the context answers as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                scene = S.matched((63, 64, 257)[k % 3], (64, 63, 257)[k % 3], seed=2 + k % 3)
                w.ctx.feature_knn(scene[3], scene[1], 1 + k % 60)
                w.ctx.search_set_input(scene[2])
                w.ctx.scp_align(*scene[:2], scene[3], **{**SCP, "max_iterations": 33, "seed": k})
            w.step(op)
        assert w.n_obs > 10
        assert answers(w.ctx) == fresh_answers()


def test_a_context_with_history_answers_as_a_new_one():
    want = fresh_answers()
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw = scan(20000, 6)
    big = S.matched(1500, 1500)
    with Context(0) as c:
        for method in (hm.P2P, hm.GICP, hm.P2PLANE, hm.NDT):
            c.set_params(method=method, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.radius_outlier_removal(raw, 0.3, 5)
        c.voxel_grid(raw, 0.4)
        c.feature_knn(big[3], big[1], 33)                  # larger calls of their own first
        c.search_set_input(big[2])
        c.scp_align(*big[:2], big[3], **{**SCP, "similarity_threshold": 0.0, "max_iterations": 70})
        c.search_set_input(raw)                            # another search cloud: searches, normals, histograms, a clustering, a segmentation
        c.search_knn(scan(300, 9), 20)
        normals, _ = c.normal_estimation(None, k=20)
        c.fpfh_estimation(normals, scan(300, 9), radius=0.5)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        assert answers(c) == want
        c.statistical_outlier_removal(scan(2000), 8, 1.0)
        c.search_radius(scan(300, 9), 1.0)
        assert answers(c) == want


def observations(c, src, tgt, raw, queries, normals):
    """An alignment per method, both filters, the voxel filter, searches, normal and FPFH estimations, clusterings and a segmentation:
    everything as bytes."""
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
    out += list(c.fpfh_estimation(normals, None, k=10, want_spfh=True) + c.fpfh_estimation(normals, queries, radius=0.6))
    out += list(c.euclidean_cluster_extraction(0.5) + c.euclidean_cluster_extraction(0.25, 2, 50))
    rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*SAC)
    assert rc == 0
    out += [coeff, np.int64([n_inliers, iterations, found]), c.sac_extract(False)]
    return [np.asarray(a).tobytes() for a in out]


def test_everything_else_returns_the_same_bits_after_the_calls():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries, normals = scan(20000, 6), scan(2000), scan(300, 9), normals_of(2000)
    source = S.moved(cloud[::7], np.linalg.inv(S.rigid(0.5, 0.0, 0.02, (1.0, -2.0, 0.1))))
    tf = S.descriptors(2000, 3)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, queries, normals)
        c.feature_knn(tf, tf[::7], 5)                       # both calls, the alignment on the same search cloud
        c.feature_knn(S.descriptors(700, 4), tf, 64)
        r = c.scp_align(source, tf[::7], tf, **{**SCP, "k_correspondences": 1})
        assert r["converged"] and r["inliers"].size > 200
        c.scp_align(source, tf[::7], tf, **{**SCP, "similarity_threshold": 0.0, "max_iterations": 70})
        second = observations(c, src, tgt, raw, queries, normals)
    assert first == second


def test_unfetched_results_survive_each_other():
    cloud, queries, normals = scan(2000), scan(300, 9), normals_of(2000)
    source = S.moved(cloud[::7], np.linalg.inv(S.rigid(0.5, 0.0, 0.02, (1.0, -2.0, 0.1))))
    tf = S.descriptors(2000, 3)
    scene = (source, tf[::7], cloud, tf)
    want_clusters = CR.extract(cloud, 0.5, 2, 50)
    r = SR.segment(cloud, *SAC)
    with Context(0) as c:
        c.search_set_input(cloud)
        want_alignment = alignment(c, scene, k_correspondences=1)
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert (rc, n_clusters, n_clustered) == (0, want_clusters[0].size - 1, want_clusters[1].size)
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*SAC)
        assert rc == 0 and found == 1
        rc, T, n_in, fit, conv, aligned = c.scp_align_raw(source, tf[::7], tf, **{**SCP, "k_correspondences": 1})      # the alignment over both unfetched results
        assert rc == 0 and conv == 1
        c.feature_knn(tf, tf[::7], 5)                       # ... and the feature search, searches, normals and histograms over all three
        c.search_knn(queries, 20)
        c.search_radius(queries, 1.0)
        c.normal_estimation(None, k=10)
        c.fpfh_estimation(normals, queries, radius=0.6)
        c.feature_knn(S.descriptors(700, 4), tf, 64)
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and all(np.asarray(g).dtype == w.dtype and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(arrays, want_clusters))
        rc, f = c.sac_fetch_raw(n_inliers, iterations)
        assert rc == 0
        got = [coeff, np.int64([n_inliers, iterations, found, f["best_t"], f["n_unrefined"]])] + [f[name] for name in SAC_NAMES]
        got += [c.sac_extract(False), c.sac_extract(True)]
        want = [r["coeff"], np.int64([r["inliers"].size, r["iterations"], r["found"], r["best_t"], r["n_unrefined"]])] + [r[name] for name in SAC_NAMES]
        want += [SR.extract(cloud, r["inliers"], False), SR.extract(cloud, r["inliers"], True)]
        assert [np.asarray(a).tobytes() for a in got] == [np.ascontiguousarray(a).tobytes() for a in want]
        f = c.scp_fetch()                                   # the alignment's result, after a clustering and a segmentation as well
        c.cluster_extract_raw(0.25, 2, 50)
        c.sac_segment_raw(0.1, 70, 0.99, 9, True, None, 0.0)
        f2 = c.scp_fetch()
        got = [T, np.float64([n_in, fit, conv, f["best_t"]]), aligned] + [f[name] for name in SCP_NAMES]
        assert [np.asarray(a).tobytes() for a in got] == want_alignment
        assert all(np.asarray(f[name]).tobytes() == np.asarray(f2[name]).tobytes() for name in SCP_NAMES)
        c.search_set_input(cloud)                           # the same cloud again: the result is dropped all the same
        assert c.scp_fetch_raw(129, 2000, 3)[0] == _lib.ERR_INVALID_ARG
        assert c._L.icpgpu_scp_stats(c._h, None, None, None) == _lib.ERR_INVALID_ARG
