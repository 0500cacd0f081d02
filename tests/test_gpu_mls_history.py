"""Moving least squares and the rest of a context: a context with any history answers
icpgpu_moving_least_squares and icpgpu_mls_fetch as a new one does; the calls change nothing an alignment, a filter, a search, a normal
estimation, a histogram, a clustering or a segmentation reads; unfetched clustering, segmentation, sample-consensus and ISS results
survive them and their own record survives those; icpgpu_search_set_input drops it."""
import functools

import numpy as np
import pytest

import cluster_restated as CR
import history_model as hm
import iss_restated as IR
import mls_restated as R
import normals_restated as N
import sac_restated as SR
import scp_scenes as S
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
SAC = (0.2, 50, 0.99, 3, True, None, 0.0)
SAC_NAMES = ("counts", "sample", "coeff_unrefined", "moments", "inliers")
SCP = dict(nr_samples=3, k_correspondences=1, similarity_threshold=0.9, max_correspondence_distance=0.3, inlier_fraction=0.25, max_iterations=129, seed=7)
SCP_NAMES = ("status", "source_idx", "target_idx", "transforms", "count", "sum", "error", "inliers")
ISS = (1.5, 1.0, 0.975, 0.975, 5)
CALLS = ((None, 1.5, 2, 0.0), (None, 1.0, 3, 0.0), ("queries", 0.8, 2, 0.3), (None, 2.0, 0, 0.0))     # (queries, radius, order, s)

scan = S.scan


def canonical(a):
    """An array's bytes with every NaN the same NaN (a computed NaN's sign and payload are the processor's)."""
    a = np.ascontiguousarray(a)
    return np.where(np.isnan(a), np.nan, a).astype(a.dtype).tobytes() if a.dtype.kind == "f" else a.tobytes()


@functools.lru_cache(maxsize=None)
def normals_of(n: int, seed: int = 5) -> np.ndarray:
    nrm = N.estimate(scan(n, seed), None, k=10)[0]
    nrm.setflags(write=False)
    return nrm


def as_bytes(result):
    return [np.int64(result["n_out"]).tobytes()] + [canonical(result[f]) for f in R.FIELDS]


def one_call(c, queries, radius, order, s):
    rc, m, pts, nrm, index = c.moving_least_squares_raw(queries, radius, order, s)
    assert rc == 0 and c.mls_stats() == 2
    rc, rec = c.mls_fetch_raw(len(index))
    assert rc == 0
    return {"n_out": m, "points": pts[:m], "normals": nrm[:m], "index": index[:m], **rec}


def projections(c, cloud):
    """Four calls over one search cloud, each with its fetch, as bytes."""
    c.search_set_input(cloud)
    out = []
    for queries, radius, order, s in CALLS:
        out += as_bytes(one_call(c, None if queries is None else scan(300, 9), radius, order, s))
    return out


@functools.lru_cache(maxsize=None)
def fresh_projections():
    cloud = scan(2000)
    with Context(0) as fresh:
        want = projections(fresh, cloud)
    restated = []
    for queries, radius, order, s in CALLS:
        restated += as_bytes(R.project(cloud, None if queries is None else scan(300, 9), radius, order, s))
    assert want == restated
    return want


def test_a_context_with_a_modelled_history_answers_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with MLS calls over other clouds between the steps: the walk's observations do not move (the model knows nothing of the call),
    and at the end the context answers as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                n = (1025, 700, 257)[k % 3]
                w.ctx.search_set_input(scan(n, 9 + k % 3))
                w.ctx.moving_least_squares(0.5 + 0.25 * (k % 5), k % 4, queries=None if k % 8 == 1 else scan(100, 4))
            w.step(op)
        assert w.n_obs > 10
        assert projections(w.ctx, scan(2000)) == fresh_projections()


def test_a_context_with_history_answers_as_a_new_one():
    want = fresh_projections()
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
        c.search_set_input(raw)                       # another, larger search cloud first: searches, normals, projections, keypoints, a clustering
        c.search_knn(scan(300, 9), 20)
        c.normal_estimation(None, k=20)
        c.moving_least_squares(0.4, 3)
        c.iss_keypoints(0.6, 0.4)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        assert projections(c, scan(2000)) == want
        c.statistical_outlier_removal(scan(2000), 8, 1.0)   # a filter, a clustering and a segmentation between two calls on the same cloud
        c.euclidean_cluster_extraction(0.5)
        c.sac_plane_segmentation(0.2, 50, 0.99, 3)
        assert as_bytes(one_call(c, *CALLS[0])) == want[:8]


def observations(c, src, tgt, raw, queries, normals):
    """An alignment per method, both filters, the voxel filter, searches, normal estimations, histograms, clusterings, a segmentation
    and the ISS keypoints: everything as bytes."""
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
    out += list(c.fpfh_estimation(normals, queries, radius=0.6, want_spfh=True))
    out += list(c.euclidean_cluster_extraction(0.5) + c.euclidean_cluster_extraction(0.25, 2, 50))
    rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*SAC)
    assert rc == 0
    out += [coeff, np.int64([n_inliers, iterations, found]), c.sac_extract(False)]
    iss = c.iss_keypoints(*ISS)
    out += [iss[f] for f in IR.FIELDS]
    return [np.asarray(a).tobytes() for a in out]


def test_everything_else_returns_the_same_bits_after_the_calls():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(2000), scan(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, queries, normals_of(2000))
        got = []
        for q, radius, order, s in CALLS:               # on the same search cloud
            got += as_bytes(one_call(c, None if q is None else scan(300, 9), radius, order, s))
        assert got == fresh_projections()
        second = observations(c, src, tgt, raw, queries, normals_of(2000))
    assert first == second


def test_unfetched_results_survive_the_call_and_its_own_survives_them():
    cloud, queries, normals = scan(2000), scan(300, 9), normals_of(2000)
    source = S.moved(cloud[::7], np.linalg.inv(S.rigid(0.5, 0.0, 0.02, (1.0, -2.0, 0.1))))
    tf = S.descriptors(2000, 3)
    want_clusters = CR.extract(cloud, 0.5, 2, 50)
    r = SR.segment(cloud, *SAC)
    want_iss = IR.keypoints(cloud, *ISS)
    want_mls = fresh_projections()[:8]
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, T, n_in, fit, conv, aligned = c.scp_align_raw(source, tf[::7], tf, **SCP)
        assert rc == 0
        f = c.scp_fetch()
        want_alignment = [np.asarray(a).tobytes() for a in [T, np.float64([n_in, fit, conv, f["best_t"]]), aligned] + [f[name] for name in SCP_NAMES]]
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert (rc, n_clusters, n_clustered) == (0, want_clusters[0].size - 1, want_clusters[1].size)
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*SAC)
        assert rc == 0 and found == 1
        rc, T, n_in, fit, conv, aligned = c.scp_align_raw(source, tf[::7], tf, **SCP)
        assert rc == 0
        rc, n_keypoints = c.iss_keypoints_raw(*ISS)
        assert (rc, n_keypoints) == (0, want_iss["n_keypoints"])
        for q, radius, order, s in CALLS[::-1]:           # the projections over all four unfetched results; the last call's record stays
            rc, m, pts, nrm, index = c.moving_least_squares_raw(None if q is None else queries, radius, order, s)
            assert rc == 0
        first = [np.int64(m).tobytes(), canonical(pts[:m]), canonical(nrm[:m]), canonical(index[:m])]
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and all(np.asarray(g).dtype == w.dtype and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(arrays, want_clusters))
        rc, f = c.sac_fetch_raw(n_inliers, iterations)
        assert rc == 0
        got = [coeff, np.int64([n_inliers, iterations, found, f["best_t"], f["n_unrefined"]])] + [f[name] for name in SAC_NAMES]
        got += [c.sac_extract(False), c.sac_extract(True)]
        want = [r["coeff"], np.int64([r["inliers"].size, r["iterations"], r["found"], r["best_t"], r["n_unrefined"]])] + [r[name] for name in SAC_NAMES]
        want += [SR.extract(cloud, r["inliers"], False), SR.extract(cloud, r["inliers"], True)]
        assert [np.asarray(a).tobytes() for a in got] == [np.ascontiguousarray(a).tobytes() for a in want]
        f = c.scp_fetch()
        got = [T, np.float64([n_in, fit, conv, f["best_t"]]), aligned] + [f[name] for name in SCP_NAMES]
        assert [np.asarray(a).tobytes() for a in got] == want_alignment
        rc, out = c.iss_fetch_raw(n_keypoints)
        assert rc == 0 and all(np.ascontiguousarray(out[name]).tobytes() == np.ascontiguousarray(want_iss[name]).tobytes() for name in IR.FIELDS)
        # the MLS record, unfetched so far, after searches, normals, histograms, a clustering, a segmentation, an alignment and keypoints
        c.search_knn(queries, 20)
        c.search_radius(queries, 1.0)
        c.normal_estimation(None, k=10)
        c.fpfh_estimation(normals, queries, radius=0.6)
        c.cluster_extract_raw(0.25, 2, 50)
        c.sac_segment_raw(0.1, 70, 0.99, 9, True, None, 0.0)
        c.scp_align_raw(source, tf[::7], tf, **{**SCP, "max_iterations": 33})
        c.iss_keypoints_raw(0.8, 1.6, 0.9, 0.6, 3)
        for _ in range(2):
            rc, rec = c.mls_fetch_raw(2000)
            assert rc == 0 and c.mls_stats() == 2
            assert first + [canonical(rec[name]) for name in ("status", "n_neighbours", "plane7", "coeff10")] == want_mls
        c.search_set_input(cloud)                           # the same cloud again: the record is dropped all the same
        assert c.mls_fetch_raw(2000)[0] == _lib.ERR_INVALID_ARG
        assert c._L.icpgpu_mls_stats(c._h, None) == _lib.ERR_INVALID_ARG
        assert c.moving_least_squares_raw(*CALLS[0])[:2] == (0, m)
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): whatever it returns
        assert rc == _lib.ERR_INVALID_ARG and c.mls_fetch_raw(2000)[0] == _lib.ERR_INVALID_ARG
