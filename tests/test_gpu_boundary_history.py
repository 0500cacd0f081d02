"""The boundary estimation, ISS border estimation and the rest of a context: a context with any history answers
icpgpu_boundary_estimation and icpgpu_iss_keypoints_border as a new one does; the calls change nothing an alignment, a filter, a
search, a normal estimation, a histogram, a clustering or a segmentation reads; unfetched clustering, segmentation, sample-consensus
and ISS results survive the boundary call, the border result survives it too, and icpgpu_search_set_input drops the border result.
The observations and their scenes are tests/test_gpu_iss_history.py's."""
import functools
import math

import numpy as np
import pytest

import boundary_restated as B
import cluster_restated as CR
import history_model as hm
import iss_border_restated as IB
import sac_restated as SR
import scp_scenes as S
import test_gpu_iss_history as H
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
BOUNDARY = ((30, 0.0, math.pi / 2), (0, 1.5, 2.5), (3, 0.0, math.pi))
BORDER = ((1.5, 1.0, 0.975, 0.975, 5, 1.0, math.pi, None, 1.5), (0.8, 1.6, 0.9, 0.6, 3, 0.7, 2.5, "given", 0.0))
scan, normals_of = H.scan, H.normals_of


def as_bytes(result, fields):
    return [np.ascontiguousarray(result[f]).tobytes() for f in fields]


def answers(c, cloud):
    """Every BOUNDARY and BORDER call over one search cloud, as bytes, with the border calls' waits."""
    normals = normals_of(len(cloud))
    c.search_set_input(cloud)
    out = []
    for k, radius, angle in BOUNDARY:
        out += as_bytes(c.boundary_estimation(normals, None, k, radius, angle), B.FIELDS)
    for *args, given, normal_radius in BORDER:
        got = c.iss_keypoints_border(*args, normals if given else None, normal_radius)
        out += [np.int64([got["n_keypoints"], c.iss_stats()]).tobytes()] + as_bytes(got, IB.FIELDS)
    return out


@functools.lru_cache(maxsize=None)
def fresh_answers():
    cloud, normals = scan(2000), normals_of(2000)
    with Context(0) as fresh:
        want = answers(fresh, cloud)
    restated = []
    for k, radius, angle in BOUNDARY:
        restated += as_bytes(B.estimate(cloud, None, normals, k, radius, angle), B.FIELDS)
    for *args, given, normal_radius in BORDER:
        r = IB.keypoints_border(cloud, *args, normals if given else None, normal_radius)
        restated += [np.int64([r["n_keypoints"], 2 if given else 3]).tobytes()] + as_bytes(r, IB.FIELDS)
    assert want == restated
    return want


def test_a_context_with_a_modelled_history_answers_as_a_new_one():
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                n = (1025, 700, 257)[k % 3]
                w.ctx.search_set_input(scan(n, 9 + k % 3))
                nrm, _ = w.ctx.normal_estimation(None, k=10)
                w.ctx.boundary_estimation(nrm, None, 0, 0.5 + 0.25 * (k % 5), 1.0 + 0.5 * (k % 4))
                w.ctx.iss_keypoints_border(0.5 + 0.25 * (k % 5), 0.4 + 0.3 * (k % 3), 0.975, 0.975, k % 7, 0.4 + 0.2 * (k % 3), 2.0, None, 0.8)
            w.step(op)
        assert w.n_obs > 10
        assert answers(w.ctx, scan(2000)) == fresh_answers()


def test_a_context_with_history_answers_as_a_new_one():
    want = fresh_answers()
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw = scan(20000, 6)
    with Context(0) as c:
        for method in (hm.P2P, hm.GICP, hm.P2PLANE, hm.NDT):
            c.set_params(method=method, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.voxel_grid(raw, 0.4)
        c.search_set_input(raw)                       # another, larger search cloud first
        nrm, _ = c.normal_estimation(None, k=20)
        c.boundary_estimation(nrm, None, 20)
        c.boundary_estimation(nrm[:300], raw[:300], 0, 0.4, 2.0)
        c.iss_keypoints_border(0.6, 0.4, 0.975, 0.975, 5, 0.3, 2.0, nrm)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        assert answers(c, scan(2000)) == want
        c.statistical_outlier_removal(scan(2000), 8, 1.0)
        c.fpfh_estimation(normals_of(2000), None, k=10)
        assert answers(c, scan(2000)) == want


def test_everything_else_returns_the_same_bits_after_the_calls():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(2000), scan(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = H.observations(c, src, tgt, raw, queries, normals_of(2000))
        plain = H.as_bytes(c.iss_keypoints(*H.CALLS[0]))
        assert answers(c, cloud) == fresh_answers()         # (on the same search cloud, set again)
        assert H.as_bytes(c.iss_keypoints(*H.CALLS[0])) == plain
        second = H.observations(c, src, tgt, raw, queries, normals_of(2000))
    assert first == second


def test_unfetched_results_survive_the_boundary_call_and_the_border_result_survives_the_rest():
    cloud, queries, normals = scan(2000), scan(300, 9), normals_of(2000)
    source = S.moved(cloud[::7], np.linalg.inv(S.rigid(0.5, 0.0, 0.02, (1.0, -2.0, 0.1))))
    tf = S.descriptors(2000, 3)
    want_clusters = CR.extract(cloud, 0.5, 2, 50)
    r = SR.segment(cloud, *H.SAC)
    args = BORDER[0][:7]
    want_border = IB.keypoints_border(cloud, *args, None, 1.5)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert (rc, n_clusters, n_clustered) == (0, want_clusters[0].size - 1, want_clusters[1].size)
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*H.SAC)
        assert rc == 0 and found == 1
        rc, T, n_in, fit, conv, aligned = c.scp_align_raw(source, tf[::7], tf, **H.SCP)
        assert rc == 0
        f = c.scp_fetch()
        want_alignment = [np.asarray(a).tobytes() for a in [T, np.float64([n_in, fit, conv, f["best_t"]]), aligned] + [f[name] for name in H.SCP_NAMES]]
        rc, m = c.iss_keypoints_border_raw(*args, None, 1.5)
        assert (rc, m) == (0, want_border["n_keypoints"])
        for k, radius, angle in BOUNDARY:                   # the boundary calls over all four unfetched results
            c.boundary_estimation(normals, None, k, radius, angle)
        c.boundary_estimation(normals[:300], queries, 0, 1.0, 2.0)
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and all(np.asarray(g).tobytes() == w.tobytes() for g, w in zip(arrays, want_clusters))
        rc, f = c.sac_fetch_raw(n_inliers, iterations)
        assert rc == 0 and np.asarray(f["inliers"]).tobytes() == np.ascontiguousarray(r["inliers"]).tobytes()
        f = c.scp_fetch()
        got = [T, np.float64([n_in, fit, conv, f["best_t"]]), aligned] + [f[name] for name in H.SCP_NAMES]
        assert [np.asarray(a).tobytes() for a in got] == want_alignment
        # the border result, unfetched so far, after searches, normals, histograms, a clustering, a segmentation and an alignment
        c.search_knn(queries, 20)
        c.search_radius(queries, 1.0)
        c.normal_estimation(None, radius=0.9)
        c.fpfh_estimation(normals, queries, radius=0.6)
        c.cluster_extract_raw(0.25, 2, 50)
        c.sac_segment_raw(0.1, 70, 0.99, 9, True, None, 0.0)
        c.scp_align_raw(source, tf[::7], tf, **{**H.SCP, "max_iterations": 33})
        for _ in range(2):
            rc, out = c.iss_fetch_raw(m)
            rc2, more = c.iss_fetch_border_raw()
            assert rc == 0 and rc2 == 0 and c.iss_stats() == 3
            assert IB.same_bits({**out, **more, "n_keypoints": m}, want_border) == []
        c.search_set_input(cloud)                           # the same cloud again: the result is dropped all the same
        assert c.iss_fetch_border_raw()[0] == _lib.ERR_INVALID_ARG and c.iss_fetch_raw(m)[0] == _lib.ERR_INVALID_ARG
        assert c.iss_keypoints_border_raw(*args, None, 1.5) == (0, m)
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): whatever it returns
        assert rc == _lib.ERR_INVALID_ARG and c.iss_fetch_border_raw()[0] == _lib.ERR_INVALID_ARG
