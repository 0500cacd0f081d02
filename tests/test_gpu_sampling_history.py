"""The cropping and sampling filters and the rest of a context: a context with any history answers
icpgpu_pass_through, icpgpu_crop_box, icpgpu_uniform_sampling, icpgpu_farthest_point_sampling and their observers as a new one does;
the calls change nothing an alignment, a filter, a search, a normal estimation, a clustering, a segmentation, a ground filter, the ISS
keypoints or a moving least squares projection reads; unfetched clustering, segmentation, ground filter, ISS, moving least squares and
outlier results survive them, and their own result survives all of those -- icpgpu_search_set_input included."""
import functools

import numpy as np
import pytest

import history_model as hm
import sampling_cases as SC
import sampling_restated as R
from icpslam_amd import Context, synth

pytestmark = pytest.mark.gpu
BOX = ((-8.0, -6.0, -2.0), (10.0, 6.0, 1.0))
T_POSE = R.crop_box_matrix(None, (0.4, -0.2, 0.1), (0.02, -0.03, 0.3))
SAC = (0.2, 50, 0.99, 3, True, None, 0.0)
ISS = (1.5, 1.0, 0.975, 0.975, 5)
PMF = (9, 0.7, 0.15, 10.0, 1.0, 2.0, True)


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = SC.with_bad_rows(SC.scan(n, seed), [3, n // 2, n - 1])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def plain(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def canonical(a):
    """An array's bytes with every NaN the same NaN (a computed NaN's sign and payload are the processor's)."""
    a = np.ascontiguousarray(a)
    return np.where(np.isnan(a), np.nan, a).astype(a.dtype).tobytes() if a.dtype.kind == "f" else a.tobytes()


def as_bytes(arrays):
    return [canonical(a) for a in arrays]


def fetched(c):
    f = c.subset_fetch()
    return [f["kept"], f["removed"], f["measure"], np.int64(f["n_in"])]


def the_five(c, cloud):
    """The five calls over one cloud, each with its fetch, as bytes."""
    out = []
    for call in (lambda: c.pass_through(cloud, 2, -1.2, 2.0, True), lambda: c.crop_box(cloud, *BOX, None, False),
                 lambda: c.crop_box(cloud, *BOX, T_POSE, True, view=True), lambda: c.uniform_sampling(cloud, 0.8),
                 lambda: c.farthest_point_sampling(cloud, 90, 17, view=True)):
        out += as_bytes([call()] + fetched(c))
    return out


@functools.lru_cache(maxsize=None)
def fresh_five():
    cloud = scan(2000)
    with Context(0) as fresh:
        want = the_five(fresh, cloud)
    restated = []
    for kept, measure in ((R.pass_through(cloud, 2, -1.2, 2.0, True), None), (R.crop_box(cloud, *BOX, None, False), None),
                          (R.crop_box(cloud, *BOX, T_POSE, True), None), R.uniform_sampling(cloud, 0.8), R.farthest_point_sampling(cloud, 90, 17)):
        measure = np.zeros(len(kept), np.float32) if measure is None else measure
        restated += as_bytes([cloud[kept], kept, R.removed_of(len(cloud), kept), measure, np.int64(len(cloud))])
    assert want == restated
    return want


def test_a_context_with_a_modelled_history_filters_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with filter calls over other clouds between the steps: the walk's observations do not move (the model knows nothing of the
    calls), and at the end the context answers as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                other = scan((1025, 700, 257)[k % 3], 9 + k % 3)
                (w.ctx.pass_through, w.ctx.uniform_sampling, w.ctx.farthest_point_sampling)[k % 3](other, *((2, -1.0, 1.0), (0.3 + 0.1 * k,), (40 + k,))[k % 3])
                if k % 8 == 1:
                    w.ctx.crop_box(other, *BOX, T_POSE, True)
                    w.ctx.subset_fetch()
            w.step(op)
        assert w.n_obs > 10
        assert the_five(w.ctx, scan(2000)) == fresh_five()


def observations(c, src, tgt, raw, queries):
    """An alignment per method, both outlier filters, the voxel filter, searches, normal estimations, clusterings, a segmentation, the
    ground filter, the ISS keypoints and a projection: everything as bytes."""
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
    out += others(c, fetch_now=True)
    return [canonical(a) for a in out]


def others(c, fetch_now: bool, pending=None):
    """The four other kept results over the search cloud.  fetch_now: each computed and fetched at once, as arrays.  Otherwise
    pending = None computes them all and returns what their fetches need; given that, fetches them all."""
    out = []
    if pending is None:
        rc, coeff, n_inliers, iterations, found = c.sac_segment_raw(*SAC)
        rc2, n_ground, n_passes = c.pmf_filter_raw(*PMF)
        rc3, n_keypoints = c.iss_keypoints_raw(*ISS)
        rc4, m, pts, nrm, index = c.moving_least_squares_raw(None, 1.5, 2, 0.0)
        assert (rc, rc2, rc3, rc4) == (0, 0, 0, 0)
        pending = (n_inliers, iterations, n_ground, n_passes, n_keypoints, len(index))
        out = [coeff, np.int64(pending), pts[:m], nrm[:m], index[:m]]
        if not fetch_now:
            return out, pending
    n_inliers, iterations, n_ground, n_passes, n_keypoints, n_q = pending
    rc, sac = c.sac_fetch_raw(n_inliers, iterations)
    rc2, pmf = c.pmf_fetch_raw(n_ground, n_passes)
    rc3, iss = c.iss_fetch_raw(n_keypoints)
    rc4, mls = c.mls_fetch_raw(n_q)
    assert (rc, rc2, rc3, rc4) == (0, 0, 0, 0)
    for d in (sac, pmf, iss, mls):
        out += [np.asarray(d[name]) for name in sorted(d)]
    return out


def test_everything_else_returns_the_same_bits_after_the_calls():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = plain(20000, 6), plain(2000), plain(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, queries)
        assert the_five(c, scan(2000)) == fresh_five()
        second = observations(c, src, tgt, raw, queries)
        c.uniform_sampling(raw, 0.5)                                  # ... and with a result left unfetched, over the outlier filters' cloud
        third = observations(c, src, tgt, raw, queries)
    assert first == second == third


def test_unfetched_results_survive_the_calls_and_their_own_survives_them():
    search_cloud, cloud, queries = plain(2000), scan(2000), plain(300, 9)
    want = fresh_five()
    with Context(0) as c:
        c.search_set_input(search_cloud)
        want_clusters = as_bytes(c.euclidean_cluster_extraction(0.5, 2, 50))
        want_others = as_bytes(others(c, fetch_now=True))
        c.statistical_outlier_removal(search_cloud, 8, 1.0)
        want_outlier = as_bytes([c.outlier_fetch()[k] for k in ("measure", "kept", "removed")])
        # six unfetched results, then the five calls over them
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert rc == 0
        head, pending = others(c, fetch_now=False)
        c.statistical_outlier_removal(search_cloud, 8, 1.0)
        assert the_five(c, cloud) == want
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and as_bytes(arrays) == want_clusters
        assert as_bytes(head + others(c, fetch_now=False, pending=pending)) == want_others
        assert as_bytes([c.outlier_fetch()[k] for k in ("measure", "kept", "removed")]) == want_outlier
        # the last call's result, fetched only now, after searches, normals, a clustering, a segmentation, a ground filter, keypoints, a
        # projection, both outlier filters, the voxel filter, an alignment and a new search cloud
        src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
        c.search_knn(None, 64)
        c.search_radius(None, 2.0)
        c.normal_estimation(queries, radius=0.8)
        c.cluster_extract_raw(0.25, 2, 50)
        c.sac_segment_raw(0.1, 70, 0.99, 9, True, None, 0.0)
        c.pmf_filter_raw(17, 1.0, 0.3, 3.0, 1.0, 2.0, True)
        c.iss_keypoints_raw(0.8, 1.6, 0.9, 0.6, 3)
        c.moving_least_squares_raw(queries, 1.0, 3, 0.0)
        c.statistical_outlier_removal(search_cloud, 8, 1.0)
        c.radius_outlier_removal(search_cloud, 0.3, 5)
        c.voxel_grid(search_cloud, 0.4)
        c.set_source(src)
        c.set_target(tgt)
        c.align(want_cloud=True, want_fitness=True)
        c.search_set_input(queries)
        for _ in range(2):
            assert as_bytes(fetched(c)) == want[-4:]
