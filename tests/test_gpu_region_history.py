"""Region growing and the rest of a context: a context with any history answers icpgpu_region_growing and
icpgpu_region_fetch as a new one does; the calls change nothing an alignment, a filter, a search, a normal estimation, a clustering,
a segmentation, a ground filter, the ISS keypoints or a moving least squares projection reads; unfetched clustering, segmentation,
ground filter, ISS and moving least squares results survive them and their own result survives those; icpgpu_search_set_input drops
it."""
import functools

import numpy as np
import pytest

import history_model as hm
import normals_restated as N
import region_cases as RC
import region_restated as R
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
COS30 = RC.cos_of(30)
CALLS = ((12, COS30, 1e-4, 1, INT_MAX), (30, RC.cos_of(10), 1e-5, 2, 50), (5, COS30, float("inf"), 5, 5))  # (k, cos, threshold, lo, hi)
SAC = (0.2, 50, 0.99, 3, True, None, 0.0)
ISS = (1.5, 1.0, 0.975, 0.975, 5)
PMF = (9, 0.7, 0.15, 10.0, 1.0, 2.0, True)


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def normals_of(n: int, seed: int = 5) -> np.ndarray:
    nrm = N.estimate(scan(n, seed), None, k=12)[0]
    nrm.setflags(write=False)
    return nrm


def canonical(a):
    """An array's bytes with every NaN the same NaN (a computed NaN's sign and payload are the processor's)."""
    a = np.ascontiguousarray(a)
    return np.where(np.isnan(a), np.nan, a).astype(a.dtype).tobytes() if a.dtype.kind == "f" else a.tobytes()


def as_bytes(arrays):
    return [canonical(a) for a in arrays]


def growings(c, cloud, normals):
    """Three calls over one search cloud, each with its fetch, as bytes."""
    c.search_set_input(cloud)
    out = []
    for k, cos, threshold, lo, hi in CALLS:
        out += as_bytes(c.region_growing(normals, k, smoothness_cos=cos, curvature_threshold=threshold, min_size=lo, max_size=hi))
    return out


@functools.lru_cache(maxsize=None)
def fresh_growings():
    cloud, normals = scan(2000), normals_of(2000)
    with Context(0) as fresh:
        want = growings(fresh, cloud, normals)
    restated = []
    for k, cos, threshold, lo, hi in CALLS:
        restated += as_bytes(R.grow(cloud, normals, k, cos, threshold, lo, hi))
    assert want == restated
    return want


def test_a_context_with_a_modelled_history_grows_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with region growing calls over other clouds between the steps: the walk's observations do not move (the model knows nothing of
    the call), and at the end the context answers as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                n = (1025, 700, 257)[k % 3]
                w.ctx.search_set_input(scan(n, 9 + k % 3))
                w.ctx.region_growing(normals_of(n, 9 + k % 3), 5 + 9 * (k % 5), curvature_threshold=1e-4 * (1 + k % 2))
                if k % 8 == 1:
                    w.ctx.region_growing_raw(normals_of(n, 9 + k % 3), 30, COS30, 0.05, 1, INT_MAX)   # (unfetched results are left lying, too)
            w.step(op)
        assert w.n_obs > 10
        assert growings(w.ctx, scan(2000), normals_of(2000)) == fresh_growings()


def test_a_context_with_history_grows_as_a_new_one():
    want = fresh_growings()
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
        c.search_set_input(raw)                       # another, larger search cloud first: searches, normals, a growing, a clustering, ...
        c.search_knn(scan(300, 9), 20)
        normals, _ = c.normal_estimation(None, k=20)
        c.region_growing(normals, 40)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        c.iss_keypoints(0.6, 0.4)
        assert growings(c, scan(2000), normals_of(2000)) == want
        c.statistical_outlier_removal(scan(2000), 8, 1.0)   # a filter, a clustering and a segmentation between two calls on the same cloud
        c.euclidean_cluster_extraction(0.5)
        c.sac_plane_segmentation(0.2, 50, 0.99, 3)
        k, cos, threshold, lo, hi = CALLS[0]
        assert as_bytes(c.region_growing(normals_of(2000), k, smoothness_cos=cos, curvature_threshold=threshold, min_size=lo, max_size=hi)) == want[:6]


def observations(c, src, tgt, raw, queries):
    """An alignment per method, both filters, the voxel filter, searches, normal estimations, clusterings, a segmentation, the ground
    filter, the ISS keypoints and a projection: everything as bytes."""
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
    raw, cloud, queries = scan(20000, 6), scan(2000), scan(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, queries)
        got = []
        for k, cos, threshold, lo, hi in CALLS:                 # on the same search cloud: the search state must stay as it is
            got += as_bytes(c.region_growing(normals_of(2000), k, smoothness_cos=cos, curvature_threshold=threshold, min_size=lo, max_size=hi))
        assert got == fresh_growings()
        second = observations(c, src, tgt, raw, queries)
        c.region_growing_raw(normals_of(2000), 30, COS30, 0.05, 1, INT_MAX)   # ... and with a result left unfetched
        third = observations(c, src, tgt, raw, queries)
    assert first == second == third


def test_unfetched_results_survive_the_call_and_its_own_survives_them():
    cloud, queries, normals = scan(2000), scan(300, 9), normals_of(2000)
    want = fresh_growings()
    with Context(0) as c:
        c.search_set_input(cloud)
        want_clusters = as_bytes(c.euclidean_cluster_extraction(0.5, 2, 50))
        want_others = as_bytes(others(c, fetch_now=True))
        # five unfetched results, then the growings over them
        rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 50)
        assert rc == 0
        head, pending = others(c, fetch_now=False)
        for k, cos, threshold, lo, hi in CALLS[::-1]:            # (the last call's result stays)
            rc, n_regions, n_in = c.region_growing_raw(normals, k, cos, threshold, lo, hi)
            assert rc == 0
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and as_bytes(arrays) == want_clusters
        assert as_bytes(head + others(c, fetch_now=False, pending=pending)) == want_others
        # the region result, unfetched so far, after searches, normals, a clustering, a segmentation, a ground filter, keypoints, a projection
        c.search_knn(None, 64)
        c.search_knn(queries, 20)
        c.search_radius(None, 2.0)                               # (rows far longer than the result's arrays: the search scratch grows)
        c.normal_estimation(None, k=20, want_moments=True)
        c.normal_estimation(queries, radius=0.8)
        c.cluster_extract_raw(0.25, 2, 50)
        c.sac_segment_raw(0.1, 70, 0.99, 9, True, None, 0.0)
        c.pmf_filter_raw(17, 1.0, 0.3, 3.0, 1.0, 2.0, True)
        c.iss_keypoints_raw(0.8, 1.6, 0.9, 0.6, 3)
        c.moving_least_squares_raw(queries, 1.0, 3, 0.0)
        c.statistical_outlier_removal(cloud, 8, 1.0)
        for _ in range(2):
            rc, *arrays = c.region_fetch_raw(n_regions, n_in)
            assert rc == 0 and as_bytes(arrays) == want[:6]


def test_search_set_input_drops_the_result():
    cloud, normals = scan(1025), normals_of(1025)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_regions, n_in = c.region_growing_raw(normals, 12, COS30, 1e-4, 1, INT_MAX)
        assert rc == 0 and c.region_fetch_raw(n_regions, n_in)[0] == 0
        c.search_set_input(cloud)                     # the same cloud again: the result is gone all the same
        assert c.region_fetch_raw(n_regions, n_in)[0] == _lib.ERR_INVALID_ARG
        assert c.region_growing_raw(normals, 12, COS30, 1e-4, 1, INT_MAX) == (0, n_regions, n_in)
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): whatever it returns
        assert rc == _lib.ERR_INVALID_ARG
        assert c.region_fetch_raw(n_regions, n_in)[0] == _lib.ERR_INVALID_ARG
        assert c.region_growing_raw(normals, 12, COS30, 1e-4, 1, INT_MAX)[0] == _lib.ERR_INVALID_ARG   # (and there is no search cloud any more)
