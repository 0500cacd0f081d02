"""The segmentation from normals and the rest of a context: a context with any history segments as a new one
does; the call (and an extract over it) changes nothing an alignment, a filter, a search, a normal estimation or a clustering reads;
unfetched clustering, region growing, ground filter, ISS and moving least squares results survive it and its own unfetched result
survives them; icpgpu_search_set_input drops the result; a plane segmentation replaces it, and the other way round."""
import functools

import numpy as np
import pytest

import history_model as hm
import sac_normals_cases as CS
import sac_normals_restated as R
import sac_restated as SR
from icpslam_amd import Context, _lib, synth

pytestmark = pytest.mark.gpu
PLANE, CYL = R.NORMAL_PLANE, R.CYLINDER
# model, threshold, weight, radius limits, max_iterations, probability, seed, optimize, axis, eps_angle
CALLS = ((PLANE, 0.08, 0.1, 0.0, 0.0, 100, 0.99, 1, True, None, 0.0), (CYL, 0.03, 0.1, 0.05, 0.3, 300, 0.99, 4, True, (0, 0, 1), 0.1),
         (CYL, 0.05, 0.3, 0.0, 0.0, 70, 0.9, 9, False, None, 0.0))
NAMES = ("counts", "sample", "coeff_unrefined", "moments", "cylinder_sums", "inliers")


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def fetched(c, head, n_inliers, iterations):
    rc, f = c.sac_normals_fetch_raw(n_inliers, iterations)
    assert rc == 0
    out = list(head) + [np.int64([f["best_t"], f["n_unrefined"], f["cylinder_passes"], f["cylinder_stop"]])] + [f[name] for name in NAMES]
    out += [c.sac_extract(False), c.sac_extract(True, view=True)]
    return [np.asarray(a).tobytes() for a in out]


def segmentation(c, normals, args):
    """Everything one call and its fetch and extracts hand out, as bytes."""
    rc, coeff, n_coeff, n_inliers, iterations, found = c.sac_segmentation_from_normals_raw(args[0], normals, *args[1:])
    assert rc == 0
    return fetched(c, [coeff, np.int64([n_coeff, n_inliers, iterations, found])], n_inliers, iterations)


def segmentations(c):
    cloud, normals = CS.street(1)
    c.search_set_input(cloud)
    return [segmentation(c, normals, args) for args in CALLS]


@functools.lru_cache(maxsize=None)
def fresh_segmentations():
    with Context(0) as fresh:
        want = segmentations(fresh)
    cloud, normals = CS.street(1)
    for args, got in zip(CALLS, want):                                    # (anchored: the unrefined stages are the restatement's)
        r = R.segment(args[0], cloud, normals, *args[1:])
        assert r["found"] == 1 and got[3] == r["counts"].tobytes() and got[4] == r["sample"].tobytes()
    return want


def test_a_context_with_a_modelled_history_segments_as_a_new_one():
    """tests/history_model.py walks a context through a scenario with segmentations from normals and extracts over other clouds
    between the steps: the walk's observations do not move, and at the end the context segments as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    cloud, normals, _ = CS.pole_and_pipe()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                w.ctx.search_set_input(cloud)
                w.ctx.sac_segmentation_from_normals_raw(CYL if k % 8 == 1 else PLANE, normals, 0.02 + 0.01 * (k % 3), 0.1, 0.0, 0.0, 50 + 40 * (k % 2),
                                                        0.99, k)
                if k % 8 == 1:
                    w.ctx.sac_extract(True, view=True)
            w.step(op)
        assert w.n_obs > 10
        assert segmentations(w.ctx) == fresh_segmentations()


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
        c.voxel_grid(raw, 0.4)
        c.search_set_input(raw)                       # another, larger search cloud first
        normals = c.normal_estimation(None, k=20)[0]
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        c.sac_segmentation_from_normals(CYL, normals, 0.1, 0.1, 0.0, 0.0, 100, 0.99, 2)
        c.sac_extract(True)
        assert segmentations(c) == want


def observations(c, src, tgt, raw, queries):
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
    raw, queries = scan(20000, 6), scan(300, 9)
    cloud, normals = CS.street(1)
    want = fresh_segmentations()
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, queries)
        for args, w in zip(CALLS, want):                                  # on the same search cloud: the search state must stay as it is
            assert segmentation(c, normals, args) == w
        second = observations(c, src, tgt, raw, queries)
        c.sac_segmentation_from_normals_raw(CYL, normals, 0.05, 0.2, 0.0, 0.0, 200, 0.999, 8)   # ... and with a result left unfetched
        third = observations(c, src, tgt, raw, queries)
    assert first == second == third


def others(c, cloud, normals):
    """Five results left unfetched in the context and, for each, the function that fetches it as bytes."""
    rc, n_clusters, n_clustered = c.cluster_extract_raw(0.5, 2, 500)
    assert rc == 0
    rc, n_regions, n_in = c.region_growing_raw(normals, 12, 0.95, 0.1, 5, 2**31 - 1)
    assert rc == 0
    rc, n_ground, n_passes = c.pmf_filter_raw(9, 0.7, 0.15, 3.0, 1.0, 2.0, True)
    assert rc == 0
    rc, n_key = c.iss_keypoints_raw(0.6, 0.4)
    assert rc == 0
    mls = c.moving_least_squares_raw(None, 0.5, 2)
    assert mls[0] == 0

    def fetch():
        out = []
        for rc, *arrays in (c.cluster_fetch_raw(n_clusters, n_clustered), c.region_fetch_raw(n_regions, n_in)):
            assert rc == 0
            out += arrays
        for rc, d in (c.pmf_fetch_raw(n_ground, n_passes), c.iss_fetch_raw(n_key), c.mls_fetch_raw(len(cloud))):
            assert rc == 0
            out += [d[k] for k in sorted(d)]
        return [np.asarray(a).tobytes() for a in out]
    return fetch


def test_unfetched_results_survive_each_other():
    cloud, normals = CS.street(1)
    want = fresh_segmentations()
    with Context(0) as ref:
        ref.search_set_input(cloud)
        want_others = others(ref, cloud, normals)()
    with Context(0) as c:
        c.search_set_input(cloud)
        fetch = others(c, cloud, normals)
        for args in CALLS[:2]:                                            # segmentations from normals over the five unfetched results
            rc, coeff, n_coeff, n_inliers, iterations, found = c.sac_segmentation_from_normals_raw(args[0], normals, *args[1:])
            assert rc == 0 and found == 1
            c.sac_extract(True, view=True)
        assert fetch() == want_others
        others(c, cloud, normals)                                         # ... and the five again over the unfetched segmentation
        c.search_knn(None, 20)
        c.normal_estimation(None, k=12)
        c.statistical_outlier_removal(cloud, 8, 1.0)
        assert fetched(c, [coeff, np.int64([n_coeff, n_inliers, iterations, found])], n_inliers, iterations) == want[1]


def test_search_set_input_drops_the_result_and_the_two_segmentations_replace_each_other():
    cloud, normals = CS.street(1)
    with Context(0) as c:
        c.search_set_input(cloud)
        args = CALLS[0]
        rc, coeff, n_coeff, n_inliers, iterations, found = c.sac_segmentation_from_normals_raw(args[0], normals, *args[1:])
        assert rc == 0 and found == 1 and c.sac_normals_fetch_raw(n_inliers, iterations)[0] == 0
        c.search_set_input(cloud)                     # the same cloud again: the result is gone all the same
        assert c.sac_normals_fetch_raw(n_inliers, iterations)[0] == _lib.ERR_INVALID_ARG
        with pytest.raises(_lib.IcpGpuError):
            c.sac_extract(False)
        with pytest.raises(_lib.IcpGpuError):
            c.sac_normals_host_waits()
        again = c.sac_segmentation_from_normals_raw(args[0], normals, *args[1:])
        assert again[0] == 0 and again[2:] == (n_coeff, n_inliers, iterations, found) and again[1].tobytes() == coeff.tobytes()
        # a plane segmentation replaces it ...
        plane = SR.segment(cloud, 0.08, 100, 0.99, 1, True)
        rc, pc, pn, pit, pfound = c.sac_segment_raw(0.08, 100, 0.99, 1, True)
        assert rc == 0 and c.sac_normals_fetch_raw(n_inliers, iterations)[0] == _lib.ERR_INVALID_ARG
        rc, f = c.sac_fetch_raw(pn, pit)
        assert rc == 0 and f["inliers"].tobytes() == plane["inliers"].tobytes() and pc.tobytes() == plane["coeff"].tobytes()
        assert c.sac_extract(True).tobytes() == SR.extract(cloud, plane["inliers"], True).tobytes()
        # ... and the other way round
        again = c.sac_segmentation_from_normals_raw(args[0], normals, *args[1:])
        assert again[0] == 0 and c.sac_fetch_raw(pn, pit)[0] == _lib.ERR_INVALID_ARG
        rc, f = c.sac_normals_fetch_raw(n_inliers, iterations)
        assert rc == 0 and c.sac_extract(False).tobytes() == cloud[f["inliers"]].tobytes()
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): whatever it returns
        assert rc == _lib.ERR_INVALID_ARG
        assert c.sac_normals_fetch_raw(n_inliers, iterations)[0] == _lib.ERR_INVALID_ARG
        assert c.sac_segmentation_from_normals_raw(args[0], normals, *args[1:])[0] == _lib.ERR_INVALID_ARG
