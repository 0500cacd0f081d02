"""The segment moments and the rest of a context: a context with any history answers icpgpu_segment_moments as a
new one does; the call changes nothing an alignment, a filter, a search, a normal estimation, a clustering, a region growing, a
segmentation, a ground filter, the ISS keypoints or a moving least squares projection reads; unfetched clustering, region, segmentation,
ground filter, ISS and moving least squares results survive it -- the very cluster or region result it reads included; and
icpgpu_search_set_input makes the device-resident sources refuse."""
import functools

import numpy as np
import pytest

import history_model as hm
import segment_restated as R
from icpslam_amd import Context, _lib, synth
from test_gpu_region_history import canonical, normals_of, observations, others, scan

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
COS30 = np.float32(np.cos(np.radians(30.0)))
CLUSTERING = (0.5, 2, 50)
GROWING = (12, COS30, 1e-4, 1, INT_MAX)


def host_segments(n: int):
    """Three segment lists over a cloud of n points: many short rows, one long row among short ones, overlapping unsorted rows."""
    rng = np.random.default_rng(n)
    return [R.csr([rng.integers(0, n, m).tolist() for m in lengths])
            for lengths in ([5] * 200, [3] * 20 + [n] + [3] * 20, rng.integers(0, 700, 30).tolist())]


def moments(c, cloud, normals):
    """Three HOST calls and both device-resident sources over one search cloud, as bytes."""
    c.search_set_input(cloud)
    out = [canonical(c.segment_moments(start, idx).view(np.uint8)) for start, idx in host_segments(len(cloud))]
    rc, n_clusters, _ = c.cluster_extract_raw(*CLUSTERING)
    rc2, n_regions, _ = c.region_growing_raw(normals, *GROWING)
    assert rc == rc2 == 0
    out.append(c.segment_moments(source="clusters", n_segments=n_clusters).tobytes())
    out.append(c.segment_moments(source="regions", n_segments=n_regions).tobytes())
    return out


@functools.lru_cache(maxsize=None)
def fresh_moments():
    cloud, normals = scan(2000), normals_of(2000)
    with Context(0) as fresh:
        want = moments(fresh, cloud, normals)
    for got, (start, idx) in zip(want, host_segments(len(cloud))):
        assert R.same_records(np.frombuffer(got, R.RECORD), R.records(cloud, start, idx)) == []
    return want


def test_a_context_with_a_modelled_history_answers_as_a_new_one():
    """tests/history_model.py walks a context through a scenario -- every observation of the walk is compared with a new context's --
    with segment moment calls over other clouds between the steps: the walk's observations do not move (the model knows nothing of
    the call), and at the end the context answers as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                n = (1025, 700, 257)[k % 3]
                w.ctx.search_set_input(scan(n, 9 + k % 3))
                for start, idx in host_segments(n)[: 1 + k % 3]:
                    w.ctx.segment_moments(start, idx)
                if k % 8 == 1:
                    rc, n_clusters, _ = w.ctx.cluster_extract_raw(0.4, 1, INT_MAX)
                    w.ctx.segment_moments(source="clusters", n_segments=n_clusters)
            w.step(op)
        assert w.n_obs > 10
        assert moments(w.ctx, scan(2000), normals_of(2000)) == fresh_moments()


def test_a_context_with_history_answers_as_a_new_one():
    want = fresh_moments()
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
        c.search_set_input(raw)                       # another, larger search cloud first: its scratch is larger than the next calls need
        c.search_knn(scan(300, 9), 20)
        normals, _ = c.normal_estimation(None, k=20)
        rc, n_regions, _ = c.region_growing_raw(normals, 40, COS30, 0.05, 1, INT_MAX)
        c.segment_moments(source="regions", n_segments=n_regions)
        start, idx = host_segments(len(raw))[1]
        c.segment_moments(start, idx)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        c.iss_keypoints(0.6, 0.4)
        assert moments(c, scan(2000), normals_of(2000)) == want
        c.statistical_outlier_removal(scan(2000), 8, 1.0)   # a filter and a segmentation between two calls on the same cloud
        c.sac_plane_segmentation(0.2, 50, 0.99, 3)
        start, idx = host_segments(2000)[0]
        assert canonical(c.segment_moments(start, idx).view(np.uint8)) == want[0]


def test_everything_else_returns_the_same_bits_after_the_calls():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(2000), scan(300, 9)
    with Context(0) as c:
        c.search_set_input(cloud)
        first = observations(c, src, tgt, raw, queries)
        for start, idx in host_segments(len(cloud)):            # on the same search cloud: the search state must stay as it is
            c.segment_moments(start, idx)
        second = observations(c, src, tgt, raw, queries)
        rc, n_clusters, _ = c.cluster_extract_raw(*CLUSTERING)
        c.segment_moments(source="clusters", n_segments=n_clusters)
        third = observations(c, src, tgt, raw, queries)
    assert first == second == third


def test_unfetched_results_survive_the_call():
    cloud, normals = scan(2000), normals_of(2000)
    as_bytes = lambda arrays: [canonical(a) for a in arrays]   # noqa: E731
    with Context(0) as c:
        c.search_set_input(cloud)
        want_clusters = as_bytes(c.euclidean_cluster_extraction(*CLUSTERING))
        want_regions = as_bytes(c.region_growing(normals, GROWING[0], smoothness_cos=GROWING[1], curvature_threshold=GROWING[2]))
        want_others = as_bytes(others(c, fetch_now=True))
        # six unfetched results, then the calls over them -- the cluster and the region result are read by two of the calls
        rc, n_clusters, n_clustered = c.cluster_extract_raw(*CLUSTERING)
        rc2, n_regions, n_in = c.region_growing_raw(normals, *GROWING)
        assert rc == rc2 == 0
        head, pending = others(c, fetch_now=False)
        for start, idx in host_segments(len(cloud)):
            c.segment_moments(start, idx)
        from_clusters = c.segment_moments(source="clusters", n_segments=n_clusters)
        from_regions = c.segment_moments(source="regions", n_segments=n_regions)
        rc, *arrays = c.cluster_fetch_raw(n_clusters, n_clustered)
        assert rc == 0 and as_bytes(arrays) == want_clusters
        rc, *regions = c.region_fetch_raw(n_regions, n_in)
        assert rc == 0 and as_bytes(regions) == want_regions
        assert as_bytes(head + others(c, fetch_now=False, pending=pending)) == want_others
        assert R.same_records(from_clusters, R.records(cloud, arrays[0], arrays[1])) == []
        assert R.same_records(from_regions, R.records(cloud, regions[0], regions[1])) == []


def test_search_set_input_makes_the_device_sources_refuse():
    cloud, normals = scan(1025), normals_of(1025)
    with Context(0) as c:
        c.search_set_input(cloud)
        rc, n_clusters, _ = c.cluster_extract_raw(*CLUSTERING)
        rc2, n_regions, _ = c.region_growing_raw(normals, *GROWING)
        assert rc == rc2 == 0
        assert c.segment_moments_raw(_lib.SEGMENTS_CLUSTERS, n_clusters)[0] == 0 and c.segment_moments_raw(_lib.SEGMENTS_REGIONS, n_regions)[0] == 0
        c.search_set_input(cloud)                     # the same cloud again: the results are gone all the same
        assert c.segment_moments_raw(_lib.SEGMENTS_CLUSTERS, n_clusters)[0] == _lib.ERR_INVALID_ARG
        assert c.segment_moments_raw(_lib.SEGMENTS_REGIONS, n_regions)[0] == _lib.ERR_INVALID_ARG
        start, idx = host_segments(len(cloud))[0]
        assert c.segment_moments_raw(_lib.SEGMENTS_HOST, len(start) - 1, start, idx)[0] == 0       # (the HOST source needs no result)
        rc = c._L.icpgpu_search_set_input(c._h, None, 5)   # a refused cloud (null pointer with n = 5): there is no search cloud any more
        assert rc == _lib.ERR_INVALID_ARG
        assert c.segment_moments_raw(_lib.SEGMENTS_HOST, len(start) - 1, start, idx)[0] == _lib.ERR_INVALID_ARG
