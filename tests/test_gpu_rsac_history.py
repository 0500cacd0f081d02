"""The sample-consensus rejector and the rest of a context, for the stage and for the call of its own: a
context with any history answers as a new one does; the stage and the call change nothing an alignment, a filter, a search, a normal
estimation or a clustering returns; unfetched clustering, segmentation, ISS and ground-filter results survive them and their own
result survives those calls -- and icpgpu_search_set_input, since it reads no search cloud."""
import functools

import numpy as np
import pytest

import history_model as hm
import rsac_restated as R
import rsac_scenes as S
from icpslam_amd import Context, synth

pytestmark = pytest.mark.gpu
NAMES = ("moments9", "counts", "ranks", "transforms", "best_T")
SCALARS = ("m", "sample_d2", "iterations", "status", "best_t", "n_kept", "host_waits")
CALLS = (("m513", None), ("runs_to_200", None), ("nan_rows", None))
STAGE = (R.KIND, *S.BLOCK_STAGE)


@functools.lru_cache(maxsize=None)
def scan(n: int, seed: int = 5) -> np.ndarray:
    c = synth.scan(synth.make_scene(3), np.eye(4), n, seed)
    c.setflags(write=False)
    return c


def fetched(c):
    f = c.rejector_sac_fetch()
    return [np.asarray(f[k]).tobytes() for k in NAMES] + [np.float64([f[k] for k in SCALARS]).tobytes()]


def one_call(c, name):
    P, Q, thr, it, seed = S.core_cases()[name]
    r = c.reject_sample_consensus(P, Q, np.arange(len(P)), np.arange(len(P)), thr, it, seed)
    return [r["kept"].tobytes(), r["best_T"].tobytes(), np.int64(r["n_kept"]).tobytes()] + fetched(c)


def one_stage(c):
    src, tgt, _, _ = S.moved_block()
    c.set_params(method=hm.P2P, max_correspondence_distance=1.0, max_iterations=3)
    c.set_source(src)
    c.set_target(tgt)
    c.set_correspondence_rejectors([STAGE])
    idx, d2 = c.correspondences(np.eye(4))
    out = [idx.tobytes(), d2.tobytes()] + fetched(c)
    r = c.align()
    out += [r["T"].tobytes(), np.int64([r["iterations"], r["n_corr"]]).tobytes()] + fetched(c)
    c.set_correspondence_rejectors([])
    return out


def everything(c):
    return [one_call(c, name) for name, _ in CALLS] + [one_stage(c)]


@functools.lru_cache(maxsize=None)
def fresh():
    with Context(0) as c:
        return everything(c)


def test_a_context_with_a_modelled_history_answers_as_a_new_one():
    """tests/history_model.py walks a context through a scenario with calls of the rejector between the steps: the walk's
    observations do not move (the model knows nothing of the rejector), and at the end the context answers as a new one does."""
    ops = hm.scenario_p2plane_promote_recognition()
    P, Q = S.pairs(300, 0.5, 12)
    with hm.Walk(hm.GpuBackend()) as w:
        for k, op in enumerate(ops):
            if k % 4 == 1:
                w.ctx.reject_sample_consensus(P, Q, np.arange(300), np.arange(300), 0.05 + 0.05 * (k % 3), 40 + 40 * (k % 2), k, want_flags=k % 8 == 1)
            w.step(op)
        assert w.n_obs > 10
        assert everything(w.ctx) == fresh()


def observations(c, src, tgt, raw, cloud, queries):
    """An alignment per method, both filters, the voxel filter, searches, normal estimations and clusterings: everything as bytes."""
    out = []
    c.search_set_input(cloud)
    for method in (hm.P2P, hm.GICP, hm.P2PLANE, hm.NDT):
        c.set_params(method=method, max_iterations=6, max_correspondence_distance=1.0)
        c.set_source(src)
        c.set_target(tgt)
        r = c.align(want_cloud=True, want_fitness=True)
        out += [r["T"], r["cloud"]] + [np.float64(r[k]) for k in ("iterations", "n_corr", "converged", "fitness", "mse")]
    out += [c.statistical_outlier_removal(raw, 19, 1.0), c.outlier_fetch()["measure"], c.radius_outlier_removal(raw, 0.3, 5), c.voxel_grid(raw, 0.4)]
    out += list(c.search_knn(None, 20) + c.search_radius(queries, 3.0, 70))
    out += list(c.normal_estimation(None, k=20, want_moments=True))
    out += list(c.euclidean_cluster_extraction(0.5))
    return [np.asarray(a).tobytes() for a in out]


def test_everything_else_returns_the_same_bits_after_the_rejector():
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw, cloud, queries = scan(20000, 6), scan(3000), scan(300, 9)
    with Context(0) as c:
        first = observations(c, src, tgt, raw, cloud, queries)
        assert everything(c) == fresh()
        second = observations(c, src, tgt, raw, cloud, queries)
        P, Q, thr, it, seed = S.core_cases()["m3000"]
        c.reject_sample_consensus(P, Q, np.arange(3000), np.arange(3000), thr, it, seed, want_flags=False)     # ... left unfetched
        third = observations(c, src, tgt, raw, cloud, queries)
    assert first == second == third


def bits(d):
    return {k: np.asarray(v).tobytes() for k, v in d.items()}


def leave_four_results(c):
    """A clustering, a segmentation, ISS keypoints and a ground filter, none fetched: what the calls return."""
    return [c.cluster_extract_raw(0.5, 2, 50), c.sac_segment_raw(0.2, 50, 0.99, 3), c.iss_keypoints_raw(1.0, 0.7), c.pmf_filter_raw()]


def fetch_four(c, left):
    (_, n_clusters, n_clustered), (_, _, n_inliers, iterations, _), (_, n_keypoints), (_, n_ground, n_passes) = left
    rc, *clusters = c.cluster_fetch_raw(n_clusters, n_clustered)
    out = [rc] + [np.asarray(a).tobytes() for a in clusters]
    for rc, d in (c.sac_fetch_raw(n_inliers, iterations), c.iss_fetch_raw(n_keypoints), c.pmf_fetch_raw(n_ground, n_passes)):
        out += [rc, bits(d)]
    return out


def test_unfetched_results_survive_each_other():
    cloud = scan(3000)
    P, Q, thr, it, seed = S.core_cases()["m513"]
    with Context(0) as c, Context(0) as ref:
        for x in (c, ref):
            x.search_set_input(cloud)
        left, left_ref = leave_four_results(c), leave_four_results(ref)
        assert repr(left) == repr(left_ref) and all(r[0] == 0 for r in left)
        mine = one_call(c, "m513")                                    # the call and the stage over the four unfetched results
        stage = one_stage(c)
        assert fetch_four(c, left) == fetch_four(ref, left_ref)
        assert mine == fresh()[0] and stage == fresh()[-1]
        # ... and its own result survives those calls, and a new search cloud
        c.reject_sample_consensus(P, Q, np.arange(513), np.arange(513), thr, it, seed)
        before = fetched(c)
        leave_four_results(c)
        c.search_set_input(scan(1025))
        c.search_knn(None, 8)
        c.normal_estimation(None, k=10)
        assert fetched(c) == before == mine[3:]
