"""The symmetric objective, the caller's source normals and the rest of a context: a context that has done
other things answers a symmetric alignment as a new one does; supplied source normals belong to the cloud they came with -- every
call that replaces the source drops them, icpgpu_promote_source_to_target moves them to the target."""
import numpy as np
import pytest

from icpslam_amd import GICP, NDT, P2PLANE, P2P_SVD, Context, synth

pytestmark = pytest.mark.gpu
F = np.float32
N = 4                                                                  # ICPGPU_REJECT_SURFACE_NORMAL


def bits(a):
    return np.asarray(a).tobytes()


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 4)).astype(F)
    v[:, :3] /= np.linalg.norm(v[:, :3], axis=1, keepdims=True)
    return v


def symmetric_align(c, src, tgt, sn=None):
    c.set_params(method=P2PLANE, max_iterations=10)
    c.set_source(src)
    c.set_target(tgt)
    if sn is not None:
        c.set_source_normals(sn)
    c.set_p2plane_symmetric(True)
    c.set_correspondence_rejectors([(N, 0.5)])
    out = c.align(want_cloud=True, want_fitness=True)
    return out, c.rejector_stats(), c.normals(of_target=False), c.normals(of_target=True)


@pytest.mark.parametrize("supplied", [False, True])
def test_a_context_with_history_answers_as_a_new_one(supplied):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=61)
    other_src, other_tgt, _ = synth.make_pair(2500, 2700, seed=5)
    raw = synth.scan(synth.make_scene(3), np.eye(4), 20000, 6)
    sn = unit_normals(src.shape[0], 3) if supplied else None
    with Context(0) as fresh:
        want = symmetric_align(fresh, src, tgt, sn)
    with Context(0) as c:
        c.search_set_input(raw)                                       # searches
        c.search_knn(other_src, 8)
        c.search_radius(other_src[:200], 0.5)
        c.voxel_grid(raw, 0.2)                                        # filters
        c.statistical_outlier_removal(raw, 20, 1.0)
        for method in (NDT, P2PLANE, GICP, P2P_SVD):                  # other methods, plain P2PLANE among them
            c.set_params(method=method, max_iterations=5)
            c.set_source(other_src)
            c.set_target(other_tgt)
            c.align()
        c.set_source_normals(unit_normals(other_src.shape[0], 4))     # another cloud's normals, an earlier symmetric run, a chain
        c.set_p2plane_symmetric(True, False)
        c.set_params(method=P2PLANE)
        c.set_correspondence_rejectors([(N, 0.0), (3,)])
        c.set_reciprocal_correspondences(True)
        c.align()
        c.set_reciprocal_correspondences(False)
        got = symmetric_align(c, src, tgt, sn)
        again = symmetric_align(c, src, tgt, sn)
    for other in (got, again):
        for k in ("T", "cloud"):
            assert bits(other[0][k]) == bits(want[0][k]), k
        for k in ("iterations", "n_corr", "converged", "state", "fitness", "mse"):
            assert bits(np.float64(other[0][k])) == bits(np.float64(want[0][k])), k
        assert other[1] == want[1]
        assert bits(other[2]) == bits(want[2]) and bits(other[3]) == bits(want[3])
    assert want[0]["iterations"] > 2 and 0 < want[1][0]["pairs_out"] < want[1][0]["pairs_in"]


def test_source_replacing_calls_drop_the_supplied_normals():
    import torch
    raw = synth.scan(synth.make_scene(3), np.eye(4), 20000, 6)
    with Context(0) as c, Context(0) as fresh:
        filtered = c.voxel_grid(raw, 0.5).copy()
        n = filtered.shape[0]
        assert n >= 100
        sup = unit_normals(n, 1)
        other = filtered.copy()
        other[:, 0] += F(0.25)                                          # another cloud of the same size
        fresh.set_source(filtered)
        est = fresh.normals(of_target=False)                           # what a context without supplied normals answers
        fresh.set_source(other)
        est_other = fresh.normals(of_target=False)
        assert bits(est) != bits(sup) and bits(est_other) != bits(sup) and bits(est) != bits(est_other)

        def supply():
            c.set_source_normals(sup)
            assert bits(c.normals(of_target=False)) == bits(sup)       # icpgpu_normals(ctx, 0) returns the caller's

        c.set_source(other)
        supply()
        adopted = c.profile().sources_adopted
        c.set_source(filtered)                                         # icpgpu_set_source, adopted from the filter's result in HBM
        assert c.profile().sources_adopted == adopted + 1
        assert bits(c.normals(of_target=False)) == bits(est)
        supply()
        c.set_source(other)                                            # icpgpu_set_source, uploaded
        assert c.profile().sources_adopted == adopted + 1
        assert bits(c.normals(of_target=False)) == bits(est_other)
        c.set_source(filtered)
        supply()
        dev = torch.from_numpy(other.copy()).cuda()
        torch.cuda.synchronize()
        c.set_source_device(dev.data_ptr(), n)                         # icpgpu_set_source_device
        assert bits(c.normals(of_target=False)) == bits(est_other)
        c.set_source(filtered)
        supply()
        assert c.set_source_voxel_filtered(raw, 0.5) == n               # icpgpu_set_source_voxel_filtered
        assert bits(c.normals(of_target=False)) == bits(est)
        c.set_source(filtered)                                         # (the external buffer is let go before it is freed)
        del dev


def test_promote_moves_supplied_source_normals_to_the_target():
    a, b, _ = synth.make_pair(3000, 3000, seed=12)
    sup = unit_normals(a.shape[0], 2)
    with Context(0) as c, Context(0) as fresh:
        c.set_params(method=P2PLANE)
        c.set_target(b)
        c.set_source(a)
        c.set_source_normals(sup)
        c.set_target_normals(unit_normals(b.shape[0], 9))
        launches = c.profile().gicp_cov_launches
        c.promote_source_to_target()
        assert c.n_source == 0 and c.n_target == a.shape[0]
        assert bits(c.normals(of_target=True)) == bits(sup)            # moved, bit for bit: nothing is estimated
        assert c.profile().gicp_cov_launches == launches
        c.set_source(b)                                                # the next scan: no normals come with it
        fresh.set_source(b)
        assert bits(c.normals(of_target=False)) == bits(fresh.normals(of_target=False))
        assert bits(c.normals(of_target=True)) == bits(sup)
        # the odometer's protocol: every scan's normals are supplied once, as the source's, and serve again as the target's
        c.set_source_normals(unit_normals(b.shape[0], 5))
        c.set_p2plane_symmetric(True)
        first = c.align()
        c.promote_source_to_target()
        assert bits(c.normals(of_target=True)) == bits(unit_normals(b.shape[0], 5))
        c.set_target(a)                                                # a new target drops them
        fresh.set_target(a)
        assert bits(c.normals(of_target=True)) == bits(fresh.normals(of_target=True))
        assert first["iterations"] >= 1


def test_promote_without_supplied_normals_re_estimates():
    a, b, _ = synth.make_pair(3000, 3000, seed=12)
    with Context(0) as c, Context(0) as fresh:
        c.set_params(method=P2PLANE)
        c.set_target(b)
        c.set_source(a)
        c.set_target_normals(unit_normals(b.shape[0], 9))
        c.set_p2plane_symmetric(True)
        c.align()                                                      # (the source's normals are estimated and cached here)
        launches = c.profile().gicp_cov_launches
        c.promote_source_to_target()
        fresh.set_target(a)
        assert bits(c.normals(of_target=True)) == bits(fresh.normals(of_target=True))
        assert c.profile().gicp_cov_launches == launches + 1           # as before this feature: the new target's are estimated


def test_a_recognised_target_leaves_the_normals_with_the_source():
    a, b, _ = synth.make_pair(3000, 3000, seed=12)
    sup = unit_normals(a.shape[0], 2)
    with Context(0) as c, Context(0) as fresh:
        c.set_target(b)
        c.set_source(a)
        c.set_source_normals(sup)
        recognised = c.profile().targets_recognised
        c.set_target(a)                                                # the source's content: the promote path inside set_target
        assert c.profile().targets_recognised == recognised + 1
        assert c.n_source == a.shape[0]
        assert bits(c.normals(of_target=False)) == bits(sup)
        fresh.set_target(a)
        assert bits(c.normals(of_target=True)) == bits(fresh.normals(of_target=True))   # set_target hands the target none
