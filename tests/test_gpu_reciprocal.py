"""GPU tests of reciprocal correspondences (icp_reciprocal.hip, icpgpu_reject.cpp) against the NumPy restatement
(tests/reciprocal_restated.py): the kept set index for index and d2 bit for bit, the edges, whole alignments, that nothing else
moved, and that a context with history answers as a new one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reciprocal_restated as RR  # noqa: E402
import rejectors_restated as R  # noqa: E402
from test_gpu_rejectors import CHAINS, T_FIXED, _align_bits  # noqa: E402
from test_rejectors_host import moved_object_pair  # noqa: E402

from icpslam_amd import Context, IcpGpuError, _lib, synth  # noqa: E402
from icpslam_amd import registration as reg  # noqa: E402

pytestmark = pytest.mark.gpu

# the flag alone, and the flag in front of each of these chains
WITH = {"alone": [], **{k: CHAINS[k] for k in ("median", "trimmed", "one_to_one", "median_one_to_one")}}
MODES = [_lib.NN_BRUTE, _lib.NN_GRID]
_restated = {}      # (cloud key, T bytes, gate) -> RR.reciprocal's result: computed once, shared by the chains and the parameters


def _reciprocal_once(key, src, tgt, T, max_dist):
    k = (key, np.asarray(T, np.float32).tobytes(), float(max_dist))
    if k not in _restated:
        _restated[k] = RR.reciprocal(src, tgt, T, max_dist)
    return _restated[k]


def _check_kept(ctx, key, src, tgt, chains=WITH, T=T_FIXED, max_dist=1.0, both_outcomes=True):
    """ctx.correspondences / reciprocal_stats / rejector_stats against the restatement for the flag in front of every chain"""
    fidx, fd2, rkept, rstats = _reciprocal_once(key, src, tgt, T, max_dist)
    if both_outcomes:     # a comparison of two empty or two full sets shows nothing
        assert 0 < rstats["pairs_out"] < rstats["pairs_in"], rstats
    ctx.set_reciprocal_correspondences(True)
    assert ctx.get_reciprocal_correspondences()
    out = None
    for name, chain in chains.items():
        ctx.set_correspondence_rejectors(chain)
        idx, d2 = ctx.correspondences(T)
        st, cst = ctx.reciprocal_stats(), ctx.rejector_stats()
        kept, want_cst = R.apply_chain(np.where(rkept, fidx, -1), fd2, max_dist, chain)
        ridx = np.where(kept, fidx, -1).astype(np.int32)
        rd2 = np.where(kept, fd2, np.float32(np.inf)).astype(np.float32)
        assert np.array_equal(idx, ridx), (name, int((idx != ridx).sum()), idx.size)
        assert np.array_equal(d2.view(np.uint32), rd2.view(np.uint32)), name                     # bit for bit
        assert st == rstats, (name, st, rstats)
        assert [(s["pairs_in"], s["pairs_out"]) for s in cst] == [(s["pairs_in"], s["pairs_out"]) for s in want_cst], name
        idx2, d22 = ctx.correspondences(T)                                                       # the same twice in a row
        assert np.array_equal(idx, idx2) and np.array_equal(d2.view(np.uint32), d22.view(np.uint32))
        assert ctx.reciprocal_stats() == st and ctx.rejector_stats() == cst
        if name == "alone":
            out = idx
    return out


@pytest.fixture(scope="module")
def pair3k(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=17)
    return src, tgt


# ---- the kept set -----------------------------------------------------------------------------------------------------------------
# (the kernels' launch geometry: workgroups of 256 threads, one thread per source point, and LDS tiles of 256 transformed points in
#  the brute flavour -- 255 / 256 / 257 sit around both, 1025 in the fifth workgroup and tile)
@pytest.mark.parametrize("method", [_lib.P2P_SVD, _lib.P2PLANE])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000])
def test_kept_set_small_sources(pair3k, n, mode, method):
    src, tgt = pair3k
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode, method=method)
        ctx.set_source(src[:n])
        ctx.set_target(tgt)
        # (from 63 points on the restatement rejects and keeps at least one gated pair; below, the sets are what they are)
        _check_kept(ctx, ("3k", n), src[:n], tgt, both_outcomes=n >= 63)


def test_counts_of_the_3k_pair(pair3k):
    """the figures of tests/test_reciprocal_host.py, from the device"""
    src, tgt = pair3k
    for n, want in ((3000, (2913, 1661)), (1025, (992, 761)), (64, (63, 61))):
        with Context(0) as ctx:
            ctx.set_source(src[:n])
            ctx.set_target(tgt)
            ctx.set_reciprocal_correspondences(True)
            idx, _ = ctx.correspondences(T_FIXED)
            st = ctx.reciprocal_stats()
        assert (st["pairs_in"], st["pairs_out"]) == want and int((idx >= 0).sum()) == want[1]


def test_kept_set_behind_the_forward_search_of_large_sources(built):
    """from 32768 source points on the forward grid search is another kernel (four queries per quad, previous-neighbour bounds);
    the stage behind it is the same"""
    src, tgt, _ = synth.make_pair(40000, 40000, seed=23)
    with Context(0) as ctx:
        ctx.set_source(src)
        ctx.set_target(tgt)
        _check_kept(ctx, "40k", src, tgt, chains={k: WITH[k] for k in ("alone", "median_one_to_one")})


# ---- edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_duplicates_and_non_finite(pair3k, mode):
    src, tgt = pair3k
    tgt_dup = np.concatenate([tgt, tgt[:700]])                        # duplicated target points: the lowest index is the neighbour
    src_dup = np.concatenate([src[:1500], src[:1500], src[100:400]])  # duplicated sources: equal reverse distances, lowest index stays
    src_nf = src_dup.copy()
    src_nf[5, 0] = np.nan                                             # (its copy, 1505, becomes the first finite one)
    src_nf[77, 1] = np.inf
    src_nf[300, 2] = -np.inf
    tgt_nf = tgt_dup.copy()
    tgt_nf[9, 0] = np.nan
    tgt_nf[1200, 2] = np.inf
    for name, s, t in (("dup_t", src, tgt_dup), ("dup_s", src_dup, tgt), ("dup_st", src_dup, tgt_dup), ("nf", src_nf, tgt_nf)):
        with Context(0) as ctx:
            ctx.set_params(nn_mode=mode)
            ctx.set_source(s)
            ctx.set_target(t)
            idx = _check_kept(ctx, name, s, t)
            if name == "dup_s":
                assert (idx[1500:] == -1).all()                       # a copy never beats its original
            if name == "nf":
                assert (idx[[5, 77, 300]] == -1).all()


@pytest.mark.parametrize("mode", MODES)
def test_gate_removes_everything_and_empty_target(pair3k, mode):
    src, tgt = pair3k
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode, max_correspondence_distance=1e-4)
        ctx.set_source(src)
        ctx.set_target(tgt)
        idx = _check_kept(ctx, "3k_gate", src, tgt, max_dist=1e-4, both_outcomes=False)
        assert (idx == -1).all() and ctx.reciprocal_stats() == dict(pairs_in=0, pairs_out=0)
        r = ctx.align()
        assert (r["converged"], r["state"], r["n_corr"]) == (False, 5, 0)
        assert ctx.reciprocal_stats() == dict(pairs_in=0, pairs_out=0)
        ctx.set_params(nn_mode=mode, max_correspondence_distance=1.0)
        ctx.set_target(np.zeros((0, 4), np.float32))
        idx = _check_kept(ctx, "empty_t", src, np.zeros((0, 4), np.float32), both_outcomes=False)
        assert (idx == -1).all()
        r = ctx.align()
        assert not r["converged"] and r["iterations"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_a_third_of_the_source_far_outside_the_targets_box(pair3k, mode):
    src, tgt = pair3k
    far = src.copy()
    far[::3, :3] += np.float32(500.0)                                 # 500 m along every axis: dropped by the binning, nobody's pair
    near = src.copy()
    near[1::3, 2] += np.float32(0.9)                                  # ... and a third lifted by less than the gate: some leave the box
    for name, s in (("far", far), ("near", near)):
        with Context(0) as ctx:
            ctx.set_params(nn_mode=mode)
            ctx.set_source(s)
            ctx.set_target(tgt)
            idx = _check_kept(ctx, name, s, tgt)
            if name == "far":
                assert (idx[::3] == -1).all()


@pytest.mark.parametrize("mode", MODES)
def test_thousands_of_transformed_points_in_one_target_cell(pair3k, mode):
    """the source scaled by 0.01 about a target point: every transformed point within 1 m of it, so one cell of the target's lattice
    (and its neighbours) holds the whole source -- the binning has no population cap, the walk just gets longer"""
    src, tgt = pair3k
    c = tgt[1234, :3]
    s = src.copy()
    s[:, :3] = c + np.float32(0.01) * (src[:, :3] - c)
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode)
        ctx.set_source(s)
        ctx.set_target(tgt)
        _check_kept(ctx, "shrunk", s, tgt, T=np.eye(4, dtype=np.float32))
    # and the other way round: the whole scene inside a couple of metres (a cell table of a few cells)
    s2, t2 = src.copy(), tgt.copy()
    s2[:, :3] *= np.float32(0.02)
    t2[:, :3] *= np.float32(0.02)
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode, max_correspondence_distance=0.05)
        ctx.set_source(s2)
        ctx.set_target(t2)
        _check_kept(ctx, "small_scene", s2, t2, T=np.eye(4, dtype=np.float32), max_dist=0.05, chains={"alone": []})


@pytest.mark.parametrize("mode", MODES)
def test_a_guess_with_a_metre_and_ten_degrees(pair3k, mode):
    src, tgt = pair3k
    T = synth.pose_matrix(0.8, -0.5, 0.3, 0.02, -0.03, np.deg2rad(10.0)).astype(np.float32)
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode)
        ctx.set_source(src)
        ctx.set_target(tgt)
        _check_kept(ctx, "3k", src, tgt, T=T)
    G = T.copy()
    G[:3, :3] *= np.float32(1.02)                                     # not rigid: the stage takes any matrix the search takes
    G[0, 1] += np.float32(0.01)
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode)
        ctx.set_source(src)
        ctx.set_target(tgt)
        _check_kept(ctx, "3k", src, tgt, T=G, chains={"alone": []})


def test_mapper_nn_cloud_as_target(built):
    """many source points share a target point, and the target repeats its points: the grid is over the distinct ones"""
    scan, submap, _ = synth.make_scan_vs_submap(20000, 60000, seed=7)
    with Context(0) as ctx:
        ctx.map_reset(0.5)
        ctx.map_add_points(submap, np.eye(4))
        ctx.set_source(scan)
        nn_cloud = ctx.map_nn_target(np.eye(4), np.eye(4))
        assert nn_cloud.shape[0] == scan.shape[0]
        idx = _check_kept(ctx, "nn_cloud", scan, nn_cloud, chains={k: WITH[k] for k in ("alone", "one_to_one", "median")})
        kept = idx[idx >= 0]
        assert kept.size == np.unique(kept).size < scan.shape[0] // 2


def test_ties_across_the_workgroup_and_tile_boundary(pair3k):
    """257 and 513 source points whose LAST point repeats the first (the second / third workgroup of 256 threads and, in the brute
    flavour, the second / third LDS tile of 256 transformed points): the winner sits in one tile, its equal in another"""
    src, tgt = pair3k
    for n in (257, 513):
        s = src[:n].copy()
        s[n - 1] = s[0]
        for mode in MODES:
            with Context(0) as ctx:
                ctx.set_params(nn_mode=mode)
                ctx.set_source(s)
                ctx.set_target(tgt)
                idx = _check_kept(ctx, ("tile", n), s, tgt)
                assert idx[n - 1] == -1


# ---- whole alignments ---------------------------------------------------------------------------------------------------------
def _alignment_clouds(which):
    if which == "moved_object":
        src, tgt, _ = moved_object_pair()
    else:
        src, tgt, _ = synth.make_pair(3000, 3000, seed=17)
    return src, tgt


@pytest.mark.parametrize("method", ["p2p", "p2plane"])
@pytest.mark.parametrize("chain", ["alone", "median_one_to_one"])
@pytest.mark.parametrize("which", ["moved_object", "3k"])
def test_whole_alignments(built, which, chain, method):
    src, tgt = _alignment_clouds(which)
    ref = RR.align(src, tgt, WITH[chain], method=method)
    with Context(0) as ctx:
        ctx.set_params(method=_lib.P2PLANE if method == "p2plane" else _lib.P2P_SVD)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_reciprocal_correspondences(True)
        ctx.set_correspondence_rejectors(WITH[chain])
        got = ctx.align()
        st, cst = ctx.reciprocal_stats(), ctx.rejector_stats()
    dR = float(np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max())
    dt = float(np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]))
    print(f"{which} {chain} {method}: iters {got['iterations']}/{ref['iterations']} state {got['state']}/{ref['state']} "
          f"n_corr {got['n_corr']}/{ref['n_corr']} stats {st}/{ref['reciprocal']} dR {dR:.2e} dt {dt:.2e}")
    assert (got["iterations"], got["state"], got["converged"], got["n_corr"]) == (ref["iterations"], ref["state"], ref["converged"], ref["n_corr"])
    assert dR <= 1e-4 and dt <= 1e-3
    assert st == ref["reciprocal"] and 0 < st["pairs_out"] < st["pairs_in"]
    assert [(s["pairs_in"], s["pairs_out"]) for s in cst] == [(s["pairs_in"], s["pairs_out"]) for s in ref["stats"]]


def test_mirror_classes_on_the_device(built):
    src, tgt, _ = synth.make_pair(1500, 1500, seed=1)
    for cls, method in ((reg.IterativeClosestPoint, "p2p"), (reg.IterativeClosestPointWithNormals, "p2plane")):
        icp = cls()
        assert not icp.getUseReciprocalCorrespondences()
        icp.setUseReciprocalCorrespondences(True)
        assert icp.getUseReciprocalCorrespondences()
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        icp.align()
        ref = RR.align(src, tgt, [], method=method)
        assert icp.result["n_corr"] == ref["n_corr"] and icp.result["iterations"] == ref["iterations"]
        plain = cls()                                                 # an object without the flag clears it on the shared context
        plain.setInputSource(src)
        plain.setInputTarget(tgt)
        plain.align()
        off = R.align(src, tgt, [], method=method)
        assert plain.result["n_corr"] == off["n_corr"] > ref["n_corr"]


# ---- nothing else moved -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4000, 120000])
def test_flag_off_and_set_then_cleared_change_nothing(built, n):
    src, tgt, _ = synth.make_pair(n, n, seed=13)

    def set_then_clear(ctx):
        ctx.set_reciprocal_correspondences(True)
        assert ctx.get_reciprocal_correspondences()
        ctx.set_reciprocal_correspondences(False)
        assert not ctx.get_reciprocal_correspondences()

    def chain_and(prepare):
        def f(ctx):
            ctx.set_correspondence_rejectors(CHAINS["median_one_to_one"])
            prepare(ctx)
        return f

    for method in (_lib.P2P_SVD, _lib.P2PLANE):
        fresh = _align_bits(method, src, tgt, lambda ctx: None)
        assert _align_bits(method, src, tgt, lambda ctx: ctx.set_reciprocal_correspondences(False)) == fresh
        assert _align_bits(method, src, tgt, set_then_clear) == fresh
        fresh_chain = _align_bits(method, src, tgt, chain_and(lambda ctx: None))
        assert fresh_chain != fresh
        assert _align_bits(method, src, tgt, chain_and(set_then_clear)) == fresh_chain


def test_gicp_and_ndt_ignore_the_flag(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=19)
    for method in (_lib.GICP, _lib.NDT):
        plain = _align_bits(method, src, tgt, lambda ctx: None)
        assert _align_bits(method, src, tgt, lambda ctx: ctx.set_reciprocal_correspondences(True)) == plain


def test_batches_refuse_the_flag(built):
    pairs = [synth.make_pair(2000, 2000, seed=s)[:2] for s in (3, 4, 5)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    with Context(0) as ctx:
        before = ctx.align_batch(srcs, tgts)
        ctx.set_reciprocal_correspondences(True)
        for method in (_lib.P2P_SVD, _lib.GICP):
            ctx.set_params(method=method)
            with pytest.raises(IcpGpuError) as e:
                ctx.align_batch(srcs, tgts)
            assert e.value.code == _lib.ERR_UNSUPPORTED
        ctx.set_params(method=_lib.P2P_SVD)
        ctx.set_reciprocal_correspondences(False)
        after = ctx.align_batch(srcs, tgts)
    for a, b in zip(before, after):
        assert a["T"].tobytes() == b["T"].tobytes() and (a["iterations"], a["n_corr"]) == (b["iterations"], b["n_corr"])


# ---- history --------------------------------------------------------------------------------------------------------------------
def _observe(ctx, what, T=T_FIXED):
    if what == "align":
        r = ctx.align()
        out = (r["T"].tobytes(), r["iterations"], r["state"], r["n_corr"], np.float64(r["mse"]).tobytes())
    else:
        idx, d2 = ctx.correspondences(T)
        out = (idx.tobytes(), d2.tobytes())
    return out + (tuple(sorted(ctx.reciprocal_stats().items())), tuple((s["pairs_in"], s["pairs_out"]) for s in ctx.rejector_stats()))


def _fresh(src, tgt, flag, chain, method, what):
    """a new context given only the logical state"""
    with Context(0) as ctx:
        ctx.set_params(method=method, max_iterations=4)
        ctx.set_target(tgt)
        ctx.set_source(src)
        ctx.set_reciprocal_correspondences(flag)
        ctx.set_correspondence_rejectors(chain)
        return _observe(ctx, what)


@pytest.mark.parametrize("method", [_lib.P2P_SVD, _lib.P2PLANE])
def test_a_context_with_history_answers_as_a_new_one(built, method):
    """aligns with the flag; changes the target; promotes; toggles the flag; runs correspondences -- after each step the answer of a
    new context; the statistics do not outlive a run without the flag"""
    A, B, _ = synth.make_pair(3000, 3000, seed=17)
    A2, B2, _ = synth.make_pair(2500, 3500, seed=21)
    chain = CHAINS["trimmed"]
    with Context(0) as ctx:
        ctx.set_params(method=method, max_iterations=4)
        ctx.set_target(B)
        ctx.set_source(A)
        ctx.set_reciprocal_correspondences(True)
        got = _observe(ctx, "align")
        assert got == _fresh(A, B, True, [], method, "align") and dict(got[-2])["pairs_out"] > 0
        ctx.set_target(B2)                                            # another target: another lattice for the binning
        assert _observe(ctx, "align") == _fresh(A, B2, True, [], method, "align")
        assert _observe(ctx, "corr") == _fresh(A, B2, True, [], method, "corr")
        ctx.promote_source_to_target()                                # the source and its grid become the target
        ctx.set_source(A2)
        assert _observe(ctx, "align") == _fresh(A2, A, True, [], method, "align")
        ctx.set_correspondence_rejectors(chain)
        assert _observe(ctx, "align") == _fresh(A2, A, True, chain, method, "align")
        ctx.set_reciprocal_correspondences(False)                     # off: the chain alone, and no statistics of the stage
        got = _observe(ctx, "align")
        assert got == _fresh(A2, A, False, chain, method, "align")
        assert ctx.reciprocal_stats() == dict(pairs_in=0, pairs_out=0)
        got = _observe(ctx, "corr")
        assert got == _fresh(A2, A, False, chain, method, "corr") and ctx.reciprocal_stats() == dict(pairs_in=0, pairs_out=0)
        ctx.set_reciprocal_correspondences(True)                      # ... and on again
        got = _observe(ctx, "corr")
        assert got == _fresh(A2, A, True, chain, method, "corr") and dict(got[-2])["pairs_out"] > 0
        ctx.set_params(method=_lib.GICP, max_iterations=2)            # a method that ignores the flag leaves the statistics alone
        ctx.align()
        assert tuple(sorted(ctx.reciprocal_stats().items())) == got[-2]
