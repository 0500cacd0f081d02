"""The surface-normal rejector on the device (icp_reject.hip: reject_normal_kernel; icpgpu_reject.cpp) against its NumPy restatement
(tests/symmetric_restated.py): icpgpu_correspondences index for index and d2 bit for bit, the stage's statistics, its place in a
chain, whole alignments of every method that reads the chain, and a thin wall."""
import os
import re

import numpy as np
import pytest

import oracle
import rejectors_restated as R
import symmetric_restated as S
from icpslam_amd import P2PLANE, P2P_SVD, Context, CorrespondenceRejectorSurfaceNormal, IcpGpuError, IterativeClosestPoint, _lib, synth

pytestmark = pytest.mark.gpu
F = np.float32
N = S.SURFACE_NORMAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_FIXED = synth.pose_matrix(0.05, -0.02, 0.01, 0.01, -0.02, 0.03).astype(F)
THRESHOLDS = (-1.0, 0.0, 0.5, 0.9999, 1.0)
R_TOL, T_TOL = 1e-4, 1e-3                                          # BASELINE.json / DESIGN.md section 3


def stage_capacity():
    """pairs one trip of the stage's capped grid is sized for: 4 x block x block cap, from the kernel's own constants"""
    text = open(os.path.join(ROOT, "icpslam_amd", "csrc", "icp_reject.hip")).read()
    block = int(re.search(r"constexpr int RJ_BLOCK = (\d+);", text).group(1))
    cap = int(re.search(r"constexpr int kRejectMaxBlocks = (\d+);", text).group(1))
    return 4 * block * cap


def check_kept(ctx, src, tgt, sn, tn, chain, T=T_FIXED, max_dist=1.0, reciprocal=False):
    ctx.set_correspondence_rejectors(chain)
    ctx.set_reciprocal_correspondences(reciprocal)
    idx, d2 = ctx.correspondences(T)
    stats = ctx.rejector_stats()
    ridx, rd2, rstats = S.correspondences(src, tgt, T, max_dist, chain, sn, tn, reciprocal=reciprocal)
    assert np.array_equal(idx, ridx), (int((idx != ridx).sum()), idx.size)
    assert np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    assert len(stats) == len(rstats) == len(chain)
    for a, b, stage in zip(stats, rstats, chain):
        assert (a["pairs_in"], a["pairs_out"]) == (b["pairs_in"], b["pairs_out"])
        assert F(a["cut"]).view(np.uint32) == F(b["cut"]).view(np.uint32)
        if stage[0] == N:
            assert float(a["cut"]) == 0.0
    return idx, stats


def cloud_pair(n, n_t, seed):
    """a source of n points around a target of n_t, and both clouds' normals with every kind of angle between them"""
    rng = np.random.default_rng(seed)
    tgt = synth.make_pair(64, n_t, seed=seed)[1]
    src = np.ones((n, 4), F)
    src[:, :3] = tgt[rng.integers(0, n_t, n), :3] + rng.normal(scale=0.05, size=(n, 3)).astype(F)
    sn, tn = rng.normal(size=(n, 4)).astype(F), rng.normal(size=(n_t, 4)).astype(F)
    sn[:, :3] /= np.linalg.norm(sn[:, :3], axis=1, keepdims=True)
    tn[:, :3] /= np.linalg.norm(tn[:, :3], axis=1, keepdims=True)
    return src, tgt, sn, tn


@pytest.fixture(scope="module")
def big(built):
    return cloud_pair(stage_capacity() + 1, 2048, 7)


@pytest.mark.parametrize("method", [P2P_SVD, P2PLANE])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 4097])
def test_kept_set_sizes_and_thresholds(big, n, method):
    src, tgt, sn, tn = (a[:n] if k in (0, 2) else a for k, a in enumerate(big))
    with Context(0) as ctx:
        ctx.set_params(method=method)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_source_normals(sn)
        ctx.set_target_normals(tn)
        kept = []
        for thr in THRESHOLDS:
            idx, stats = check_kept(ctx, src, tgt, sn, tn, [(N, thr)])
            kept.append(stats[0]["pairs_out"])
        assert kept == sorted(kept, reverse=True) and kept[-1] == 0      # random unit normals never reach a float32 dot above 1
        if n >= 255:
            assert kept[0] == stats[0]["pairs_in"] > 0 and 0 < kept[2] < kept[1] < kept[0]


def test_kept_set_past_the_block_cap(big):
    src, tgt, sn, tn = big
    assert src.shape[0] == 1048577
    with Context(0) as ctx:
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_source_normals(sn)
        ctx.set_target_normals(tn)
        _, stats = check_kept(ctx, src, tgt, sn, tn, [(N, 0.5)])
        assert stats[0]["pairs_in"] > 1000000 and 0 < stats[0]["pairs_out"] < stats[0]["pairs_in"] // 2


def test_dots_exactly_on_the_threshold_and_nan_normals(built):
    """lattice normals under a pure translation (the rotation's products are exact): dots of exactly -1, 0, 0.5 and 1 are rejected
    at those thresholds (the comparison is strict) and kept just below them; a NaN on either side is rejected at every threshold"""
    g = np.arange(8, dtype=F)
    xx, yy, zz = np.meshgrid(g, g, g, indexing="ij")
    tgt = np.column_stack([xx.ravel(), yy.ravel(), zz.ravel(), np.ones(xx.size)]).astype(F)
    T = synth.pose_matrix(0.125, 0.0, -0.0625, 0.0, 0.0, 0.0).astype(F)
    src = tgt.copy()
    src[:, :3] += np.array([-0.0625, 0.0625, 0.125], F)                # T * src lies (1/16, 1/16, 1/16) beside its own node: pair i -> i
    n = tgt.shape[0]
    lattice = np.array([[1, 0, 0, 0], [0.5, 0.5, 0, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0.5, 0, -0.5, 0], [np.nan, 0, 0, 0], [1, 0, 0, 0]], F)
    sn = lattice[np.arange(n) % 7].copy()
    tn = np.tile(np.array([1, 0, 0, 0], F), (n, 1))
    tn[6::7, 1] = np.nan                                               # (the seventh of every seven: the NaN is the target's)
    dots = np.array([1, 0.5, 0, -1, 0.5, np.nan, np.nan])
    with Context(0) as ctx:
        ctx.set_params(max_correspondence_distance=0.5)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_source_normals(sn)
        ctx.set_target_normals(tn)
        for thr in (-1.0, float(np.nextafter(F(-1), F(-2))), 0.0, -1e-30, 0.5, float(np.nextafter(F(0.5), F(0))), 1.0,
                    float(np.nextafter(F(1), F(0)))):
            idx, stats = check_kept(ctx, src, tgt, sn, tn, [(N, thr)], T=T, max_dist=0.5)
            with np.errstate(invalid="ignore"):
                want = dots[np.arange(n) % 7] > thr
            assert stats[0]["pairs_in"] == n and np.array_equal(idx >= 0, want) and np.array_equal(idx[want], np.flatnonzero(want))


CHAINS = {
    "first": [(N, 0.0), (R.MEDIAN, 1.5), (R.ONE_TO_ONE,)],
    "last": [(R.MEDIAN, 1.5), (R.ONE_TO_ONE,), (N, 0.0)],
    "twice": [(N, -0.5), (R.ONE_TO_ONE,), (N, 0.5), (R.MEDIAN, 1.0)],
}


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("mode", [_lib.NN_BRUTE, _lib.NN_GRID])
def test_the_stage_in_a_chain(built, mode, reciprocal):
    src, tgt, sn, tn = cloud_pair(3000, 2500, 11)
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_source_normals(sn)
        ctx.set_target_normals(tn)
        for chain in CHAINS.values():
            _, stats = check_kept(ctx, src, tgt, sn, tn, chain, reciprocal=reciprocal)
            assert all(s["pairs_out"] > 0 for s in stats)
        rs = ctx.reciprocal_stats()
        assert (rs["pairs_out"] > 0) == reciprocal


def test_estimated_normals_and_small_clouds(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=61)
    sn, tn = oracle.gicp_normals(src), oracle.gicp_normals(tgt)
    with Context(0) as ctx:
        ctx.set_source(src)
        ctx.set_target(tgt)
        _, stats = check_kept(ctx, src, tgt, sn, tn, [(N, 0.9)])         # nothing supplied: GICP's plane on both clouds
        assert 0 < stats[0]["pairs_out"] < stats[0]["pairs_in"]
        ctx.set_source(src[:19])                                        # too small to estimate, nothing supplied
        with pytest.raises(IcpGpuError) as e:
            ctx.correspondences(np.eye(4))
        assert e.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(IcpGpuError) as e:
            ctx.align()
        assert e.value.code == _lib.ERR_INVALID_ARG
        ctx.set_source_normals(sn[:19])
        check_kept(ctx, src[:19], tgt, sn[:19], tn, [(N, 0.9)])
        ctx.set_target(np.zeros((0, 4), F))                             # no pair: the stage reads no normal and keeps nothing
        idx, stats = check_kept(ctx, src[:19], np.zeros((0, 4), F), sn[:19], tn[:0], [(N, 0.9)])
        assert (idx == -1).all() and stats[0]["pairs_in"] == 0


# ---- whole alignments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["p2p", "p2plane", "symmetric"])
def test_whole_alignments_with_the_stage(built, method):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=61)
    sn, tn = oracle.gicp_normals(src), oracle.gicp_normals(tgt)
    chain = [(N, 0.8), (R.MEDIAN, 2.0)]
    ref = S.align(src, tgt, sn, tn, chain=chain, method=method)
    assert S.decisions_clear(ref) and ref["iterations"] > 2
    assert 0 < ref["stats"][0]["pairs_out"] < ref["stats"][0]["pairs_in"]
    with Context(0) as ctx:
        ctx.set_params(method=P2P_SVD if method == "p2p" else P2PLANE)
        ctx.set_source(src)
        ctx.set_target(tgt)
        if method != "p2plane":                                          # (p2plane: both estimated)
            ctx.set_source_normals(sn)
            ctx.set_target_normals(tn)
        ctx.set_p2plane_symmetric(method == "symmetric")
        ctx.set_correspondence_rejectors(chain)
        got = ctx.align()
        stats = ctx.rejector_stats()
    assert (got["converged"], got["iterations"], got["state"], got["n_corr"]) == (ref["converged"], ref["iterations"], ref["state"], ref["n_corr"])
    assert np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max() <= R_TOL and np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]) <= T_TOL
    assert [(s["pairs_in"], s["pairs_out"]) for s in stats] == [(s["pairs_in"], s["pairs_out"]) for s in ref["stats"]]


def test_thin_wall(built):
    """Two parallel sheets 5 cm apart with opposite normals, the source 4 cm off the front sheet (1 cm from the back one): without
    the stage pairs reach across to the back sheet, with threshold 0 none does."""
    rng = np.random.default_rng(2)
    n = 1500
    xy = rng.uniform(-3, 3, (n, 2))
    front = np.column_stack([xy, np.zeros(n), np.ones(n)]).astype(F)
    back = np.column_stack([xy + rng.normal(scale=0.01, size=(n, 2)), np.full(n, 0.05), np.ones(n)]).astype(F)
    tgt = np.concatenate([front, back])
    tn = np.concatenate([np.tile(np.array([0, 0, -1, 0], F), (n, 1)), np.tile(np.array([0, 0, 1, 0], F), (n, 1))])
    src = front.copy()
    src[:, 2] = F(0.04)
    sn = np.tile(np.array([0, 0, -1, 0], F), (n, 1))                     # the source saw the front sheet
    with Context(0) as ctx:
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_source_normals(sn)
        ctx.set_target_normals(tn)
        without, _ = check_kept(ctx, src, tgt, sn, tn, [])
        with_stage, stats = check_kept(ctx, src, tgt, sn, tn, [(N, 0.0)])
    assert (without >= n).sum() > n // 2                                # the nearer sheet is the wrong one
    assert (with_stage >= n).sum() == 0 and stats[0]["pairs_out"] == (without < n).sum()
    ridx, _, _ = S.correspondences(src, tgt, np.eye(4), 1.0, [(N, 0.0)], sn, tn)
    assert (ridx >= n).sum() == 0


# ---- the setter, the mirrors --------------------------------------------------------------------------------------------------------
def test_setter_refusals_keep_the_chain(built):
    with Context(0) as ctx:
        ctx.set_correspondence_rejectors([(N, 0.25), (R.TRIMMED, 0.25, 7)])
        assert ctx.get_correspondence_rejectors() == [(N, 0.25, 0), (R.TRIMMED, 0.25, 7)]
        for bad in ([(N, float("nan"))], [(N, float("-inf"))], [(N, float("inf"))], [(N, 0.5)] * 5, [(5, 0.5)]):
            with pytest.raises(IcpGpuError) as e:
                ctx.set_correspondence_rejectors(bad)
            assert e.value.code == _lib.ERR_INVALID_ARG
            assert ctx.get_correspondence_rejectors() == [(N, 0.25, 0), (R.TRIMMED, 0.25, 7)]
        ctx.set_correspondence_rejectors([(N, -1e300), (N, 1e300)])      # any finite threshold


def test_plain_icp_mirror_feeds_the_stage(built):
    """IterativeClosestPoint (point-to-point) with setSourceNormals / setTargetNormals and the rejector class"""
    src, tgt, _ = synth.make_pair(3000, 3000, seed=61)
    sn, tn = oracle.gicp_normals(src), oracle.gicp_normals(tgt)
    ref = S.align(src, tgt, sn, tn, chain=[(N, 0.8)], method="p2p")
    assert S.decisions_clear(ref)
    icp = IterativeClosestPoint()
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.setSourceNormals(sn)
    icp.setTargetNormals(tn)
    rej = CorrespondenceRejectorSurfaceNormal()
    rej.setThreshold(0.8)
    icp.addCorrespondenceRejector(rej)
    icp.align()
    r = icp.result
    assert (r["iterations"], r["state"], r["n_corr"]) == (ref["iterations"], ref["state"], ref["n_corr"])
    assert np.abs(r["T"][:3, :3] - ref["T"][:3, :3]).max() <= R_TOL and np.linalg.norm(r["T"][:3, 3] - ref["T"][:3, 3]) <= T_TOL
