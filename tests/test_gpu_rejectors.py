"""GPU tests of the correspondence rejectors (icp_reject.hip, icpgpu_reject.cpp) against the NumPy restatement
(tests/rejectors_restated.py): the kept set index for index, whole alignments, and that nothing else moved."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rejectors_restated as R  # noqa: E402
from test_rejectors_host import motion_error, moved_object_pair  # noqa: E402

from icpslam_amd import Context, IcpGpuError, _lib, synth  # noqa: E402
from icpslam_amd import registration as reg  # noqa: E402

pytestmark = pytest.mark.gpu

CHAINS = {
    "median": [(R.MEDIAN, 1.0)],
    "median_wide": [(R.MEDIAN, 2.5)],
    "trimmed": [(R.TRIMMED, 0.5)],
    "trimmed_min": [(R.TRIMMED, 0.1, 40)],
    "one_to_one": [(R.ONE_TO_ONE,)],
    "median_one_to_one": [(R.MEDIAN, 2.0), (R.ONE_TO_ONE,)],
    "one_to_one_trimmed": [(R.ONE_TO_ONE,), (R.TRIMMED, 0.75, 10)],
}
T_FIXED = synth.pose_matrix(0.05, -0.02, 0.01, 0.0, 0.0, 0.01).astype(np.float32)


def _check_kept(ctx, src, tgt, chain, T=T_FIXED, max_dist=1.0):
    ctx.set_correspondence_rejectors(chain)
    idx, d2 = ctx.correspondences(T)
    stats = ctx.rejector_stats()
    ridx, rd2, rstats = R.correspondences(src, tgt, T, max_dist, chain)
    assert np.array_equal(idx, ridx), (int((idx != ridx).sum()), idx.size)
    assert np.array_equal(d2, rd2)
    assert len(stats) == len(rstats) == len(chain)
    for a, b in zip(stats, rstats):
        assert (a["pairs_in"], a["pairs_out"]) == (b["pairs_in"], b["pairs_out"])
        assert np.float32(a["cut"]).view(np.uint32) == np.float32(b["cut"]).view(np.uint32)      # bit for bit
    idx2, d22 = ctx.correspondences(T)                                                           # the same twice in a row
    assert np.array_equal(idx, idx2) and np.array_equal(d2, d22) and ctx.rejector_stats() == stats
    return idx


@pytest.fixture(scope="module")
def pair3k(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=17)
    return src, tgt


@pytest.mark.parametrize("method", [_lib.P2P_SVD, _lib.P2PLANE])
@pytest.mark.parametrize("mode", [_lib.NN_BRUTE, _lib.NN_GRID])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000])
def test_kept_set_small_sources(pair3k, n, mode, method):
    src, tgt = pair3k
    with Context(0) as ctx:
        ctx.set_params(nn_mode=mode, method=method)
        ctx.set_source(src[:n])
        ctx.set_target(tgt)
        for chain in CHAINS.values():
            _check_kept(ctx, src[:n], tgt, chain)


@pytest.mark.parametrize("n", [200000, 262143, 262145, 1048577])       # the last three: around one grid stride of the stages
def test_kept_set_large_sources(built, n):
    src, tgt, _ = synth.make_pair(n, 200000, seed=23)
    with Context(0) as ctx:
        ctx.set_source(src)
        ctx.set_target(tgt)
        for name in ("median", "trimmed", "median_one_to_one", "one_to_one_trimmed") if n == 200000 else ("median_one_to_one",):
            _check_kept(ctx, src, tgt, CHAINS[name])


def test_kept_set_1m5_once(built):
    src, tgt, _ = synth.make_pair(1500000, 1500000, seed=29)
    with Context(0) as ctx:
        ctx.set_params(method=_lib.P2PLANE)
        ctx.set_source(src)
        ctx.set_target(tgt)
        _check_kept(ctx, src, tgt, [(R.ONE_TO_ONE,), (R.TRIMMED, 0.6), (R.MEDIAN, 1.0)])


@pytest.mark.parametrize("mode", [_lib.NN_BRUTE, _lib.NN_GRID])
def test_kept_set_ties_duplicates_non_finite(pair3k, mode):
    src, tgt = pair3k
    tgt_dup = np.concatenate([tgt, tgt[:700]])                       # duplicated target points: the lowest index is the neighbour
    src_dup = np.concatenate([src[:1500], src[:1500], src[100:400]]) # duplicated sources: equal d2 at the cuts and at the winners
    src_nf = src_dup.copy()
    src_nf[5, 0] = np.nan
    src_nf[77, 1] = np.inf
    src_nf[300, 2] = -np.inf
    tgt_nf = tgt_dup.copy()
    tgt_nf[9, 0] = np.nan
    tgt_nf[1200, 2] = np.inf
    for s, t in ((src, tgt_dup), (src_dup, tgt), (src_dup, tgt_dup), (src_nf, tgt_nf)):
        with Context(0) as ctx:
            ctx.set_params(nn_mode=mode)
            ctx.set_source(s)
            ctx.set_target(t)
            for chain in CHAINS.values():
                _check_kept(ctx, s, t, chain)
            _check_kept(ctx, s, t, [(R.TRIMMED, 1.0)])               # keeps everything the gate left
            _check_kept(ctx, s, t, [(R.TRIMMED, 0.0)])               # keeps nothing
            _check_kept(ctx, s, t, [(R.MEDIAN, 0.0)])
            _check_kept(ctx, s, t, [(R.MEDIAN, 1e300)])


def test_gate_removes_everything_and_empty_target(pair3k):
    src, tgt = pair3k
    with Context(0) as ctx:
        ctx.set_params(max_correspondence_distance=1e-4)
        ctx.set_source(src)
        ctx.set_target(tgt)
        for chain in CHAINS.values():
            idx = _check_kept(ctx, src, tgt, chain, max_dist=1e-4)
            assert (idx == -1).all()
        ctx.set_correspondence_rejectors(CHAINS["median_one_to_one"])
        r = ctx.align()
        assert (r["converged"], r["state"], r["n_corr"]) == (False, 5, 0)
        assert [s["pairs_in"] for s in ctx.rejector_stats()] == [0, 0]
        ctx.set_target(np.zeros((0, 4), np.float32))
        idx, _ = ctx.correspondences(np.eye(4))
        assert (idx == -1).all()
        r = ctx.align()
        assert not r["converged"] and r["iterations"] == 0


def test_kept_set_mapper_nn_cloud_as_target(built):
    """many source points share a target point: one-to-one's hardest case"""
    scan, submap, _ = synth.make_scan_vs_submap(20000, 60000, seed=7)
    with Context(0) as ctx:
        ctx.map_reset(0.5)
        ctx.map_add_points(submap, np.eye(4))
        ctx.set_source(scan)
        nn_cloud = ctx.map_nn_target(np.eye(4), np.eye(4))
        assert nn_cloud.shape[0] == scan.shape[0]
        for name in ("one_to_one", "median_one_to_one", "one_to_one_trimmed"):
            idx = _check_kept(ctx, scan, nn_cloud, CHAINS[name])
            kept = idx[idx >= 0]
            assert kept.size == np.unique(kept).size < scan.shape[0] // 2


# ---- whole alignments ---------------------------------------------------------------------------------------------------------
# The device's transform can differ from the restatement's in the last float32 bit.  A rotation entry off by one ulp (2^-24
# relative to entries <= 1, i.e. up to 2^-23 after rounding) moves a point at distance `extent` from the origin by extent x 2^-23,
# and a squared distance d^2 by 2 d x that.  Relative to d^2 that is 2 extent 2^-23 / d.  The synthetic scans reach 80 m from the
# sensor (synth.make_scene's extent 60 m plus the motion), so a cut is safe when its margin exceeds 2 x 80 x 2^-23 / d, d the
# distance the margin was measured at.  Alignments with a thinner margin in any iteration are not pinned (at most a quarter).
EXTENT_M = 80.0
SEEDS = (1, 4, 9, 11)


def _required_margin(d2_at):
    return 2.0 * EXTENT_M * 2.0 ** -23 / max(float(np.sqrt(d2_at)), 1e-30)


@pytest.mark.parametrize("method", ["p2p", "p2plane"])
@pytest.mark.parametrize("name", ["median", "trimmed", "one_to_one", "median_one_to_one"])
def test_whole_alignments(built, name, method):
    chain = CHAINS[name]
    pinned = 0
    for seed in SEEDS:
        src, tgt, _ = synth.make_pair(1500, 1500, seed=seed)
        ref = R.align(src, tgt, chain, method=method)
        safe = all(m > _required_margin(at) for it in ref["margins"] for m, at in it if np.isfinite(m))
        with Context(0) as ctx:
            ctx.set_params(method=_lib.P2PLANE if method == "p2plane" else _lib.P2P_SVD)
            ctx.set_source(src)
            ctx.set_target(tgt)
            ctx.set_correspondence_rejectors(chain)
            got = ctx.align()
            stats = ctx.rejector_stats()
        dR = float(np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max())
        dt = float(np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]))
        print(f"{name} {method} seed {seed}: safe={safe} iters {got['iterations']}/{ref['iterations']} n_corr {got['n_corr']}/{ref['n_corr']} "
              f"dR {dR:.2e} dt {dt:.2e}")
        if not safe:
            continue
        pinned += 1
        assert (got["iterations"], got["state"], got["converged"], got["n_corr"]) == (ref["iterations"], ref["state"], ref["converged"], ref["n_corr"])
        assert dR <= 1e-4 and dt <= 1e-3
        assert [(s["pairs_in"], s["pairs_out"]) for s in stats] == [(s["pairs_in"], s["pairs_out"]) for s in ref["stats"]]
    assert 4 * (len(SEEDS) - pinned) <= len(SEEDS)


def test_fixture_alignments(built):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "rejectors_1k5.npz"))
    for name in ("median", "trimmed", "one_to_one", "median_one_to_one", "one_to_one_trimmed"):
        chain = [tuple(row) for row in g[f"{name}_chain"]]
        with Context(0) as ctx:
            ctx.set_source(g["src"])
            ctx.set_target(g["tgt"])
            ctx.set_correspondence_rejectors(chain)
            idx, _ = ctx.correspondences(g["T_fixed"])
            assert np.array_equal(idx, g[f"{name}_idx"])
            st = ctx.rejector_stats()
            assert [[s["pairs_in"], s["pairs_out"], int(np.float32(s["cut"]).view(np.uint32))] for s in st] == g[f"{name}_stats"].tolist()


def test_moved_object_pair(built):
    src, tgt, T_true = moved_object_pair()
    for chain in ([], [(R.TRIMMED, 0.7)]):
        ref = R.align(src, tgt, chain, max_iterations=30)
        with Context(0) as ctx:
            ctx.set_params(max_iterations=30)
            ctx.set_source(src)
            ctx.set_target(tgt)
            ctx.set_correspondence_rejectors(chain)
            got = ctx.align()
        dR = float(np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max())
        dt = float(np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]))
        print(f"moved object, chain {chain}: {motion_error(got['T'], T_true):.4f} m from the true motion; dR {dR:.2e} dt {dt:.2e}")
        assert dR <= 1e-4 and dt <= 1e-3


# ---- nothing else moved -------------------------------------------------------------------------------------------------------
_COUNTERS = ("nn_launches", "reduce_launches", "grid_launches", "transform_launches", "iterations", "aligns", "grid_builds",
             "gicp_cov_launches", "gicp_cost_launches")


def _align_bits(method, src, tgt, prepare):
    with Context(0) as ctx:
        ctx.set_params(method=method)
        ctx.set_source(src)
        ctx.set_target(tgt)
        prepare(ctx)
        ctx.profile_reset()
        r = ctx.align(want_fitness=True)
        p = ctx.profile()
    return r["T"].tobytes(), r["iterations"], r["state"], r["n_corr"], np.float64(r["mse"]).tobytes(), np.float64(r["fitness"]).tobytes(), tuple(getattr(p, k) for k in _COUNTERS)


@pytest.mark.parametrize("n", [4000, 120000])
def test_empty_chain_and_set_then_clear_change_nothing(built, n):
    src, tgt, _ = synth.make_pair(n, n, seed=13)

    def set_then_clear(ctx):
        ctx.set_correspondence_rejectors(CHAINS["median_one_to_one"])
        assert len(ctx.get_correspondence_rejectors()) == 2
        ctx.set_correspondence_rejectors([])
        assert ctx.get_correspondence_rejectors() == []

    for method in (_lib.P2P_SVD, _lib.P2PLANE):
        fresh = _align_bits(method, src, tgt, lambda ctx: None)
        assert _align_bits(method, src, tgt, lambda ctx: ctx.set_correspondence_rejectors([])) == fresh
        assert _align_bits(method, src, tgt, set_then_clear) == fresh


def test_gicp_and_ndt_ignore_the_chain(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=19)
    for method in (_lib.GICP, _lib.NDT):
        plain = _align_bits(method, src, tgt, lambda ctx: None)
        assert _align_bits(method, src, tgt, lambda ctx: ctx.set_correspondence_rejectors(CHAINS["one_to_one_trimmed"])) == plain


def test_statistics_outlive_gicp_ndt_and_fitness_until_the_next_p2p_alignment(pair3k):
    """include/icpgpu.h: both statistics are those of "the last P2P_SVD / P2PLANE alignment" -- a GICP or NDT alignment and
    icpgpu_fitness leave them alone; the next point-to-point alignment, with no chain and the flag off, empties them."""
    src, tgt = pair3k
    with Context(0) as ctx:
        ctx.set_params(max_iterations=3)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_correspondence_rejectors(CHAINS["median_one_to_one"])
        ctx.set_reciprocal_correspondences(True)
        ctx.align()
        rej, rcp = ctx.rejector_stats(), ctx.reciprocal_stats()
        assert len(rej) == 2 and rej[0]["pairs_in"] > 0 and rcp["pairs_in"] > 0
        for step in (lambda: (ctx.set_params(method=_lib.GICP), ctx.align()), lambda: (ctx.set_params(method=_lib.NDT), ctx.align()),
                     ctx.fitness):
            step()
            assert ctx.rejector_stats() == rej and ctx.reciprocal_stats() == rcp
        ctx.set_params(method=_lib.P2P_SVD)
        ctx.set_correspondence_rejectors([])
        ctx.set_reciprocal_correspondences(False)
        ctx.align()
        assert ctx.rejector_stats() == [] and ctx.reciprocal_stats() == dict(pairs_in=0, pairs_out=0)


# ---- the ends an alignment reaches without iterating: one record, one count, and the transform icpgpu_fitness goes on with ------
_EDGE_GUESS = synth.pose_matrix(0.03, -0.02, 0.01, 0.002, -0.001, 0.004).astype(np.float32)
_DBL_MAX = float(np.finfo(np.float64).max)


def _edge_align(method, src, tgt):
    """A fresh context's alignment from _EDGE_GUESS -> (the record without its two time fields, or the error's code; the
    alignments counted; icpgpu_fitness afterwards, as bytes)"""
    with Context(0) as ctx:
        ctx.set_params(method=method, max_iterations=3)
        ctx.set_source(src)
        ctx.set_target(tgt)
        before = ctx.profile().aligns
        try:
            r = ctx.align(guess=_EDGE_GUESS, want_fitness=True)
            rec = (r["T"].tobytes(), r["converged"], r["iterations"], r["state"], r["n_corr"], np.float64(r["mse"]).tobytes(),
                   np.float64(r["fitness"]).tobytes(), r["gicp_solver"])
        except IcpGpuError as e:
            rec = e.code
        return rec, ctx.profile().aligns - before, np.float64(ctx.fitness()).tobytes()


def _fitness_at(src, tgt, T):
    """getFitnessScore at T: a point-to-point alignment that may not move (no pair count reaches its minimum) and then sweeps"""
    if len(tgt) == 0:
        return _DBL_MAX
    with Context(0) as ctx:
        ctx.set_params(min_correspondences=1 << 30)
        ctx.set_source(src)
        ctx.set_target(tgt)
        r = ctx.align(guess=T, want_fitness=True)
        assert r["iterations"] == 0 and r["T"].tobytes() == np.asarray(T, np.float32).tobytes()
        return r["fitness"]


_EYE = np.eye(4, dtype=np.float32)
_EDGES = {  # case -> (source points, target points, {method: the transform today's code ends with; None: an error, nothing recorded})
    "empty_target": (3000, 0, {_lib.P2P_SVD: _EYE, _lib.P2PLANE: _EYE, _lib.NDT: _EYE, _lib.GICP: _EYE}),
    "empty_source": (0, 3000, {_lib.P2P_SVD: _EDGE_GUESS, _lib.P2PLANE: _EDGE_GUESS, _lib.NDT: _EDGE_GUESS, _lib.GICP: _EYE}),
    "source_of_19": (19, 3000, {_lib.P2PLANE: "moved", _lib.GICP: _EYE}),      # below kGicpK: GICP refuses (PCL: converged_ = false, T = I);
    "target_of_19": (3000, 19, {_lib.P2PLANE: None, _lib.GICP: _EYE}),         # P2PLANE estimates the target's normals only: an argument error
}


@pytest.mark.parametrize("case,method", [(k, m) for k, v in _EDGES.items() for m in v[2]])
def test_edge_alignments_record_once_and_consistently(pair3k, case, method):
    n_s, n_t, ends = _EDGES[case]
    src, tgt = pair3k[0][:n_s], pair3k[1][:n_t]
    rec, counted, fit = _edge_align(method, src, tgt)
    assert counted == 1
    assert _edge_align(method, src, tgt) == (rec, counted, fit)
    want = ends[method]
    if want is None:
        assert rec == _lib.ERR_INVALID_ARG
        T = _EYE                                     # nothing was recorded: a fresh context's icpgpu_fitness uses the identity
    else:
        T = np.frombuffer(rec[0], np.float32).reshape(4, 4)
        if isinstance(want, str):
            assert rec[2] >= 1 and rec[0] != _EDGE_GUESS.tobytes()
        else:
            assert rec[0] == want.tobytes() and rec[2] == 0
    assert fit == np.float64(_fitness_at(src, tgt, T)).tobytes()


def test_batches_refuse_a_chain(built):
    pairs = [synth.make_pair(2000, 2000, seed=s)[:2] for s in (3, 4, 5)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    from icpslam_amd.sharding import COMM_HOST, align_batch_multi
    with Context(0) as ctx:
        before = ctx.align_batch(srcs, tgts)
        params = ctx.default_params()      # (explicit: the library's own contexts keep whatever parameters they were last given)
        multi_before = align_batch_multi([0], srcs, tgts, params=params, communicator=COMM_HOST)[0]
        for method in (_lib.P2P_SVD, _lib.GICP):
            ctx.set_params(method=method)
            ctx.set_correspondence_rejectors(CHAINS["trimmed"])
            with pytest.raises(IcpGpuError) as e:
                ctx.align_batch(srcs, tgts)
            assert e.value.code == _lib.ERR_UNSUPPORTED
        ctx.set_params(method=_lib.P2P_SVD)
        from icpslam_amd.sequence import run_odometry_batched
        with pytest.raises(IcpGpuError) as e:
            run_odometry_batched(ctx, srcs)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        # align_batch_multi runs on contexts of the library's own: a chain on this one does not reach it
        multi = align_batch_multi([0], srcs, tgts, params=params, communicator=COMM_HOST)[0]
        ctx.set_correspondence_rejectors([])
        after = ctx.align_batch(srcs, tgts)
    for a, b, m0, m1 in zip(before, after, multi_before, multi):
        assert a["T"].tobytes() == b["T"].tobytes() and (a["iterations"], a["n_corr"]) == (b["iterations"], b["n_corr"])
        assert m0["T"].tobytes() == m1["T"].tobytes() and (m0["iterations"], m0["n_corr"]) == (m1["iterations"], m1["n_corr"])


def test_setter_refusals_keep_the_chain(built):
    with Context(0) as ctx:
        ctx.set_correspondence_rejectors([(R.TRIMMED, 0.25, 7)])
        for bad in ([(0, 1.0)], [(9, 1.0)], [(R.MEDIAN, float("nan"))], [(R.MEDIAN, -1.0)], [(R.TRIMMED, 1.5)], [(R.TRIMMED, -0.5)],
                    [(R.ONE_TO_ONE,)] * 5):
            with pytest.raises(IcpGpuError) as e:
                ctx.set_correspondence_rejectors(bad)
            assert e.value.code == _lib.ERR_INVALID_ARG
            assert ctx.get_correspondence_rejectors() == [(R.TRIMMED, 0.25, 7)]


# ---- the callers that take a context --------------------------------------------------------------------------------------------
def test_run_odometry_with_a_chain(built):
    from icpslam_amd.sequence import run_odometry
    scene = synth.make_scene(5)
    scans = [synth.scan(scene, synth.pose_matrix(0.3 * k, 0.05 * k, 0.0, 0.0, 0.0, 0.01 * k), 3000, seed=50 + k) for k in range(5)]
    chain = [(R.MEDIAN, 2.0), (R.ONE_TO_ONE,)]
    with Context(0) as ctx:
        ctx.set_correspondence_rejectors(chain)
        _, records = run_odometry(ctx, scans)
    assert len(records) == 4
    target = scans[0]
    for rec, scan in zip(records, scans[1:]):
        ref = R.align(scan, target, chain)
        dR = float(np.abs(rec["T"][:3, :3] - ref["T"][:3, :3]).max())
        dt = float(np.linalg.norm(rec["T"][:3, 3] - ref["T"][:3, 3]))
        print(f"scan {rec['scan']}: iters {rec['iterations']}/{ref['iterations']} n_corr {rec['n_corr']}/{ref['n_corr']} dR {dR:.2e} dt {dt:.2e}")
        assert dR <= 1e-4 and dt <= 1e-3
        if rec["accepted"]:
            target = scan


def test_mirror_classes_on_the_device(built):
    src, tgt, _ = synth.make_pair(1500, 1500, seed=1)
    for cls, method in ((reg.IterativeClosestPoint, "p2p"), (reg.IterativeClosestPointWithNormals, "p2plane")):
        icp = cls()
        med = reg.CorrespondenceRejectorMedianDistance()
        med.setMedianFactor(2.0)
        icp.addCorrespondenceRejector(med)
        icp.addCorrespondenceRejector(reg.CorrespondenceRejectorOneToOne())
        assert len(icp.getCorrespondenceRejectors()) == 2
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        icp.align()
        ref = R.align(src, tgt, [(R.MEDIAN, 2.0), (R.ONE_TO_ONE,)], method=method)
        assert icp.result["n_corr"] == ref["n_corr"] and icp.result["iterations"] == ref["iterations"]
        assert np.float32(med.getMedianDistance()) == ref["stats"][0]["cut"]
        assert icp.removeCorrespondenceRejector(1) and not icp.removeCorrespondenceRejector(5)
        icp.clearCorrespondenceRejectors()
        plain = cls()
        plain.setInputSource(src)
        plain.setInputTarget(tgt)
        icp.align()
        a = icp.result
        plain.align()
        assert a["T"].tobytes() == plain.result["T"].tobytes()


def test_mapper_refine_with_a_chain(built):
    """OctreeMapper.refineTransformAndGrowMap takes a context: a chain set on it applies to its single alignment (point-to-point;
    the target is the map's nn cloud, where many scan points share a map point)."""
    from icpslam_amd.mapper import OctreeMapper, identity_pose
    scene = synth.make_scene(6)
    first = synth.scan(scene, synth.pose_matrix(0, 0, 0, 0, 0, 0), 8000, seed=70)
    second = synth.scan(scene, synth.pose_matrix(0.25, 0.05, 0.0, 0.0, 0.0, 0.01), 4000, seed=71)
    chain = [(R.ONE_TO_ONE,), (R.TRIMMED, 0.8)]
    with Context(0) as ctx:
        ctx.set_correspondence_rejectors(chain)
        mapper = OctreeMapper(ctx, method=_lib.P2P_SVD)
        ok, _, _, info = mapper.refineTransformAndGrowMap(first, identity_pose())
        assert not ok and info["seeded"]
        nn_cloud = mapper.approxNearestNeighbors(second, identity_pose())          # the target the alignment will run against
        ok, _, _, info = mapper.refineTransformAndGrowMap(second, identity_pose())
        stats = ctx.rejector_stats()
    got = info["icp"]
    ref = R.align(second, nn_cloud, chain, max_iterations=30)
    dR = float(np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max())
    dt = float(np.linalg.norm(got["T"][:3, 3] - ref["T"][:3, 3]))
    print(f"mapper: iters {got['iterations']}/{ref['iterations']} n_corr {got['n_corr']}/{ref['n_corr']} dR {dR:.2e} dt {dt:.2e}")
    assert len(stats) == 2 and stats[0]["pairs_out"] < stats[0]["pairs_in"]
    assert dR <= 1e-4 and dt <= 1e-3
