"""The sample-consensus rejector on the device (icp_reject_sac.hip, icpgpu_reject_sac.cpp) against tests/rsac_restated.py.  m,
sample_d2, moments9, the ranks, status, iterations, best_t, the counts, the kept set and best_T are compared bit for bit with the
restatement FED THE DEVICE'S OWN TRANSFORMS; the transforms themselves with float32(oracle.umeyama(sums)) to one ulp plus 1e-10 on
well-spread samples (scp_scenes.well_spread; at most 10 % of the evaluated hypotheses may be left out of that comparison), and EVERY evaluated hypothesis' transform with tests/solve_reference.py's float32 check on its own
sums."""
import ctypes as C
import functools

import numpy as np
import pytest

import reciprocal_restated as RCP
import rejectors_restated as RR
import rsac_restated as R
import rsac_scenes as S
import scp_scenes as SC
import solve_reference as SR
from icpslam_amd import Context, CorrespondenceRejectorSampleConsensus, IcpGpuError, IterativeClosestPoint, _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
SCALARS = ("m", "sample_d2", "iterations", "status", "best_t", "n_kept")
ARRAYS = ("moments9", "counts", "ranks", "best_T")


@pytest.fixture
def ctx(built):
    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def cases():
    return S.core_cases()


def call(ctx, P, Q, thr, it, seed, want_flags=True):
    """The call of its own over pair lists that name every row once: P_r = P[r], Q_r = Q[r]."""
    m = len(P)
    r = ctx.reject_sample_consensus(P if m else np.zeros((0, 4), F32), Q if m else np.zeros((0, 4), F32), np.arange(m), np.arange(m), thr, it, seed,
                                    want_flags)
    return r, ctx.rejector_sac_fetch()


def compare_core(f, want, what=""):
    for k in SCALARS:
        assert f[k] == want[k], (what, k, f[k], want[k])
    for k in ARRAYS:
        g, w = np.asarray(f[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, g[:4], w[:4])
    # validity: an INVALID hypothesis reads as zeros; the evaluated ones against the oracle's solve
    it = want["iterations"]
    assert f["transforms"].shape == (it, 4, 4)
    assert np.array_equal(np.any(f["transforms"] != 0, axis=(1, 2)), want["valid"]), what
    ev = np.flatnonzero(want["valid"])
    spread = np.array([SC.well_spread(want["sums17"][t]) for t in ev], bool)
    assert (~spread).sum() <= 0.1 * max(1, ev.size), (what, (~spread).sum(), ev.size)
    for t in ev[spread]:
        ref = want["solved"][t]
        tol = np.spacing(np.abs(ref)).astype(np.float64) + 1e-10
        assert (np.abs(f["transforms"][t].astype(np.float64) - ref.astype(np.float64)) <= tol).all(), (what, t, f["transforms"][t], ref)
    for t in ev:                                                # EVERY hypothesis, skinny samples included: a proper rotation that maximises the trace
        SR.check32(want["sums17"][t], f["transforms"][t])


def check_call(ctx, P, Q, thr, it, seed, what=""):
    r, f = call(ctx, P, Q, thr, it, seed)
    want = R.run(P, Q, thr, it, seed, transforms=f["transforms"])
    compare_core(f, want, what)
    assert np.array_equal(r["kept"], want["kept"]), what
    assert r["n_kept"] == want["n_kept"] and r["best_T"].tobytes() == want["best_T"].tobytes()
    assert f["host_waits"] == (0 if want["m"] == 0 else want["host_waits"] + 1), (what, f["host_waits"], want["batches"])
    return r, f, want


@pytest.mark.parametrize("name", sorted(S.core_cases()))
def test_core_cases(ctx, name):
    P, Q, thr, it, seed = cases()[name]
    r, f, want = check_call(ctx, P, Q, thr, it, seed, name)
    if name == "stops_in_batch_one":
        assert want["batches"] == 1 and f["host_waits"] == 4
    if name == "runs_to_200":
        assert f["iterations"] == 200 and want["batches"] == 4 and f["host_waits"] == 10
    if name in ("threshold_zero", "coincident", "m1", "m2", "it0", "all_nan_p"):
        assert f["status"] == 1 and r["kept"].all() and np.array_equal(r["best_T"], np.eye(4, dtype=F32))
    if name == "m0":
        assert f["status"] == 0 and r["n_kept"] == 0
    if name == "across_grid_cap":
        assert f["m"] > S.GRID_CAP_PAIRS and f["status"] == 3 and 0 < r["n_kept"] < f["m"]


def test_waits_without_the_flags_and_five_identical_runs(ctx):
    P, Q, thr, it, seed = cases()["runs_to_200"]
    first = None
    for _ in range(5):
        r, f = call(ctx, P, Q, thr, it, seed, want_flags=False)
        assert r["kept"] is None and f["host_waits"] == 1 + 2 * 4
        rec = tuple(np.asarray(f[k]).tobytes() for k in ARRAYS + ("transforms",)) + tuple(f[k] for k in SCALARS)
        first = first or rec
        assert rec == first
    r2, _ = call(ctx, P, Q, thr, it, seed)
    assert r2["n_kept"] == r["n_kept"] and int(r2["kept"].sum()) == r["n_kept"]


def test_repeated_query_indices_and_index_lists(ctx):
    """Pairs are judged one by one: a source point paired with several targets keeps exactly the pairs that fit."""
    P, Q = S.pairs(200, 1.0, 8)
    rng = np.random.default_rng(3)
    iq = np.concatenate([np.arange(200), np.arange(50), np.arange(50)]).astype(np.int32)
    im = np.concatenate([np.arange(200), rng.integers(0, 200, 50), np.arange(50)]).astype(np.int32)
    r = ctx.reject_sample_consensus(P, Q, iq, im, 0.05, 100, 3)
    f = ctx.rejector_sac_fetch()
    want = R.reject(P, Q, iq, im, 0.05, 100, 3, transforms=f["transforms"])
    compare_core(f, want)
    assert np.array_equal(r["kept"], want["kept"]) and r["kept"][:200].all() and r["kept"][250:].all() and not r["kept"][200:250].all()


def raw_call(ctx, src, n_s, tgt, n_t, iq, im, n, thr, it, n_kept="own", T="own", kept=None):
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    nk, Tb = C.c_size_t(99), (C.c_float * 16)()
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return ctx._L.icpgpu_correspondence_rejector_sample_consensus(ctx._h, p(src, fp), n_s, p(tgt, fp), n_t, p(iq, ip), p(im, ip), n, thr, it, 1, kept,
                                                                  C.byref(nk) if n_kept == "own" else None, Tb if T == "own" else None)


def test_refusals_drop_the_previous_result(ctx):
    P, Q = (np.ascontiguousarray(a) for a in S.pairs(20, 0.6, 1))
    iq = np.arange(20, dtype=np.int32)
    good = dict(src=P, n_s=20, tgt=Q, n_t=20, iq=iq, im=iq, n=20, thr=0.05, it=10)
    bad_q, bad_m, neg = iq.copy(), iq.copy(), iq.copy()
    bad_q[7], bad_m[19], neg[0] = 20, 20, -1
    refusals = [dict(iq=bad_q), dict(im=bad_m), dict(iq=neg), dict(im=neg), dict(src=None), dict(tgt=None), dict(iq=None), dict(im=None),
                dict(thr=-0.1), dict(thr=float("nan")), dict(thr=float("inf")), dict(it=-1), dict(it=_lib.RSAC_MAX_ITERATIONS + 1),
                dict(n_kept=None), dict(T=None), dict(n_s=5), dict(n_t=19)]
    for change in refusals:
        assert raw_call(ctx, **good) == 0
        assert ctx.rejector_sac_fetch(per_hypothesis=False)["m"] == 20
        assert raw_call(ctx, **{**good, **change}) == _lib.ERR_INVALID_ARG, change
        with pytest.raises(IcpGpuError):
            ctx.rejector_sac_fetch()
    assert raw_call(ctx, None, 0, None, 0, None, None, 0, 0.05, 10) == 0           # nothing at all is no refusal: status 0
    f = ctx.rejector_sac_fetch()
    assert (f["m"], f["status"], f["host_waits"], f["iterations"]) == (0, 0, 0, 0)


def test_fetch_capacities_and_null_outputs(ctx):
    P, Q, thr, it, seed = cases()["it65"]
    call(ctx, P, Q, thr, it, seed)
    L, h = ctx._L, ctx._h
    ip = C.POINTER(C.c_int32)
    n = C.c_int32(0)
    assert L.icpgpu_rejector_sac_fetch(h, 0, None, None, None, C.byref(n), None, None, None, None, None, None, None, None) == 0 and n.value == 65
    assert L.icpgpu_rejector_sac_fetch(h, 0, None, None, None, None, None, None, None, None, None, None, None, None) == 0
    counts = np.full(65, 77, np.int32)
    for cap in (0, 64):
        assert L.icpgpu_rejector_sac_fetch(h, cap, None, None, None, None, None, counts.ctypes.data_as(ip), None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
        assert (counts == 77).all()
    assert L.icpgpu_rejector_sac_fetch(h, 65, None, None, None, None, None, counts.ctypes.data_as(ip), None, None, None, None, None, None) == 0
    assert np.array_equal(counts, ctx.rejector_sac_fetch()["counts"])
    with Context(0) as fresh:
        with pytest.raises(IcpGpuError):
            fresh.rejector_sac_fetch()


# ---- the stage inside the chain ------------------------------------------------------------------------------------------------
STAGE = (R.KIND, *S.BLOCK_STAGE)


def check_chain(ctx, src, tgt, T, max_dist, chain, reciprocal=False, seed=R.DEFAULT_SEED):
    ctx.set_correspondence_rejectors(chain)
    ctx.set_reciprocal_correspondences(reciprocal)
    idx, d2 = ctx.correspondences(T)
    f = ctx.rejector_sac_fetch()
    nn = None
    if reciprocal:
        i0, d0, kept, _ = RCP.reciprocal(src, tgt, T, max_dist)
        nn = (np.where(kept, i0, -1), d0)
    widx, wd2, wstats, rec = R.correspondences(src, tgt, T, max_dist, chain, seed, nn=nn, transforms=f["transforms"])
    compare_core(f, rec, str(chain))
    assert np.array_equal(idx, widx) and d2.tobytes() == wd2.tobytes(), chain
    stats = ctx.rejector_stats()
    assert len(stats) == len(chain)
    for got, want, st in zip(stats, wstats, chain):
        assert (got["pairs_in"], got["pairs_out"]) == (want["pairs_in"], want["pairs_out"]), (chain, got, want)
        if int(st[0]) == R.KIND:
            assert got["cut"] == 0.0
    assert f["host_waits"] == rec["host_waits"] == 1 + 2 * rec["batches"]
    return f, rec, stats


@pytest.mark.parametrize("method", [_lib.P2P_SVD, _lib.P2PLANE])
def test_stage_in_the_chain(ctx, method):
    src, tgt, truth, block = S.moved_block()
    ctx.set_params(method=method, max_correspondence_distance=1.0)
    ctx.set_source(src)
    ctx.set_target(tgt)
    T = np.eye(4)
    f, rec, stats = check_chain(ctx, src, tgt, T, 1.0, [STAGE])
    assert f["status"] == 3 and stats[0]["pairs_out"] < stats[0]["pairs_in"] == 3000
    check_chain(ctx, src, tgt, T, 1.0, [(RR.MEDIAN, 2.0), STAGE])
    check_chain(ctx, src, tgt, T, 1.0, [STAGE, (RR.ONE_TO_ONE,)])
    check_chain(ctx, src, tgt, T, 1.0, [(RR.TRIMMED, 0.9), STAGE, (RR.ONE_TO_ONE,), (RR.MEDIAN, 3.0)])
    check_chain(ctx, src, tgt, T, 1.0, [STAGE], reciprocal=True)
    check_chain(ctx, src, tgt, SC.rigid(0.02, 0, 0, (0.05, 0, 0)), 1.0, [(R.KIND, 0.1, 1)])      # a single hypothesis
    ctx.set_params(method=method, max_correspondence_distance=1e-5)
    f, _, _ = check_chain(ctx, src, tgt, T, 1e-5, [STAGE])                                        # the gate leaves nothing: m = 0, one wait
    assert (f["m"], f["status"], f["host_waits"]) == (0, 0, 1)
    ctx.set_reciprocal_correspondences(False)


def test_stage_with_an_empty_cloud_waits_nowhere(ctx):
    src, tgt, _, _ = S.moved_block()
    ctx.set_source(src)
    ctx.set_target(np.zeros((0, 4), F32))
    ctx.set_correspondence_rejectors([STAGE])
    idx, _ = ctx.correspondences(np.eye(4))
    f = ctx.rejector_sac_fetch()
    assert (idx == -1).all() and (f["m"], f["status"], f["host_waits"]) == (0, 0, 0)
    assert ctx.rejector_stats()[0]["pairs_in"] == 0


def test_one_icp_iteration_is_the_correspondences_call(ctx):
    src, tgt, _, _ = S.moved_block()
    G = SC.rigid(0.005, 0, 0, (0.05, -0.03, 0.0))
    for method in (_lib.P2P_SVD, _lib.P2PLANE):
        ctx.set_params(method=method, max_correspondence_distance=1.0, max_iterations=1)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_correspondence_rejectors([(RR.MEDIAN, 2.0), STAGE])
        r = ctx.align(guess=G)
        a, sa = ctx.rejector_sac_fetch(), ctx.rejector_stats()
        ctx.correspondences(G)
        b, sb = ctx.rejector_sac_fetch(), ctx.rejector_stats()
        for k in SCALARS + ("host_waits",):
            assert a[k] == b[k], k
        for k in ARRAYS + ("transforms",):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        assert r["iterations"] == 1 and r["n_corr"] == sa[1]["pairs_out"] == sb[1]["pairs_out"] == a["n_kept"]


_COUNTERS = ("nn_launches", "reduce_launches", "grid_launches", "transform_launches", "iterations", "aligns", "grid_builds")


def test_a_chain_without_the_stage_is_untouched_by_one_with_it(built):
    """The counters and the bits of a MEDIAN + ONE_TO_ONE alignment are the same on a fresh context and on one that ran the stage
    before; and that alignment leaves the stage's last result alone."""
    src, tgt, _, _ = S.moved_block()
    plain = [(RR.MEDIAN, 2.0), (RR.ONE_TO_ONE,)]

    def run(before):
        with Context(0) as c:
            c.set_params(max_correspondence_distance=1.0, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            kept = None
            if before:
                c.set_correspondence_rejectors([STAGE] + plain)
                c.align()
                kept = c.rejector_sac_fetch()
            c.set_correspondence_rejectors(plain)
            c.profile_reset()
            r = c.align(want_fitness=True)
            p = c.profile()
            if before:
                after = c.rejector_sac_fetch()
                assert all(np.asarray(kept[k]).tobytes() == np.asarray(after[k]).tobytes() for k in ARRAYS + ("transforms",))
            return r["T"].tobytes(), r["iterations"], r["n_corr"], np.float64(r["fitness"]).tobytes(), tuple(getattr(p, k) for k in _COUNTERS), c.rejector_stats()

    assert run(False) == run(True)


def test_the_seed_setter_changes_the_draws(ctx):
    src, tgt, _, _ = S.moved_block()
    assert ctx.get_rejector_sac_seed() == 12345 == R.DEFAULT_SEED
    ctx.set_params(max_correspondence_distance=1.0)
    ctx.set_source(src)
    ctx.set_target(tgt)
    a, _, _ = check_chain(ctx, src, tgt, np.eye(4), 1.0, [STAGE])
    ctx.set_rejector_sac_seed(2 ** 64 - 3)
    assert ctx.get_rejector_sac_seed() == 2 ** 64 - 3
    b, _, _ = check_chain(ctx, src, tgt, np.eye(4), 1.0, [STAGE], seed=2 ** 64 - 3)
    assert not np.array_equal(a["ranks"][:4], b["ranks"][:4])
    with pytest.raises(IcpGpuError):
        ctx.set_correspondence_rejectors([(R.KIND, -0.1, 10)])
    with pytest.raises(IcpGpuError):
        ctx.set_correspondence_rejectors([(R.KIND, 0.1, _lib.RSAC_MAX_ITERATIONS + 1)])
    with pytest.raises(IcpGpuError):
        ctx.set_correspondence_rejectors([(R.KIND, 0.1, -1)])
    with pytest.raises(IcpGpuError):
        ctx.set_correspondence_rejectors([(R.KIND, 0.1, 0)])              # a stage of no hypotheses is refused (the call takes 0)
    with pytest.raises(IcpGpuError):
        ctx.set_correspondence_rejectors([(R.KIND, 0.5)])
    assert ctx.get_correspondence_rejectors() == [(R.KIND, S.BLOCK_STAGE[0], S.BLOCK_STAGE[1])]


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.BLOCK_SEEDS)
def test_moved_block_icp_ends_at_the_truth(built, seed):
    """A quarter of the source sits 0.5 m off in the target: ICP with the stage ends within twice the restatement's worst error
    (tests/test_rsac_host.py), and far closer than the gate alone."""
    src, tgt, truth, _ = S.moved_block()
    errs = []
    for chain in ([], [S.BLOCK_STAGE]):
        icp = IterativeClosestPoint()
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        icp.setMaximumIterations(S.BLOCK_KW["max_iterations"])
        icp.setMaxCorrespondenceDistance(S.BLOCK_KW["max_correspondence_distance"])
        icp.setTransformationEpsilon(S.BLOCK_KW["transformation_epsilon"])
        rej = None
        for thr, it in chain:
            rej = CorrespondenceRejectorSampleConsensus()
            rej.setInlierThreshold(thr)
            rej.setMaximumIterations(it)
            icp.addCorrespondenceRejector(rej)
        icp._ctx.set_rejector_sac_seed(seed)
        icp.align()
        errs.append(SC.pose_error(icp.getFinalTransformation(), truth))
        if rej is not None:
            assert np.array_equal(rej.getBestTransformation(), icp._ctx.rejector_sac_fetch(per_hypothesis=False)["best_T"])
            assert not np.array_equal(rej.getBestTransformation(), np.eye(4, dtype=F32))
    print(f"seed {seed}: gate alone {errs[0]}, with the stage {errs[1]}")
    assert errs[1][0] <= S.E2E_BOUND[0] and errs[1][1] <= S.E2E_BOUND[1]
    assert errs[1][1] < 0.1 * errs[0][1]


@pytest.mark.parametrize("seed", S.MATCH_SEEDS)
def test_descriptor_matches_through_the_call(ctx, seed):
    """FPFH -> icpgpu_feature_knn(k = 1) -> the call: best_T within rsac_scenes.MATCH_BOUND of the truth."""
    source, target, truth = SC.e2e_clouds()
    feats = []
    for cloud in (source, target):
        ctx.search_set_input(cloud)
        feats.append(ctx.fpfh_estimation(ctx.normal_estimation(None, k=SC.E2E_NORMAL_K)[0], None, radius=SC.E2E_FPFH_RADIUS)[0])
    idx, _, found = ctx.feature_knn(feats[1], feats[0], 1)
    ok = found > 0
    rej = CorrespondenceRejectorSampleConsensus(ctx)
    rej.setInputSource(source)
    rej.setInputTarget(target)
    rej.setInlierThreshold(S.MATCH_KW["inlier_threshold"])
    rej.setMaximumIterations(S.MATCH_KW["max_iterations"])
    rej._seed = seed
    rej.setInputCorrespondences(np.flatnonzero(ok), idx[ok, 0])
    q, m = rej.getRemainingCorrespondences()
    rot, trans = SC.pose_error(rej.getBestTransformation(), truth)
    print(f"seed {seed}: {rot:.4f} degrees, {trans:.3g} m, {q.size} of {int(ok.sum())} pairs stay")
    assert rot <= S.MATCH_BOUND[0] and trans <= S.MATCH_BOUND[1] and q.size > 200 and (q == m).mean() > 0.95
