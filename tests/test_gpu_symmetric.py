"""The symmetric point-to-plane objective on the device (icp_p2plane.hip: p2plane_sym_reduce_kernel; icpgpu_p2plane.cpp) against
its NumPy restatement (tests/symmetric_restated.py), never against the library itself.

reduction: ctx.nn's keys (pinned elsewhere) are taken from the device and the 29 sums restated from them: count and sum d2 exact,
           every other sum within 1e-12 * sum |terms| of the exact sum -- the project's P2PLANE bound (a fixed-order float64 tree
           over at most 2^21 terms: at most 30 roundings of 2^-53 each per sum).  sum d2 is exact BY CONSTRUCTION of the case: every
           d2 lies in [2^-10, 1), so every float32 term is a multiple of 2^-33, and fewer than 2^20 terms below 1 sum to less than
           2^20 -- 53 bits hold every partial sum whatever the order.
whole:     ctx.align against the restated loop: iterations, state and n_correspondences equal, T within BASELINE's tolerance
           (1e-4 max-abs R, 1e-3 m)."""
import os
import re

import numpy as np
import pytest

import oracle
import symmetric_restated as S
from icpslam_amd import GICP, NDT, P2PLANE, Context, IcpGpuError, _lib, synth

pytestmark = pytest.mark.gpu
F = np.float32
R_TOL, T_TOL = 1e-4, 1e-3                                          # BASELINE.json / DESIGN.md section 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rows_f", "symmetric_1k5.npz")
T_MOVE = synth.pose_matrix(0.4, -0.25, 0.1, 0.02, -0.015, 0.03).astype(F)
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)


def stride_points():
    """points one trip of the capped grid covers: 4 x block x block cap, from the kernel's own constants"""
    text = open(os.path.join(ROOT, "icpslam_amd", "csrc", "icp_p2plane.hip")).read()
    block = int(re.search(r"constexpr int PP_BLOCK = (\d+);", text).group(1))
    cap = int(re.search(r"constexpr int kP2planeMaxBlocks = (\d+);", text).group(1))
    return 4 * block * cap


def unit(rng, n):
    v = rng.normal(size=(n, 4)).astype(F)
    v[:, :3] /= np.linalg.norm(v[:, :3], axis=1, keepdims=True)
    v[:, 3] = 0
    return v


@pytest.fixture(scope="module")
def target2k(built):
    return sparse_target()


def sparse_target():
    """2197 points, one per node of a 2 m lattice, each moved by up to 0.2 m per axis: a point within 0.5 m of one of them is more
    than a metre from every other, so its pair and its d2 are known by construction"""
    rng = np.random.default_rng(41)
    g = np.arange(13, dtype=np.float64) * 2.0 - 12.0
    xx, yy, zz = np.meshgrid(g, g, g, indexing="ij")
    tgt = np.ones((xx.size, 4), F)
    tgt[:, :3] = (np.column_stack([xx.ravel(), yy.ravel(), zz.ravel()]) + rng.uniform(-0.2, 0.2, (xx.size, 3))).astype(F)
    tgt.setflags(write=False)
    return tgt


def source_around(tgt, n, seed, T):
    """n points whose images under T lie 0.05 .. 0.5 m beside target points: d2 in [2^-10, 1) (checked by the caller)"""
    rng = np.random.default_rng(seed)
    off = unit(rng, n)[:, :3].astype(np.float64) * rng.uniform(0.05, 0.5, (n, 1))
    at = tgt[rng.integers(0, tgt.shape[0], n), :3].astype(np.float64) + off
    Ti = np.linalg.inv(np.asarray(T, np.float64))
    src = np.ones((n, 4), F)
    src[:, :3] = (at @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    return src


def check_sums(ctx, src, tgt, sn, tn, T, enforce, max_dist=1.0, d2_exact=True):
    idx, d2 = ctx.nn(T)
    got = ctx.reduce_symmetric_point_to_plane(T, max_dist, enforce)
    want, mag = S.sums(src, tgt, sn, tn, T, idx, d2, max_dist, enforce, want_abs=True)
    assert got[0] == want[0]
    if d2_exact:
        alive = d2[(idx >= 0) & (d2.astype(np.float64) <= max_dist * max_dist)]
        assert alive.size == 0 or (alive.min() >= F(2.0 ** -10) and alive.max() < 1.0 and alive.size < 2 ** 20 + 2)
        assert got[1] == want[1], (got[1], want[1])
    err = np.abs(got - want)
    assert np.all(err[2:] <= 1e-12 * mag[2:]), (err[2:] / np.maximum(mag[2:], 1e-300)).max()
    return got


@pytest.mark.parametrize("n_s", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, "stride+1"])
def test_reduction_sizes(target2k, n_s):
    n_s = stride_points() + 1 if n_s == "stride+1" else n_s
    if n_s > 4097:
        assert n_s == 1048577 and -(-n_s // stride_points()) == 2     # the parent's constants: the stride loop runs twice
    tgt = target2k
    rng = np.random.default_rng(n_s)
    src = source_around(tgt, n_s, 100 + n_s % 1000, T_MOVE)
    sn, tn = unit(rng, n_s), unit(rng, tgt.shape[0])
    with Context(0) as ctx:
        ctx.set_params(method=P2PLANE)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_source_normals(sn)
        ctx.set_target_normals(tn)
        a = check_sums(ctx, src, tgt, sn, tn, T_MOVE, True)
        assert a[0] == n_s                                             # (every pair is within the gate by construction)
        if n_s > 4097:                                                 # (one restatement of a million pairs is seconds of NumPy)
            return
        b = check_sums(ctx, src, tgt, sn, tn, T_MOVE, False)
        if n_s >= 63:
            assert not np.array_equal(a[2:], b[2:])                    # random normals: `enforce` flips about half of the pairs
        if 63 <= n_s <= 4097:                                          # estimated normals (GICP's plane) on both clouds
            ctx.set_source(src)                                        # (replacing the clouds drops the supplied normals)
            ctx.set_target(tgt.copy())
            es, et = ctx.normals(of_target=False), ctx.normals(of_target=True)
            assert np.isfinite(es[:, :3]).all(axis=1).sum() > n_s // 2 and not np.array_equal(es, sn)   # (pinned to the oracle elsewhere)
            for enforce in (True, False):
                check_sums(ctx, src, tgt, es, et, T_MOVE, enforce)
            check_sums(ctx, src, tgt, es, et, np.eye(4, dtype=F), True, d2_exact=False)


def test_reduction_needs_normals_for_small_clouds(target2k):
    with Context(0) as ctx:
        ctx.set_params(method=P2PLANE)
        ctx.set_source(source_around(target2k, 19, 1, np.eye(4)))
        ctx.set_target(target2k)
        ctx.nn(np.eye(4))
        with pytest.raises(IcpGpuError) as e:
            ctx.reduce_symmetric_point_to_plane(np.eye(4), 1.0)
        assert e.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(IcpGpuError) as e:
            ctx.set_source_normals(np.zeros((18, 4), F))
        assert e.value.code == _lib.ERR_INVALID_ARG
    with Context(0) as ctx:
        with pytest.raises(IcpGpuError) as e:
            ctx.set_source_normals(np.zeros((18, 4), F))
        assert e.value.code == _lib.ERR_NO_INPUT


# ---- whole alignments ---------------------------------------------------------------------------------------------------------------
def whole(got, ref):
    assert (got["converged"], got["iterations"], got["state"], got["n_corr"]) == \
        (ref["converged"], ref["iterations"], ref["state"], ref["n_corr"]), (got, {k: ref[k] for k in ("converged", "iterations", "state", "n_corr")})
    dR = float(np.abs(got["T"][:3, :3].astype(np.float64) - ref["T"][:3, :3]).max())
    dt = float(np.linalg.norm(got["T"][:3, 3].astype(np.float64) - ref["T"][:3, 3]))
    assert dR <= R_TOL and dt <= T_TOL, (dR, dt)


def run(src, tgt, sn=None, tn=None, guess=None, enforce=True, chain=(), **kw):
    with Context(0) as ctx:
        ctx.set_params(method=P2PLANE, **kw)
        ctx.set_source(src)
        ctx.set_target(tgt)
        if sn is not None:
            ctx.set_source_normals(sn)
        if tn is not None:
            ctx.set_target_normals(tn)
        ctx.set_p2plane_symmetric(True, enforce)
        assert ctx.get_p2plane_symmetric() == (True, enforce)
        ctx.set_correspondence_rejectors(chain)
        return ctx.align(guess=guess)


CASES = {3000: 61, 6000: 62}                                           # size -> seed (decisions_clear holds: checked below)


@pytest.mark.parametrize("n", sorted(CASES))
def test_whole_alignments_both_nn_modes(built, n):
    src, tgt, _ = synth.make_pair(n, n, seed=CASES[n])
    sn, tn = oracle.gicp_normals(src), oracle.gicp_normals(tgt)
    if n == 6000:                                                      # supplied, not unit length, some flipped, some NaN
        sn, tn = sn.copy(), tn.copy()
        sn[::7, :3] *= F(1.5)
        tn[::5, :3] *= F(-1.0)
        tn[::11, 1] = np.nan
    ref = S.align(src, tgt, sn, tn)
    assert S.decisions_clear(ref) and ref["iterations"] > 2
    supplied = n == 6000
    runs = [run(src, tgt, sn if supplied else None, tn if supplied else None, nn_mode=m) for m in (_lib.NN_BRUTE, _lib.NN_GRID)]
    for got in runs:
        whole(got, ref)
    assert runs[0]["T"].tobytes() == runs[1]["T"].tobytes() and runs[0]["mse"] == runs[1]["mse"]


def test_enforce_off_differs_and_matches(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=61)
    sn, tn = oracle.gicp_normals(src), oracle.gicp_normals(tgt).copy()
    tn[::2, :3] *= F(-1.0)                                             # half of the target's normals point the other way
    ref_on, ref_off = S.align(src, tgt, sn, tn, enforce=True), S.align(src, tgt, sn, tn, enforce=False)
    assert S.decisions_clear(ref_on) and S.decisions_clear(ref_off)
    whole(run(src, tgt, sn, tn, enforce=True), ref_on)
    whole(run(src, tgt, sn, tn, enforce=False), ref_off)
    assert not np.array_equal(ref_on["T"], ref_off["T"])


def test_fixture_with_a_guess(built):
    g = np.load(GOLDEN)
    got = run(g["src"], g["tgt"], guess=g["guess"])                    # estimated normals: bit for bit the fixture's
    assert (got["iterations"], got["state"], got["n_corr"]) == (int(g["plain_iterations"]), int(g["plain_state"]), int(g["plain_n_corr"]))
    assert np.abs(got["T"][:3, :3] - g["plain_T"][:3, :3]).max() <= R_TOL and np.linalg.norm(got["T"][:3, 3] - g["plain_T"][:3, 3]) <= T_TOL
    got = run(g["src"], g["tgt"], g["src_nrm"], g["tgt_nrm"], guess=g["guess"], chain=((S.SURFACE_NORMAL, 0.5),))
    assert (got["iterations"], got["state"], got["n_corr"]) == (int(g["rej_iterations"]), int(g["rej_state"]), int(g["rej_n_corr"]))
    assert np.abs(got["T"][:3, :3] - g["rej_T"][:3, :3]).max() <= R_TOL and np.linalg.norm(got["T"][:3, 3] - g["rej_T"][:3, 3]) <= T_TOL


# ---- degenerate inputs --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair3k(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=61)
    return src, tgt, oracle.gicp_normals(src), oracle.gicp_normals(tgt)


def test_source_with_non_finite_points(pair3k):
    src, tgt, sn, tn = pair3k
    src = src.copy()
    src[::97, 1] = np.nan
    src[5::101, 0] = np.inf
    ref = S.align(src, tgt, sn, tn)
    assert S.decisions_clear(ref) and ref["iterations"] > 1
    whole(run(src, tgt, sn, tn), ref)


@pytest.mark.parametrize("with_guess", [False, True])
def test_all_source_normals_nan_is_singular(pair3k, with_guess):
    src, tgt, sn, tn = pair3k
    guess = synth.pose_matrix(0.1, 0.0, 0.0, 0.0, 0.0, 0.02).astype(F) if with_guess else None
    got = run(src, tgt, np.full_like(sn, np.nan), tn, guess=guess)
    assert (got["state"], got["iterations"], got["converged"]) == (NOT_CONVERGED, 0, False)
    assert got["n_corr"] > 1000                                        # the pairs stay correspondences
    assert np.array_equal(got["T"], np.eye(4, dtype=F) if guess is None else guess)


def test_target_normals_nan_on_half_the_points(pair3k):
    src, tgt, sn, tn = pair3k
    tn = tn.copy()
    tn[::2, 2] = np.nan
    ref = S.align(src, tgt, sn, tn)
    assert S.decisions_clear(ref) and ref["iterations"] > 1
    got = run(src, tgt, sn, tn)
    whole(got, ref)


def test_empty_target(pair3k):
    src, _, sn, _ = pair3k
    got = run(src, np.zeros((0, 4), F), sn, None, guess=T_MOVE)
    assert (got["converged"], got["iterations"], got["state"], got["n_corr"]) == (False, 0, NOT_CONVERGED, 0)
    assert np.array_equal(got["T"], np.eye(4, dtype=F))                # PCL: align() without a target leaves T = identity


def test_min_correspondences_at_its_boundary(pair3k):
    src, tgt, sn, tn = pair3k
    n0 = S.align(src, tgt, sn, tn, max_iterations=1)["trace"][0]["n_corr"]
    got = run(src, tgt, sn, tn, min_correspondences=n0, max_iterations=2)
    assert got["iterations"] >= 1
    got = run(src, tgt, sn, tn, min_correspondences=n0 + 1)
    assert (got["state"], got["iterations"], got["n_corr"]) == (NO_CORRESPONDENCES, 0, n0)


# ---- the flag off, and who ignores it -----------------------------------------------------------------------------------------------
def counters(ctx):
    """every integer field of the profile (launches, bytes, builds, ...): the timings are the only fields left out -- the *_ms
    sums and the *_timed counts of the sweeps the context chose to time (one in 13 of all it has ever issued)"""
    import ctypes as C
    p = ctx.profile()
    return {name: getattr(p, name) for name, kind in _lib.Profile._fields_ if kind is C.c_uint64 and not name.endswith("_timed")}


def test_flag_off_is_the_parent(pair3k):
    """toggle on, align, toggle off: a P2PLANE alignment returns a fresh context's bits and launches what a context that has run one
    plain alignment launches for its next one (both hold the clouds' grid and normals by then)"""
    src, tgt, _, _ = pair3k

    def plain(ctx):
        ctx.profile_reset()
        return ctx.align(want_cloud=True, want_fitness=True), counters(ctx)

    with Context(0) as fresh:
        fresh.set_params(method=P2PLANE)
        fresh.set_source(src)
        fresh.set_target(tgt)
        want, _ = plain(fresh)
        _, want_prof = plain(fresh)
    with Context(0) as ctx:
        ctx.set_params(method=P2PLANE)
        ctx.set_source(src)
        ctx.set_target(tgt)
        ctx.set_p2plane_symmetric(True, False)
        sym = ctx.align()
        ctx.set_p2plane_symmetric(False, True)
        assert ctx.get_p2plane_symmetric() == (False, True)
        got, got_prof = plain(ctx)
    assert not np.array_equal(sym["T"], want["T"])
    for k in ("T", "cloud"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in ("iterations", "n_corr", "converged", "state", "mse", "fitness"):
        assert got[k] == want[k], k
    assert got_prof == want_prof and got_prof["reduce_launches"] == got["iterations"] + 1      # (+ the fitness sweep)


def test_reduce_bytes_count_the_source_normals(pair3k):
    src, tgt, sn, tn = pair3k
    per = {}
    for on in (False, True):
        with Context(0) as ctx:
            ctx.set_params(method=P2PLANE, max_iterations=1)
            ctx.set_source(src)
            ctx.set_target(tgt)
            ctx.set_source_normals(sn)
            ctx.set_target_normals(tn)
            ctx.set_p2plane_symmetric(on)
            ctx.profile_reset()
            ctx.align()
            p = ctx.profile()
            per[on] = (p.reduce_bytes, p.reduce_launches)
    assert per[False][1] == per[True][1] == 1
    assert per[True][0] - per[False][0] == 16 * src.shape[0]            # 72 B against 56 B per pair


def test_batches_refuse_the_flag(pair3k):
    src, tgt, _, _ = pair3k
    with Context(0) as ctx:
        ctx.set_p2plane_symmetric(True)
        with pytest.raises(IcpGpuError) as e:
            ctx.align_batch([src], [tgt])
        assert e.value.code == _lib.ERR_UNSUPPORTED
        ctx.set_p2plane_symmetric(False)
        assert len(ctx.align_batch([src], [tgt])) == 1


@pytest.mark.parametrize("method", [GICP, NDT, _lib.P2P_SVD])
def test_other_methods_ignore_the_flag(pair3k, method):
    src, tgt, _, _ = pair3k
    out = []
    for on in (False, True):
        with Context(0) as ctx:
            ctx.set_params(method=method, max_iterations=8)
            ctx.set_source(src)
            ctx.set_target(tgt)
            ctx.set_p2plane_symmetric(on, not on)
            out.append(ctx.align(want_cloud=True, want_fitness=True))
    for k in ("T", "cloud"):
        assert out[0][k].tobytes() == out[1][k].tobytes(), k
    for k in ("iterations", "n_corr", "converged", "fitness", "mse"):
        assert np.float64(out[0][k]).tobytes() == np.float64(out[1][k]).tobytes(), k
