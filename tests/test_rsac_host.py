"""The sample-consensus rejector's rule on the CPU (include/icpgpu.h, "sample-consensus rejector"): tests/rsac_restated.py against its
own literal loop, the generator, the edges of every comparison, the loop, the library's ABI, and the end-to-end scene's bound.

END TO END.  The moved-block scene (rsac_scenes.moved_block: 3000 points, a quarter of them displaced by 0.5 m in the target),
point-to-point ICP from the identity, gate 1 m.  Measured with the restatement (rotation error in degrees, translation error in m):
    the gate alone                                  0.309 deg   0.0902 m
    with the stage (0.1 m, 200 iterations), seed 12345   0.016 deg   0.0026 m
                                            seed 1       0.000 deg   0.0010 m
                                            seed 2       0.000 deg   0.0010 m
The device test's bound is twice the restatement's worst over the three seeds (test_scp_host.py's pattern): rsac_scenes.E2E_BOUND.

COLLINEAR P.  Under the rule as stated a collinear sample is a good draw whenever its points are spaced (PCL's isSampleGood accepts
it too) and the Umeyama solve of three collinear pairs is finite, so on a collinear cloud hypotheses are evaluated; only coincident
P makes every hypothesis INVALID.  Both keep every pair of a rigid image, which is what is asserted."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rsac_restated as R
import rsac_scenes as S
import scp_scenes as SC
from icpslam_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = np.float32, np.float64
SYMBOLS = ("icpgpu_set_rejector_sac_seed", "icpgpu_get_rejector_sac_seed", "icpgpu_correspondence_rejector_sample_consensus",
           "icpgpu_rejector_sac_fetch")


def same(a, b):
    for k in ("m", "sample_d2", "iterations", "status", "best_t", "n_kept"):
        assert a[k] == b[k], k
    for k in ("moments9", "counts", "ranks", "kept", "best_T"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["transforms"][:a["iterations"]].view(np.uint32), b["transforms"].view(np.uint32))


@pytest.mark.parametrize("m", [0, 1, 2, 3, 4, 40])
def test_restatement_equals_the_literal_loop(built, m):
    P, Q = S.pairs(m, 0.6, 1)
    same(R.run(P, Q, 0.05, 100, 7), R.run_literal(P, Q, 0.05, 100, 7))


def test_restatement_equals_the_literal_loop_on_nan_rows_and_duplicates(built):
    P, Q = S.with_nan_rows(*S.pairs(30, 0.6, 5))
    same(R.run(P, Q, 0.05, 70, 3), R.run_literal(P, Q, 0.05, 70, 3))
    P, Q = S.with_duplicates(*S.pairs(12, 0.6, 6))
    same(R.run(P, Q, 0.05, 70, 3), R.run_literal(P, Q, 0.05, 70, 3))


def test_generator_against_python_integers():
    for seed, m in ((0, 3), (12345, 1000), (2 ** 64 - 1, 2 ** 31 - 5000), (7, 65)):
        got = R.ranks_of(seed, 65500, 36, m)
        for e, t in enumerate(range(65500, 65536)):
            for d in range(R.DRAWS):
                assert [R.rank_int(seed, t, d, c, m) for c in range(3)] == got[e, d].tolist()


def test_redraws_take_the_first_good_draw(built):
    P, Q = S.with_nan_rows(*S.pairs(12, 0.6, 5), seed=2)
    P[::2, 0] = np.nan                                     # half of the pairs can not be sampled: most first draws are bad
    r = R.run(P, Q, 0.05, 64, 5)
    fin = np.isfinite(P[:, :3]).all(axis=1) & np.isfinite(Q[:, :3]).all(axis=1)
    later = 0
    for t in range(r["iterations"]):
        first = -1
        for d in range(R.DRAWS):
            k = [R.rank_int(5, t, d, c, 12) for c in range(3)]
            if len(set(k)) == 3 and fin[k].all() and all(float(SC_d2(P[k[a]], P[k[b]])) > r["sample_d2"] for a, b in ((0, 1), (0, 2), (1, 2))):
                first = d
                break
        assert r["draw"][t] == first
        assert r["ranks"][t].tolist() == ([R.rank_int(5, t, first, c, 12) for c in range(3)] if first >= 0 else [-1, -1, -1])
        later += first > 0
    assert later > 5 and (r["draw"] < 0).any() and (r["counts"][r["draw"] < 0] == -1).all()


def SC_d2(p, q):
    return R.d2_points(np.asarray(p, F32)[None, :3], np.asarray(q, F32)[None, :3])[0]


def test_spacing_exactly_on_sample_d2_is_not_good_and_its_nextafter_is():
    P = np.array([[0, 0, 0, 1], [0.75, 0, 0, 1], [0, 3, 0, 1]], F32)      # the smallest spacing: d2 = 0.5625, exact
    Q = P.copy()
    v = float(SC_d2(P[0], P[1]))
    assert v == 0.5625
    _, good, _, _ = R.hypotheses(P, Q, 1, 0, 64, v)
    assert not good.any()                                   # (double)d2 > sample_d2 is strict
    ranks, good, sums, _ = R.hypotheses(P, Q, 1, 0, 64, math.nextafter(v, 0.0))
    assert good.any() and (sums[good, 0] == 3.0).all() and all(sorted(k) == [0, 1, 2] for k in ranks[good].tolist())


def test_pair_exactly_on_the_threshold_is_no_inlier():
    P = np.array([[0, 0, 0, 1]], F32)
    Q = np.array([[0.25, 0, 0, 1]], F32)                      # d2 = 0.0625 = 0.25 * 0.25 exactly
    eye = np.eye(4, dtype=F32)
    assert not R.inlier_mask(eye, P, Q, 0.25)[0]
    assert R.inlier_mask(eye, P, Q, math.nextafter(0.25, 1.0))[0]
    Q[0, 0] = np.nextafter(F32(0.25), F32(0))
    assert R.inlier_mask(eye, P, Q, 0.25)[0]
    assert not R.inlier_mask(eye, np.array([[np.nan, 0, 0, 1]], F32), Q, 10.0)[0] and not R.inlier_mask(eye, P, np.array([[0, np.inf, 0, 1]], F32), 10.0)[0]


def test_small_m_and_the_degenerate_arguments(built):
    r = R.run(*S.pairs(0), 0.05, 50, 1)
    assert (r["status"], r["n_kept"], r["iterations"], r["host_waits"]) == (0, 0, 0, 0)
    for m in (1, 2):
        r = R.run(*S.pairs(m), 0.05, 50, 1)
        assert (r["status"], r["n_kept"], r["iterations"], r["batches"]) == (1, m, 50, 0) and (r["counts"] == -1).all() and (r["ranks"] == -1).all()
        assert np.array_equal(r["best_T"], np.eye(4, dtype=F32))
    r = R.run(*S.pairs(3, 1.0), 0.05, 50, 1)
    assert r["status"] == 3 and r["n_kept"] == 3
    r = R.run(*S.pairs(65), 0.05, 0, 1)
    assert (r["status"], r["n_kept"], r["iterations"], r["host_waits"]) == (1, 65, 0, 1)
    r = R.run(*S.pairs(65), 0.0, 70, 1)                   # a threshold of 0: nothing is ever an inlier, every pair stays
    assert (r["status"], r["n_kept"], r["iterations"]) == (1, 65, 70) and (r["counts"] <= 0).all() and r["kept"].all()
    for bad in ((-1.0, 5), (math.nan, 5), (math.inf, 5), (0.1, -1), (0.1, R.MAX_ITERATIONS + 1)):
        with pytest.raises(R.Refused):
            R.run(*S.pairs(5), *bad)
    with pytest.raises(R.Refused):
        R.reject(*S.pairs(5), [0, 5], [0, 1])


def test_a_best_count_of_two_keeps_everything(built):
    rng = np.random.default_rng(0)
    P = np.concatenate([rng.uniform(-1, 1, (3, 3)), np.ones((3, 1))], 1).astype(F32)
    Q = P.copy()
    Q[:, :3] += rng.normal(0, 0.05, (3, 3)).astype(F32)
    r = R.run(P, Q, 0.03, 20, 5)
    assert r["status"] == 2 and r["counts"].max() == 2 and r["kept"].all() and np.array_equal(r["best_T"], np.eye(4, dtype=F32)) and r["best_t"] >= 0
    same(r, R.run_literal(P, Q, 0.03, 20, 5))


def test_coincident_and_collinear_p_keep_every_pair(built):
    Pc = np.tile(np.array([[1, 2, 3, 1]], F32), (10, 1))
    r = R.run(Pc, SC.moved(Pc, S.TRUTH), 0.05, 70, 1)
    assert r["sample_d2"] == 0.0 and (r["counts"] == -1).all() and (r["status"], r["iterations"], r["n_kept"]) == (1, 70, 10)
    t = np.linspace(-3, 3, 30)
    Pl = np.stack([t, 2 * t + 1, -t, np.ones(30)], 1).astype(F32)
    r = R.run(Pl, SC.moved(Pl, S.TRUTH), 0.05, 70, 1)
    assert r["n_kept"] == 30 and r["kept"].all()              # (see the module's note: the rule evaluates spaced collinear samples)
    same(r, R.run_literal(Pl, SC.moved(Pl, S.TRUTH), 0.05, 70, 1))


def test_a_negative_eigenvalue_counts_as_zero():
    rng = np.random.default_rng(142)
    n = rng.integers(3, 40)
    t = rng.uniform(-1, 1, n)
    d = rng.normal(0, 1, 3)
    P = np.concatenate([100 * rng.normal(0, 1, 3) + np.outer(t, d), np.ones((n, 1))], 1).astype(F32)
    mom, nf = R.moments_of(P)
    e = R.eigenvalues_of(mom, nf)
    assert e[0] < 0.0 <= e[1]
    s = ((0.0 + math.sqrt(e[1])) + math.sqrt(e[2])) / 3.0
    assert R.sample_d2_of(mom, nf) == s * s and math.isfinite(s)


def test_the_loop_stops_in_batch_one_at_90_percent_and_runs_on_at_20(built):
    c = S.core_cases()
    r = R.run(*c["stops_in_batch_one"])
    assert r["batches"] == 1 and r["iterations"] < 64 and r["status"] == 3 and r["host_waits"] == 3
    best = r["counts"][r["best_t"]]
    assert r["iterations"] == math.ceil(R.next_k(int(best), r["m"], 0.99)) or r["iterations"] > r["best_t"]
    r = R.run(*S.pairs(513, 0.2, 2, scatter=True), 0.05, 1000, 12345)
    assert r["batches"] >= 4 and 64 * (r["batches"] - 1) < r["iterations"] <= 64 * r["batches"] and r["iterations"] < 1000
    assert r["host_waits"] == 1 + 2 * r["batches"] and r["status"] == 3


@pytest.mark.parametrize("name", sorted(S.core_cases()))
def test_the_well_spread_cut_leaves_out_under_ten_percent(built, name):
    r = R.run(*S.core_cases()[name])
    ev = np.flatnonzero(r["valid"])
    if ev.size:
        cut = sum(not SC.well_spread(r["sums17"][t]) for t in ev)
        assert cut < 0.1 * ev.size, (cut, ev.size)


def test_new_symbols_are_exported_and_declared(built):
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(HERE), "include", "icpgpu.h")).read()
    for symbol in SYMBOLS:
        assert f" T {symbol}\n" in names
        assert f"int {symbol}(" in header and symbol in _lib.EXPORTS
    assert "ICPGPU_REJECT_SAMPLE_CONSENSUS = 5" in header and _lib.REJECT_SAMPLE_CONSENSUS == R.KIND == 5
    assert "#define ICPGPU_RSAC_MAX_ITERATIONS 65536" in header and _lib.RSAC_MAX_ITERATIONS == R.MAX_ITERATIONS == 65536
    assert "#define ICPGPU_RSAC_DRAWS 16" in header and _lib.RSAC_DRAWS == R.DRAWS == 16
    assert C.sizeof(_lib.Rejector) == 16
    assert "sample-consensus and feature rejectors" not in header and "Not provided: the var-trimmed and feature rejectors" in header


def test_the_struct_stays_16_bytes_in_c(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){ icpgpu_rejector r = {ICPGPU_REJECT_SAMPLE_CONSENSUS, 1000, 0.05};\n'
                   '  printf("%d %d %d %d\\n", (int)r.kind, (int)sizeof(icpgpu_rejector), ICPGPU_RSAC_MAX_ITERATIONS, ICPGPU_RSAC_DRAWS); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["5", "16", "65536", "16"]


def test_entry_points_refuse_a_null_context(built):
    L = _lib.load()
    seed = C.c_uint64(77)
    assert L.icpgpu_set_rejector_sac_seed(None, 1) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_get_rejector_sac_seed(None, C.byref(seed)) == _lib.ERR_INVALID_ARG and seed.value == 77
    assert L.icpgpu_correspondence_rejector_sample_consensus(None, None, 0, None, 0, None, None, 0, 0.05, 10, 0, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_rejector_sac_fetch(None, 0, None, None, None, None, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG


def test_front_end_and_its_defaults():
    import icpslam_amd as pkg
    rej = pkg.CorrespondenceRejectorSampleConsensus()
    assert (rej.getInlierThreshold(), rej.getMaximumIterations()) == (0.05, 1000)
    rej.setInlierThreshold(0.2)
    rej.setMaximumIterations(77)
    e = rej._entry()
    assert (e.kind, e.value, e.min_correspondences) == (5, 0.2, 77)
    rej.setRefineModel(False)
    with pytest.raises(NotImplementedError):
        rej.setRefineModel(True)
    assert np.array_equal(rej.getBestTransformation(), np.eye(4))


def test_the_stage_beats_the_gate_alone_on_the_moved_block(built):
    src, tgt, truth, block = S.moved_block()
    assert 0.2 < block.mean() < 0.3
    gate = SC.pose_error(R.align(src, tgt, [], **S.BLOCK_KW)["T"], truth)
    worst = [0.0, 0.0]
    for seed in S.BLOCK_SEEDS:
        r = R.align(src, tgt, [(R.KIND, *S.BLOCK_STAGE)], seed=seed, **S.BLOCK_KW)
        err = SC.pose_error(r["T"], truth)
        print(seed, err, r["iterations"], r["n_corr"])
        assert err[1] < 0.1 * gate[1] and err[0] < 0.1 * gate[0]
        worst = [max(worst[0], err[0]), max(worst[1], err[1])]
    assert worst[0] <= S.E2E_WORST[0] and worst[1] <= S.E2E_WORST[1]   # the recorded worst, which the device's bound doubles


def test_descriptor_matches_through_the_call_reach_the_truth(built):
    """scp_scenes' end-to-end clouds, restated FPFH, feature k-nearest with k = 1 (about a fifth of the matches are right), the call:
    best_T within rsac_scenes.MATCH_BOUND of the truth.  Measured: 0.000 deg 1.2e-7 m, 0.000 deg 2.8e-8 m, 0.009 deg 3.3e-7 m; 281 of
    1500 pairs stay."""
    import fpfh_restated as FR
    import normals_restated as NR
    import scp_restated as SCP
    source, target, truth = SC.e2e_clouds()
    sf, tf = (FR.estimate(c, NR.estimate(c, None, k=SC.E2E_NORMAL_K)[0], None, radius=SC.E2E_FPFH_RADIUS)[0] for c in (source, target))
    idx, _, found = SCP.feature_knn(tf, sf, 1)
    ok = found > 0
    for seed in S.MATCH_SEEDS:
        r = R.reject(source, target, np.flatnonzero(ok), idx[ok, 0], S.MATCH_KW["inlier_threshold"], S.MATCH_KW["max_iterations"], seed)
        rot, trans = SC.pose_error(r["best_T"], truth)
        print(seed, rot, trans, r["n_kept"], r["iterations"])
        assert r["status"] == 3 and rot <= S.MATCH_BOUND[0] and trans <= S.MATCH_BOUND[1] and r["n_kept"] > 200
