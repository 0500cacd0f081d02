"""CPU tests of reciprocal correspondences (include/icpgpu.h, "reciprocal correspondences"): the properties the rule rests on, checked
on the oracle's primitives; the NumPy restatement (tests/reciprocal_restated.py) against a literal double loop; the new symbols and
the argument checks that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reciprocal_restated as RR  # noqa: E402
import rejectors_restated as R  # noqa: E402

from icpslam_amd import _lib, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icpgpu_set_reciprocal_correspondences", "icpgpu_get_reciprocal_correspondences", "icpgpu_reciprocal_stats")
T_FIXED = synth.pose_matrix(0.05, -0.02, 0.01, 0.0, 0.0, 0.01).astype(np.float32)      # tests/test_gpu_rejectors.py's
I4 = np.eye(4, dtype=np.float32)
# source sizes of the 3k pair -> (pairs past the gate, reciprocal pairs) at T_FIXED and gate 1.0
COUNTS = {3000: (2913, 1661), 1025: (992, 761), 64: (63, 61)}


@pytest.fixture(scope="module")
def pair3k(built):
    src, tgt, _ = synth.make_pair(3000, 3000, seed=17)
    return src, tgt


@pytest.mark.parametrize("n", sorted(COUNTS))
def test_properties_on_the_oracle(pair3k, n):
    import oracle
    src, tgt = pair3k[0][:n], pair3k[1]
    X = oracle.transform_cloud(src, T_FIXED)
    idx, d2 = oracle.nn(src, tgt, T_FIXED)
    idx_x, d2_x = oracle.nn(X, tgt, I4)
    # searching the transformed cloud under the identity is searching the cloud under T, bit for bit
    assert np.array_equal(idx, idx_x) and np.array_equal(d2.view(np.uint32), d2_x.view(np.uint32))
    ridx, rd2, kept, st = RR.reciprocal(src, tgt, T_FIXED, 1.0)
    assert (st["pairs_in"], st["pairs_out"]) == COUNTS[n]
    assert 0 < st["pairs_out"] < st["pairs_in"]                       # both outcomes occur: the sets below are neither empty nor full
    # the reverse distance of a kept pair is its forward d2, bit for bit (the expression is symmetric, negation included)
    k, kd2 = RR.reverse_nn(src, tgt, T_FIXED)
    who = np.flatnonzero(kept)
    assert np.array_equal(k[ridx[who]], who)
    assert np.array_equal(kd2[ridx[who]].view(np.uint32), rd2[who].view(np.uint32))
    # ... and never exceeds the forward d2 of any gated pair (PCL's second test is implied)
    alive = RR.gate(idx, d2, 1.0)
    assert (kd2[idx[alive]] <= d2[alive]).all()
    # reciprocal is the stricter rule: a subset of one-to-one's kept set on the same pairs
    one, _ = R.one_to_one(idx, d2, alive)
    assert not (kept & ~one).any() and one.sum() > kept.sum()


def _literal(src, tgt, T, max_dist):
    """the rule as a double loop in float32, on a small input"""
    import oracle
    X = oracle.transform_cloud(src, T)
    idx, d2 = oracle.nn(src, tgt, T)
    kept = []
    for i in range(src.shape[0]):
        j = int(idx[i])
        if j < 0 or not float(d2[i]) <= max_dist * max_dist:
            continue
        best, best_k = None, -1
        for k in range(src.shape[0]):
            if not np.isfinite(X[k, :3]).all():
                continue
            dk = oracle.nn(tgt[j:j + 1], X[k:k + 1], I4)[1][0]
            if best is None or dk < best:                              # strict: the lowest source index wins a tie
                best, best_k = dk, k
        if best_k == i:
            kept.append(i)
    return kept


def test_restatement_against_the_literal_rule_ties_and_non_finite(pair3k):
    src, tgt = pair3k[0][:120].copy(), pair3k[1]
    src = np.concatenate([src, src[:40], src[10:20]])                  # duplicated source points: equal reverse distances
    src[7, 0] = np.nan
    src[130, 1] = np.inf                                               # a duplicate of point 10 that is not finite
    ridx, _, kept, st = RR.reciprocal(src, tgt, T_FIXED, 1.0)
    assert list(np.flatnonzero(kept)) == _literal(src, tgt, T_FIXED, 1.0)
    assert 0 < st["pairs_out"] < st["pairs_in"]
    # the tie rule: of a duplicated source point only the first finite copy can stay (point 7 is not finite: its copy, 127, is the
    # first), and where the original stays without its copies (cut off the duplicates) it stays with them
    assert not np.delete(kept[120:], 7).any()
    ridx0, _, kept0, _ = RR.reciprocal(src[:120], tgt, T_FIXED, 1.0)
    assert np.array_equal(kept[:120], kept0)
    assert not kept[7] and ridx[7] == -1


def test_chain_runs_on_the_survivors(pair3k):
    src, tgt = pair3k[0][:1025], pair3k[1]
    _, _, kept, rst = RR.reciprocal(src, tgt, T_FIXED, 1.0)
    idx, d2, stats, rstats = RR.correspondences(src, tgt, T_FIXED, 1.0, [(R.TRIMMED, 0.5)])
    assert rstats == rst and stats[0]["pairs_in"] == rst["pairs_out"]
    assert 0 < stats[0]["pairs_out"] < stats[0]["pairs_in"] and (idx >= 0).sum() == stats[0]["pairs_out"]
    assert not ((idx >= 0) & ~kept).any()
    # reciprocal then one-to-one: one-to-one has nothing left to remove
    _, _, stats, rstats = RR.correspondences(src, tgt, T_FIXED, 1.0, [(R.ONE_TO_ONE,)])
    assert stats[0]["pairs_in"] == stats[0]["pairs_out"] == rstats["pairs_out"]
    # flag off: the chain alone, and the stage reports zeroes
    idx0, d20, stats0, rstats0 = RR.correspondences(src, tgt, T_FIXED, 1.0, [(R.TRIMMED, 0.5)], use_reciprocal=False)
    ref = R.correspondences(src, tgt, T_FIXED, 1.0, [(R.TRIMMED, 0.5)])
    assert np.array_equal(idx0, ref[0]) and np.array_equal(d20, ref[1]) and rstats0 == dict(pairs_in=0, pairs_out=0)


def test_restated_align_wraps_the_chain_loop(pair3k):
    src, tgt = pair3k[0][:1025], pair3k[1]
    saved = R.correspondences
    off = RR.align(src, tgt, [(R.MEDIAN, 2.0)], use_reciprocal=False, max_iterations=4)
    assert R.correspondences is saved                                  # put back
    ref = R.align(src, tgt, [(R.MEDIAN, 2.0)], max_iterations=4)
    assert off["T"].tobytes() == ref["T"].tobytes() and off["n_corr"] == ref["n_corr"] and off["reciprocal"] == dict(pairs_in=0, pairs_out=0)
    on = RR.align(src, tgt, [(R.MEDIAN, 2.0)], max_iterations=4)
    assert 0 < on["reciprocal"]["pairs_out"] < on["reciprocal"]["pairs_in"]
    assert on["stats"][0]["pairs_in"] == on["reciprocal"]["pairs_out"] and on["n_corr"] == on["stats"][0]["pairs_out"] < ref["n_corr"]


# ---- the library's boundary (fail on a library without the feature) ---------------------------------------------------------------
def test_new_symbols_exported(built):
    _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in _lib.EXPORTS


def test_null_context_is_refused(built):
    """Without a device there is no context: the refusals reached with a null one."""
    L = _lib.load()
    on = C.c_int(7)
    a, b = C.c_uint32(5), C.c_uint32(6)
    assert L.icpgpu_set_reciprocal_correspondences(None, 1) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_get_reciprocal_correspondences(None, C.byref(on)) == _lib.ERR_INVALID_ARG and on.value == 7
    assert L.icpgpu_reciprocal_stats(None, C.byref(a), C.byref(b)) == _lib.ERR_INVALID_ARG and (a.value, b.value) == (5, 6)


def test_header_compiles_as_c_and_refuses(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){ int on = 0; uint32_t a = 0, b = 0;\n'
                   '  printf("%d %d %d\\n", icpgpu_set_reciprocal_correspondences(NULL, 1), icpgpu_get_reciprocal_correspondences(NULL, &on),\n'
                   '         icpgpu_reciprocal_stats(NULL, &a, &b)); return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [_lib.ERR_INVALID_ARG] * 3


def test_mirror_classes_carry_pcl_names():
    from icpslam_amd import registration as reg
    for cls in (reg.IterativeClosestPoint, reg.IterativeClosestPointWithNormals, reg.GeneralizedIterativeClosestPoint,
                reg.NormalDistributionsTransform):
        assert hasattr(cls, "setUseReciprocalCorrespondences") and hasattr(cls, "getUseReciprocalCorrespondences"), cls
    for name in ("set_reciprocal_correspondences", "get_reciprocal_correspondences", "reciprocal_stats"):
        assert hasattr(reg.Context, name), name
