"""The host step of every point-to-point iteration -- solve_umeyama, svd3x3 and ConvergenceCriteria in icpslam_amd/csrc/icp_solver.cpp --
and the oracle's copy of it, against tests/solve_reference.py (exact sums, numpy's singular values; nothing shared with either) on the
cases of tests/solve_cases.py.  No GPU.

Measured on these cases (worst per family, product / oracle): the optimality deficit |opt - tr(R^T Sigma)| in u mag, max |R^T R - I| in
u, and the translation's error as a fraction of its bound 4 u (|mu_q| + |R| |mu_p|); u = 2^-53.  Caps: 1600 u mag, 512 u, 1.

    family      deficit (u mag)      R^T R - I (u)      t (of its bound)
    mirror        3.4 /   3.4          4.9 /   4.9      0.153 / 0.153
    offset        0.0 /   0.0          4.4 /   4.4      0.135 / 0.135
    planar        0.4 /   0.4          5.0 /   5.0      0.034 / 0.034
    scaled        2.0 /   2.0          5.9 /   5.9      0.154 / 0.154
    slab          1.7 /   1.7          4.7 /   4.7      0.204 / 0.186
    slabcut       0.6 /   0.5          4.1 /   4.0      0.210 / 0.224
    small         0.5 /   0.5          3.6 /   3.6      0.138 / 0.138
    three         3.1 /   3.1          6.4 /   6.4      0.266 / 0.266
    tie           7.5 /   4.5          9.5 /   5.5      0.000 / 0.000
    turn          3.5 /   3.5          7.0 /   7.0      0.081 / 0.081
    unrelated     0.0 /   0.0          9.0 /   4.6      0.181 / 0.084

The caps are the derived ones, 200 and 50 times above the worst measured; they are not fitted to these figures.  As float32 transforms
(each solve cast once, the float32 caps 9 u32 mag, 8 u32 and 1): 0.57 u32 mag, 1.23 u32 and 0.91 of the translation's bound at worst.

svd3x3 over the same Sigmas and the hand matrices at 2^-1000 .. 2^1000 (256 matrices; product / oracle): reconstruction 6.5 / 7.1 u s0
(cap 16), U^T U - I 4.4 / 4.4 u and V^T V - I 7.5 / 7.4 u (cap 512), |s - numpy's| 6.9 / 6.9 u s0 (cap 8).

What these tests notice and tests/test_abi.py::test_host_solve_matches_oracle does not (one-line changes to scratch copies of
icp_solver.cpp): without the reflection sign, det R < 0 on 10 cases (collinear, coincident, planar:four, patch64, slab:1e-12 .. 1e-14,
mirror:full, unrelated, n2); with the 1e-17 skip at 1e-9, R^T R - I of 1e3 .. 7e6 u on 12 cases and as many Sigmas.  An ascending
sort it does notice; here 17 cases miss the trace by 1e13 u mag and up, and 100 matrices fail.  Without the power-of-two scaling
71 matrices fail, all of them hand matrices at 2^k with |k| >= 300, and nothing else does: rank1 and dense from 2^300 up (aa * bb
overflows, every rotation is skipped), diag(3, 1e-9, 0) from 2^-500 down, and from |k| = 600 on every matrix but zeros (the column
norms themselves leave the format); the matrices that need no rotation pass up to |k| = 500."""
import ctypes as C
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle
import solve_cases as S
import solve_reference as R
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
NAMES = [name for name, _, _ in S.cases()]


def product_solve(sums):
    sums = np.ascontiguousarray(sums, np.float64)
    Tk = np.full(16, 7.0)
    rc = _lib.load().icpgpu_solve(sums.ctypes.data_as(DP), Tk.ctypes.data_as(DP))
    return rc, Tk.reshape(4, 4).T.copy()


def oracle_solve(sums):
    sums = np.ascontiguousarray(sums, np.float64)
    Tk = np.full(16, 7.0)
    rc = oracle.lib().orc_umeyama(sums.ctypes.data_as(DP), Tk.ctypes.data_as(DP))
    return rc, Tk.reshape(4, 4).T.copy()


SOLVERS = {"product": product_solve, "oracle": oracle_solve}


# ---- the solve -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_both_solvers_maximise_the_trace_on_every_case(built, name):
    _, p, q = S.case(name)
    sums = S.sums_of(p, q)
    ex = R.exact(sums)
    got = {}
    for who, solve in SOLVERS.items():
        rc, T = solve(sums)
        assert rc == 0, (who, rc)
        m = R.check(sums, T, ex=ex)
        print(f"{name} {who}: deficit {m['deficit']:.1f} u mag, orth {m['orth']:.1f} u, t {m['t']:.3f} of its bound")
        got[who] = T
    s = [float(v) for v in ex["s"]]
    if s[1] >= 1e-3 * s[0] and s[0] > 0:                   # the rotation is determined and well conditioned: the two agree, as before
        reach = 1.0 + float(max(abs(v) for v in ex["mu_p"] + ex["mu_q"]))     # (t = mu_q - R mu_p carries R's difference times |mu_p|)
        assert np.abs(got["product"][:3, :3] - got["oracle"][:3, :3]).max() <= 1e-12
        assert np.abs(got["product"][:3, 3] - got["oracle"][:3, 3]).max() <= 1e-12 * reach


def test_the_device_cases_are_paired_by_construction():
    """What tests/test_gpu_solve_edges.py relies on (and asserts again from the device's own search): the motion is at least 20 times
    below the spacing, so each p's nearest q is its own."""
    for name in S.GPU_CASES:
        _, p, q = S.case(name)
        d = np.linalg.norm(q[:, None] - q[None], axis=2)
        d[np.diag_indices(len(q))] = np.inf
        assert d.min() >= 20.0 * np.linalg.norm(q - p, axis=1).max(), name
        near = np.linalg.norm(p[:, None] - q[None], axis=2).argmin(axis=1)
        assert near.tolist() == list(range(len(p))), name


@pytest.mark.parametrize("who", sorted(SOLVERS))
def test_what_cannot_be_solved_is_refused_with_the_identity(built, who):
    for name, sums in S.rejected():
        rc, T = SOLVERS[who](sums)
        assert rc != 0 and T.tobytes() == np.eye(4).tobytes(), (name, rc, T)


# ---- svd3x3 and ConvergenceCriteria, which the library does not export --------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("solve_host") / "solve_host_check")
    csrc = os.path.join(ROOT, "icpslam_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "solve_host_check.cpp"),
                           os.path.join(csrc, "icp_solver.cpp"), "-o", out])
    return out


def word(x) -> str:
    return struct.pack(">d", float(x)).hex()


def unword(w) -> float:
    return struct.unpack(">d", bytes.fromhex(w))[0]


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    answers = out.stdout.splitlines()
    assert len(answers) == len(lines)
    return answers


def product_svd(exe, mats):
    res = []
    for line in ask(exe, ["svd " + " ".join(word(x) for x in np.asarray(A).reshape(9)) for A in mats]):
        w = line.split()
        assert w[0] == "svd" and len(w) == 22
        v = np.array([unword(x) for x in w[1:]])
        res.append((v[:9].reshape(3, 3), v[9:12], v[12:].reshape(3, 3)))
    return res


def oracle_svd(exe, mats):
    return [oracle.svd3(np.asarray(A, np.float64)) for A in mats]


def sigma_double(sums):
    """Sigma as both solvers form it, in double."""
    n = sums[0]
    return sums[7:16].reshape(3, 3) / n - np.outer(sums[4:7] / n, sums[1:4] / n)


def svd_matrices():
    return [("Sigma of " + name, sigma_double(S.sums_of(p, q))) for name, p, q in S.cases()] + S.hand_matrices()


def frac(M):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(M)]


def off_orthonormal(Q) -> Fraction:
    return max(abs(sum(Q[k][i] * Q[k][j] for k in range(3)) - (i == j)) for i in range(3) for j in range(3))


def check_svd(name, A, U, s, V) -> dict:
    assert np.isfinite(U).all() and np.isfinite(s).all() and np.isfinite(V).all(), (name, U, s, V)
    assert s[0] >= s[1] >= s[2] >= 0.0, (name, s)
    Af, Uf, Vf, sf = frac(A), frac(U), frac(V), [Fraction(float(x)) for x in s]
    s0 = sf[0]
    recon = max(abs(sum(Uf[r][k] * sf[k] * Vf[c][k] for k in range(3)) - Af[r][c]) for r in range(3) for c in range(3))
    assert recon <= 16 * R.U * s0, (name, "U s V^T - A", float(recon / (R.U * s0)) if s0 else float(recon), "u s0")
    ou, ov = off_orthonormal(Uf), off_orthonormal(Vf)
    assert ou <= R.ORTH and ov <= R.ORTH, (name, "U^T U - I, V^T V - I", float(ou / R.U), float(ov / R.U), "u")
    want = R.singular_values(Af)
    ds = max(abs(a - b) for a, b in zip(sf, want))
    assert ds <= 8 * R.U * s0, (name, "s - numpy's", float(ds / (R.U * s0)) if s0 else float(ds), "u s0", s, [float(x) for x in want])
    one = R.U * s0 if s0 else 1
    return dict(recon=float(recon / one), orth_u=float(ou / R.U), orth_v=float(ov / R.U), sigma=float(ds / one))


@pytest.mark.parametrize("who", ["product", "oracle"])
def test_svd3x3_on_every_sigma_and_the_hand_matrices_at_every_scale(built, exe, who):
    mats = svd_matrices()
    results = (product_svd if who == "product" else oracle_svd)(exe, [A for _, A in mats])
    worst, failed = {}, []
    for (name, A), (U, s, V) in zip(mats, results):
        try:
            for k, v in check_svd(name, A, U, s, V).items():
                worst[k] = max(worst.get(k, 0.0), v)
        except AssertionError as e:
            failed.append(str(e))
    print(f"{who} svd3x3 over {len(mats)} matrices, worst:", {k: round(v, 2) for k, v in worst.items()})
    assert not failed, (len(failed), failed)


# A transform whose rotation and translation are both far from their thresholds, and the identity.
FAR = (0.5, 0.5, 0.5, 1.0, 0.0, 0.0)
EYE = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
EPS = 2.0 ** -20                                            # transformation_epsilon: the thresholds are cos >= 1 - EPS and |t|^2 <= EPS
OFF = -1.7e308                                              # euclidean_fitness_epsilon as the library's defaults leave it: state 4 is off
# (name, max_iterations, transformation_epsilon, euclidean_fitness_epsilon, force, calls (nr_iterations, r00, r11, r22, tx, ty, tz, mse),
#  expected "returned:state" per call).  States: 0 not converged, 1 iterations, 2 transform, 3 absolute MSE, 4 relative MSE.  The rule,
# in order: nr >= max -> 1; force -> 0; cos >= 1 - eps and |t|^2 <= eps -> 2; |mse - prev| < 1e-12 -> 3; |mse - prev| / prev < feps -> 4;
# else prev = mse, 0.  cos = 0.5 (r00 + r11 + r22 - 1), summed left to right.
CRITERIA = [
    ("iterations, forced", 3, EPS, OFF, 1, [(1, *EYE, 0.0), (2, *EYE, 0.0), (3, *FAR, 5.0)], ["0:0", "0:0", "1:1"]),
    ("iterations, not forced", 3, EPS, OFF, 0, [(1, *FAR, 9.0), (2, *FAR, 5.0), (3, *FAR, 2.0)], ["0:0", "0:0", "1:1"]),
    ("iterations before the transform", 1, EPS, OFF, 0, [(1, *EYE, 0.0)], ["1:1"]),
    ("max_iterations 0", 0, EPS, OFF, 0, [(0, *FAR, 1.0)], ["1:1"]),
    ("the identity", 9, EPS, OFF, 0, [(1, *EYE, 3.0)], ["1:2"]),
    # r00 = 1 - 2^-19: the sum is 3 - 2^-19, cos = 1 - 2^-20 exactly; tx = 2^-10: |t|^2 = 2^-20 exactly
    ("both exactly at their thresholds", 9, EPS, OFF, 0, [(1, 1.0 - 2.0 ** -19, 1.0, 1.0, 2.0 ** -10, 0.0, 0.0, 3.0)], ["1:2"]),
    # one ulp of the sum (2^-51 at 3) below: cos = 1 - 2^-20 - 2^-52, the nearest value under the threshold this sum can give
    ("the rotation one step outside", 9, EPS, OFF, 0, [(1, 1.0 - 2.0 ** -19 - 2.0 ** -51, 1.0, 1.0, 2.0 ** -10, 0.0, 0.0, 3.0)], ["0:0"]),
    # tx one ulp above 2^-10: |t|^2 rounds to 2^-20 (1 + 2^-51)
    ("the translation one ulp outside", 9, EPS, OFF, 0, [(1, 1.0 - 2.0 ** -19, 1.0, 1.0, float(np.nextafter(2.0 ** -10, 1.0)), 0.0, 0.0, 3.0)], ["0:0"]),
    ("the translation on another axis", 9, EPS, OFF, 0, [(1, 1.0, 1.0, 1.0 - 2.0 ** -19, 0.0, 0.0, -(2.0 ** -10), 3.0)], ["1:2"]),
    ("absolute MSE just below 1e-12", 9, EPS, OFF, 0, [(1, *FAR, 0.0), (2, *FAR, float(np.nextafter(1e-12, 0.0)))], ["0:0", "1:3"]),
    ("absolute MSE at 1e-12", 9, EPS, OFF, 0, [(1, *FAR, 0.0), (2, *FAR, 1e-12)], ["0:0", "0:0"]),
    ("absolute MSE, rising", 9, EPS, OFF, 0, [(1, *FAR, 1.0), (2, *FAR, 1.0 + 2.0 ** -40)], ["0:0", "1:3"]),
    ("absolute MSE, twice the step", 9, EPS, OFF, 0, [(1, *FAR, 1.0), (2, *FAR, 1.0 + 2.0 ** -39)], ["0:0", "0:0"]),
    ("mse == mse_prev == 0", 9, EPS, OFF, 0, [(1, *FAR, 0.0), (2, *FAR, 0.0)], ["0:0", "1:3"]),
    ("relative MSE just below", 9, EPS, 2.0 ** -10, 0, [(1, *FAR, 1.0), (2, *FAR, 1.0 + 2.0 ** -10 - 2.0 ** -52)], ["0:0", "1:4"]),
    ("relative MSE at the threshold", 9, EPS, 2.0 ** -10, 0, [(1, *FAR, 1.0), (2, *FAR, 1.0 + 2.0 ** -10)], ["0:0", "0:0"]),
    # a stop leaves prev alone: the fourth call is still measured from 2.0, and sits exactly at the threshold
    ("relative MSE, falling, prev is the last call's", 9, EPS, 2.0 ** -10, 0,
     [(1, *FAR, 4.0), (2, *FAR, 2.0), (3, *FAR, 2.0 - 2.0 ** -9 + 2.0 ** -51), (4, *FAR, 2.0 - 2.0 ** -9)], ["0:0", "0:0", "1:4", "0:0"]),
    # the first call compares with DBL_MAX: |mse - DBL_MAX| is not below 1e-12, and the ratio is 1 - mse / DBL_MAX: exactly 1 for any
    # mse below 1e292, and 1 - 5.6e-9 at 1e300 -- under no threshold that means anything (PCL's rule is the same)
    ("first call, small mse", 9, EPS, 0.5, 0, [(1, *FAR, 1e-30)], ["0:0"]),
    ("first call, mse 0", 9, EPS, 1.0, 0, [(1, *FAR, 0.0)], ["0:0"]),
    ("first call, mse 1e6, threshold 1", 9, EPS, 1.0, 0, [(1, *FAR, 1e6)], ["0:0"]),
    ("first call, large mse", 9, EPS, 0.5, 0, [(1, *FAR, 1e300)], ["0:0"]),
    ("forced: nothing but the count", 9, EPS, 2.0 ** -10, 1, [(1, *EYE, 0.0), (2, *EYE, 0.0), (8, *EYE, 0.0), (9, *EYE, 0.0)], ["0:0", "0:0", "0:0", "1:1"]),
]


def test_convergence_criteria_at_every_threshold(exe):
    lines = []
    for _, max_it, teps, feps, force, calls, _ in CRITERIA:
        lines.append(f"conv {max_it} {word(teps)} {word(feps)} {force} {len(calls)} " + " ".join(f"{c[0]} " + " ".join(word(x) for x in c[1:]) for c in calls))
    for (name, *_, want), line in zip(CRITERIA, ask(exe, lines)):
        assert line.split() == ["conv"] + want, (name, line, want)
