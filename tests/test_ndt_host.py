"""CPU tests of the NDT mode's boundary (ICPGPU_NDT, added under C-ABI 1.2): the header, the exports, the Gauss constants, the
restatement's derivatives against finite differences of its own score, the library's host Newton step (icpgpu_ndt_step) against
the restatement (tests/ndt_restated.py), and eulerAngles(0, 1, 2)."""
import math
import os
import subprocess

import numpy as np
import pytest

import ndt_restated as nr
from icpslam_amd import _lib
from icpslam_amd.registration import ndt_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icpgpu_set_ndt_params", "icpgpu_get_ndt_params", "icpgpu_ndt_transformation_probability", "icpgpu_ndt_cells",
               "icpgpu_ndt_derivatives", "icpgpu_ndt_step")


def test_header_compiles_as_c_with_the_method(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){ icpgpu_method m = ICPGPU_NDT; double s[29] = {0}, p[6] = {0}, po[6], a; float T[16];\n'
                   '  int (*f1)(icpgpu_ctx*, double, double, double) = icpgpu_set_ndt_params;\n'
                   '  int (*f2)(const icpgpu_ctx*, double*, double*, double*) = icpgpu_get_ndt_params;\n'
                   '  int (*f3)(const icpgpu_ctx*, double*) = icpgpu_ndt_transformation_probability;\n'
                   '  int (*f4)(icpgpu_ctx*, size_t, float*, double*, double*, int32_t*, size_t*) = icpgpu_ndt_cells;\n'
                   '  int (*f5)(icpgpu_ctx*, const double*, double*) = icpgpu_ndt_derivatives;\n'
                   '  (void)f1; (void)f2; (void)f3; (void)f4; (void)f5;\n'
                   '  printf("%d %d %d\\n", (int)m, ICPGPU_HEADER_VERSION, icpgpu_ndt_step(s, p, 0.1, 0.1, po, &a, T)); return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    m, version, rc = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert m == 3 and version == 1002
    assert rc == 1                              # an all-zero system: delta = 0, PCL's loop stops


def test_version_and_new_symbols(built):
    lib = _lib.load()
    assert lib.icpgpu_version() == 1002 == _lib.HEADER_VERSION
    assert _lib.NDT == 3
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in _lib.EXPORTS


def test_gauss_constants():
    # Magnusson 2009 eq. 6.8 at PCL's defaults, worked by hand: c1 = 4.5, c2 = 0.55, d3 = -ln 0.55
    d1, d2 = nr.gauss_constants(1.0, 0.55)
    d3 = -math.log(0.55)
    assert d1 == pytest.approx(-math.log(5.05) - d3, rel=1e-15)
    assert d2 == pytest.approx(-2 * math.log((-math.log(4.5 * math.exp(-0.5) + 0.55) - d3) / d1), rel=1e-15)
    assert d1 == pytest.approx(-2.2172252, rel=1e-7) and d2 == pytest.approx(0.4331230, rel=1e-6)
    # the fitted score -d1 exp(-d2 s / 2) matches -log(c1 exp(-s/2) + c2) - d3 at s = 0 and s = 1 (the two fitting points)
    for res, ratio in ((1.0, 0.55), (0.5, 0.3), (2.0, 0.9)):
        d1, d2 = nr.gauss_constants(res, ratio)
        c1, c2 = 10 * (1 - ratio), ratio / res**3
        d3 = -math.log(c2)
        for s in (0.0, 1.0):
            assert d1 * math.exp(-d2 * s / 2) == pytest.approx(-math.log(c1 * math.exp(-s / 2) + c2) - d3, rel=1e-12)


def _fd_scene(seed):
    rng = np.random.default_rng(seed)
    # three noisy planes and a blob: cells with every shape of covariance
    n = 3000
    pts = np.concatenate([np.c_[rng.uniform(-4, 4, (n, 2)), rng.normal(0, 0.05, n)],
                          np.c_[rng.uniform(-4, 4, n), rng.normal(2, 0.05, n), rng.uniform(-1, 2, n)],
                          np.c_[rng.normal(-3, 0.05, n), rng.uniform(-4, 4, n), rng.uniform(-1, 2, n)],
                          rng.normal([1, -1, 1], 0.4, (n, 3))])
    tgt = np.c_[pts, np.ones(len(pts))].astype(np.float32)
    src = np.c_[pts[rng.choice(len(pts), 400, replace=False)] + rng.normal(0, 0.1, (400, 3)), np.ones(400)].astype(np.float32)
    return nr.Target(tgt, 1.0), src


def _score_frozen(tg, x, pi, ci, p):
    q = x @ nr.transform_double(p)[:3, :3].T + p[:3]
    return nr.pair_terms(tg, q, x, pi, ci, p, small_angle_rule=False)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restated_derivatives_match_finite_differences(seed):
    """g and H are the exact derivatives of the score with the neighbourhoods held fixed (J and H of Magnusson's 6.17-6.21)."""
    tg, src = _fd_scene(seed)
    x = src[:, :3].astype(np.float64)
    rng = np.random.default_rng(seed)
    poses = [np.r_[rng.normal(0, 0.2, 3), rng.normal(0, 0.1, 3)],
             np.r_[rng.normal(0, 0.2, 3), rng.uniform(-3e-5, 3e-5, 3)],           # the small-angle region
             np.r_[rng.normal(0, 0.2, 3), 2.5, -0.7, 1.9]]
    for p in poses:
        q = x @ nr.transform_double(p)[:3, :3].T + p[:3]
        pi, ci = tg.pairs(q.astype(np.float32))
        assert len(pi) > 100
        base = _score_frozen(tg, x, pi, ci, p)
        assert base[0] > 100                                   # pairs contribute
        g, H = base[2:8], nr.symmetric(base)
        h = 1e-6
        g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            up, dn = _score_frozen(tg, x, pi, ci, p + e), _score_frozen(tg, x, pi, ci, p - e)
            assert up[0] == dn[0] == base[0]                   # no pair crossed the exp gate
            g_fd[k] = (up[1] - dn[1]) / (2 * h)
            H_fd[k] = (up[2:8] - dn[2:8]) / (2 * h)
        assert np.abs(g - g_fd).max() <= 1e-6 * np.abs(g).max(), (g, g_fd)
        assert np.abs(H - H_fd).max() <= 1e-6 * np.abs(H).max(), np.abs(H - H_fd).max() / np.abs(H).max()


def test_small_angle_rule():
    j, h = nr.angle_terms(np.array([0, 0, 0, 5e-5, -9e-5, 2e-5]))
    j0, h0 = nr.angle_terms(np.zeros(6))
    assert np.array_equal(j, j0) and np.array_equal(h, h0)
    j1, _ = nr.angle_terms(np.array([0, 0, 0, 2e-4, 0, 0]))
    assert not np.array_equal(j1, j0)


def _random_sums(rng, rank=6, scale=1.0):
    A = rng.normal(size=(6, rank))
    H = (A @ A.T) * scale
    if rng.random() < 0.5:
        H = -H                                    # a maximum: PCL's Hessian of -score is what it solves with
    g = rng.normal(size=6) * scale
    sums = np.zeros(29)
    sums[0] = 100
    sums[1] = -50
    sums[2:8] = g
    sums[8:] = H[np.triu_indices(6)]
    return sums


def _check_step(sums, p, step_size, eps):
    st, p_out, a, T = ndt_step(sums, p, step_size, eps)
    rst, rp, ra, rT, _ = nr.step(sums, p, step_size, eps)
    assert st == rst
    assert a == pytest.approx(ra, rel=1e-9, abs=1e-15)
    assert np.abs(p_out - rp).max() <= 1e-9 * (np.abs(p).max() + ra + 1.0), (p_out, rp)   # (relative to the step's scale)
    assert np.abs(T - rT).max() <= 2e-6 * max(1.0, np.abs(rT).max())
    return st, a


def test_step_matches_restatement_on_random_systems(built):
    rng = np.random.default_rng(11)
    clamped = unclamped = 0
    for i in range(300):
        sums = _random_sums(rng, scale=10.0 ** rng.uniform(-3, 3))
        p = rng.normal(0, 0.5, 6)
        step_size, eps = float(rng.choice([0.1, 1.0, 10.0, 1e3])), float(rng.choice([1e-6, 0.01, 0.1]))
        st, a = _check_step(sums, p, step_size, eps)
        assert st == nr.STEP
        clamped += a == step_size or a == eps / 2
        unclamped += eps / 2 < a < step_size
    assert clamped > 20 and unclamped > 20


def test_step_rank_deficient_uses_the_pseudo_inverse(built):
    rng = np.random.default_rng(5)
    for rank in (1, 3, 5):
        for _ in range(30):
            sums = _random_sums(rng, rank=rank)
            # zero rows / columns: exactly singular, whatever the rounding
            H = nr.symmetric(sums)
            drop = rng.choice(6, 6 - rank, replace=False)
            H[drop, :] = 0
            H[:, drop] = 0
            sums[8:] = H[np.triu_indices(6)]
            _check_step(sums, rng.normal(0, 0.3, 6), 1e3, 1e-6)
    # singular values below sigma_max * 6 * 2^-52 count as zero: a direction with a tiny eigenvalue is not followed
    H = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 5.0 * 2.0**-52])
    sums = np.zeros(29)
    sums[8:] = H[np.triu_indices(6)]
    sums[2:8] = [0, 0, 0, 0, 0, 1.0]
    st, p_out, a, _ = ndt_step(sums, np.zeros(6), 1e3, 1e-6)
    assert st == 1 and a == 0.0                  # delta = 0: the loop stops
    sums[2:8] = [1.0, 0, 0, 0, 0, 1.0]
    st, p_out, a, _ = ndt_step(sums, np.zeros(6), 1e3, 1e-6)
    assert st == 0 and p_out[5] == 0.0 and p_out[0] != 0.0


def test_step_direction_flip_zero_and_nan(built):
    # g . d^ > 0 (H positive definite: the Newton direction of a minimum ascends -score): flipped
    sums = np.zeros(29)
    H = np.diag([2.0, 2, 2, 2, 2, 2])
    sums[8:] = H[np.triu_indices(6)]
    sums[2:8] = [1.0, 0, 0, 0, 0, 0]
    st, p_out, a, _ = ndt_step(sums, np.zeros(6), 0.1, 0.01)
    assert st == 0 and a == pytest.approx(0.1) and p_out[0] == pytest.approx(0.1)   # delta = (-0.5, 0..) flipped to +
    _check_step(sums, np.zeros(6), 0.1, 0.01)
    # H negative definite: delta = (0.5, 0, ..) already has g . d^ > 0: kept
    sums[8:] = (-H)[np.triu_indices(6)]
    st, p_out, a, _ = ndt_step(sums, np.zeros(6), 0.1, 0.01)
    assert st == 0 and p_out[0] == pytest.approx(0.1)
    # g . d^ exactly 0: a = 0 and p stays
    Hs = np.zeros((6, 6))
    Hs[0, 1] = Hs[1, 0] = 1.0
    sums = np.zeros(29)
    sums[8:] = Hs[np.triu_indices(6)]
    sums[2:8] = [1.0, 0, 0, 0, 0, 0]             # delta = (0, -1, 0..): g . d^ = 0
    p = np.array([0.5, 0, 0, 0.2, 0, 0])
    st, p_out, a, T = ndt_step(sums, p, 0.1, 0.01)
    rst, rp, ra, rT, ev = nr.step(sums, p, 0.1, 0.01)
    assert st == rst == 0 and a == ra == 0.0 and not ev
    assert np.array_equal(p_out, p) and np.abs(T - rT).max() <= 1e-6
    # zero delta (no pair: g = 0, H = 0) and NaN delta
    st, p_out, a, _ = ndt_step(np.zeros(29), p, 0.1, 0.01)
    assert st == nr.step(np.zeros(29), p, 0.1, 0.01)[0] == 1 and a == 0.0 and np.array_equal(p_out, p)
    bad = _random_sums(np.random.default_rng(1))
    bad[10] = np.nan
    st, p_out, a, _ = ndt_step(bad, p, 0.1, 0.01)
    assert st == nr.step(bad, p, 0.1, 0.01)[0] == 2 and np.array_equal(p_out, p)


def test_euler_angles_round_trip():
    rng = np.random.default_rng(3)
    for i in range(500):
        ang = rng.uniform(-math.pi, math.pi, 3)
        if i % 5 == 0:
            ang[rng.integers(3)] = 0.0
        R = nr.transform_double(np.r_[0, 0, 0, ang])[:3, :3]
        e = nr.euler_angles(R)
        assert 0.0 <= e[0] <= math.pi and -math.pi <= e[1] <= math.pi and -math.pi <= e[2] <= math.pi
        assert np.abs(nr.transform_double(np.r_[0, 0, 0, e])[:3, :3] - R).max() <= 1e-12
    # small positive angles come back as themselves; the float transform of the result is the guess's rotation to float precision
    ang = np.array([0.1, -0.2, 0.3])
    assert np.allclose(nr.euler_angles(nr.transform_double(np.r_[0, 0, 0, ang])[:3, :3]), ang, atol=1e-14)
    T = nr.transform_float(np.r_[1, 2, 3, ang])
    p0 = nr.initial_pose(T)
    assert np.allclose(p0, np.r_[1, 2, 3, ang], atol=1e-6)
    assert np.array_equal(nr.initial_pose(np.eye(4, dtype=np.float32)), np.zeros(6))


def test_fma32_is_exact():
    rng = np.random.default_rng(9)
    a = rng.normal(size=200000).astype(np.float32)
    b = rng.normal(size=200000).astype(np.float32)
    c = (rng.normal(size=200000) * 1e-3).astype(np.float32)
    got = nr.fma32(a, b, c)
    from fractions import Fraction
    for i in range(0, 200000, 997):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.int32)) & 1))
        assert got[i] == best
