"""CPU tests of the NDT More-Thuente step rule (icpgpu_set_ndt_line_search, ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE): the library's
host replay of the search (icpgpu_ndt_line_search_replay) against the NumPy restatement (tests/ndt_line_search_restated.py) on
More & Thuente's test functions and on seeded families of observations, every trial-value case and interval update, every exit,
the two deviations (a NaN candidate step, a non-finite trial), and the header as C99."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import ndt_line_search_restated as ls
from icpslam_amd import _lib
from icpslam_amd._lib import IcpGpuError
from icpslam_amd.registration import ndt_line_search_replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _replay_all(phi_0, d_phi_0, step_init, step_max, step_min, r):
    """Replays the restatement's search r through the library, prefix by prefix: every trial step, then the exit."""
    n = len(r["steps"])
    for k in range(n):
        st, a, t = ndt_line_search_replay(phi_0, d_phi_0, step_init, step_max, step_min, r["phi"][:k], r["d_phi"][:k])
        assert (st, t) == (_lib.MT_TRIAL, k), (k, st, t, r["exit"])
        assert a == r["steps"][k], (k, a, r["steps"][k])
    st, a, t = ndt_line_search_replay(phi_0, d_phi_0, step_init, step_max, step_min, r["phi"], r["d_phi"])
    assert (st, t) == (r["exit"], r["final"]), (st, t, r["exit"], r["final"])
    assert a == r["step"]
    return st


def _search_both(fn, phi_0, d_phi_0, step_init, step_max, step_min):
    r = ls.search(fn, phi_0, d_phi_0, step_init, step_max, step_min)
    _replay_all(phi_0, d_phi_0, step_init, step_max, step_min, r)
    return r


@pytest.mark.parametrize("k", [1, 2, 4])
def test_replay_matches_the_restatement_on_more_thuente_functions(built, k):
    fn = ls.mt_function(k)
    phi_0, d_phi_0 = fn(0.0)
    assert d_phi_0 < 0
    for step_init in (1e-3, 1e-1, 1e1, 1e3):
        r = _search_both(fn, phi_0, d_phi_0, step_init, 1e10, 1e-20)
        assert r["exit"] == ls.WOLFE
        a = r["step"]
        # the accepted step satisfies PCL's tests: sufficient decrease and phi'(a) <= -nu phi'(0)
        phi_a, dphi_a = fn(a)
        assert phi_a <= phi_0 + ls.MU * d_phi_0 * a
        assert dphi_a <= -ls.NU * d_phi_0


def _family(seed):
    """A seeded phi(a): a quadratic + sinusoid, with phi and phi' perturbed by seeded ripples (phi' then no longer phi's derivative),
    so that every reachable branch of the search is taken, with the search's parameters."""
    rng = np.random.default_rng(seed)
    c1 = -abs(rng.normal(1.0, 1.0)) - 1e-3
    c2 = rng.normal(0.0, 3.0)
    amp, w = abs(rng.normal(0.0, 0.5)), rng.uniform(1.0, 40.0)
    noise, phi_noise = rng.choice([0.0, 0.3, 3.0, 30.0]), rng.choice([0.0, 0.1, 1.0])
    shift = rng.normal(0.0, 1.0)

    def fn(a, c1=c1):
        phi = c1 * a + c2 * a * a + amp * math.sin(w * a) + phi_noise * math.sin(29.0 * a + shift)
        dphi = c1 + 2 * c2 * a + amp * w * math.cos(w * a)
        return phi, dphi + noise * math.sin(17.0 * a + shift)

    phi_0, d_phi_0 = fn(0.0)
    if d_phi_0 >= 0:
        c1 -= d_phi_0 + 0.1
        fn = functools.partial(fn, c1=c1)
        phi_0, d_phi_0 = fn(0.0)
    step_max = float(10 ** rng.uniform(-1.5, 1.0))
    step_min = float(step_max * 10 ** rng.uniform(-6, -0.3))
    step_init = float(10 ** rng.uniform(-3, 2))
    return fn, phi_0, d_phi_0, step_init, step_max, step_min


def test_replay_matches_the_restatement_and_reaches_every_case(built):
    """3000 seeded searches, trial by trial.  Trial-value case 2 (f_t <= f_l, g_t (a_l - a_t) > 0) is unreachable under PCL's order
    of operations: at the first selection a_l = 0, f_l = 0, and case 2's conditions imply the Wolfe test, which
    ends the search first; after an update that leaves f_t <= f_l, a_l = a_t, so g_t (a_l - a_t) = 0.  Every other case, every
    interval update and every exit but the non-finite one (tested below) is reached."""
    cases, updates, clamps, exits = set(), set(), set(), set()
    for seed in range(3000):
        fn, phi_0, d_phi_0, step_init, step_max, step_min = _family(seed)
        r = _search_both(fn, phi_0, d_phi_0, step_init, step_max, step_min)
        cases |= set(r["log"].cases)
        updates |= set(r["log"].updates)
        clamps |= set(r["log"].clamps)
        exits.add(r["exit"])
        if r["exit"] == ls.WOLFE:                                               # the accepted step passes PCL's tests
            a, k = r["step"], r["final"]
            assert r["phi"][k] - phi_0 - ls.MU * d_phi_0 * a <= 0 and r["d_phi"][k] <= -ls.NU * d_phi_0
        assert step_min <= r["step"] <= step_max
        assert len(r["steps"]) <= 1 + ls.MAX_LOOP_TRIALS
    assert cases == {1, 3, 4}, cases
    assert updates == {"U1", "U2", "U3", "converged"}, updates
    assert clamps == {"max", "min"}, clamps
    assert exits == {ls.WOLFE, ls.INTERVAL, ls.TRIAL_CAP, ls.NAN_STEP}, exits


def test_case_2_of_the_restatement():
    """Case 2 on its own (the search never reaches it): the cubic when it lies at least as far from a_t as the secant, else the
    secant."""
    log = ls.Log(1.0, 1.0, 1.0)
    a_l, f_l, g_l, a_t, f_t, g_t = 0.5, 0.0, -1.0, 0.2, -0.1, 2.0            # a_t < a_l, g_t > 0: g_t (a_l - a_t) > 0
    got = ls.trial_value(log, a_l, f_l, g_l, 0.0, 0.0, 0.0, a_t, f_t, g_t)
    z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
    w = math.sqrt(z * z - g_t * g_l)
    a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)
    a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
    assert log.cases == [2]
    assert got == (a_c if abs(a_c - a_t) >= abs(a_s - a_t) else a_s)


def test_interval_convergence_exit(built):
    """updateIntervalMT's fourth branch (f_t <= f_l and g_t (a_l - a_t) == 0): the search ends at that trial."""
    seen = 0
    for seed in range(3000):
        fn, phi_0, d_phi_0, step_init, step_max, step_min = _family(seed)
        r = ls.search(fn, phi_0, d_phi_0, step_init, step_max, step_min)
        if r["exit"] != ls.INTERVAL:
            continue
        seen += 1
        assert r["log"].updates[-1] == "converged" and r["final"] == len(r["steps"]) - 1 and r["step"] == r["steps"][-1]
        assert _replay_all(phi_0, d_phi_0, step_init, step_max, step_min, r) == _lib.MT_INTERVAL
    assert seen >= 5, seen


def test_interval_starts_converged_when_step_min_exceeds_step_max(built):
    """transformation_epsilon / 2 > step_size: (step_max - step_min) < 0, the first trial (at step_min) is the step."""
    st, a, t = ndt_line_search_replay(0.0, -1.0, 0.3, 0.1, 0.5, [10.0], [5.0])
    assert (st, a, t) == (_lib.MT_INTERVAL, 0.5, 0)


def _family_searches(pred):
    """The seeded searches of _family for which pred(r) holds, each checked against the library trial by trial."""
    out = []
    for seed in range(3000):
        args = _family(seed)
        r = ls.search(*args)
        if pred(r):
            _replay_all(*args[1:], r)
            out.append((args, r))
    return out


def test_the_trial_cap(built):
    found = _family_searches(lambda r: r["exit"] == ls.TRIAL_CAP)
    assert len(found) >= 5
    for _, r in found:
        assert len(r["steps"]) == 1 + ls.MAX_LOOP_TRIALS and r["final"] == ls.MAX_LOOP_TRIALS and r["step"] == r["steps"][-1]


def test_clamped_at_step_min_and_step_max(built):
    st, a, t = ndt_line_search_replay(0.0, -1.0, 1e-9, 0.1, 0.05, [], [])
    assert (st, a, t) == (_lib.MT_TRIAL, 0.05, 0)                              # |delta| below eps / 2
    st, a, t = ndt_line_search_replay(0.0, -1.0, 7.0, 0.1, 0.05, [], [])
    assert (st, a, t) == (_lib.MT_TRIAL, 0.1, 0)                                # |delta| above step_size
    # loop candidates below step_min land on it (in the family above, loop candidates never pass step_max: the cubic and the
    # safeguard stay within the trials seen so far)
    found = _family_searches(lambda r: r["step"] == r["steps"][-1] and len(r["steps"]) > 1 and
                             r["steps"][-1] == min(r["steps"]) and "min" in r["log"].clamps)
    assert len(found) >= 5
    for (fn, phi_0, d_phi_0, step_init, step_max, step_min), r in found:
        assert step_min in r["steps"][1:]


def test_a_nan_candidate_ends_the_search_at_the_last_trial(built):
    """Deviation 3: a cubic's square root of a negative number makes the candidate NaN, PCL's clamp passes it
    through, and here the search ends at the last trial (whose sums are known)."""
    found = _family_searches(lambda r: r["exit"] == ls.NAN_STEP)
    assert found
    for (fn, phi_0, d_phi_0, step_init, step_max, step_min), r in found:
        assert r["final"] == len(r["steps"]) - 1 and r["step"] == r["steps"][-1]


def test_a_non_finite_trial(built):
    """Deviation 4: a loop trial whose phi or phi' is not finite ends the search at the previous trial; a non-finite
    first trial is the step (as under PCL 1.8's rule: the next Newton solve sees its sums)."""
    for bad in ((math.nan, -1.0), (-1.0, math.nan), (math.inf, -1.0), (-1.0, -math.inf)):
        st, a, t = ndt_line_search_replay(0.0, -1.0, 0.08, 0.1, 0.05, [bad[0]], [bad[1]])
        assert (st, a, t) == (_lib.MT_NON_FINITE, 0.08, 0)
        # first trial rises (case 1 -> the next trial), then the bad one
        st, a, t = ndt_line_search_replay(0.0, -1.0, 0.1, 0.1, 0.01, [0.5], [4.0])
        assert st == _lib.MT_TRIAL and 0.01 <= a < 0.1
        second = a
        st, a, t = ndt_line_search_replay(0.0, -1.0, 0.1, 0.1, 0.01, [0.5, bad[0]], [4.0, bad[1]])
        assert (st, a, t) == (_lib.MT_NON_FINITE, 0.1, 0)
        r = ls.search(lambda x: (0.5, 4.0) if x == 0.1 else bad, 0.0, -1.0, 0.1, 0.1, 0.01)
        assert r["steps"] == [0.1, second] and (r["exit"], r["final"], r["step"]) == (ls.NON_FINITE, 0, 0.1)


def test_replay_refuses_bad_arguments(built):
    for args in ((0.0, 0.0, 1.0, 0.1, 0.05), (0.0, 1.0, 1.0, 0.1, 0.05), (math.nan, -1.0, 1.0, 0.1, 0.05),
                 (0.0, math.nan, 1.0, 0.1, 0.05)):
        with pytest.raises(IcpGpuError):
            ndt_line_search_replay(*args)
    with pytest.raises(IcpGpuError):                                            # an observation past the exit (Wolfe at trial 0)
        ndt_line_search_replay(0.0, -1.0, 0.1, 0.1, 0.05, [-1.0, -2.0], [0.0, 0.0])
    L = _lib.load()
    assert L.icpgpu_ndt_line_search_replay(0.0, -1.0, 0.1, 0.1, 0.05, None, None, 1, None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_set_ndt_line_search(None, 1) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_get_ndt_line_search(None, None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_ndt_line_search_trace(None, 0, None, None, None, None, None) == _lib.ERR_INVALID_ARG


def test_header_compiles_as_c_with_the_line_search(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){ icpgpu_ndt_line_search m = ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE; icpgpu_ndt_mt_exit e = '
                   'ICPGPU_NDT_MT_NON_FINITE;\n'
                   '  double phi[1] = {-1.0}, dphi[1] = {0.0}, a; int t;\n'
                   '  int (*f1)(icpgpu_ctx*, int) = icpgpu_set_ndt_line_search;\n'
                   '  int (*f2)(const icpgpu_ctx*, int*) = icpgpu_get_ndt_line_search;\n'
                   '  int (*f3)(icpgpu_ctx*, const double*, double*) = icpgpu_ndt_gradient;\n'
                   '  int (*f4)(const icpgpu_ctx*, size_t, int32_t*, double*, double*, double*, size_t*) = icpgpu_ndt_line_search_trace;\n'
                   '  int rc = icpgpu_ndt_line_search_replay(0.0, -1.0, 0.3, 0.1, 0.05, phi, dphi, 1, &a, &t);\n'
                   '  (void)f1; (void)f2; (void)f3; (void)f4;\n'
                   '  printf("%d %d %d %d %d %.17g\\n", (int)m, (int)e, ICPGPU_HEADER_VERSION, rc, t, a); return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(exe), "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    m, e, version, rc, t, a = subprocess.check_output([str(exe)], text=True).split()
    assert (int(m), int(e), int(version)) == (1, 5, 1002)
    assert (int(rc), int(t), float(a)) == (_lib.MT_WOLFE, 0, 0.1)


def test_the_python_and_cpp_front_ends_carry_the_switch(built, tmp_path):
    from icpslam_amd import NormalDistributionsTransform
    ndt = NormalDistributionsTransform.__new__(NormalDistributionsTransform)   # (no device: the setters alone)
    ndt._ndt = dict(resolution=1.0, step_size=0.1, outlier_ratio=0.55, line_search=_lib.NDT_LINE_SEARCH_PCL18)
    assert ndt.getMoreThuenteLineSearch() is False
    ndt.setMoreThuenteLineSearch(True)
    assert ndt.getMoreThuenteLineSearch() is True and ndt._ndt["line_search"] == _lib.NDT_LINE_SEARCH_MORE_THUENTE
    ndt.setMoreThuenteLineSearch(False)
    assert ndt._ndt["line_search"] == _lib.NDT_LINE_SEARCH_PCL18
    src = tmp_path / "t.cpp"
    src.write_text('#include "icpgpu_registration.hpp"\n#include <vector>\n#include <memory>\n'
                   'struct alignas(16) P { float x, y, z, w; };\n'
                   'struct Cloud { std::vector<P> points; using Ptr = std::shared_ptr<Cloud>; };\n'
                   'int main() { using N = icpgpu::NormalDistributionsTransform<Cloud>; void (N::*s)(bool) = &N::setMoreThuenteLineSearch;\n'
                   '  bool (N::*g)() const = &N::getMoreThuenteLineSearch; (void)s; (void)g; return 0; }\n')
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src)])
