"""The three brute-force search kernels at the edges of their launch arithmetic (tests/brute_edge_cases.py):
for every case and every brute_variant the keys of ctx.nn under NN_BRUTE equal oracle.nn's bit for bit, and the sweep's
ICPGPU_DEBUG line names the kernel that was meant to run, in the shape the restated plan gives -- a source grid that refuses
its cloud falls back to the plain kernel silently, and `three kernels agree` would then compare that kernel with itself.

Every expectation comes from oracle.nn, from the restated plans or from the budget in icp_brute_bf16.hip's header (2^-14, half of
tau); none from the kernels.  A test collects every (case, variant) that misses and fails with the list."""
import functools

import numpy as np
import pytest

import brute_edge_cases as B
import oracle
from icpslam_amd import NN_BRUTE, Context

pytestmark = pytest.mark.gpu

BUDGET = 2.0 ** -14
_oracle_cache = {}


def _oracle(case, T):
    key = (case.name, np.asarray(T, np.float32).tobytes())
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.nn(case.src, case.tgt, T)
    return _oracle_cache[key]


@pytest.fixture
def debug_lines(monkeypatch, capfd):
    """sweep(ctx, T) -> (idx, d2, the brute-force lines the call printed)."""
    monkeypatch.setenv("ICPGPU_DEBUG", "1")

    def sweep(c, T):
        capfd.readouterr()
        idx, d2 = c.nn(T)
        return idx, d2, B.parse_lines(capfd.readouterr().err)
    return sweep


def _load(c, case, variant):
    c.set_params(c.default_params(), nn_mode=NN_BRUTE, brute_variant=variant)
    c.set_source(case.src)
    c.set_target(case.tgt)


def _hold(failures, what, case, variant, T, got, seeded=0, check=False):
    """One sweep against the oracle and the restated plan; returns the line (or None)."""
    idx, d2, lines = got
    want_idx, want_d2 = _oracle(case, T)
    wrong = np.flatnonzero((idx != want_idx) | (d2.view(np.uint32) != want_d2.view(np.uint32)))
    if wrong.size:
        i = int(wrong[0])
        failures.append(f"{case.name} | {what}: {wrong.size} of {idx.size} keys differ, first at source row {i}: "
                        f"({idx[i]}, {d2[i]!r}) for the oracle's ({want_idx[i]}, {want_d2[i]!r})")
    if len(lines) != 1:
        failures.append(f"{case.name} | {what}: {len(lines)} brute-force lines for one sweep")
        return None
    line = lines[0]
    plan = B.expected_plan(case, variant, line["num_cus"], check)
    matrix = plan.kernel != "valu"
    want = B.line_of(plan, B.finite_rows(case.src) if matrix else case.src.shape[0], case.src.shape[0], case.tgt.shape[0],
                     line["num_cus"], seeded if matrix else 0)
    if line != want or line["num_cus"] < 1:
        failures.append(f"{case.name} | {what}: the line says {line}, the restated plan {want}")
    return line


def _run_group(cases, sweep, variants, check=False):
    failures = []
    with Context(0) as c:
        for case in cases:
            for variant in variants:
                _load(c, case, variant)
                _hold(failures, f"variant {variant}" + (" check" if check else ""), case, variant, case.T, sweep(c, case.T), check=check)
        prof = c.profile()
    assert not failures, "\n".join(failures)
    return prof


@pytest.mark.parametrize("group", list(B.GROUPS))
def test_keys_and_launch_shape(built, debug_lines, group):
    _run_group(list(B.GROUPS[group]()), debug_lines, (0, 2, 1))


def _held_budget(prof):
    assert prof.brute_bound_violations == 0
    assert prof.brute_bound_worst < BUDGET, prof.brute_bound_worst


@pytest.mark.parametrize("group", list(B.GROUPS))
def test_bound_check_shape(built, dev_flavour, debug_lines, monkeypatch, group):
    """The bf16 kernel's second instantiation <2, 512, 256, true>: every pair's bound against its exact distance."""
    if dev_flavour.delegated:     # ICPGPU_MFMA_CHECK_BOUND exists only in the development flavour (icp_env.h)
        return
    monkeypatch.setenv("ICPGPU_MFMA_CHECK_BOUND", "1")
    _held_budget(_run_group(list(B.GROUPS[group]()), debug_lines, (0,), check=True))


def _num_cus(c, sweep):
    probe = next(iter(B.target_shape_cases(33)))
    _load(c, probe, 1)
    return sweep(c, probe.T)[2][0]["num_cus"]


def _multi_tile(sweep, plans, variants, check=False):
    """(c): 65 537 sources and a target sized, from the CU count the line reports, so that every split holds two tiles and the
    last one ends in a tile of 1, 33, 64 or TILE - 1 rows."""
    failures = []
    with Context(0) as c:
        num_cus = _num_cus(c, sweep)
        cases = {}
        for variant, fn in plans.items():
            for lim in B.MULTI_TILE_LIMS[fn(1, 1, 1).tile]:
                case = cases.setdefault((B.multi_tile_targets(fn, num_cus, lim), lim), B.multi_tile_case(fn, num_cus, lim))
                for v in variants:
                    _load(c, case, v)
                    line = _hold(failures, f"variant {v}" + (" check" if check else ""), case, v, case.T, sweep(c, case.T), check=check)
                    if v == variant and line is not None:      # the shape this size was derived for was reached
                        rem = line["n_t"] - (line["splits"] - 1) * line["per"]
                        last = rem - (rem - 1) // line["TILE"] * line["TILE"]
                        if not (line["per"] >= 2 * line["TILE"] and rem > line["TILE"] and last == lim):
                            failures.append(f"{case.name} | variant {v}: the shape was not reached: {line}")
        prof = c.profile()
    assert not failures, "\n".join(failures)
    return prof


def test_several_tiles_per_split(built, debug_lines):
    _multi_tile(debug_lines, {0: B.plan_bf16, 2: B.plan_mfma}, (0, 2, 1))


def test_several_tiles_per_split_bound_check_shape(built, dev_flavour, debug_lines, monkeypatch):
    if dev_flavour.delegated:
        return
    monkeypatch.setenv("ICPGPU_MFMA_CHECK_BOUND", "1")
    _held_budget(_multi_tile(debug_lines, {0: functools.partial(B.plan_bf16, check=True)}, (0,), check=True))


@pytest.mark.parametrize("variant", [0, 2])
def test_seeded_sweeps(built, debug_lines, variant):
    """(g): a second sweep in the same context at the same pose (on the lattice: one lattice step away, where every seed is
    tied with the new neighbour but no longer the lowest row) and a third 5 m and 0.5 rad away, where most seeds are poor:
    the line says `seeded 1`, the keys are the oracle's at that pose and those of a fresh context."""
    failures = []
    with Context(0) as c:
        for case, T2, T3 in B.seeded_cases():
            _load(c, case, variant)
            _hold(failures, f"variant {variant} first sweep", case, variant, case.T, debug_lines(c, case.T))
            for what, T in (("second", T2), ("third", T3)):
                got = debug_lines(c, T)
                _hold(failures, f"variant {variant} {what} sweep", case, variant, T, got, seeded=1)
                with Context(0) as fresh:
                    _load(fresh, case, variant)
                    new = debug_lines(fresh, T)
                _hold(failures, f"variant {variant} {what} pose, fresh context", case, variant, T, new)
                if not (np.array_equal(got[0], new[0]) and np.array_equal(got[1].view(np.uint32), new[1].view(np.uint32))):
                    failures.append(f"{case.name} | variant {variant} {what} sweep: not the keys of a fresh context")
    assert not failures, "\n".join(failures)
