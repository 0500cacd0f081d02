"""One-iteration point-to-point alignments on the device over the edge cases of tests/solve_cases.py whose pairing is set by construction
(source p, target q, spacing at least 20 times the motion): the transform an alignment returns is held to tests/solve_reference.py's
float32 check on the device's OWN sums -- optimal for every input, rank-deficient and tied ones included, nothing left out."""
from fractions import Fraction

import numpy as np
import pytest

import solve_cases as S
import solve_reference as R
from icpslam_amd import Context

pytestmark = pytest.mark.gpu
F32 = np.float32
GATE = 1.0


def cloud(xyz) -> np.ndarray:
    c = np.ones((len(xyz), 4), F32)
    c[:, :3] = xyz
    assert (c[:, :3].astype(np.float64) == xyz).all()
    return c


@pytest.fixture
def one_iteration(built):
    with Context(0) as c:
        c.set_params(c.default_params(), max_iterations=1, force_iterations=1, max_correspondence_distance=GATE)
        yield c


def records(c, n, at=np.eye(4)):
    """The device's pairing at `at` (asserted: every source point with its own target point) and its two sums records."""
    idx, d2 = c.nn(at)
    assert idx.tolist() == list(range(n)) and (d2 <= GATE * GATE).all()
    by_keys = c.reduce(at, GATE)
    by_sweep = c.sweep_sums(at, GATE)
    assert by_keys[0] == by_sweep[0] == n
    return by_keys, by_sweep


@pytest.mark.parametrize("name", S.GPU_CASES)
def test_one_iteration_returns_a_maximiser(one_iteration, name):
    c = one_iteration
    _, p, q = S.case(name)
    n = len(p)
    c.set_target(cloud(q))
    c.set_source(cloud(p))
    by_keys, by_sweep = records(c, n)
    got = c.align()
    assert (got["iterations"], got["n_corr"], got["state"], got["converged"]) == (1, n, 1, True)
    assert got["T"].dtype == F32
    for what, sums in (("reduce", by_keys), ("sweep_sums", by_sweep)):
        m = R.check32(sums, got["T"])
        print(f"{name} against {what}: deficit {m['deficit']:.3f} u32 mag, orth {m['orth']:.2f} u32, t {m['t']:.3f} of its bound")
    host = S.sums_of(p, q)                                   # the case is the one the host tests solved: the same sums, to the device's order
    assert by_sweep[0] == host[0] and np.allclose(by_sweep[1:16], host[1:16], rtol=0, atol=1e-12 * np.abs(host[1:16]).max() * n)


GUESS = np.eye(4)
GUESS[:3, :3] = S.rotation((0.2, 1.0, -0.4), 0.5)
GUESS[:3, 3] = (3.0, -2.0, 1.0)
GUESS = GUESS.astype(F32).astype(np.float64)                  # what the device is given, exactly


@pytest.mark.parametrize("name", S.GPU_GUESS_CASES)
def test_one_iteration_from_a_guess(one_iteration, name):
    """The source is p moved by the guess's inverse, so the guess brings it back onto p: T = float32(Tk guess), Tk the solve of the sums
    at the guess.  T guess^-1 = Tk + (the cast's error) guess^-1 is held to the float32 check, widened by what that one cast of a
    product costs: with dR <= u32 |R_T| and dt <= u32 |t_T| entry by entry, the rotation moves by dR G^-1 (9 u32 |G|_inf more deficit)
    and the translation by dt + dR G^-1 (t_g + mu_p)."""
    c = one_iteration
    _, p, q = S.case(name)
    n = len(p)
    inv = np.eye(4)
    inv[:3, :3] = np.linalg.inv(GUESS[:3, :3])
    inv[:3, 3] = -inv[:3, :3] @ GUESS[:3, 3]
    src =S.f32(p @ inv[:3, :3].T + inv[:3, 3])
    c.set_target(cloud(q))
    c.set_source(cloud(src))
    by_keys, by_sweep = records(c, n, GUESS)
    got = c.align(GUESS)
    assert (got["iterations"], got["n_corr"], got["state"], got["converged"]) == (1, n, 1, True)
    T = got["T"].astype(np.float64)
    Tk = T @ inv
    assert np.abs(Tk[3] - (0, 0, 0, 1)).max() == 0
    Ginv, tg = np.abs(inv[:3, :3]), np.abs(GUESS[:3, 3])
    widen = np.abs(T[:3, :3]) @ Ginv
    for what, sums in (("reduce", by_keys), ("sweep_sums", by_sweep)):
        ex = R.exact(sums)
        reach = tg + np.array([float(abs(v)) for v in ex["mu_p"]])
        extra_t = [R.U32 * Fraction(float(abs(T[a, 3]) + widen[a] @ reach)) for a in range(3)]
        m = R.check(sums, Tk, f32=True, extra_deficit=9 * R.U32 * Fraction(float(np.abs(GUESS[:3, :3]).sum(axis=1).max())), extra_t=extra_t, ex=ex)
        print(f"{name} from a guess, against {what}: deficit {m['deficit']:.3f} u32 mag, orth {m['orth']:.2f} u32, t {m['t']:.3f} of its bound")
    assert np.abs(T[:3, :3] - GUESS[:3, :3]).max() < 0.02 and np.abs(T[:3, 3] - GUESS[:3, 3]).max() < 0.2      # the guess was not dropped
