"""Scenes the sample-consensus rejector's tests share (tests/test_rsac_host.py, tests/test_gpu_rsac.py, tests/test_cpp_rsac.py)."""
from __future__ import annotations

import functools

import numpy as np

import scp_scenes as SC

F32 = np.float32
TRUTH = SC.rigid(0.3, -0.04, 0.02, (1.0, -0.5, 0.2))


@functools.lru_cache(maxsize=None)
def pairs(m: int, inlier_share: float = 0.6, seed: int = 1, noise: float = 0.005, scatter: bool = False):
    """(P, Q): m pairs of float4 points; Q_r = TRUTH * P_r + noise for round(share * m) of them (shuffled), the rest follow another
    motion -- structured outliers that stay close to their P's image -- or, with scatter, lie anywhere in the box."""
    rng = np.random.default_rng(seed)
    P = np.concatenate([rng.uniform(-5, 5, (m, 3)), np.ones((m, 1))], axis=1).astype(F32)
    other = SC.rigid(0.3, -0.04, 0.02, (1.5, -0.5, 0.2))
    Q = SC.moved(P, TRUTH)
    Q[:, :3] += rng.normal(0, noise, (m, 3)).astype(F32)
    out = rng.permutation(m)[int(round(inlier_share * m)):]
    Q[out] = SC.moved(P[out], other)
    if scatter:
        Q[out, :3] = rng.uniform(-5, 5, (out.size, 3)).astype(F32)
    for a in (P, Q):
        a.setflags(write=False)
    return P, Q


# the moved-block scene: a 3000-point scan; a block of about a quarter of the source sits displaced by 0.5 m in the target
BLOCK_TRUTH = SC.rigid(0.01, 0.0, 0.0, (0.12, -0.08, 0.0))
BLOCK_KW = dict(max_iterations=20, max_correspondence_distance=1.0, transformation_epsilon=1e-9)
BLOCK_STAGE = (0.1, 200)     # the stage's inlier threshold and max_iterations
BLOCK_SEEDS = (12345, 1, 2)


# The restatement's worst pose error over BLOCK_SEEDS (degrees, metres; tests/test_rsac_host.py measures and asserts it) and the
# device's bound, twice that (test_scp_host.py's pattern)
E2E_WORST = (0.0162, 0.00258)
E2E_BOUND = (2 * E2E_WORST[0], 2 * E2E_WORST[1])
# Descriptor matches of scp_scenes.e2e_clouds() (FPFH, feature k-nearest with k = 1) through the call of its own: the source is the
# target moved in double and rounded to float32, so a hypothesis from three right matches is exact up to the format.  The restatement
# ends 0.009 degrees and 3.3e-7 m from the truth at worst (seeds 1 .. 3); twice that is below what float32 resolves -- a coordinate of
# 50 m has an ulp of 3.8e-6 m, and a float32 rotation's trace resolves angles only from about acos(1 - 2^-24) = 0.02 degrees -- so
# the bound is the format's: 1e-4 m (26 ulp of the largest coordinate) and 0.05 degrees.
MATCH_KW = dict(inlier_threshold=0.05, max_iterations=1000)
MATCH_SEEDS = (1, 2, 3)
MATCH_BOUND = (0.05, 1e-4)


@functools.lru_cache(maxsize=None)
def moved_block():
    """(source, target, truth, block mask): target = truth * source, but the block (the quarter of the points with the smallest
    azimuth) is shifted by a further 0.5 m along y."""
    source = SC.scan(3000, 5)
    az = np.arctan2(source[:, 1], source[:, 0])
    block = az <= np.quantile(az, 0.25)
    target = SC.moved(source, BLOCK_TRUTH)
    target[block, 1] += F32(0.5)
    target.setflags(write=False)
    return source, target, BLOCK_TRUTH, block


# ---- the core's cases, as the device test runs them (tests/test_gpu_rsac.py); tests/test_rsac_host.py checks on the CPU that the
# well-spread cut leaves out under 10 % of the evaluated hypotheses on every one -------------------------------------------------
GRID_CAP_PAIRS = 1024 * 512      # kSacGridCap workgroups of kSacBlockPoints pairs: one step of the capped counting grid


def with_nan_rows(P, Q, seed: int = 9):
    """Every seventh-or-so pair loses a coordinate to NaN or inf, on either side."""
    rng = np.random.default_rng(seed)
    P, Q = P.copy(), Q.copy()
    m = len(P)
    for side, bad in ((P, np.nan), (Q, np.nan), (P, np.inf), (Q, -np.inf)):
        rows = rng.permutation(m)[:max(1, m // 14)]
        side[rows, rng.integers(0, 3, rows.size)] = bad
    return P, Q


def with_duplicates(P, Q):
    """The pairs twice over, and the first ten a third time."""
    return np.concatenate([P, P, P[:10]]), np.concatenate([Q, Q, Q[:10]])


@functools.lru_cache(maxsize=None)
def core_cases() -> dict:
    """name -> (P, Q, inlier_threshold, max_iterations, seed)"""
    cases = {}
    for m in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 511, 512, 513, 3000):
        cases[f"m{m}"] = (*pairs(m, 0.6, 1), 0.05, 70, 7)
    cases["across_grid_cap"] = (*pairs(GRID_CAP_PAIRS + 513, 0.6, 4), 0.05, 3, 7)
    for it in (0, 1, 63, 64, 65, 129):
        cases[f"it{it}"] = (*pairs(257, 0.2, 3, scatter=True), 0.05, it, 11)
    cases["stops_in_batch_one"] = (*pairs(513, 0.9, 2, scatter=True), 0.05, 1000, 12345)
    cases["runs_to_200"] = (*pairs(513, 0.2, 2, scatter=True), 0.05, 200, 12345)
    cases["nan_rows"] = (*with_nan_rows(*pairs(300, 0.6, 5)), 0.05, 70, 7)
    cases["all_nan_p"] = (np.full((20, 4), np.nan, F32), pairs(20, 0.6, 1)[1], 0.05, 5, 7)
    cases["duplicates"] = (*with_duplicates(*pairs(100, 0.6, 6)), 0.05, 70, 7)
    cases["threshold_zero"] = (*pairs(65, 0.6, 1), 0.0, 70, 7)
    cases["coincident"] = (np.tile(np.array([[1, 2, 3, 1]], F32), (10, 1)), pairs(10, 0.6, 1)[1], 0.05, 70, 7)
    return cases
