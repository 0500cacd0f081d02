"""Point-to-point ICP on the device against its C restatement (oracle/icp_oracle.c, pinned to the NumPy one and to math.fsum in
tests/test_oracle.py), never against the library itself.

replay: every sweep of an oracle alignment (each iteration's float transform, and the last one) runs on the device both ways --
        keys:  ctx.nn + ctx.reduce (reduce_kernel over the keys; the keys equal oracle.nn's bit for bit),
        fused: ctx.sweep_sums (what an iteration of ctx.align launches: nn_wave_kernel below 32768 queries, nn_quad_kernel from
               there on, over the cell-ordered source from 100000 points on; the keys' reduction where no grid serves the gate)
        -- and for both sums[0] is exact, every other sum within 1e-12 * sum |terms| of the oracle's EXACT sum (DESIGN.md section
        3: the device adds in its own order), and +0.0 where sum |terms| is 0.
whole:  ctx.align against oracle.icp_align: converged, iterations, state and n_corr exact, T within the parity tolerances, mse and
        fitness within 1e-9 relative.
Every test asserts from ctx.profile() that the path it means to test is the one that ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from icpslam_amd import Context, IcpGpuError, _lib, synth

pytestmark = pytest.mark.gpu
F = np.float32
R_TOL, T_TOL = 1e-4, 1e-3                                          # BASELINE.json / DESIGN.md section 3
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
GRID, BRUTE, AUTO = _lib.NN_GRID, _lib.NN_BRUTE, _lib.NN_AUTO
QUAD_MIN, ORDER_MIN, GRID_MIN_TARGET = 32768, 100000, 4096         # use_quad, kOrderSourceMin, kGridMinTarget
WORST = {"keys": 0.0, "wave": 0.0, "quad": 0.0, "dR": 0.0, "dt": 0.0}   # reported at the end of the module (-s)
ZERO17 = np.zeros(17, np.uint64)


def _ctx(**kw):
    c = Context(0)
    c.set_params(c.default_params(), **kw)
    return c


def _oparams(kw, **oracle_only):
    return oracle.default_params(**{k: v for k, v in kw.items() if k != "nn_mode"}, **oracle_only)     # (the kd-tree: the same keys, sooner)


def _uses_grid(kw, n_t):
    mode = kw.get("nn_mode", AUTO)
    return mode == GRID or (mode == AUTO and n_t >= GRID_MIN_TARGET)


def fused_kernel(src):
    """which kernel a gated grid sweep of this source is: the cell-ordered copy (finite points only) from 100000 points on"""
    n_q = int(np.isfinite(src[:, :3]).all(axis=1).sum()) if src.shape[0] >= ORDER_MIN else src.shape[0]
    return "quad" if n_q >= QUAD_MIN else "wave"


def within_bound(got, want, mag, path):
    assert got[0] == want[0], (path, got[0], want[0])
    err = np.abs(got - want)
    assert np.all(err <= 1e-12 * mag), (path, (err / np.maximum(mag, 1e-300)).max())
    assert np.array_equal(got[mag == 0].view(np.uint64), ZERO17[: int((mag == 0).sum())]), path      # +0.0, bit for bit
    nz = mag > 0
    if nz.any():
        WORST[path] = max(WORST[path], float((err[nz] / (mag[nz] * 2.0 ** -53)).max()))


def sweeps_of(ref, guess=None):
    """the transforms an alignment sweeps at: the guess, then each iteration's result rounded to float -- the last is the final one"""
    first = np.eye(4, dtype=F) if guess is None else np.asarray(guess, F)
    return [first] + [t["final"].astype(F) for t in ref["trace"]]


def replay(ctx, src, tgt, ref, max_dist=1.0, guess=None, grid=True, keys=True, fused=True):
    """the oracle's sweeps on the device; returns (keys-path sums, fused sums) of every sweep"""
    sweeps, refs, out_keys, out_fused = sweeps_of(ref, guess), [], [], []
    for T in sweeps:
        idx, d2 = oracle.nn(src, tgt, T)
        want = oracle.reduce(src, tgt, T, idx, d2, max_dist, mode=oracle.REDUCE_EXACT)
        mag = oracle.reduce(src, tgt, T, idx, d2, max_dist, mode=oracle.REDUCE_ABS)
        refs.append((want, mag))
        if keys:
            ctx.profile_reset()
            idx_dev, d2_dev = ctx.nn(T)
            p = ctx.profile()
            assert (p.grid_launches, p.nn_launches) == ((1, 0) if grid else (0, 1))
            assert np.array_equal(idx_dev, idx) and np.array_equal(d2_dev.view(np.uint32), d2.view(np.uint32))
            got = ctx.reduce(T, max_dist)
            within_bound(got, want, mag, "keys")
            out_keys.append(got)
    if fused:
        kernel = fused_kernel(src) if grid else "keys"
        for k, (T, (want, mag)) in enumerate(zip(sweeps, refs)):
            ctx.profile_reset()
            got = ctx.sweep_sums(T, max_dist)
            p = ctx.profile()
            assert (p.grid_launches, p.nn_launches, p.reduce_launches) == ((1, 0, 1) if grid else (0, 1, 1))
            if kernel == "quad" and k >= 1:
                assert p.grid_bounded == 1                      # as an alignment's later iterations: the last sweep's neighbours bound this one
            if kernel == "wave":
                assert p.grid_bounded == 0
            within_bound(got, want, mag, kernel)
            out_fused.append(got)
    return out_keys, out_fused


def whole(got, ref, fitness=True, transform=True):
    assert (got["converged"], got["iterations"], got["state"], got["n_corr"]) == \
        (ref["converged"], ref["iterations"], ref["state"], ref["n_corr"]), (got, {k: ref[k] for k in ("converged", "iterations", "state", "n_corr")})
    if transform:
        dR = float(np.abs(got["T"][:3, :3].astype(np.float64) - ref["T"][:3, :3]).max())
        dt = float(np.linalg.norm(got["T"][:3, 3].astype(np.float64) - ref["T"][:3, 3]))
        WORST["dR"], WORST["dt"] = max(WORST["dR"], dR), max(WORST["dt"], dt)
        assert dR <= R_TOL and dt <= T_TOL, (dR, dt)
    assert abs(got["mse"] - ref["mse"]) <= 1e-9 * abs(ref["mse"]), (got["mse"], ref["mse"])
    if fitness:
        assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * abs(ref["fitness"]), (got["fitness"], ref["fitness"])


def check(src, tgt, guess=None, sweeps=True, alignment=True, oracle_only={}, **kw):
    """whole + replay for one case; asserts that the alignment's sweeps took the search the parameters ask for"""
    max_dist = kw.get("max_correspondence_distance", 1.0)
    grid = _uses_grid(kw, tgt.shape[0])
    ref = oracle.icp_align(src, tgt, _oparams(kw, **oracle_only), guess=guess, want_fitness=True, want_trace=True)
    got = sums = None
    with _ctx(**kw) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        if alignment:
            ctx.profile_reset()
            got = ctx.align(guess=guess, want_fitness=True)
            p = ctx.profile()
            n_sweeps = ref["iterations"] + (ref["state"] == NO_CORRESPONDENCES) + 1          # the gated ones and getFitnessScore's
            assert (p.grid_launches, p.nn_launches) == ((n_sweeps, 0) if grid else (0, n_sweeps))
            if grid and fused_kernel(src) == "quad":
                assert p.grid_bounded == n_sweeps - 1
            whole(got, ref)
        if sweeps:
            sums = replay(ctx, src, tgt, ref, max_dist, guess, grid=grid)
    return ref, got, sums


@functools.lru_cache(maxsize=None)
def big_pair():
    """one scan pair for every size below: sources are its first n_s points, targets its first n_t"""
    src, tgt, _ = synth.make_pair(131073, 20000, seed=501)
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt


def _iters(n_s):
    return dict(max_iterations=3) if n_s > 60000 else {}


# ---- source sizes: partial waves and workgroups, the padding workgroups, every change of points per wave, the quad kernel's
# ---- start, the cell-ordered source's start ----------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 63, 64, 65, 255, 257, 1023, 1025, 4097, 16383, 16384, 24575, 24576, 32767, 32768, 32769, 65535, 65536,
         98303, 98304, 99999, 100000, 100001, 131071, 131072, 131073]
TRIOS = [32767, 32768, 32769, 99999, 100000, 100001, 131071, 131072, 131073]


@pytest.mark.parametrize("n_s", SIZES)
def test_source_sizes_grid(n_s):
    src, tgt = big_pair()
    ref, _, _ = check(src[:n_s].copy(), tgt, nn_mode=GRID, **_iters(n_s))
    if n_s < 3:
        assert ref["state"] == NO_CORRESPONDENCES
    elif n_s >= 63:
        assert ref["iterations"] >= 1 and ref["n_corr"] > 0.9 * n_s


@pytest.mark.parametrize("n_t", [4095, 4096, 4097])
@pytest.mark.parametrize("n_s", TRIOS)
def test_source_sizes_auto_around_the_smallest_grid_target(n_s, n_t):
    """AUTO: brute force below kGridMinTarget target points (the keys' reduction is then the alignment's own), the grid from there on"""
    src, tgt = big_pair()
    assert _uses_grid({}, n_t) == (n_t >= 4096)
    ref, _, _ = check(src[:n_s].copy(), tgt[:n_t].copy(), **_iters(n_s))
    assert ref["iterations"] >= 1


# ---- keys path alone ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def million():
    """1,048,577 source points near a 5000-point target, and their oracle keys at T (a point's key does not depend on the others)"""
    tgt = np.ascontiguousarray(big_pair()[1][:5000])
    rng = np.random.default_rng(9)
    src = tgt[rng.integers(0, 5000, (1 << 20) + 1)].copy()
    src[:, :3] += rng.normal(size=(src.shape[0], 3)).astype(F) * F(0.4)
    T = synth.pose_matrix(0.05, -0.03, 0.01, 0.002, -0.001, 0.004).astype(F)
    return src, tgt, T, oracle.nn(src, tgt, T)


@pytest.mark.parametrize("n_s", [1 << 20, (1 << 20) + 1])
def test_a_million_points_run_the_reductions_stride_loop_twice(n_s):
    """reduce_kernel's grid is capped at 1024 workgroups of 256 lanes, four points a lane per trip: 1,048,576 points are exactly one
    trip of every lane, one more point is a second trip of one lane"""
    src, tgt, T, (idx, d2) = million()
    src, idx, d2 = src[:n_s], idx[:n_s], d2[:n_s]
    want = oracle.reduce(src, tgt, T, idx, d2, 1.0, mode=oracle.REDUCE_EXACT)
    mag = oracle.reduce(src, tgt, T, idx, d2, 1.0, mode=oracle.REDUCE_ABS)
    assert 0.5 * n_s < want[0] < n_s
    with _ctx(nn_mode=BRUTE) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        idx_dev, d2_dev = ctx.nn(T)
        p = ctx.profile()
        assert (p.grid_launches, p.nn_launches) == (0, 1)
        assert np.array_equal(idx_dev, idx) and np.array_equal(d2_dev.view(np.uint32), d2.view(np.uint32))
        within_bound(ctx.reduce(T, 1.0), want, mag, "keys")


def test_cell_ordered_source_drops_non_finite_rows_and_the_sums_stay():
    """from 100000 points on the gated sweep reads a cell-ordered copy of the source that holds its finite points only; the keys path
    reads the caller's cloud: the same pairs, the same sums"""
    src, tgt = big_pair()
    src = src[:110000].copy()
    src[::97, 1] = np.nan
    src[5::101, 0] = np.inf
    src[11::4099, 2] = -np.inf
    assert fused_kernel(src) == "quad" and np.isfinite(src[:, :3]).all(axis=1).sum() < 110000 - 2000
    _, _, (by_keys, by_sweep) = check(src, tgt, nn_mode=GRID, max_iterations=3)
    assert [s[0] for s in by_keys] == [s[0] for s in by_sweep]


# ---- accept threshold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [GRID, AUTO])
def test_pairs_exactly_on_the_accept_threshold(mode):
    """A lattice at 0.5 m (eleven layers: 4400 points, a grid under AUTO too) and its top layer lifted by 0.25 m: every d2 is exactly
    0.0625 = r^2 (accepted); every other point lifted one ulp more lies just outside."""
    g = np.arange(0, 10, 0.5, dtype=F)
    xx, yy, zz = np.meshgrid(g, g, g[:11], indexing="ij")
    tgt = np.column_stack([xx.ravel(), yy.ravel(), zz.ravel(), np.ones(xx.size, F)]).astype(F)
    assert tgt.shape[0] >= GRID_MIN_TARGET
    src = tgt[tgt[:, 2] == g[10]].copy()
    src[:, 2] += F(0.25)
    src[1::2, 2] = np.nextafter(src[1::2, 2], F(100))
    _, d2 = oracle.nn(src, tgt)
    half = (src.shape[0] + 1) // 2
    assert (d2 == F(0.0625)).sum() == half and (d2 > F(0.0625)).sum() == src.shape[0] // 2
    ref, got, (by_keys, by_sweep) = check(src, tgt, nn_mode=mode, max_correspondence_distance=0.25, max_iterations=1)
    assert ref["trace"][0]["n_corr"] == half and by_keys[0][0] == half and by_sweep[0][0] == half


# ---- 0, 2, 3 and 4 accepted pairs; min_correspondences -----------------------------------------------------------------------------
def _few_pairs(k):
    """k source points a few centimetres from target points spread over the scene, 300 more half a kilometre away"""
    _, tgt = big_pair()
    near = tgt[:: tgt.shape[0] // 4][:k].copy()
    near[:, :3] += np.array([0.03, -0.02, 0.01], F)
    far = tgt[100:400].copy()
    far[:, 0] += F(500.0)
    return np.concatenate([far[:150], near, far[150:]]).astype(F), tgt


@pytest.mark.parametrize("k", [0, 2, 3, 4])
def test_a_handful_of_accepted_pairs(k):
    src, tgt = _few_pairs(k)
    ref, got, (by_keys, by_sweep) = check(src, tgt, nn_mode=GRID)
    assert by_keys[0][0] == k and by_sweep[0][0] == k
    if k < 3:
        assert (ref["state"], ref["iterations"]) == (NO_CORRESPONDENCES, 0) and np.array_equal(got["T"], np.eye(4, dtype=F))
    else:
        assert ref["iterations"] >= 1
    if k == 0:                                                       # all pairs rejected: every sum +0.0
        assert np.array_equal(by_keys[0].view(np.uint64), ZERO17) and np.array_equal(by_sweep[0].view(np.uint64), ZERO17)


@pytest.mark.parametrize("k", [3, 4])
def test_min_correspondences_at_a_handful(k):
    src, tgt = _few_pairs(k)
    ref, _, _ = check(src, tgt, nn_mode=GRID, min_correspondences=k)
    assert ref["iterations"] >= 1
    ref, _, _ = check(src, tgt, nn_mode=GRID, min_correspondences=k + 1)
    assert (ref["state"], ref["iterations"]) == (NO_CORRESPONDENCES, 0)


def test_min_correspondences_at_its_boundary():
    src, tgt = big_pair()
    src = src[:3000].copy()
    n0 = oracle.icp_align(src, tgt, want_trace=True)["trace"][0]["n_corr"]
    ref, _, _ = check(src, tgt, nn_mode=GRID, min_correspondences=n0)
    assert ref["iterations"] >= 1
    ref, _, _ = check(src, tgt, nn_mode=GRID, min_correspondences=n0 + 1)
    assert (ref["state"], ref["iterations"]) == (NO_CORRESPONDENCES, 0)


# ---- guesses and the loop's parameters: each convergence state, reached on the oracle's side -----------------------------------------
@pytest.mark.parametrize("kw,state", [(dict(max_iterations=1), ITERATIONS),
                                      (dict(max_iterations=6, force_iterations=1), ITERATIONS),
                                      (dict(transformation_epsilon=1e-3), TRANSFORM),
                                      (dict(euclidean_fitness_epsilon=5e-2, max_iterations=30), REL_MSE)])
def test_loop_parameters(kw, state):
    src, tgt, _ = synth.make_pair(8000, 8000, seed=75)
    ref, _, _ = check(src, tgt, nn_mode=GRID, **kw)
    assert ref["state"] == state
    if kw.get("force_iterations"):
        assert ref["iterations"] == 6
    if state in (TRANSFORM, REL_MSE):
        assert 1 < ref["iterations"] < kw.get("max_iterations", 10)


def test_abs_mse_is_reached():
    """a noise-free pair (target = T source, permuted) with the transform test off: the mean squared error settles at the rounding of
    its float distances, and two iterations within 1e-12 of each other end the alignment"""
    src, tgt, _ = synth.make_known_answer_pair(3000, seed=0)
    ref, _, _ = check(src, tgt, nn_mode=GRID, transformation_epsilon=-1.0, max_iterations=200)
    assert ref["state"] == ABS_MSE and 2 < ref["iterations"] < 50


def test_guess():
    src, tgt, _ = synth.make_pair(20000, 20000, seed=73)
    check(src, tgt, nn_mode=GRID, guess=synth.pose_matrix(0.15, -0.1, 0.03, 0.01, -0.02, 0.03).astype(F))
    far = synth.pose_matrix(500.0, 0.0, 0.0, 0.0, 0.0, 0.0).astype(F)    # no pair within 1 m: fewer than min_correspondences
    ref, got, (by_keys, by_sweep) = check(src, tgt, nn_mode=GRID, guess=far)
    assert ref["state"] == NO_CORRESPONDENCES and ref["iterations"] == 0 and np.array_equal(got["T"], far)
    assert np.array_equal(by_sweep[0].view(np.uint64), ZERO17) and np.array_equal(by_keys[0].view(np.uint64), ZERO17)


# ---- non-finite points, duplicates, one target point for every source ------------------------------------------------------------------
def test_non_finite_points_in_both_clouds():
    src, tgt, _ = synth.make_pair(10000, 10000, seed=76)
    src[::97, 1] = np.nan
    src[5::101, 0] = np.inf
    tgt[::89, 2] = np.nan
    tgt[7::103, 1] = -np.inf
    check(src, tgt, nn_mode=GRID)


def test_300_duplicates_of_one_target_point():
    src, tgt, _ = synth.make_pair(10000, 10000, seed=82)
    tgt[5000:5300] = tgt[17]                                         # the lowest index wins; the sums see one q whichever copy is met
    ref, _, _ = check(src, tgt, nn_mode=GRID)
    idx, _ = oracle.nn(src, tgt)
    assert (idx == 17).sum() >= 1 and not ((idx >= 5000) & (idx < 5300)).any()


def test_every_source_point_matches_one_target_point():
    """a cross-covariance of rank 0: the sums are compared, the transform only where it is determined (the criterion of
    tests/test_gpu_grid.py's fuzz test) -- here it is not, and what the loop does with a rotation that is noise is nobody's contract"""
    _, tgt = big_pair()
    q = tgt[1234]
    alone = np.linalg.norm(tgt[:, :3] - q[:3], axis=1)
    assert np.partition(alone, 1)[1] > 0.02
    rng = np.random.default_rng(4)
    src = np.tile(q, (500, 1)).astype(F)
    src[:, :3] += rng.uniform(-2e-3, 2e-3, (500, 3)).astype(F)
    assert (oracle.nn(src, tgt)[0] == 1234).all()
    kw = dict(nn_mode=GRID, max_iterations=1)
    ref = oracle.icp_align(src, tgt, _oparams(kw), want_fitness=True, want_trace=True)
    sm = ref["trace"][0]["sums"]
    S = sm[7:16].reshape(3, 3) / sm[0] - np.outer(sm[4:7] / sm[0], sm[1:4] / sm[0])
    sv = np.linalg.svd(S, compute_uv=False)
    determined = sv[1] > 1e-6 * sv[0] and sv[0] > 1e-9 * max(1.0, float(np.abs(sm[1:7] / sm[0]).max()) ** 2)
    assert not determined
    with _ctx(**kw) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        replay(ctx, src, tgt, dict(trace=[]), 1.0)                     # the sweep at the identity, both ways
        got = ctx.align()
        assert (got["iterations"], got["n_corr"]) == (1, 500)


# ---- cancellation: far from the origin, a wall through the sensor --------------------------------------------------------------------
def _three_km():
    src, tgt, _ = synth.make_pair(20000, 20000, seed=79)
    off = np.array([3000.0, -1200.0, 40.0, 0.0], F)
    return src + off, tgt + off


def test_clouds_3km_from_the_origin_sweeps():
    """sum q p^T is ~1e7 a pair where the covariance it feeds is ~1e2: every sweep of the oracle's alignment, both ways"""
    src, tgt = _three_km()
    check(src, tgt, nn_mode=GRID, alignment=False)


def test_clouds_3km_from_the_origin_alignment():
    """Against the oracle's alignment on EXACT sums (p2p_sums = REDUCE_EXACT), because its sequential sums are the side in error
    here and math.fsum says so: 3 km out they keep ~1e-7 of the covariance, a rotation of that size moves the translation about
    the origin by 0.3 mm, the float32 transform's own step there is 0.2 mm, and every iteration carries the difference on.  With
    the same source in another order (the same pairs, the sums added in another order) the sequential oracle differs from ITSELF
    by |dt| 1.0e-6 m after one iteration (already another float transform: its fitness moves by 3e-7 relative), 3.4e-3 after
    three, 8.1e-3 .. 2.3e-2 and one correspondence after ten; from the exact-sum alignment it ends 2.5e-2 m away.  On the device,
    against the sequential oracle: n_corr 19863 for 19864, |dt| 7.7e-3 m.  The exact-sum alignment depends on no order -- both
    facts are asserted below before the device is looked at -- and every bound stays as it is."""
    src, tgt = _three_km()
    kw = dict(nn_mode=GRID)
    perm = np.random.default_rng(0).permutation(src.shape[0])
    seq, seq_again = oracle.icp_align(src, tgt, _oparams(kw)), oracle.icp_align(src[perm], tgt, _oparams(kw))
    assert np.linalg.norm(seq["T"][:3, 3].astype(np.float64) - seq_again["T"][:3, 3]) > T_TOL
    exact = dict(p2p_sums=oracle.REDUCE_EXACT)
    ref, ref_again = (oracle.icp_align(s, tgt, _oparams(kw, **exact), want_fitness=True) for s in (src, src[perm]))
    assert np.array_equal(ref["T"].view(np.uint32), ref_again["T"].view(np.uint32))
    assert (ref["n_corr"], ref["mse"], ref["fitness"]) == (ref_again["n_corr"], ref_again["mse"], ref_again["fitness"])
    ref, _, _ = check(src, tgt, sweeps=False, oracle_only=exact, **kw)
    assert (ref["state"], ref["iterations"]) == (ITERATIONS, 10)


def test_wall_through_the_sensor():
    wall = synth.wall_through_sensor(30000, seed=4)
    scene = synth.make_pair(20000, 20000, seed=80)[1]
    tgt = np.concatenate([wall, scene]).astype(F)
    src = oracle.transform_cloud(tgt[::2], synth.pose_matrix(0.05, 0.02, 0.0, 0.0, 0.0, 0.01))
    check(src, tgt, nn_mode=GRID)


# ---- the gate and the grid: a sweep whose gate the grid does not serve falls back to the keys --------------------------------------------
def test_a_gate_above_the_grids_cutoff_after_a_smaller_one():
    src, tgt, _ = synth.make_pair(12000, 12000, seed=83)
    T = synth.pose_matrix(0.1, -0.05, 0.02, 0.0, 0.01, 0.02).astype(F)
    idx, d2 = oracle.nn(src, tgt, T)
    with _ctx(nn_mode=GRID, max_correspondence_distance=0.5) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        counts = []
        for k, (r, grid) in enumerate(((0.5, True), (2.0, False), (0.25, True), (0.51, False))):
            ctx.profile_reset()
            got = ctx.sweep_sums(T, r)
            p = ctx.profile()
            assert (p.grid_launches, p.nn_launches, p.reduce_launches) == ((1, 0, 1) if grid else (0, 1, 1)), r
            # the target's grid, for the context's gate, once: a smaller gate keeps it too (the first brute-force sweep of 12000
            # points bins the SOURCE for the matrix-core kernel: nn_keys_brute)
            assert p.grid_builds == (1, 1, 0, 0)[k]
            within_bound(got, oracle.reduce(src, tgt, T, idx, d2, r, mode=oracle.REDUCE_EXACT),
                         oracle.reduce(src, tgt, T, idx, d2, r, mode=oracle.REDUCE_ABS), "wave" if grid else "keys")
            counts.append(got[0])
        assert counts[2] < counts[0] < counts[3] < counts[1]


# ---- the search: brute force, grid and auto ------------------------------------------------------------------------------------------
def test_nn_modes_agree_bit_for_bit():
    src, tgt, _ = synth.make_pair(6000, 6000, seed=72)
    runs = {m: check(src, tgt, nn_mode=m) for m in (BRUTE, GRID, AUTO)}
    bits = lambda sums: np.array(sums).view(np.uint64)
    for m in (GRID, AUTO):
        assert np.array_equal(bits(runs[m][2][0]), bits(runs[BRUTE][2][0]))          # the keys path: one reduction over the same keys
        assert np.array_equal(runs[m][1]["T"].view(np.uint32), runs[BRUTE][1]["T"].view(np.uint32))
    assert np.array_equal(bits(runs[GRID][2][1]), bits(runs[AUTO][2][1]))            # the fused sweep: AUTO is the grid here


# ---- the entry point's refusals ---------------------------------------------------------------------------------------------------------
def test_sweep_sums_refusals():
    src, tgt, _ = synth.make_pair(500, 500, seed=84)
    sums = np.zeros(17)
    dp = sums.ctypes.data_as(C.POINTER(C.c_double))
    with _ctx() as ctx:
        for cloud in (None, src):                                      # nothing set, then a source alone
            if cloud is not None:
                ctx.set_source(cloud)
            with pytest.raises(IcpGpuError) as e:
                ctx.sweep_sums(np.eye(4), 1.0)
            assert e.value.code == _lib.ERR_NO_INPUT
    with _ctx() as ctx:
        ctx.set_target(tgt)
        with pytest.raises(IcpGpuError) as e:                          # a target alone
            ctx.sweep_sums(np.eye(4), 1.0)
        assert e.value.code == _lib.ERR_NO_INPUT
        ctx.set_source(src)
        assert ctx._L.icpgpu_sweep_sums(ctx._h, None, 1.0, None) == _lib.ERR_INVALID_ARG
        for bad in (np.nan, np.inf, -np.inf):
            assert ctx._L.icpgpu_sweep_sums(ctx._h, None, bad, dp) == _lib.ERR_INVALID_ARG
            assert b"max_dist" in ctx._L.icpgpu_last_error(ctx._h)
        ctx.set_params(method=_lib.P2PLANE)
        assert ctx._L.icpgpu_sweep_sums(ctx._h, None, 1.0, dp) == _lib.ERR_INVALID_ARG
        ctx.set_params(method=_lib.P2P_SVD)
        got = ctx.sweep_sums(None, 1.0)                                # T NULL: the identity
        idx, d2 = oracle.nn(src, tgt)
        within_bound(got, oracle.reduce(src, tgt, np.eye(4), idx, d2, 1.0, mode=oracle.REDUCE_EXACT),
                     oracle.reduce(src, tgt, np.eye(4), idx, d2, 1.0, mode=oracle.REDUCE_ABS), "keys")
        ctx.set_target(np.zeros((0, 4), F))                            # an alignment over an empty target runs no sweep
        ctx.profile_reset()
        assert np.array_equal(ctx.sweep_sums(None, 1.0).view(np.uint64), ZERO17)
        p = ctx.profile()
        assert (p.grid_launches, p.nn_launches, p.reduce_launches) == (0, 0, 0)


# ---- the batch: pairs of different block counts in one lock-step launch ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_case():
    """four pairs and what a single alignment makes of each"""
    src, tgt = big_pair()
    srcs = [src[:33000].copy(), src[20000:60001].copy(), src[60000:125536].copy(), src[:100001].copy()]
    tgts = [tgt.copy(), tgt[:12000].copy(), tgt[3000:20001].copy(), tgt[:9000].copy()]
    assert [s.shape[0] for s in srcs] == [33000, 40001, 65536, 100001]
    single = []
    with _ctx(max_iterations=3) as ctx:
        for s, t in zip(srcs, tgts):
            ctx.set_target(t)
            ctx.set_source(s)
            single.append(ctx.align())
    return srcs, tgts, single


@pytest.mark.parametrize("depth", [1, 4])
def test_batch_of_different_sizes_equals_single_alignments(depth, monkeypatch):
    """nn_quad_batch_kernel is launched over the LARGEST pair's workgroups: with four pairs in one group (depth 4, one host thread --
    several threads would take a pair each) the smaller pairs' surplus workgroups leave at once; 100001 points are past the
    lock-step path (cell-ordered source) and run beside it.  Pair by pair the same bits as a single alignment."""
    srcs, tgts, single = batch_case()
    monkeypatch.setenv("ICPGPU_BATCH_DEPTH", str(depth))
    if depth > 1:
        monkeypatch.setenv("ICPGPU_BATCH_THREADS", "1")
    with _ctx(max_iterations=3) as ctx:
        got = ctx.align_batch(srcs, tgts)
    for k, (g, s) in enumerate(zip(got, single)):
        assert (g["converged"], g["iterations"], g["state"], g["n_corr"]) == (s["converged"], s["iterations"], s["state"], s["n_corr"]), k
        assert np.array_equal(g["T"].view(np.uint32), s["T"].view(np.uint32)), k
        assert np.float64(g["mse"]).view(np.uint64) == np.float64(s["mse"]).view(np.uint64), k
    ref = oracle.icp_align(srcs[0], tgts[0], oracle.default_params(max_iterations=3))
    whole(got[0], ref, fitness=False)


# ---- the batch's schedulers: every pair, whichever thread, group, slot or scheduler takes it, is the single alignment ---------------------
@functools.lru_cache(maxsize=None)
def scheduler_case(lockstep):
    """seven pairs of about 6000 x 7000 points, an empty source and an empty target, and what a single alignment (with its fitness)
    makes of each.  One of the seven has a target one point short of kGridMinTarget: AUTO gives it no grid.
    lockstep: the twelve pairs of the several-groups test, in the order in which one thread's groups take them.  A source below
    32768 points (use_quad, icp_grid.hip) never enters a lock-step launch, so three pairs of batch_case's sizes are added; and one
    of the seven gets a source of kOrderSourceMin points (the cell-ordered source is past the lock-step path)."""
    src, tgt, _ = synth.make_pair(6300, 7300, seed=502)
    srcs = [src[40 * k: 40 * k + 6000 + 7 * k].copy() for k in range(7)]
    tgts = [tgt[30 * k: 30 * k + 7000 + 11 * k].copy() for k in range(7)]
    tgts[2] = tgts[2][:GRID_MIN_TARGET - 1].copy()
    empty = np.zeros((0, 4), F)
    if not lockstep:
        srcs[3:3], tgts[3:3] = [empty], [tgts[0].copy()]               # an empty source in the middle, an empty target at the end
        srcs, tgts = srcs + [srcs[0].copy()], tgts + [empty]
        assert len(srcs) == 9
    else:
        big_s, big_t = big_pair()
        srcs[4], tgts[4] = big_s[:ORDER_MIN].copy(), big_t[:7000].copy()
        lock_s = [big_s[:33000].copy(), big_s[20000:60001].copy(), big_s[60000:125536].copy()]
        lock_t = [big_t.copy(), big_t[:12000].copy(), big_t[3000:20001].copy()]
        assert all(QUAD_MIN <= s.shape[0] < ORDER_MIN and t.shape[0] >= GRID_MIN_TARGET for s, t in zip(lock_s, lock_t))
        # taken in this order, two pairs to a group from the eighth on: (lock, lock), (lock, no grid), (empty target)
        srcs = [srcs[0], srcs[1], srcs[3], empty, srcs[4], srcs[5], srcs[6], lock_s[0], lock_s[1], lock_s[2], srcs[2], srcs[0].copy()]
        tgts = [tgts[0], tgts[1], tgts[3], tgts[0].copy(), tgts[4], tgts[5], tgts[6], lock_t[0], lock_t[1], lock_t[2], tgts[2], empty]
        assert len(srcs) == 12 and srcs[4].shape[0] >= ORDER_MIN and tgts[10].shape[0] < GRID_MIN_TARGET
    single = []
    with _ctx(max_iterations=3) as ctx:
        for s, t in zip(srcs, tgts):
            ctx.set_target(t)
            ctx.set_source(s)
            single.append(ctx.align(want_fitness=True))
    return srcs, tgts, single


def same_as_single(got, single, tag):
    assert len(got) == len(single)
    for k, (g, s) in enumerate(zip(got, single)):
        assert (g["converged"], g["iterations"], g["state"], g["n_corr"]) == (s["converged"], s["iterations"], s["state"], s["n_corr"]), (tag, k)
        assert np.array_equal(g["T"].view(np.uint32), s["T"].view(np.uint32)), (tag, k)
        assert np.float64(g["mse"]).view(np.uint64) == np.float64(s["mse"]).view(np.uint64), (tag, k)
        assert g["fitness"] == s["fitness"] or (np.isnan(g["fitness"]) and np.isnan(s["fitness"])), (tag, k, g["fitness"], s["fitness"])


def test_round_robin_scheduler_equals_single_alignments(built, dev_flavour, monkeypatch):
    """ICPGPU_BATCH_LOCKSTEP=0 (development flavour): a host thread drives `depth` workers round-robin, each pair a single-pair
    state machine on its worker's own stream.  One thread x three workers, then two x two, over the same nine pairs."""
    if dev_flavour.delegated:
        return
    monkeypatch.setenv("ICPGPU_BATCH_LOCKSTEP", "0")     # (read once, at the process's first batch: the delegated run is this test alone)
    srcs, tgts, single = scheduler_case(False)
    for threads, depth in ((1, 3), (2, 2)):
        monkeypatch.setenv("ICPGPU_BATCH_THREADS", str(threads))
        monkeypatch.setenv("ICPGPU_BATCH_DEPTH", str(depth))
        with _ctx(max_iterations=3) as ctx:
            got = ctx.align_batch(srcs, tgts, want_fitness=True)
        same_as_single(got, single, (threads, depth))


def test_several_lockstep_groups_on_one_thread(built, monkeypatch):
    """One host thread leading several lock-step groups -- the shape of a 64-pair call, which no other small test reaches (they all
    collapse to one group per thread).  Twelve pairs at a depth of 2: ICPGPU_BATCH_GROUPS unset gives min(8, ceil(12 / 2)) = 6
    groups on the one thread, their first fills capped at 1, 1, 1, 2, 2, 2 pairs; ICPGPU_BATCH_GROUPS=3 gives three, first fills
    1, 2, 2.  The groups take turns filling, so that both ways pairs 7 and 8 share a group and iterate in ONE lock-step launch,
    pair 9 iterates in lock-step beside pair 10 (no grid: the keys path), and the pairs below 32768 source points, the
    cell-ordered source and the empty clouds run as single-pair state machines on their groups' streams."""
    srcs, tgts, single = scheduler_case(True)
    monkeypatch.setenv("ICPGPU_BATCH_THREADS", "1")
    monkeypatch.setenv("ICPGPU_BATCH_DEPTH", "2")
    for groups in (None, 3):
        if groups is None:
            monkeypatch.delenv("ICPGPU_BATCH_GROUPS", raising=False)
        else:
            monkeypatch.setenv("ICPGPU_BATCH_GROUPS", str(groups))
        with _ctx(max_iterations=3) as ctx:
            got = ctx.align_batch(srcs, tgts, want_fitness=True)
        same_as_single(got, single, groups)


def test_zz_report_worst_differences():
    """(the largest differences against the oracle seen by this module; printed with -s)"""
    print(f"\nP2P_SVD vs oracle: worst |dR| {WORST['dR']:.3g}, |dt| {WORST['dt']:.3g} m; worst sum error in units of sum|terms| 2^-53: "
          f"keys (reduce_kernel) {WORST['keys']:.3g}, fused nn_wave_kernel {WORST['wave']:.3g}, fused nn_quad_kernel {WORST['quad']:.3g}")
