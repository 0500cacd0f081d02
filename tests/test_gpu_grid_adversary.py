"""The grid searches' early exits on clouds built ON the grid the library built (tests/grid_adversary.py):
every certificate is met at its edge from both sides, and every answer is held, bit for bit, against a CPU reference -- oracle.nn
and oracle.icp_align for the point-to-point search, tests/search_restated.py for the search cloud, tests/outlier_restated.py for
the outlier filters.  The device's brute-force kernel is a second witness only.  No tolerance anywhere but the 1e-12 (relative) on
the one-iteration alignment's mse that test_fuzz_grid_keys_equal_brute_force already grants two summation orders.

What the gadgets catch was MEASURED with one-line mutants of the device code (a wrong answer is all any of them can produce), each
run against this file and against the older tests of the code it touches (test_gpu_grid.py for (a)-(e), (i), (j), test_gpu_search.py
for (f), (g), test_gpu_outlier.py for (h)):

    mutant                                                   this file: caught by                                  older tests
    (a) margin without its z term (both octant_row's)        yes  nn, gate edge, one iteration (plain, sparse)     yes  test_grid_nn_equals_brute_and_oracle
    (b) cube certificate with rho + 1                        yes  nn, gate edge, one iteration, mis-binned         yes  test_grid_nn_equals_brute_and_oracle
    (c) xb = floorf(fx + w) - 1 in grow_cubes                yes  nn, gate edge, previous neighbour, mis-binned    yes  test_grid_nn_equals_brute_and_oracle
    (d) previous-neighbour bound taken at the old pose       yes  previous neighbour (both gates), nothing else    yes  test_cell_ordered_source_same_answer_...
    (e) r_max by floor                                       yes  gate edge, one iteration's n_corr, radius filter yes  test_align_all_modes_match_oracle
    (f) search_knn_kernel's certificate with rho + 1         yes  search_knn shell certificate                     yes  test_knn_sizes
    (g) radius R by floor                                    yes  search_radius cube                               yes  test_query_counts
    (h) the outlier walk's certificate with rho + 1          yes  outlier walk (mean_k 1 and 19)                   yes  test_sor_sizes
    (i) kGridSafety = 1                                      NO   all 32 pass                                      NO   all 341 pass
    (j) no grid_slack, no 1.03125 inflation                  yes  previous neighbour [odd], mis-binned [0.07]      yes  test_fuzz_quad_kernel_...[4]

The older tests already catch every one of (a) to (h), most within their first cases: random clouds are dense enough in edge
cases for changes of this size.  What this file adds is that each certificate is met at its bound by construction, from both
sides, on every regime of the cell plan, in about 10 s for the whole file; (d) is the one mutant a single gadget family owns.
(i) is a finding: with 63/64 replaced by 1 nothing fails anywhere -- the safety factor covers the float binning's rounding,
which the mis-binned gadgets show to be 2^-9 of a cell where an axis is ~2^14 cells long, far inside 1/64; no input here
(or in the older tests) needs it.  (j) fails only where rounding decides: a gadget whose row is tangent to the ball, and a
point binned one cell off at the far end of a long axis.

ctx.nn() has no gate (its cubes grow to four times the gate's, what is left goes to brute force), so the gate's edge -- "B at
gate * (1 + 2^-12) stays unmatched" -- is held through ctx.correspondences() (idx == -1) and the alignment's n_corr.
Queries are padded to the size a kernel takes over at (32 768: nn_quad_kernel; 100 000: the cell-ordered source) with further
copies of the gadgets' own queries: a translated copy of a gadget would need its cloud points copied too, and every copy here
still sits exactly on its edge.
"""
import math
import os
import tempfile

import numpy as np
import pytest

import grid_adversary as GA
import oracle
import outlier_restated as OR
from icpslam_amd import NN_BRUTE, NN_GRID
from test_gpu_search import check_knn, check_radius

pytestmark = pytest.mark.gpu

F32 = np.float32
LO = np.array([-13.37, 7.21, -2.9])
# Gates.  DYADIC was found on the CPU: with the host's present plan (the first cell size is the gate's cutoff / 4.5) it is a
# gate whose cell size rounds to exactly 1/4; the tests READ h and only assert what they read.
GATES = {"odd": 1.0, "dyadic": 1.12499892}
# per regime: the box (in gates), the filler (clumps x points per clump) and how many gadgets of each maker
REGIMES = {
    "plain": dict(box=(32.0, 32.0, 30.0), filler=(100, 40), octant=288, cube_signs=2, chord=48, gate=48),
    "sparse": dict(box=(66.0, 66.0, 66.0), filler=(0, 0), octant=288, cube_signs=2, chord=48, gate=48),
    "dense": dict(box=(13.9, 13.9, 15.2), filler=(2, 2000), octant=36, cube_signs=1, cube_extra=18, chord=12, gate=24),   # (r_max = 17: 36-cell blocks;
    # cube_extra: 18 more radius-1 cube gadgets, two of the first 18 are certified by the octant)
}
BOUND_ON = os.environ.get("ICPGPU_QUAD", "1") != "0" and os.environ.get("ICPGPU_PREV", "1") != "0"


def captured_stderr(fn):
    """fn() with the process's stderr (the library writes there from C) in a file: its text"""
    with tempfile.TemporaryFile(mode="w+b") as f:
        saved = os.dup(2)
        try:
            os.dup2(f.fileno(), 2)
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode(errors="replace")


def probing(ctx, action):
    """probe(cloud) -> Grid for GA.build_scene: action(cloud) makes the library build its grid over the cloud"""
    def probe(cloud):
        old = os.environ.get("ICPGPU_DEBUG")
        os.environ["ICPGPU_DEBUG"] = "1"
        try:
            text = captured_stderr(lambda: action(cloud))
        finally:
            if old is None:
                del os.environ["ICPGPU_DEBUG"]
            else:
                os.environ["ICPGPU_DEBUG"] = old
        return GA.read_grid(text, len(cloud))
    return probe


def p2p_action(ctx, gate):
    def action(cloud):
        ctx.set_params(ctx.default_params(), nn_mode=NN_GRID, max_correspondence_distance=gate)
        ctx.set_source(cloud[:1])
        ctx.set_target(cloud)
        ctx.nn(np.eye(4))
    return action


def fixed_points(gate, box, filler, seed=0):
    lo = LO
    hi = lo + np.array(box) * gate
    pts = [np.array([lo, hi], F32)]
    if filler[0]:
        side = int(math.ceil(math.sqrt(filler[0])))
        pts.append(GA.clumps(lo + 0.5 * gate, gate, side, -(-filler[0] // side), 1e-3 * gate, filler[1], seed))
    return np.concatenate(pts)


_SCENES = {}


def p2p_scene(ctx, regime, gate_name):
    key = ("p2p", regime, gate_name)
    if key not in _SCENES:
        gate, r = GATES[gate_name], REGIMES[regime]

        def plan(grid, blocks):
            return [GA.make_octant(grid, blocks.take(r["octant"])), GA.make_cube(grid, blocks.take(18 * r["cube_signs"] * len(grid.ladder()) + r.get("cube_extra", 0))),
                    GA.make_chord(grid, blocks.take(r["chord"])), GA.make_gate(grid, blocks.take(r["gate"]), gate)]
        s = GA.build_scene(probing(ctx, p2p_action(ctx, gate)), fixed_points(gate, r["box"], r["filler"]), plan,
                           lambda g: 2 * g.r_max + (2 if regime == "dense" else 3))
        s.ref = {}
        _SCENES[key] = s
    return _SCENES[key]


def padded(queries, n):
    """the gadgets' queries, repeated up to at least n of them"""
    return np.tile(queries, (-(-n // len(queries)), 1)) if n > len(queries) else queries


def oracle_nn(scene, n):
    """oracle.nn of the padded queries against the scene's cloud, once per scene and size"""
    if ("nn", n) not in scene.ref:
        io, do = oracle.nn(scene.queries, scene.cloud, np.eye(4))
        reps = -(-n // len(scene.queries)) if n > len(scene.queries) else 1
        scene.ref[("nn", n)] = (np.tile(io, reps), np.tile(do, reps))
    return scene.ref[("nn", n)]


def same_keys(got, want, what):
    (ig, dg), (iw, dw) = got, want
    bad = np.flatnonzero((ig != iw) | (dg.view(np.uint32) != dw.view(np.uint32)))
    assert bad.size == 0, (what, bad.size, bad[:8], ig[bad[:8]], iw[bad[:8]], dg[bad[:8]], dw[bad[:8]])


def nn_both_modes(ctx, src, cloud, gate):
    out = {}
    for mode in (NN_GRID, NN_BRUTE):
        ctx.set_params(ctx.default_params(), nn_mode=mode, max_correspondence_distance=gate)
        ctx.set_source(src)
        ctx.set_target(cloud)
        ctx.profile_reset()
        out[mode] = ctx.nn(np.eye(4))
        p = ctx.profile()
        assert (p.grid_launches, p.nn_launches) == ((1, 0) if mode == NN_GRID else (0, 1))
    return out


def regime_asserts(scene, regime, plain_h=None):
    g = scene.grid
    if regime == "plain":
        assert g.attempt == 0 and 20.0 <= g.pop, g            # the first cell size is kept
    elif regime == "sparse":
        assert g.attempt >= 1 and g.pop < 20.0, g             # doubled cells
    else:
        assert g.attempt == 1 and g.pop > 44.0, g             # shrunk cells
    if plain_h is not None and regime != "plain":
        assert (g.h > plain_h) if regime == "sparse" else (g.h < plain_h), (g.h, plain_h)


# ---- point-to-point search --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate_name", list(GATES))
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("n_q", [0, 32768])
def test_nn_on_the_grids_own_edges(ctx, regime, gate_name, n_q):
    """ctx.nn with NN_GRID against oracle.nn, index and d2 bits; NN_BRUTE on the device as a second witness.  n_q = 0: the gadgets'
    queries as they are (nn_wave_kernel); 32 768: nn_quad_kernel.  Gadgets per predicted stage (plain / sparse / dense regime):
    octant 144/144/18 'octant' and as many 'cube1'; cube >= 9 per radius of the ladder and >= 9 'unmatched'; chord 48/48/12;
    gate 24/24/12 inside and as many outside -- each class asserted >= 8 below."""
    scene = p2p_scene(ctx, regime, gate_name)
    gate = GATES[gate_name]
    scene.assert_classes(8)
    regime_asserts(scene, regime, p2p_scene(ctx, "plain", gate_name).grid.h)
    if regime == "plain":
        m = math.frexp(float(scene.grid.h))[0]
        assert (m == 0.5) == (gate_name == "dyadic"), float(scene.grid.h).hex()
    src = padded(scene.queries, n_q)
    got = nn_both_modes(ctx, src, scene.cloud, gate)
    want = oracle_nn(scene, n_q)
    same_keys(got[NN_GRID], want, "grid against the oracle")
    same_keys(got[NN_BRUTE], want, "device brute force against the oracle")
    # and the certificates as the helper walks them agree with the oracle (the helper's own check, here on the real grid)
    pred = np.tile(scene.want, len(src) // len(scene.want))
    assert np.array_equal(want[0][pred >= 0], pred[pred >= 0])


@pytest.mark.parametrize("gate_name", list(GATES))
@pytest.mark.parametrize("n_q", [0, 32768])
def test_gate_edge_leaves_the_point_beyond_unmatched(ctx, gate_name, n_q):
    """ctx.correspondences (the gated search of an iteration): B at gate * (1 - 2^-12) is matched, at gate * (1 + 2^-12) it is
    not (idx == -1), whatever the cubes saw; against oracle.nn cut at the gate's float32 threshold.  24 gadgets inside, 24
    outside, along an axis, an edge and a diagonal; the largest cell offset equals r_max (asserted)."""
    scene = p2p_scene(ctx, "plain", gate_name)
    gate = GATES[gate_name]
    gd = [g for g in scene.gadgets if g.family == "gate"][0]
    assert gd.extra["offset"].max() == scene.grid.r_max and (gd.stage == "inside").sum() >= 8 and (gd.stage == "outside").sum() >= 8
    src = padded(scene.queries, n_q)
    io, do = oracle_nn(scene, n_q)
    thr = F32(gate * gate)
    if float(thr) > gate * gate:
        thr = np.nextafter(thr, F32(-np.inf))
    keep = do <= thr
    for mode in (NN_GRID, NN_BRUTE):
        ctx.set_params(ctx.default_params(), nn_mode=mode, max_correspondence_distance=gate)
        ctx.set_source(src)
        ctx.set_target(scene.cloud)
        idx, d2 = ctx.correspondences(np.eye(4))
        assert np.array_equal(idx, np.where(keep, io, -1)), np.flatnonzero(idx != np.where(keep, io, -1))[:8]
        assert np.array_equal(d2[keep].view(np.uint32), do[keep].view(np.uint32))
    fam = np.tile(scene.family, len(src) // len(scene.family))
    stage = np.tile(scene.stage, len(src) // len(scene.stage))
    assert (idx[(fam == "gate") & (stage == "outside")] == -1).all() and (idx[(fam == "gate") & (stage == "inside")] >= 0).all()


@pytest.mark.parametrize("gate_name", list(GATES))
def test_previous_neighbour_bound_under_a_second_pose(ctx, gate_name):
    """Two ctx.nn calls without re-setting the clouds (32 768 queries: nn_quad_kernel): the identity, then a translation under
    which the neighbour N of the first call is at D' and B at D'(1 - 2^-10), inside the octant, in the row at the rim of N's
    ball.  64 'bounded' gadgets (the second pose brings the query nearer to N) and 64 'stale' (it takes it farther: a bound
    kept from the first pose would prune B).  Both calls against oracle.nn; grid_bounded == 1 on the second."""
    gate = GATES[gate_name]
    key = ("prev", gate_name)
    if key not in _SCENES:
        def plan(grid, blocks):
            shift = np.array([0.0, -0.1 * float(grid.h), 0.0], F32)
            return [GA.make_prev(grid, blocks.take(128), shift), GA.make_chord(grid, blocks.take(24))]
        _SCENES[key] = GA.build_scene(probing(ctx, p2p_action(ctx, gate)), fixed_points(gate, (32.0, 32.0, 12.0), (100, 40)), plan,
                                      lambda g: 2 * g.r_max + 3)
    scene = _SCENES[key]
    scene.assert_classes(8)
    gd = scene.gadgets[0]
    shift = np.array([0.0, -0.1 * float(scene.grid.h), 0.0], F32)
    src1 = np.ones((len(scene.queries), 4), F32)
    src1[:len(gd.query), :3] = gd.extra["source"]
    src1[len(gd.query):, :3] = (scene.queries[len(gd.query):, :3] - shift).astype(F32)
    src = padded(src1, 32768)
    T2 = np.eye(4)
    T2[:3, 3] = shift.astype(np.float64)
    ctx.set_params(ctx.default_params(), nn_mode=NN_GRID, max_correspondence_distance=gate)
    ctx.set_source(src)
    ctx.set_target(scene.cloud)
    reps = len(src) // len(src1)
    for k, T in enumerate((np.eye(4), T2)):
        ctx.profile_reset()
        got = ctx.nn(T)
        assert ctx.profile().grid_bounded == (1 if k and BOUND_ON else 0)
        io, do = oracle.nn(src1, scene.cloud, T)
        same_keys(got, (np.tile(io, reps), np.tile(do, reps)), f"pose {k + 1}")
        first = scene.slots[0][np.arange(len(gd.query)), 0 if k == 0 else 1]     # N under pose 1, B under pose 2
        assert np.array_equal(io[:len(gd.query)], first)
    ctx.set_params(ctx.default_params(), nn_mode=NN_BRUTE, max_correspondence_distance=gate)
    same_keys(ctx.nn(T2), (np.tile(io, reps), np.tile(do, reps)), "device brute force, pose 2")


def one_iteration(ctx, src, cloud, gate, mode):
    ctx.set_params(ctx.default_params(), nn_mode=mode, max_correspondence_distance=gate, max_iterations=1, force_iterations=1)
    ctx.set_source(src)
    ctx.set_target(cloud)
    return ctx.align(guess=np.eye(4))


@pytest.mark.parametrize("regime,gate_name,n_q", [("plain", "odd", 0), ("plain", "dyadic", 32768), ("sparse", "odd", 32768),
                                                   ("dense", "odd", 0), ("dense", "dyadic", 32768), ("plain", "odd", 131072)])
def test_one_forced_iteration_counts_the_same_pairs(ctx, regime, gate_name, n_q):
    """The fused variant of each kernel over the same gadgets (131 072 queries: with the cell-ordered source): one forced
    iteration from the identity; n_corr equals the oracle's and the brute-force path's, mse the brute-force path's as
    test_fuzz_grid_keys_equal_brute_force demands.  The gadget classes are those of test_nn_on_the_grids_own_edges."""
    scene = p2p_scene(ctx, regime, gate_name)
    gate = GATES[gate_name]
    scene.assert_classes(8)
    src = padded(scene.queries, n_q)
    res = {mode: one_iteration(ctx, src, scene.cloud, gate, mode) for mode in (NN_GRID, NN_BRUTE)}
    assert res[NN_GRID]["n_corr"] == res[NN_BRUTE]["n_corr"]
    assert abs(res[NN_GRID]["mse"] - res[NN_BRUTE]["mse"]) <= 1e-12 * max(1.0, res[NN_BRUTE]["mse"])
    io, do = oracle_nn(scene, n_q)
    assert res[NN_GRID]["n_corr"] == int((do.astype(np.float64) <= gate * gate).sum())
    if ("align", n_q) not in scene.ref and n_q <= 32768:
        scene.ref[("align", n_q)] = oracle.icp_align(src, scene.cloud, oracle.default_params(
            max_correspondence_distance=gate, max_iterations=1, force_iterations=1), guess=np.eye(4))["n_corr"]
    if n_q <= 32768:
        assert res[NN_GRID]["n_corr"] == scene.ref[("align", n_q)]


def test_batch_of_four_scenes_equals_the_four_alignments(ctx):
    """align_batch (nn_quad_batch_kernel) over four gadget scenes -- plain and sparse regime, both gates' grids under ONE gate
    -- against the four single alignments: the same bits."""
    gate = GATES["odd"]
    scenes = [p2p_scene(ctx, r, g) for r, g in (("plain", "odd"), ("sparse", "odd"), ("plain", "dyadic"), ("dense", "odd"))]
    for s in scenes:
        s.assert_classes(8)
    srcs = [padded(s.queries, 32768) for s in scenes]
    tgts = [s.cloud for s in scenes]
    ctx.set_params(ctx.default_params(), nn_mode=NN_GRID, max_correspondence_distance=gate, max_iterations=2, force_iterations=1)
    batch = ctx.align_batch(srcs, tgts)
    for s, t, b in zip(srcs, tgts, batch):
        ctx.set_source(s)
        ctx.set_target(t)
        one = ctx.align()
        assert (one["n_corr"], one["iterations"], one["state"]) == (b["n_corr"], b["iterations"], b["state"])
        assert np.array_equal(one["T"].view(np.uint32), b["T"].view(np.uint32))
        assert np.float64(one["mse"]).view(np.uint64) == np.float64(b["mse"]).view(np.uint64)


# ---- float binning against exact binning ------------------------------------------------------------------------------------
# 0.07 was chosen on the CPU: over a 300 m box its cells grow by the host's 1.15 steps to ~0.0206 m (no power of two), ~14 600 of
# them along x, where consecutive floats are 2^-9.4 of a cell apart and some land in another cell than exact arithmetic puts them.
@pytest.mark.parametrize("gate,length", [(0.07, 300.0), (0.0625, 160.0)])
def test_misbinned_points(ctx, gate, length):
    """Octant gadgets whose QUERY, and cube gadgets whose B, is a float that float32 binning and exact binning put into
    different cells, at the far end of an axis of ~2^14 cells: >= 8 of each (asserted; a grid without such floats skips, and
    says so).  ctx.nn against oracle.nn, bit for bit, and NN_BRUTE as the second witness."""
    lo = np.array([-3.7, 0.0, 0.0])
    fixed = np.concatenate([np.array([lo, lo + [length, 0.62, 0.62]], F32), GA.clumps(lo + 0.05, 0.1, 60, 1, 1e-4, 40)])
    found_any = []

    def plan(grid, blocks):
        pitch = 2 * grid.r_max + 3
        faces = np.arange(grid.dims[0] - pitch - 1, grid.dims[0] // 2, -pitch)[:1200]
        mid = (grid.dims[1] // 2, grid.dims[2] // 2)
        centre = np.array(grid.o, np.float64) + (np.array([0, mid[0], mid[1]]) + 0.5) * float(grid.h)
        found = GA.find_misbinned(grid, 0, faces, centre)
        found = tuple(v[:96] for v in found)
        found_any.append(len(found[0]))
        return [GA.make_misbinned(grid, 0, found, mid)] if len(found[0]) else []
    scene = GA.build_scene(probing(ctx, p2p_action(ctx, gate)), fixed, plan, lambda g: 2 * g.r_max + 3)
    nx = scene.grid.dims[0]
    assert 8192 < nx < 16384, scene.grid                          # the box-growing rule caps the axis under 2^14: the real nx
    if not found_any[-1]:
        pytest.skip(f"no float within 6 places of a cell face is mis-binned on this grid (h = {float(scene.grid.h).hex()}, nx = {nx})")
    scene.assert_classes(8)
    gd = scene.gadgets[0]
    assert (np.abs(gd.extra["float_cell"] - gd.extra["exact_cell"]) == 1).all()
    got = nn_both_modes(ctx, scene.queries, scene.cloud, gate)
    want = oracle.nn(scene.queries, scene.cloud, np.eye(4))
    same_keys(got[NN_GRID], want, "grid against the oracle")
    same_keys(got[NN_BRUTE], want, "device brute force against the oracle")
    res = {mode: one_iteration(ctx, scene.queries, scene.cloud, gate, mode) for mode in (NN_GRID, NN_BRUTE)}
    assert res[NN_GRID]["n_corr"] == res[NN_BRUTE]["n_corr"] == int((want[1].astype(np.float64) <= gate * gate).sum())


# ---- the search cloud -------------------------------------------------------------------------------------------------------
SHELLS = 6          # search_knn_kernel walks shells 0 .. 6 before the far list (icp_search.hip)
OUTSIDE = 64        # cells a query may lie outside the grid and still be walked (icp_search_device.h)


def search_scene(ctx, own: bool):
    """own: the cloud holds the queries themselves (the outlier filters query every cloud point): k = 2 and 20 gadgets; else
    k = 1, 20, 64 and the radius gadgets of R = 1, 8, 9.

    The k-NN grid's first cell size spreads the cloud's points evenly over its box, 32 to a cell, and the count pass then shrinks
    the cells by the point-weighted population, down to a 16th: a cloud of isolated gadgets alone would get a handful of cells.
    The filler is therefore ONE dense blob (1/70 of the box across) next to the low corner: it drives the population so high that
    the cells take their smallest size, which depends on the box and the point count alone -- and the builder checks, as always,
    that moving the gadget points inside their cells left the descriptor as it was."""
    key = ("search", own)
    if key not in _SCENES:
        def plan(grid, blocks):
            if own:
                return [GA.make_knn(grid, blocks.take(96), k, SHELLS, True) for k in (2, 20)]
            return ([GA.make_knn(grid, blocks.take(96), k, SHELLS, False) for k in (1, 20, 64)] +
                    [GA.make_radius(grid, blocks.take(48), R, False) for R in (1, 8, 9)])
        box, blob, pitch = (30.0, 16000, 2 * (SHELLS + 2) + 2) if own else (44.0, 60000, 2 * 9 + 3)
        fixed = np.concatenate([np.array([LO, LO + box], F32), GA.clumps(LO + 0.02 * box, 0.0, 1, 1, box / 70.0, blob)])
        s = GA.build_scene(probing(ctx, lambda cloud: ctx.search_set_input(cloud)), fixed, plan, lambda g: pitch)
        assert s.grid.max_pop <= 4096, s.grid          # (the grid serves the cloud: beyond 4096 points in a cell it is refused)
        s.cloud.setflags(write=False)
        _SCENES[key] = s
    return _SCENES[key]


def test_search_knn_shell_certificate(ctx):
    """ctx.search_knn for k = 1, 20, 64 on gadgets made for each k (A, the candidate k-th, on both sides of the shell bound; B
    beyond the shell) against tests/search_restated.py, bit for bit: per k, >= 8 gadgets certified in each of shells 1 .. 6 and
    >= 8 left to the far list (asserted); and queries 63, 64 and 65 cells outside the box (walked, walked, listed)."""
    scene = search_scene(ctx, False)
    scene.assert_classes(8)
    g = scene.grid
    out = []
    for cells in (OUTSIDE - 1, OUTSIDE, OUTSIDE + 1):
        q = scene.queries[:24].copy()
        q[:, 0] = F32(float(g.o[0]) - (cells - 0.5) * float(g.h))
        assert (GA.cell_of(g, q)[:, 0] == -cells).all()
        out.append(q)
    queries = np.concatenate([scene.queries] + out)
    queries.setflags(write=False)
    ctx.search_set_input(scene.cloud)
    for gd, slot in zip(scene.gadgets, scene.slots):
        if gd.family.startswith("knn"):
            idx, _, _ = check_knn(ctx, "adversary", scene.cloud, queries, gd.extra["k"])
            # the helper's walk of the certificate agrees with the restatement on what the k nearest are
            at = int(np.flatnonzero(scene.family == gd.family)[0])
            want = np.take_along_axis(slot, gd.want, axis=1)
            assert np.array_equal(idx[at:at + len(want)], want)


def test_search_radius_cube(ctx):
    """ctx.search_radius at radii whose cube is R = 1, 8 and 9 cells (9: the whole-cloud path), chosen from the h that was read:
    B at radius * (1 - 2^-12) in the cell R cells away is the last entry of rows of 64 and 65 entries, at radius * (1 + 2^-12)
    it is no neighbour; 12 gadgets of each of the four kinds per R (asserted >= 8)."""
    scene = search_scene(ctx, False)
    scene.assert_classes(8)
    ctx.search_set_input(scene.cloud)
    for gd, slot in zip(scene.gadgets, scene.slots):
        if not gd.family.startswith("radius"):
            continue
        R, radius = gd.extra["R"], gd.extra["radius"]
        assert math.ceil(radius / (float(scene.grid.h) * float(GA.SAFETY))) == R and (gd.extra["offset"] == R).all()
        row_start, idx, d2 = check_radius(ctx, "adversary", scene.cloud, scene.queries, radius)
        at = int(np.flatnonzero(scene.family == gd.family)[0])
        rows = np.diff(row_start)[at:at + len(gd.query)]
        assert np.array_equal(rows, gd.want) and set(rows) == {63, 64, 65}
        last = idx[row_start[at + 1:at + 1 + len(gd.query)] - 1]
        inside = gd.extra["inside"]
        assert np.array_equal(last[inside], slot[inside, -1])                   # the rim point closes its row
        check_radius(ctx, "adversary", scene.cloud, scene.queries, radius, 64)  # cut at max_nn: the 65-entry rows lose it


@pytest.mark.parametrize("mean_k", [1, 19])
def test_outlier_walk_shell_certificate(ctx, mean_k):
    """statistical_outlier_removal (icp_outlier.hip's own copy of the walk) on a cloud that holds its queries: gadgets for
    k = mean_k + 1 with the candidate k-th on both sides of every shell's bound; the measure array against
    tests/outlier_restated.py, bit for bit.  >= 8 gadgets per shell 1 .. 6 and for the far list (asserted)."""
    scene = search_scene(ctx, True)
    scene.assert_classes(8)
    key = ("sor", mean_k)
    if key not in _SCENES:
        _SCENES[key] = OR.sor_distances(scene.cloud, mean_k)
    ctx.statistical_outlier_removal(scene.cloud, mean_k, 1.0)
    got = ctx.outlier_fetch()["measure"]
    bad = np.flatnonzero(got.view(np.uint32) != _SCENES[key].view(np.uint32))
    assert bad.size == 0, (bad[:8], got[bad[:8]], _SCENES[key][bad[:8]])


def test_radius_outlier_removal_at_the_radius_edge(ctx):
    """radius_outlier_removal builds its own grid with the radius as the gate: gate gadgets on THAT grid (the cloud holds the
    queries), B at radius * (1 -+ 2^-12) with the cell offset reaching r_max; counts against tests/outlier_restated.py."""
    radius = 0.8
    key = ("ror",)
    if key not in _SCENES:
        def plan(grid, blocks):
            return [GA.make_gate(grid, blocks.take(96), radius, with_query_point=True)]
        _SCENES[key] = GA.build_scene(probing(ctx, lambda cloud: ctx.radius_outlier_removal(cloud, radius, 1)),
                                      fixed_points(radius, (30.0, 30.0, 30.0), (36, 40)), plan, lambda g: 2 * g.r_max + 3)
    scene = _SCENES[key]
    scene.assert_classes(8)
    gd = scene.gadgets[0]
    assert gd.extra["offset"].max() == scene.grid.r_max
    k = OR.ror_counts(scene.cloud, radius)
    ctx.radius_outlier_removal(scene.cloud, radius, 1)
    got = ctx.outlier_fetch()["measure"]
    assert np.array_equal(got, k.astype(F32)), np.flatnonzero(got != k)[:8]
    q_at = scene.slots[0][:, 0]
    assert np.array_equal(k[q_at], np.where(gd.stage == "inside", 2, 1))
