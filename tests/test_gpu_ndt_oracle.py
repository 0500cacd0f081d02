"""NDT on the device against its C restatement (oracle/ndt_oracle.c, pinned to tests/ndt_restated.py in tests/test_ndt_oracle.py),
never against the library itself.

Every pass asserts: the pair count exact; each of the 29 sums within 1e-12 mag[k] of the oracle (mag = the sums of |factors|,
which also bounds the device's regrouping of PCL's per-pair terms into b, A and M per point), both over the device's own cells
(ctx.ndt_cells(): the pass in isolation) and over the oracle's cells (end to end); ctx.ndt_gradient(p) = ctx.ndt_derivatives(p)[:8]
bit for bit.  Cells: n, float centroid and mean bit for bit, validity outside the oracle's binary128 margin (1e-12), icov within
1e-12 max|icov|.

d2 stays below 1 over resolution {0.05 .. 5} x outlier ratio {0.01 .. 0.99} (tests/test_ndt_oracle.py), so for a PSD icov
d2 e <= d2 < 1 and PCL's `d2 e > 1 / < 0 / NaN` skip rule cannot fire: the passes assert that the oracle skipped nothing."""
import numpy as np
import pytest

import oracle
from icpslam_amd import NDT, Context, synth
from icpslam_amd._lib import NDT_LINE_SEARCH_MORE_THUENTE
from icpslam_amd.registration import ndt_step
from test_ndt_oracle import cell_scene, cloud, excess_scene, far_scene

pytestmark = pytest.mark.gpu
F = np.float32
WORST = {"sum": 0.0, "icov": 0.0, "passes": 0, "cells": 0}                 # reported at the end of the module (-s)


def _ctx(resolution=1.0, ratio=0.55, **kw):
    c = Context(0)
    kw.setdefault("max_iterations", 35)
    kw.setdefault("transformation_epsilon", 0.1)
    c.set_params(c.default_params(), method=NDT, **kw)
    c.set_ndt_params(resolution, 0.1, ratio)
    return c


def _sums_close(got, ref):
    assert got[0] == ref["pairs"], (got[0], ref["pairs"])
    assert ref["skipped"] == 0
    n = len(got)
    err = np.abs(got - ref["sums"][:n])
    mag = ref["mag"][:n]
    assert (err <= 1e-12 * mag).all(), (np.nonzero(err > 1e-12 * mag)[0], (err / np.maximum(mag, 1e-300)).max())
    nz = mag > 0
    if nz.any():
        WORST["sum"] = max(WORST["sum"], float((err[nz] / mag[nz]).max()))


def check_pass(ctx, src, p, resolution, ratio=0.55, O=None, dev_cells=None, near_ok=False):
    """One evaluation at p: the 29 sums over the device's cells and (O given) over the oracle's; the trial pass's bits."""
    got = ctx.ndt_derivatives(p)
    assert np.array_equal(ctx.ndt_gradient(p).view(np.uint64), got[:8].view(np.uint64))
    dev_cells = ctx.ndt_cells() if dev_cells is None else dev_cells
    ref = oracle.ndt_derivatives(dev_cells, src, p, resolution, ratio)
    if not near_ok:
        assert ref["near"] == 0
    _sums_close(got, ref)
    if O is not None:
        _sums_close(got, oracle.ndt_derivatives(O, src, p, resolution, ratio))
    WORST["passes"] += 1
    return got, ref


def check_cells(ctx, tgt, resolution):
    """ctx.ndt_cells() against oracle.ndt_cells: -> the oracle's result"""
    O = oracle.ndt_cells(tgt, resolution)
    c = O["cells"]
    dev = ctx.ndt_cells()
    # the device's valid cells, matched by (n, mean bits) -- both sides list them in key order
    index = {(int(n), m.tobytes()): i for i, (n, m) in enumerate(zip(c["n"], c["mean"]))}
    idx = np.array([index[(int(n), m.tobytes())] for n, m in zip(dev["n_points"], dev["mean"])], np.int64)
    assert (np.diff(idx) > 0).all()
    assert np.array_equal(dev["centroid"].view(np.uint32), c["centroid"][idx].view(np.uint32))
    clear = c["margin"] > 1e-12
    dev_valid = np.zeros(len(c), bool)
    dev_valid[idx] = True
    assert np.array_equal(dev_valid[clear], c["valid"][clear] != 0)
    both = idx[clear[idx]]
    if len(both):
        sel = clear[idx]
        scale = np.abs(c["icov"][both]).reshape(-1, 9).max(axis=1)
        rel = np.abs(dev["icov"][sel] - c["icov"][both]).reshape(-1, 9).max(axis=1) / scale
        assert (rel <= 1e-12).all(), rel.max()
        WORST["icov"] = max(WORST["icov"], float(rel.max()))
    WORST["cells"] += len(idx)
    return O


def _target(n=60000, seed=5):
    return synth.scan(synth.make_scene(seed), np.eye(4), n, seed=seed)


# ---- 1. source sizes around the grid-stride loop (1024 workgroups of 256) ----------------------------------------------------------
def test_source_sizes_around_the_stride_loop():
    tgt = _target()
    big = synth.scan(synth.make_scene(5), synth.pose_matrix(0.3, 0.1, 0.0, 0.0, 0.0, 0.02), 600000, seed=11)
    poses = [np.r_[0.05, -0.03, 0.01, 0.0, 0.0, 0.01], np.r_[-0.2, 0.1, 0.02, 0.01, -0.015, 0.03]]
    with _ctx() as ctx:
        ctx.set_target(tgt)
        O = check_cells(ctx, tgt, 1.0)
        dev_cells = ctx.ndt_cells()
        for n in (1, 255, 256, 257, 262143, 262144, 262145, 600000):
            src = big[:n]
            ctx.set_source(src)
            for k, p in enumerate(poses):
                # (the large sources: end to end at one pose, to keep the oracle's time down)
                got, _ = check_pass(ctx, src, p, 1.0, dev_cells=dev_cells, O=O if (n < 262143 or k == 1) else None)
                if n >= 262143:
                    assert got[0] > 100000


# ---- 2. replays of alignments ---------------------------------------------------------------------------------------------------
def test_replay_of_pcl18_alignments():
    for seed in range(3):
        src, tgt, _ = synth.make_pair(8000, 20000, seed=200 + seed)
        with _ctx() as ctx:
            ctx.set_target(tgt)
            ctx.set_source(src)
            res = ctx.align()
            O = check_cells(ctx, tgt, 1.0)
            dev_cells = ctx.ndt_cells()
            p, T = np.zeros(6), np.eye(4, dtype=F)
            sums, _ = check_pass(ctx, src, p, 1.0, O=O, dev_cells=dev_cells)
            nr_ = 0
            assert sums[0] > 0
            while True:
                st, p_new, a, T_new = ndt_step(sums, p, 0.1, 0.1)
                if st != 0:
                    break
                if a > 0:
                    p, T = p_new, T_new
                    sums, _ = check_pass(ctx, src, p, 1.0, O=O, dev_cells=dev_cells)
                cap = nr_ > 35
                if cap or (nr_ and abs(a) < 0.1):
                    nr_ += 1
                    break
                nr_ += 1
            assert nr_ == res["iterations"]
            assert np.array_equal(T.view(np.uint32), res["T"].view(np.uint32))


def test_more_thuente_trials_of_the_first_iteration():
    """The 8-term pass at every trial pose of the first More-Thuente iteration: x = p0 + a_t d (icpgpu_ndt_step with step_size =
    a_t and eps = 2 a_t gives exactly that pose), its phi the trace's bit for bit."""
    src, tgt, _ = synth.make_pair(8000, 20000, seed=7)
    with _ctx(transformation_epsilon=1e-3) as ctx:
        ctx.set_ndt_line_search(NDT_LINE_SEARCH_MORE_THUENTE)
        ctx.set_target(tgt)
        ctx.set_source(src)
        ctx.align()
        tr = ctx.ndt_line_search_trace()
        dev_cells = ctx.ndt_cells()
        p0 = np.zeros(6)
        sums0, _ = check_pass(ctx, src, p0, 1.0, dev_cells=dev_cells)
        first = np.nonzero(tr["iteration"] == 0)[0]
        assert len(first) >= 1
        for k in first:
            a_t = tr["step"][k]
            st, x, a, _ = ndt_step(sums0, p0, a_t, 2 * a_t)
            assert st == 0 and a == a_t
            g8 = ctx.ndt_gradient(x)
            assert -g8[1] == tr["phi"][k]
            _sums_close(g8, oracle.ndt_derivatives(dev_cells, src, x, 1.0))


# ---- 3. centroids outside their cell --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution", [0.7, 0.3])
def test_centroids_outside_their_cell(resolution):
    tgt, found = excess_scene(resolution)
    O = oracle.ndt_cells(tgt, resolution)
    c = O["cells"]
    assert O["max_excess"] > 0 and (c["excess"] > 0).all() and c["valid"].all()
    r = F(resolution)
    q = []
    for (kind, _), cen in zip(found, c["centroid"]):            # (one cell per boundary, in key order = the order found)
        s = 1 if kind == "up" else -1                           # away from the keyed cell
        x = F(cen[0] + s * r)
        for k in range(-2, 3):
            xq = x
            for _ in range(abs(k)):
                xq = np.nextafter(xq, F(np.inf) if k > 0 else F(-np.inf))
            q.append([xq, cen[1], cen[2]])
    src = cloud(np.array(q, F))
    ref = oracle.ndt_derivatives(O, src, np.zeros(6), resolution, pairs=10000)
    # at least one pair lies outside the unwidened stencil floor((q -+ r) / L): only the widening by e finds it
    inv = float(O["inv_leaf_f"])
    outside = 0
    for i, j in zip(ref["pair_pt"], ref["pair_cell"]):
        ix = int(c["key"][j]) % O["mul_y"] + O["minb"][0]
        qx = float(src[i, 0])
        if not (np.floor((qx - float(r)) * inv) <= ix <= np.floor((qx + float(r)) * inv)):
            outside += 1
    assert outside > 0
    with _ctx(resolution) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        check_cells(ctx, tgt, resolution)
        check_pass(ctx, src, np.zeros(6), resolution, O=O, near_ok=True)


# ---- 4. cells against binary128 -------------------------------------------------------------------------------------------------
def test_cells_against_binary128():
    rng = np.random.default_rng(8)
    one = cloud(rng.normal([0.5, 0.5, 0.5], [0.12, 0.1, 0.02], (100000, 3)).clip(0.01, 0.99))     # one cell of 100k points
    with _ctx() as ctx:
        for tgt, res in ((far_scene(), 1.0), (far_scene(1, sigma=1e-4), 0.3), (cell_scene(), 1.0), (cell_scene(4), 0.3),
                         (cell_scene(5, offset=(-3000.0, 2000.0, 1000.0)), 2.5), (one, 1.0)):
            ctx.set_ndt_params(res, 0.1, 0.55)
            ctx.set_target(tgt)
            O = check_cells(ctx, tgt, res)
            if tgt is one:
                assert len(O["cells"]) == 1 and O["cells"]["n"][0] == 100000
            src = tgt[rng.choice(len(tgt), 2000, replace=False)]
            ctx.set_source(src)
            check_pass(ctx, src, np.r_[0.01, -0.02, 0.005, 0.001, 0.002, -0.003], res, near_ok=True)


# ---- 5. targets at the scan and sort tiles (4096 ints per tile, 1024 lanes) -------------------------------------------------------------
def test_targets_at_the_scan_tiles():
    rng = np.random.default_rng(9)
    base = rng.uniform([0, 0, 0], [40, 40, 30], (4500000, 3)).astype(F)
    src = cloud(rng.uniform([2, 2, 2], [38, 38, 28], (3000, 3)))
    with _ctx() as ctx:
        ctx.set_source(src)
        for n in (2047, 2048, 2049, 4095, 4096, 4097, 4194304, 4194305, 4500000):
            tgt = cloud(base[:n] if n > 5000 else base[:n] * F(0.1))   # (the small ones dense enough to make cells)
            ctx.set_target(tgt)
            O = check_cells(ctx, tgt, 1.0)
            assert (O["cells"]["valid"] != 0).sum() > 0
            if n in (4097, 4194305):
                check_pass(ctx, src, np.r_[0.1, -0.1, 0.05, 0.01, 0.0, -0.02], 1.0, O=O)


# ---- 6. a lattice just below INT32_MAX cells -----------------------------------------------------------------------------------------
def test_lattice_just_below_int32_max():
    """1290^3 = 2 146 689 000 cells: the key sort runs with end_bit 31 (eight radix passes), the far corner's key is within 0.04 % of
    2^31 and non-finite points (the sentinel 0x7FFFFFFF) sort among them."""
    rng = np.random.default_rng(10)
    spots = np.array([[0.5, 0.5, 0.5], [1289.5, 1289.5, 1289.5], [1289.5, 0.5, 1289.5], [0.5, 1289.5, 1289.5], [645.5, 645.5, 645.5],
                      [1289.5, 1289.5, 1288.5], [1200.5, 1289.5, 1289.5]])
    tgt = cloud(np.concatenate([s + rng.uniform(-0.4, 0.4, (40, 3)) for s in spots]))
    tgt = np.concatenate([tgt, cloud([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]] * 5)])
    tgt = tgt[rng.permutation(len(tgt))]
    O = oracle.ndt_cells(tgt, 1.0)
    assert O["divb"] == [1290, 1290, 1290] and O["cells"]["key"].max() > 2**31 - 2**21
    src = cloud(np.concatenate([s + rng.uniform(-1.2, 1.2, (300, 3)) for s in spots]))
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        check_cells(ctx, tgt, 1.0)
        assert len(ctx.ndt_cells()["n_points"]) == len(spots)
        check_pass(ctx, src, np.r_[0.05, 0.02, -0.03, 0.0, 0.0, 0.0], 1.0, O=O)


# ---- 7. parameters and poses -------------------------------------------------------------------------------------------------------
def test_resolution_and_outlier_ratio_grid():
    src, tgt, _ = synth.make_pair(3000, 30000, seed=21)
    p = np.r_[0.1, -0.05, 0.02, 0.01, -0.01, 0.02]
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        for res in (0.05, 0.3, 1.0, 2.5, 5.0):
            O = None
            for ratio in (0.01, 0.55, 0.99):
                ctx.set_ndt_params(res, 0.1, ratio)
                if O is None:
                    O = check_cells(ctx, tgt, res)
                got, ref = check_pass(ctx, src, p, res, ratio, O=O)
                assert got[0] > 0 or res < 0.3


def test_poses_and_source_edges():
    src, tgt, _ = synth.make_pair(5000, 30000, seed=22)
    src = src.copy()
    src[:5, 0] = np.nan
    src[5:8, 2] = np.inf
    src[8:20, :3] = [1e7, -1e7, 3e6]                               # far outside the lattice
    src[20:25, :3] = [3e38, 3e38, 3e38]                            # the transform overflows
    angles = [0.0, 9.9999e-5, -9.9999e-5, 1e-4, -1e-4, 1.0001e-4, -1.0001e-4]
    poses = [np.r_[0.1, -0.1, 0.0, a, b, c] for a, b, c in zip(angles, angles[::-1], angles[3:] + angles[:3])]
    poses += [np.r_[0.2, -0.1, 0.0, 3.0, -1.2, 2.0], np.r_[0.0, 0.0, 0.0, np.pi, -np.pi, 7.0], np.r_[0.0, 0.0, 0.0, -9.5, 100.0, 0.5]]
    with _ctx() as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        O = check_cells(ctx, tgt, 1.0)
        for p in poses:
            check_pass(ctx, src, p, 1.0, O=O)
        # kilometres away: the source and the target moved together (T's translation cancels the offset)
        off = np.array([2500.0, -1800.0, 300.0], F)
        tgt_far = tgt.copy()
        tgt_far[:, :3] += off
        ctx.set_target(tgt_far)
        O = check_cells(ctx, tgt_far, 1.0)
        for p in (np.r_[off.astype(np.float64), 0.0, 0.0, 0.0], np.r_[off.astype(np.float64) + 0.05, 0.002, -0.001, 0.003]):
            got, _ = check_pass(ctx, src, p, 1.0, O=O)
            assert got[0] > 1000


def test_zz_report_worst_ratios():
    """(the largest differences against the oracle seen by this module; printed with -s)"""
    print(f"\nNDT vs oracle: {WORST['passes']} passes, worst |sum - oracle| / mag {WORST['sum']:.3g}; {WORST['cells']} cells, worst "
          f"|icov - oracle| / max|icov| {WORST['icov']:.3g}")
