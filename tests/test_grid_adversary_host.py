"""tests/grid_adversary.py without a device: the helper's float32 arithmetic against exact rationals, every maker's claims against
brute force, and the scene builder against a stand-in probe that answers with a hand-written descriptor."""
import numpy as np
import pytest

import grid_adversary as GA

F32 = np.float32

# The line icpgpu_index.cpp prints under ICPGPU_DEBUG, by hand: a dyadic grid (h = 1/4, origin on the lattice) and one that is not
# (h = float32(1 / 4.5), an origin that is no multiple of it).
DYADIC = ("[icpgpu] grid n=%d binned=%d h=0.2500 dims=400x400x220 pop=32.0 max=40 attempt=0 "
          "desc=0x1p-2,0x1p+2,-0x1.4p+3,0x1p+2,-0x1.8p+1 sy=88000 sz=400 r_max=5\n")
H_ODD = float(F32(1.0 / 4.5))
ODD = ("[icpgpu] grid n=%%d binned=%%d h=0.2222 dims=400x400x220 pop=32.0 max=40 attempt=0 desc=%s,%s,%s,%s,%s sy=88000 sz=400 r_max=5\n"
       % tuple(float(F32(v)).hex() for v in (H_ODD, F32(1.0) / F32(H_ODD), -13.37, 7.21, -2.9)))
LINES = {"dyadic": DYADIC, "odd": ODD}


def grid_of(name, n=7):
    return GA.read_grid("noise\n" + LINES[name] % (n - 1, n - 1) + LINES[name] % (n, n) + "[icpgpu] other\n", n)


def test_read_grid_round_trips_the_hex_floats():
    g = grid_of("dyadic")
    assert float(g.h) == float.fromhex("0x1p-2") == 0.25 and float(g.inv_h) == 4.0
    assert g.o == (F32(-10.0), F32(4.0), F32(-3.0)) and g.dims == (400, 400, 220) and (g.sy, g.sz, g.r_max) == (88000, 400, 5)
    assert (g.n, g.binned, g.pop, g.max_pop, g.attempt) == (7, 7, 32.0, 40, 0)
    o = grid_of("odd")
    assert float(o.h) == H_ODD and float.fromhex(float(o.h).hex()) == H_ODD
    assert o.ladder() == [1, 2, 4, 5] and o.ladder(20) == [1, 2, 4, 8, 16, 20]
    # the line every older test parses still parses the old way
    import re
    assert re.findall(r"\[icpgpu\] grid n=7 .* max=(\d+) ", ODD % (7, 7)) == ["40"]
    assert re.findall(r"\[icpgpu\] grid n=\d+ .* h=([0-9.]+) ", ODD % (7, 7)) == ["0.2222"]


def test_cell_of_equals_cell_exact_on_a_dyadic_grid():
    g = grid_of("dyadic")
    rng = np.random.default_rng(1)
    # h and the origin are powers of two or small integers: the multiplication is exact, and so is x - o for every x on a
    # 2^-12 lattice this near the origin (19 significant bits)
    p = (np.round(rng.uniform(-12, 95, (3000, 3)) * 4096) / 4096).astype(F32)
    p[:500] = (np.round(p[:500] * 4) / 4).astype(F32)          # on cell faces
    p[500:1000] = p[:500] - F32(2.0 ** -12)                      # one lattice step under them
    assert (GA.cell_of(g, p) == GA.cell_exact(g, p)).all()
    # ... but not for every float: one float under a face, x - o rounds ONTO the face (the subtraction, not h, mis-bins it)
    x = np.nextafter(F32(0.25), F32(-np.inf))
    q = np.array([[x, 5.0, 0.0]], F32)
    assert GA.cell_of(g, q)[0, 0] == 41 and GA.cell_exact(g, q)[0, 0] == 40


def test_far_cells_of_a_non_dyadic_grid_hold_misbinned_floats():
    """h = 0.01 * 1.15^k style cells, 2^14 of them along x: next to the far faces float32 binning and exact arithmetic part."""
    h = F32(0.0123)
    g = GA.Grid(h=h, inv_h=F32(1.0) / h, o=(F32(-3.7), F32(0.0), F32(0.0)), dims=(16000, 30, 30), sy=16000, sz=480000, r_max=5)
    xs, fc, ec = GA.find_misbinned(g, 0, np.arange(15000, 15400), (0.0, 0.1, 0.1))
    assert len(xs) >= 16
    p = np.zeros((len(xs), 3), F32)
    p[:, 0], p[:, 1:] = xs, 0.1
    assert (GA.cell_of(g, p)[:, 0] == fc).all() and (GA.cell_exact(g, p)[:, 0] == ec).all() and (np.abs(fc - ec) == 1).all()


def test_misbinned_gadgets():
    """make_misbinned on such a grid: the query (even copies) or B (odd copies) sits on a float whose two cells differ; brute force
    over the scene agrees with what the certificates keep."""
    h = F32(0.0205722)
    thin = GA.Grid(h=h, inv_h=F32(1.0) / h, o=(F32(-3.72), F32(-0.02), F32(-0.02)), dims=(14585, 33, 33), sy=14585, sz=481305, r_max=4)
    lo = np.array(thin.o, np.float64) + float(h)
    fixed = np.array([lo, lo + (np.array(thin.dims) - 3) * float(h)], F32)

    def plan(grid, blocks):
        found = GA.find_misbinned(grid, 0, np.arange(14500, 7000, -11), np.array(grid.o, np.float64) + 16.5 * float(grid.h))
        return [GA.make_misbinned(grid, 0, tuple(v[:96] for v in found), (16, 16))]
    s = GA.build_scene(lambda cloud: thin, fixed, plan, lambda g: 2 * g.r_max + 3)
    s.assert_classes(8)
    gd = s.gadgets[0]
    on_q, on_b = gd.stage == "query", gd.stage == "B"
    assert (GA.cell_of(thin, gd.query[on_q])[:, 0] != GA.cell_exact(thin, gd.query[on_q])[:, 0]).all()
    assert (GA.cell_of(thin, gd.pts[on_b, 1])[:, 0] != GA.cell_exact(thin, gd.pts[on_b, 1])[:, 0]).all()
    idx, _ = GA.brute_force(s.cloud, s.queries)
    decided = s.want >= 0
    assert decided.sum() >= 80 and np.array_equal(idx[decided], s.want[decided])


def test_d2_emulation_is_the_exact_expression():
    rng = np.random.default_rng(2)
    p, q = rng.uniform(-50, 50, (300, 3)).astype(F32), rng.uniform(-50, 50, (300, 3)).astype(F32)
    q[:100] = p[:100] + rng.uniform(-1e-3, 1e-3, (100, 3)).astype(F32)
    got = GA.d2_f32(p, q)
    for i in range(300):
        assert got[i].view(np.uint32) == GA.d2_exact_rounded(p[i], q[i]).view(np.uint32)


def test_fraction_codes_and_bisection():
    for name in LINES:
        g = grid_of(name)
        cell = np.arange(17, 17 + 8 * 40, 8)
        for a in range(3):
            x = [GA.at_fraction(g, a, cell, np.full(len(cell), code)) for code in range(8)]
            u = [GA.cell_u(g, np.stack([v] * 3, axis=1))[:, a] - cell for v in x]
            assert (u[0] >= 0).all() and (GA.cell_u(g, np.stack([GA.step(x[0], -1)] * 3, axis=1))[:, a] < cell).all()
            assert (u[3] < 0.5).all() and (u[4] >= 0.5).all() and (GA.step(x[3], 1) == x[4]).all() and (GA.step(x[4], 1) == x[5]).all()
            assert (u[7] < 1).all() and (GA.cell_u(g, np.stack([GA.step(x[7], 1)] * 3, axis=1))[:, a] >= cell + 1).all()
            assert (u[2] >= 0.25).all() and (u[6] >= 0.75).all() and (GA.step(x[0], 1) == x[1]).all()


GATE = 1.0


def _plan(grid, blocks, gate=GATE):
    return [GA.make_octant(grid, blocks.take(288)), GA.make_cube(grid, blocks.take(36 * len(grid.ladder()))),
            GA.make_chord(grid, blocks.take(48)), GA.make_gate(grid, blocks.take(48), gate)]


def _scene(name, plan=_plan, reach=0):
    base = grid_of(name)
    lo = np.array(base.o, np.float64) + float(base.h)
    hi = lo + (np.array(base.dims) - 3) * float(base.h)
    fixed = np.concatenate([np.array([lo, hi], F32), GA.clumps(lo + 2.0, 1.0, 6, 6, 1e-3, 40)])
    calls = []

    def probe(cloud):
        calls.append(len(cloud))
        return GA.read_grid(LINES[name] % (len(cloud), len(cloud)), len(cloud))
    scene = GA.build_scene(probe, fixed, plan, lambda g: 2 * max(g.r_max, reach) + 3)
    assert len(calls) == 3 and calls[1] == calls[2] and scene.passes == 1
    return scene


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = _scene(name)
    return _SCENES[name]


@pytest.mark.parametrize("name", list(LINES))
def test_every_predicted_class_is_populated(name):
    c = scene(name).assert_classes(8)
    assert {f for f, _ in c} == {"octant", "cube", "chord", "gate"}


@pytest.mark.parametrize("name", list(LINES))
def test_gadgets_do_not_interact_and_the_certificates_keep_the_nearest(name):
    """Brute force over the WHOLE scene (anchors, filler and every other gadget included) gives each query the point its own
    gadget's certificates keep: the gadgets are decided by their own points, and the certificates as restated are right."""
    s = scene(name)
    idx, d2 = GA.brute_force(s.cloud, s.queries)
    matched = s.want >= 0
    assert np.array_equal(idx[matched], s.want[matched]), np.flatnonzero(matched & (idx != s.want))[:8]
    # unmatched by the gated ladder: the nearest is still one of the gadget's own points
    own = [row for sl in s.slots for row in sl]
    assert len(own) == len(idx)
    assert all(idx[i] in own[i] for i in np.flatnonzero(~matched))


@pytest.mark.parametrize("name", list(LINES))
def test_makers_keep_their_claims(name):
    s = scene(name)
    g = s.grid
    for gd, slot in zip(s.gadgets, s.slots):
        q, pts = gd.query, gd.pts
        d2 = GA.d2_f32(np.broadcast_to(q[:, None, :], pts.shape), pts)
        qc = GA.cell_of(g, q)
        if gd.family == "octant":
            t, has_b = gd.extra["t_code"], gd.extra["has_b"]
            assert set(gd.extra["margin_axis"]) == {0, 1, 2}
            _, lowc, margin, f = GA._octant_low(g, q)
            assert len({tuple(r) for r in (f < 0.5)}) == 8                      # all 8 orientations
            bc, ac = GA.cell_of(g, pts[:, 1]), GA.cell_of(g, pts[:, 0])
            assert ((ac >= lowc) & (ac <= lowc + 1)).all()                       # A inside the octant
            assert (((bc < lowc) | (bc > lowc + 1)).any(axis=1) | ~has_b).all()  # B outside it
            assert (d2[has_b & (t == 5), 1] < d2[has_b & (t == 5), 0]).all()     # B strictly nearer where t > 1
            assert (d2[has_b & (t <= 4), 0] < d2[has_b & (t <= 4), 1]).all()
            lim = (margin * g.h * GA.SAFETY).astype(F32) ** 2
            assert (d2[t == 2, 0] <= lim[t == 2]).all() and (d2[t == 3, 0] > lim[t == 3]).all()   # both sides, one float apart
            assert (gd.stage[t <= 2] == "octant").all() and (gd.stage[t >= 3] != "octant").all()
        elif gd.family == "cube":
            t, rho = gd.extra["t_code"], gd.extra["rho"]
            assert set(rho) == set(g.ladder())
            assert (np.abs(GA.cell_of(g, pts[:, 0]) - qc).max(axis=1) <= rho).all()          # A inside the cube
            assert (np.abs(GA.cell_of(g, pts[:, 1]) - qc).max(axis=1) == rho + 1).all()      # B in the first cell beyond it
            assert (d2[t == 5, 1] < d2[t == 5, 0]).all() and (d2[t <= 4, 0] < d2[t <= 4, 1]).all()
            lim = ((rho.astype(F32) * g.h).astype(F32) * GA.SAFETY) ** 2
            assert (d2[t == 2, 0] <= lim[t == 2]).all() and (d2[t == 3, 0] > lim[t == 3]).all()
            cert = np.array([f"cube{r}" for r in rho], dtype=object)
            # (the corner query's octant margin is one float short of 1: it certifies rho = 1 before the cube does)
            assert ((gd.stage[t <= 2] == cert[t <= 2]) | (gd.stage[t <= 2] == "octant")).all() and (gd.stage[t >= 3] != cert[t >= 3]).all()
        elif gd.family == "chord":
            assert (d2[:, 1] < d2[:, 0]).all()
            _, lowc, _, _ = GA._octant_low(g, q)
            bc = GA.cell_of(g, pts[:, 1])
            assert ((bc < lowc) | (bc > lowc + 1)).any(axis=1).all() and (gd.stage == "cube1").all()
            assert set((bc - qc)[np.arange(len(q)), gd.extra["axis"]]) == {-1, 0, 1}   # the chord's first, only, last cell
        elif gd.family == "gate":
            inside = gd.extra["inside"]
            assert (gd.stage[inside] == "inside").all() and (gd.stage[~inside] == "outside").all()
            assert gd.extra["offset"].max() == g.r_max                          # the cell offset reaches r_max
            assert (gd.extra["grid_stage"][~inside & (gd.extra["offset"] > g.r_max)] == "unmatched").all()


def test_previous_neighbour_gadgets():
    for name in LINES:
        def plan(grid, blocks):
            return [GA.make_prev(grid, blocks.take(64), np.array([0.0, -0.1 * float(grid.h), 0.0], F32))]
        s = _scene(name, plan)
        gd = s.gadgets[0]
        assert s.assert_classes(8)
        src, q2, pts = gd.extra["source"], gd.query, gd.pts
        assert (gd.extra["first_pose_want"] == 0).all()                         # pose 1 finds N
        d2 = GA.d2_f32(np.broadcast_to(q2[:, None, :], pts.shape), pts)
        assert (d2[:, 1] < d2[:, 0]).all() and (gd.want == 1).all()             # pose 2: B, strictly
        d1 = GA.d2_f32(src, pts[:, 0])
        stale = gd.stage == "stale"
        assert (d1[stale] < d2[stale, 0]).all() and (d1[~stale] > d2[~stale, 0]).all()
        # the stale ball does not reach B's row: a bound taken at the old pose would drop it
        assert (np.sqrt(d1[stale].astype(float)) * 1.04 / float(s.grid.h) + 0.04 < 0.25).all()
        idx, _ = GA.brute_force(s.cloud, s.queries)
        assert np.array_equal(idx, s.want)


@pytest.mark.parametrize("k,own", [(1, False), (20, True), (64, False)])
def test_knn_gadgets(k, own):
    g = grid_of("odd")

    def plan(grid, blocks):
        return [GA.make_knn(grid, blocks.take(96), k, 6, own)]
    s = _scene("odd", plan, reach=8)
    s.assert_classes(8)
    gd = s.gadgets[0]
    t, rho = gd.extra["t_code"], gd.extra["rho"]
    q, pts = gd.query, gd.pts
    d2 = GA.d2_f32(np.broadcast_to(q[:, None, :], pts.shape), pts)
    ia, ib = gd.role.index("A"), gd.role.index("B")
    assert (d2[:, :ia].max(axis=1) < d2[:, ia]).all() if ia else True           # the inner points are nearer than A
    assert (d2[t == 5, ib] < d2[t == 5, ia]).all() and (d2[t <= 4, ia] < d2[t <= 4, ib]).all()
    qc = GA.cell_of(g, q)
    assert (np.abs(GA.cell_of(g, pts[:, ib]) - qc).max(axis=1) == rho + 1).all()
    assert (np.abs(GA.cell_of(g, pts[:, ia]) - qc).max(axis=1) <= rho).all()
    kth = np.where(t == 5, ib, ia)
    assert (gd.want[:, k - 1] == kth).all()                                     # the k-th kept is A, or B where t > 1
    cert = np.array([f"shell{r}" if r <= 6 else "far" for r in rho], dtype=object)
    # (t = 63/64 is the last float with d2 <= bound: certified by the strict test only where no float hits the bound itself)
    assert (gd.stage[t <= 1] == cert[t <= 1]).all() and (gd.stage[(t >= 3) & (rho <= 6)] != cert[(t >= 3) & (rho <= 6)]).all()


@pytest.mark.parametrize("R", [1, 8, 9])
def test_radius_gadgets(R):
    import math
    g = grid_of("odd")

    def plan(grid, blocks):
        return [GA.make_radius(grid, blocks.take(96), R, False)]
    s = _scene("odd", plan, reach=9)
    s.assert_classes(8)
    gd = s.gadgets[0]
    radius = gd.extra["radius"]
    assert math.ceil(radius / (float(g.h) * float(GA.SAFETY))) == R
    assert (gd.extra["offset"] == R).all()                                      # B in the rim cell of the R-cube
    inside = gd.extra["inside"]
    assert (np.char.startswith(gd.stage.astype(str), "in") == inside).all()
    assert set(gd.want) == {63, 64, 65}
    # rows counted over the whole scene equal the gadget's own count
    r2 = F32(radius * radius)
    for i in range(0, len(s.queries), 16):
        d = GA.d2_f32(np.broadcast_to(s.queries[i, :3], (len(s.cloud), 3)), s.cloud[:, :3])
        assert int((d < r2).sum()) == gd.want[i]
