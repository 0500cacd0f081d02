"""Clouds at the edges of the three brute-force search kernels' launch arithmetic (icpslam_amd/csrc/icp_kernels.hip: nn_brute_kernel;
icp_brute_mfma.hip; icp_brute_bf16.hip, as shipped <2, 1024, 512> and in its bound-check shape <2, 512, 256>), shared by
tests/test_brute_cases_host.py (no GPU) and tests/test_gpu_brute_edges.py, and a restatement of the three launch plans in Python
integers.  Nothing here calls the library; every expectation comes from oracle.nn or from the restated plans.

What the matrix-core kernels are launched over is the source's FINITE rows (the source grid's n_binned), while the 8192-point
threshold is on the row counts -- so a source of 8192 rows of which 8191 are NaN launches them with one source, and every small
launch shape is reachable.  A case is (name, src, tgt, T) plus what the sweep's debug line must say (`matrix`: the matrix-core
kernels run unless brute_variant is 1)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
MIN_MATRIX = 8192            # kMfmaMinPoints: both clouds need this many ROWS for the matrix-core kernels
STEP = 32                    # targets per MFMA step


# ---- the three launch plans, restated -------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    kernel: str
    g: int          # groups of 32 sources per wave (matrix kernels); source points per lane (valu)
    tile: int
    block: int
    grid_x: int
    splits: int
    per: int        # targets per split: whole tiles

    def last_lim(self, n_t: int) -> int:
        """Rows of the last split's last tile."""
        rem = n_t - (self.splits - 1) * self.per
        return rem - (rem - 1) // self.tile * self.tile

    def last_tiles(self, n_t: int) -> int:
        """Tiles of the last split."""
        return -(-(n_t - (self.splits - 1) * self.per) // self.tile)


def _split(n_t: int, want_splits: int, tile: int, at_least_one_tile: bool):
    splits = min(want_splits, -(-n_t // tile))
    splits = max(splits, 1)
    per = -(-n_t // splits)
    per = -(-per // tile) * tile
    if at_least_one_tile:
        per = max(per, tile)
    return max(-(-n_t // per), 1 if at_least_one_tile else 0), per


def plan_valu(n_s: int, n_t: int, num_cus: int) -> Plan:
    """plan_nn_brute, variant 0 or 1: 256 threads x 4 sources, tiles of 1024, ~8 workgroups per CU."""
    grid_x = max(-(-n_s // 1024), 1)
    splits, per = _split(n_t, -(-num_cus * 8 // grid_x), 1024, True)
    return Plan("valu", 4, 1024, 256, grid_x, splits, per)


def plan_mfma(n_q: int, n_t: int, num_cus: int) -> Plan:
    """plan_nn_brute_mfma: 4 waves x 2 groups of 32 sources, tiles of 1024, ~32 waves per SIMD."""
    grid_x = -(-n_q // 256)
    splits, per = _split(n_t, -(-num_cus * 32 // grid_x), 1024, False)
    return Plan("mfma", 2, 1024, 256, grid_x, splits, per)


def plan_bf16(n_q: int, n_t: int, num_cus: int, check: bool = False) -> Plan:
    """plan_nn_brute_bf16: as shipped 8 waves x 2 groups, tiles of 1024; the bound-check shape 4 waves x 2 groups, tiles of 512."""
    tile, block = (512, 256) if check else (1024, 512)
    waves = block // 64
    grid_x = -(-n_q // (waves * 64))
    splits, per = _split(n_t, -(-(num_cus * 32 * 4 // waves) // grid_x), tile, False)
    return Plan("bf16-check" if check else "bf16", 2, tile, block, grid_x, splits, per)


def expected_plan(case: "Case", variant: int, num_cus: int, check: bool = False) -> Plan:
    """What the debug line of a sweep over `case` must say."""
    n_s, n_t = case.src.shape[0], case.tgt.shape[0]
    if variant == 1 or not case.matrix:
        return plan_valu(n_s, n_t, num_cus)
    n_q = finite_rows(case.src)
    return plan_mfma(n_q, n_t, num_cus) if variant == 2 else plan_bf16(n_q, n_t, num_cus, check)


LINE_FIELDS = ("n_q", "n_s", "n_t", "num_cus", "G", "TILE", "BLOCK", "grid_x", "splits", "per", "seeded")


def parse_lines(stderr: str):
    """The `[icpgpu] brute kernel=... key=value ...` lines of a captured stderr, as dicts (kernel: str, the rest int)."""
    out = []
    for ln in stderr.splitlines():
        if not ln.startswith("[icpgpu] brute "):
            continue
        kv = dict(w.split("=", 1) for w in ln.split()[2:])
        out.append({k: (v if k == "kernel" else int(v)) for k, v in kv.items()})
    return out


def line_of(plan: Plan, n_q: int, n_s: int, n_t: int, num_cus: int, seeded: int) -> dict:
    return dict(kernel=plan.kernel, n_q=n_q, n_s=n_s, n_t=n_t, num_cus=num_cus, G=plan.g, TILE=plan.tile, BLOCK=plan.block,
                grid_x=plan.grid_x, splits=plan.splits, per=plan.per, seeded=seeded)


# ---- building blocks ------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    src: np.ndarray
    tgt: np.ndarray
    T: np.ndarray
    matrix: bool = True                          # False: the line must say `valu` for every variant
    ties: list = field(default_factory=list)     # (source row, lower target row, higher target row)
    bad: list = field(default_factory=list)      # (non-finite target row, [source rows copied from its step and half])
    tail: list = field(default_factory=list)     # source rows whose neighbour must lie in the last tile

    def __iter__(self):
        return iter((self.name, self.src, self.tgt, self.T))


def finite_rows(c) -> int:
    return int(np.isfinite(np.asarray(c)[:, :3]).all(axis=1).sum())


def cloud(xyz) -> np.ndarray:
    xyz = np.asarray(xyz)
    c = np.ones((xyz.shape[0], 4), F32)
    c[:, :3] = xyz[:, :3]
    return c


def pose(tx=0.3, ty=-0.2, tz=0.05, roll=0.01, pitch=-0.02, yaw=0.04) -> np.ndarray:
    from icpslam_amd import synth
    return synth.pose_matrix(tx, ty, tz, roll, pitch, yaw).astype(F32)


IDENTITY = np.eye(4, dtype=F32)


def preimage(T, xyz) -> np.ndarray:
    """Points s with T s ~ xyz (to a float rounding): sources that land on chosen targets under a pose."""
    T = np.asarray(T, np.float64)
    return ((np.asarray(xyz, np.float64)[:, :3] - T[:3, 3]) @ T[:3, :3]).astype(F32)


def bad_rows(k: int, first: int = 0) -> np.ndarray:
    """k non-finite rows: NaN, +inf, -inf cycled through x, y, z (the other coordinates finite)."""
    rows = np.ones((k, 4), F32)
    i = np.arange(first, first + k)
    rows[:, :3] = (i[:, None] % 7 - 3.0 + np.arange(3)[None, :]).astype(F32)
    rows[np.arange(k), (i // 3) % 3] = np.array([np.nan, np.inf, -np.inf], F32)[i % 3]
    return rows


def pad_source(finite: np.ndarray, rows: int = MIN_MATRIX, seed: int = 0):
    """`finite` (n_b, 4) spread, in order, through max(rows, n_b) rows; the others are non-finite.  The non-finite rows take
    the first row, the last row and the rows around the wave boundaries first, then random places -- never a block at the
    end.  Returns (cloud, where): where[i] = the row finite[i] went to."""
    n_b = finite.shape[0]
    n = max(rows, n_b)
    n_bad = n - n_b
    edges = [0, n - 1] + [r for w in range(64, n - 1, 64) for r in (w, w - 1)]
    rng = np.random.default_rng(1000 + seed)
    rest = np.setdiff1d(np.arange(n), edges)
    order = np.concatenate([np.array(edges[: max(n_bad, 0)], np.int64), rng.permutation(rest)])[:n_bad]
    is_bad = np.zeros(n, bool)
    is_bad[order] = True
    out = np.empty((n, 4), F32)
    out[is_bad] = bad_rows(n_bad)
    where = np.flatnonzero(~is_bad)
    out[where] = finite
    return out, where


@functools.lru_cache(maxsize=None)
def _scans():
    from icpslam_amd import synth
    s, t, _ = synth.make_pair(66000, 70000, seed=41)
    s.setflags(write=False)
    t.setflags(write=False)
    return s, t


def scan_source(n: int) -> np.ndarray:
    return _scans()[0][:n].copy()


def scan_target(n: int) -> np.ndarray:
    return _scans()[1][:n].copy()


# ---- (a) source shapes, (b) target shapes ---------------------------------------------------------------------------------
SOURCE_COUNTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 8191, 8192, 8193)
TARGET_COUNTS = (8191, 8192, 8193) + tuple(8192 + d for d in (31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025))


def source_shape_cases():
    tgt = scan_target(MIN_MATRIX + 33)
    for n_b in SOURCE_COUNTS:
        src, _ = pad_source(scan_source(n_b), seed=n_b)
        yield Case(f"a: {n_b} finite sources in {src.shape[0]} rows", src, tgt, pose())
    src, _ = pad_source(scan_source(4000), rows=MIN_MATRIX - 1, seed=5)
    yield Case("a: 8191 source rows (below the threshold)", src, tgt, pose(), matrix=False)


def target_shape_cases(n_b: int):
    src, _ = pad_source(scan_source(n_b), seed=n_b)
    for n_t in TARGET_COUNTS:
        yield Case(f"b: {n_t} targets, {n_b} finite sources", src, scan_target(n_t), pose(), matrix=n_t >= MIN_MATRIX)


# ---- (c) several tiles per split ------------------------------------------------------------------------------------------
MULTI_TILE_SOURCES = 65537
MULTI_TILE_LIMS = {512: (1, 33, 64, 511), 1024: (1, 33, 64, 1023)}


def multi_tile_targets(plan_fn, num_cus: int, lim: int, n_q: int = MULTI_TILE_SOURCES) -> int:
    """The n_t at which plan_fn(n_q, n_t, num_cus) gives splits of exactly two tiles, the last split's second tile `lim` rows."""
    tile = plan_fn(n_q, 1 << 20, num_cus).tile
    for splits in range(1, 4096):
        n_t = (splits - 1) * 2 * tile + tile + lim
        p = plan_fn(n_q, n_t, num_cus)
        if p.splits == splits and p.per == 2 * tile:
            return n_t
    raise AssertionError("no target size gives two tiles per split")


def multi_tile_case(plan_fn, num_cus: int, lim: int) -> Case:
    """65 537 sources; every split two tiles; ties across the tiles of a split, across two splits and across the whole cloud;
    64 sources whose neighbours are the last tile's rows."""
    n_t = multi_tile_targets(plan_fn, num_cus, lim)
    p = plan_fn(MULTI_TILE_SOURCES, n_t, num_cus)
    T = pose()
    tgt = scan_target(n_t)
    pairs = [(p.tile - 1, p.tile), (7, 7 + p.per), (p.per + 40, 2 * p.per + 40 + p.tile), (0, n_t - 1)]
    for lo, hi in pairs:
        tgt[hi] = tgt[lo]
    src = scan_source(MULTI_TILE_SOURCES)
    ties = []
    for k, (lo, hi) in enumerate(pairs):
        src[100 + k, :3] = preimage(T, tgt[lo:lo + 1])
        ties.append((100 + k, lo, hi))
    rng = np.random.default_rng(lim)
    last = np.arange(n_t - lim, n_t)[-64:]
    last = last[last != n_t - 1] if lim > 1 else last      # (the cloud's last row is the copy of row 0 above)
    rows = 200 + np.arange(last.size)
    if lim > 1:
        src[rows, :3] = preimage(T, tgt[last]) + rng.normal(0, 2e-4, (last.size, 3)).astype(F32)
    return Case(f"c: {n_t} targets in splits of two {p.tile}-row tiles, last tile of {lim}", src, tgt, T, ties=ties, tail=list(rows) if lim > 1 else [])


# ---- (d) a non-finite target in every row position of a step --------------------------------------------------------------
def _half_mates(row: int) -> list:
    """The other rows of a step that the same half-wave folds (rows with an equal bit 2)."""
    return [r for r in range(STEP) if (r ^ row) & 4 == 0 and r != row]


def nonfinite_slot_case(name: str, n_t: int, placing: dict) -> Case:
    """placing: residue -> step (of 32 targets) that holds a non-finite row at that residue.

    The target is built so that nothing else can send that step through the exact path: all sources and the 15 rows the bad
    row's half-wave folds with it lie within 2 cm of the origin; every other row is `background`, 50 m away and farther with
    every row of its 512-row tile (5 cm a row: more than the sources' spread), so that after a tile's first step no background
    row undercuts a bound.  The bad steps are never a tile's first (bounds are infinite there and every lane looks exactly).
    A fold that a NaN poisons therefore loses the neighbours of the 15 sources copied from those rows."""
    rng = np.random.default_rng(len(name) + n_t)
    i = np.arange(n_t)
    d = rng.normal(size=(n_t, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tgt = cloud(d * (50.0 + 0.05 * (i % 512))[:, None])
    finite, bad = [], []
    for k, (res, step) in enumerate(sorted(placing.items())):
        assert step % 16 != 0, "a tile's first step is looked at exactly whatever the fold says"
        base = step * STEP
        mates = [base + r for r in _half_mates(res) if base + r < n_t]
        tgt[mates, :3] = rng.uniform(-0.01, 0.01, (len(mates), 3))
        tgt[base + res] = bad_rows(1, first=k)[0]
        first = len(finite)
        finite.extend(tgt[mates, :3] + rng.normal(0, 1e-4, (len(mates), 3)))
        bad.append((base + res, list(range(first, first + len(mates)))))
    src, where = pad_source(cloud(np.array(finite)), seed=n_t)
    bad = [(row, [int(where[s]) for s in rows]) for row, rows in bad]
    return Case(name, src, tgt, IDENTITY, bad=bad)


def nonfinite_slot_cases():
    # whole tiles: residue r in 512-row tile r / 2, at a step that is no tile's first
    yield nonfinite_slot_case("d: a non-finite target at every row position, whole tiles", MIN_MATRIX + 33,
                              {r: 16 * (r // 2) + 1 + (7 * r) % 15 for r in range(32)})
    # the partial last tile of 1023 rows (tiles of 1024) / 511 rows (tiles of 512): residues 0..30 at steps 1..31 behind row
    # 8192 (the last one is the cloud's last row), then residues 17..31 inside the last 511 rows
    yield nonfinite_slot_case("d: non-finite targets in the partial last tile, residues 0-30", MIN_MATRIX + 1023,
                              {r: 256 + 1 + r for r in range(31) if r != 15})
    yield nonfinite_slot_case("d: non-finite targets in the last 511 rows, residues 17-31", MIN_MATRIX + 1023,
                              {r: 256 + 17 + (r - 16) % 15 for r in range(17, 32)})


# ---- (e) ties across every seam -------------------------------------------------------------------------------------------
def seam_pairs(n_t: int):
    """(what, lower row, higher row): duplicated target points on both sides of every seam of the three kernels."""
    return [("two halves of a step", 32 * 9 + 3, 32 * 9 + 4),
            ("two halves of a step, tail slots", 32 * 21 + 27, 32 * 21 + 30),
            ("two steps of a trip", 64 * 5 + 31, 64 * 5 + 32),
            ("two trips", 64 * 9 + 63, 64 * 10),
            ("two tiles of 512", 511, 512),
            ("two tiles of 1024 (two splits)", 1023, 1024),
            ("two splits of 512, j and j + per", 100, 612),
            ("two splits of 1024, j and j + per", 2100, 3124),
            ("far splits", 77, 7 * 1024 + 77),
            ("the partial last tile", 8000, n_t - 2),
            ("first and last row", 0, n_t - 1)]


def tie_cases():
    n_t = MIN_MATRIX + 33
    tgt = scan_target(n_t)
    pairs = seam_pairs(n_t)
    for _, lo, hi in pairs:
        tgt[hi] = tgt[lo]
    finite = scan_source(MIN_MATRIX - 8)
    ties = []
    rng = np.random.default_rng(3)
    for k, (_, lo, hi) in enumerate(pairs):
        finite[40 * k + 5, :3] = tgt[lo, :3]                                           # exactly on it: d2 = 0 twice
        finite[40 * k + 6, :3] = tgt[lo, :3] + rng.normal(0, 1e-3, 3).astype(F32)      # beside it: the same d2 twice
        ties += [(40 * k + 5, lo, hi), (40 * k + 6, lo, hi)]
    src, where = pad_source(finite, seed=8)
    yield Case("e: duplicated targets across every seam", src, tgt, IDENTITY, ties=[(int(where[s]), lo, hi) for s, lo, hi in ties])
    one = np.tile(np.array([[3.0, -2.0, 0.5, 1.0]], F32), (n_t, 1))
    src, _ = pad_source(scan_source(MIN_MATRIX - 3), seed=9)
    yield Case("e: all targets coincident", src, one, pose())


def lattice_case() -> Case:
    """Every distance tied eight times: sources at the cell centres of a 32 x 32 x 10 lattice of targets."""
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(10)), -1).reshape(-1, 3).astype(F32) * F32(0.25)
    return Case("e: lattice, every distance tied", cloud(g + F32(0.125)), cloud(g), IDENTITY)


def lattice_shift() -> np.ndarray:
    """One lattice step along -x (exact in float32): rows are ordered (y, x, z), so a source's old neighbour -- the lowest row
    of its eight corners -- is a corner of its new cell too, tied with the new lowest one and no longer it."""
    T = np.eye(4, dtype=F32)
    T[0, 3] = -0.25
    return T


# ---- (f) degenerate centres -----------------------------------------------------------------------------------------------
def degenerate_cases():
    n_t = MIN_MATRIX + 33
    rng = np.random.default_rng(12)
    # one workgroup of coincident sources (P = 0) at the origin; targets exactly on them (scale 0), a hair beside them (scale
    # below kTinyScale = 1e-18), and ordinary ones
    zero = np.zeros((512, 4), F32)
    zero[:, 3] = 1.0
    src, _ = pad_source(zero, seed=1)
    tgt = scan_target(n_t)
    tgt[[5000, 8200, 40, 7000], :3] = 0.0
    tgt[[41, 6000], :3] = (1e-10, 0.0, 0.0)
    tgt[300:364, :3] = rng.normal(0, 1e-11, (64, 3)).astype(F32)
    yield Case("f: 512 coincident sources, targets on and beside the centre", src, tgt, IDENTITY)
    tgt = scan_target(n_t)
    tgt[[6000, 41], :3] = (0.0, 2e-10, 0.0)
    tgt[300:364, :3] = rng.normal(0, 1e-9, (64, 3)).astype(F32) + F32(1e-9)
    yield Case("f: 512 coincident sources, nearest targets a hair away", src.copy(), tgt, IDENTITY)
    # the same away from the origin: targets on the centre and one float step beside it
    c = np.array([1.5, -2.25, 0.75], F32)
    src, _ = pad_source(np.tile(np.append(c, F32(1.0))[None, :], (512, 1)), seed=2)
    tgt = scan_target(n_t)
    tgt[[7100, 90], :3] = c
    tgt[[89, 6100], :3] = np.nextafter(c, F32(np.inf))
    yield Case("f: 512 coincident sources off the origin", src, tgt, IDENTITY)
    # 50 far outliers inside one workgroup: a large P
    s = scan_source(MIN_MATRIX)
    s[rng.permutation(MIN_MATRIX)[:50], :3] = (900.0, -700.0, 80.0)
    yield Case("f: 50 far outliers among the sources", s, scan_target(n_t), pose())
    # 4096 coincident sources (the most a grid cell may hold) and 4096 spread ones
    s = scan_source(MIN_MATRIX)
    s[rng.permutation(MIN_MATRIX)[:4096], :3] = (200.0, 200.0, 50.0)
    yield Case("f: 4096 coincident sources and 4096 spread", s, scan_target(n_t), pose())
    # 8192 coincident sources: the source grid refuses them (one cell of 8192), the plain kernel answers
    s = np.tile(np.array([[2.0, 1.0, 0.5, 1.0]], F32), (MIN_MATRIX, 1))
    yield Case("f: 8192 coincident sources (the grid refuses)", s, scan_target(n_t), pose(), matrix=False)
    t = bad_rows(n_t)
    t[4321] = (1.0, 2.0, 3.0, 1.0)
    yield Case("f: every target non-finite but one", scan_source(MIN_MATRIX), t, pose())
    yield Case("f: every target non-finite", scan_source(MIN_MATRIX), bad_rows(n_t), pose())


# ---- (g) seeded sweeps ----------------------------------------------------------------------------------------------------
def far_pose() -> np.ndarray:
    """5 m and 0.5 rad from pose(): the neighbours of a sweep at pose() are poor seeds for one here."""
    return pose(0.3 + 3.0, -0.2 - 4.0, 0.05, 0.01, -0.02, 0.04 + 0.5)


def seeded_cases():
    """The subset of (a)-(e) that is swept three times in one context; (case, T of the second sweep, T of the third)."""
    a = {c.name: c for c in source_shape_cases()}
    for n_b in (1, 33, 513, 8193):
        c = next(v for k, v in a.items() if k.startswith(f"a: {n_b} finite"))
        yield c, c.T, far_pose()
    b = list(target_shape_cases(33))
    for c in b:
        if c.tgt.shape[0] in (8192, 8192 + 33, 8192 + 1023, 8192 + 1025):
            yield c, c.T, far_pose()
    for c in nonfinite_slot_cases():
        yield c, c.T, far_pose()
    for c in tie_cases():
        yield c, c.T, far_pose()
    lat = lattice_case()
    yield lat, lattice_shift(), far_pose()


GROUPS = {
    "a-source-shapes": source_shape_cases,
    "b-target-shapes-8192": lambda: target_shape_cases(8192),
    "b-target-shapes-33": lambda: target_shape_cases(33),
    "d-nonfinite-slots": nonfinite_slot_cases,
    "e-ties": lambda: list(tie_cases()) + [lattice_case()],
    "f-degenerate": degenerate_cases,
}
