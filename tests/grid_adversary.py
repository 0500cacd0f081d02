"""Clouds built ON the grid the library built, so that every early exit of the grid searches is met at its
edge from both sides.  CPU only: NumPy float32 for the arithmetic the kernels do, fractions.Fraction where the exact value matters.
No device code, no restatement of the host's cell-size plan: the grid is READ from the library's ICPGPU_DEBUG line (read_grid) and
the scene is rebuilt on it until the line no longer changes (build_scene).

A gadget is one query with the few cloud points that decide it: A, the candidate an early exit would like to keep, and B, the
point it must not miss.  Every maker returns Gadgets: query, points, roles and the stage the float32 arithmetic of the kernels
predicts (predict_nn / predict_knn walk the certificates as icp_grid_device.h and icp_search.hip state them, on the gadget's own
points, without any pruning -- so a prediction is also the certificates' answer, which the host test compares with brute force).

    octant      the 2x2x2 octant's margin: A inside at t * margin * h, B across the nearest face at margin * h * (1 + 2^-12)
    cube        the cube certificate at every radius of the ladder: A inside at t * rho * h, B in the first cell beyond the cube
    chord       ball pruning: B in a row whose slab is tangent to the ball of the known A, in the chord's first / last cell
    prev        the previous-neighbour bound: two poses; N found under the first bounds the search under the second
    gate        B alone at gate * (1 -+ 2^-12): the last cube and the gate
    knn         the shell certificate of the k-nearest walk (and the outlier filter's copy): k - 1 inner points, A, B
    radius      the radius cube: B at radius * (1 -+ 2^-12) in the rim cell of the R-cube, rows of 64 and 65 entries
    misbinned   octant / cube gadgets whose query or B is a point that float32 binning puts into another cell than exact arithmetic

t runs over T_SET: both sides of 63/64 (kGridSafety) at 2^-10 and at one float of the point's position, and both sides of 1.

What geometry does not allow (written down here because the tests cannot have it):
  * a point at distance rho * h * (1 + 2^-12) that lies beyond a cube face is within 0.023 * rho cells of the query's axis, so
    the "edge" and "corner" variants of the cube and radius gadgets sit in the rows diagonally next to the query's (the query is
    one float short of the face on two or three axes), not in the cube's far edge or corner;
  * with the 3 % inflation of the ball, `rem` in grow_cubes is never within ulps of 0 for a B that is nearer than A: the chord
    gadget puts B's slab tangent to the TRUE ball (its slab distance is B's own distance), which is the nearest a correct input
    gets -- mutant (j) of the issue (no inflation) is what moves `rem` to 0 there.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from search_restated import _d2_pairs

F32, F64 = np.float32, np.float64
SAFETY = F32(0.984375)          # kGridSafety (icp_kernels.h): the 63/64 the issue's t-sets straddle
CELL_LIMIT = 1048576.0          # cell_of's clamp (icp_grid_device.h)
T_NAMES = ("63/64-2^-10", "63/64-ulp", "63/64", "63/64+ulp", "1-2^-10", "1+2^-10")
FRAC_NAMES = ("0", "0+ulp", "0.25", "0.5-ulp", "0.5", "0.5+ulp", "0.75", "1-ulp")
_INF32 = F32(np.inf)


# ---- the grid --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Grid:
    h: np.float32
    inv_h: np.float32
    o: tuple            # (ox, oy, oz) float32
    dims: tuple         # (nx, ny, nz)
    sy: int
    sz: int
    r_max: int
    n: int = 0
    binned: int = 0
    pop: float = 0.0
    max_pop: int = 0
    attempt: int = 0

    def descriptor(self):
        return (float(self.h).hex(), float(self.inv_h).hex(), tuple(float(v).hex() for v in self.o), self.dims, self.sy, self.sz, self.r_max)

    def origin(self):
        return np.array(self.o, F32)

    def ladder(self, r_max=None):
        """the radii grow_cubes takes: 1, 2, 4, ... capped at r_max"""
        r_max, out, r = int(self.r_max if r_max is None else r_max), [], 1
        while True:
            out.append(r)
            if r >= r_max:
                return out
            r = min(2 * r, r_max)


_LINE = re.compile(r"\[icpgpu\] grid n=(\d+) binned=(\d+) h=\S+ dims=(\d+)x(\d+)x(\d+) pop=([0-9.]+) max=(\d+) attempt=(\d+) "
                   r"desc=(\S+),(\S+),(\S+),(\S+),(\S+) sy=(\d+) sz=(\d+) r_max=(\d+)")


def read_grid(err_text: str, n: int) -> Grid:
    """The descriptor of the LAST grid the library built over an n-point cloud, from its ICPGPU_DEBUG line."""
    found = [m for m in _LINE.finditer(err_text) if int(m.group(1)) == n]
    assert found, f"no grid line for n={n} in {err_text[-400:]!r}"
    g = found[-1].groups()
    hx = [F32(float.fromhex(v)) for v in g[8:13]]
    for v, s in zip(hx, g[8:13]):
        assert float(v) == float.fromhex(s), ("not a float32", s)
    return Grid(h=hx[0], inv_h=hx[1], o=tuple(hx[2:5]), dims=(int(g[2]), int(g[3]), int(g[4])), sy=int(g[13]), sz=int(g[14]),
                r_max=int(g[15]), n=int(g[0]), binned=int(g[1]), pop=float(g[5]), max_pop=int(g[6]), attempt=int(g[7]))


def cell_u(grid: Grid, xyz) -> np.ndarray:
    """(x - o) * inv_h in float32, operation for operation what icp_grid_device.h::cell_of floors"""
    xyz = np.asarray(xyz, F32)
    return ((xyz[..., :3] - grid.origin()) * grid.inv_h).astype(F32)


def cell_of(grid: Grid, xyz) -> np.ndarray:
    """floorf((x - o) * inv_h), clamped: the cell the kernels bin a point into (int64, (..., 3))"""
    with np.errstate(invalid="ignore"):
        f = np.floor(cell_u(grid, xyz))
    return np.clip(np.nan_to_num(f, nan=-CELL_LIMIT), -CELL_LIMIT, CELL_LIMIT).astype(np.int64)   # (an absent point: NaN)


def cell_exact(grid: Grid, xyz) -> np.ndarray:
    """The same coordinate from the same float inputs in exact rational arithmetic"""
    xyz = np.atleast_2d(np.asarray(xyz, F32))[:, :3]
    inv = Fraction(float(grid.inv_h))
    out = np.empty(xyz.shape, np.int64)
    for i, p in enumerate(xyz):
        for a in range(3):
            u = (Fraction(float(p[a])) - Fraction(float(grid.o[a]))) * inv
            out[i, a] = max(-int(CELL_LIMIT), min(int(CELL_LIMIT), u.numerator // u.denominator))
    return out


def d2_f32(p, q) -> np.ndarray:
    """the arithmetic contract's squared distance (icp_device.h dist2), float32, element by element"""
    return _d2_pairs(np.asarray(p, F32), np.asarray(q, F32))


def d2_exact_rounded(p, q) -> np.float32:
    """dist2 of ONE pair with every rounding done on exact rationals (what d2_f32's emulation is checked against)"""
    def rn(v: Fraction) -> Fraction:   # round to nearest even float32 (normal range)
        if v == 0:
            return v
        e = 0
        while abs(v) * Fraction(2) ** -e >= 1 << 24:
            e += 1
        while abs(v) * Fraction(2) ** -e < 1 << 23:
            e -= 1
        s = v * Fraction(2) ** -e
        f = s.numerator // s.denominator
        r = s - f
        if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2):
            f += 1
        return Fraction(f) * Fraction(2) ** e
    d = [rn(Fraction(float(F32(q[a]))) - Fraction(float(F32(p[a])))) for a in range(3)]
    return F32(float(rn(d[2] * d[2] + rn(d[1] * d[1] + rn(d[0] * d[0])))))


# ---- floats as an ordered line: bisection over consecutive floats --------------------------------------------------------
def _ord(x):
    i = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _flt(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32).view(F32)


def step(x, n: int):
    """the float n places up (n > 0) or down the ordered line of floats"""
    return _flt(_ord(x) + n)


def first_true(cond, lo, hi) -> np.ndarray:
    """cond is False at lo, True at hi and changes once between them (lo > hi: walking down): the first float where it is True"""
    a, b = _ord(lo), _ord(hi)
    assert not cond(_flt(a)).any() and cond(_flt(b)).all(), "first_true: the bracket does not hold the change"
    while (np.abs(b - a) > 1).any():
        mid = (a + b) // 2
        mid = np.where(np.abs(b - a) > 1, mid, b)
        t = cond(_flt(mid))
        b, a = np.where(t, mid, b), np.where(t, a, mid)
    return _flt(b)


def x_ge(grid: Grid, axis, u_target) -> np.ndarray:
    """the smallest float x whose float32 cell coordinate on `axis` (per element) is >= u_target"""
    ut = np.asarray(u_target, F64)
    axis = np.broadcast_to(np.asarray(axis), ut.shape)
    o, h = grid.origin()[axis], F64(grid.h)
    guess = o.astype(F64) + ut * h
    span = 2.0 * h + np.abs(guess) * 1e-5

    def cond(x):
        return ((x - o) * grid.inv_h).astype(F32).astype(F64) >= ut
    return first_true(cond, (guess - span).astype(F32), (guess + span).astype(F32))


def at_fraction(grid: Grid, axis, cell, code) -> np.ndarray:
    """a coordinate inside `cell` on `axis` at the fraction FRAC_NAMES[code] (`ulp`: one float of the coordinate)"""
    cell, code = np.asarray(cell, F64), np.asarray(code)
    base = np.choose(code, [0.0, 0.0, 0.25, 0.5, 0.5, 0.5, 0.75, 1.0])
    nudge = np.choose(code, [0, 1, 0, -1, 0, 1, 0, -1])
    return _flt(_ord(x_ge(grid, axis, cell + base)) + nudge)


def at_distance(q, axis, sign, t_code, bound_sq, unit) -> np.ndarray:
    """The coordinate on `axis` of a point on the query's axis line, on side `sign`, at T_SET[t_code] of `unit` (a length):
    the 2^-10 members by their nominal distance, the three around 63/64 by bisection on the float32 d2 against bound_sq
    (the certificate's own right-hand side): the last float with d2 <= bound_sq, its inner neighbour, the first beyond."""
    n = len(q)
    qa = q[np.arange(n), axis].astype(F32)
    sign = np.asarray(sign, F64)
    nominal = np.choose(t_code, [63.0 / 64 - 2.0 ** -10, 0, 0, 0, 1 - 2.0 ** -10, 1 + 2.0 ** -10]) * unit
    x_nom = (qa.astype(F64) + sign * nominal).astype(F32)

    def beyond(x):
        d = (x - qa).astype(F32)
        return (d * d).astype(F32) > bound_sq
    far = (qa.astype(F64) + sign * 2.0 * unit).astype(F32)
    first_out = first_true(beyond, qa, far)
    inward = -np.sign(_ord(far) - _ord(qa))           # one float towards the query
    edge = _flt(_ord(first_out) + np.choose(t_code, [0, 2, 1, 0, 0, 0]) * inward)
    return np.where((t_code >= 1) & (t_code <= 3), edge, x_nom).astype(F32)


# ---- gadgets ---------------------------------------------------------------------------------------------------------------
@dataclass
class Gadgets:
    """n gadgets of one maker.  pts (n, m, 3): the cloud points of each (NaN rows: none); role (m,): 'A', 'B', 'N' or 'i' (inner);
    b_first (n,): B gets the lower index in the cloud; stage (n,): the predicted stage; want (n,): the slot of pts the
    certificates keep (-1: unmatched) -- the host test holds it against brute force."""
    family: str
    query: np.ndarray
    pts: np.ndarray
    role: tuple
    b_first: np.ndarray
    stage: np.ndarray = None
    want: np.ndarray = None
    classes: tuple = ()
    extra: dict = field(default_factory=dict)


def _octant_low(grid, q):
    """(own cell, the octant's lower cell, margin): octant_row's arithmetic"""
    u = cell_u(grid, q)
    c = np.floor(u)
    f = (u - c).astype(F32)
    lean = f < F32(0.5)
    margin = np.maximum(f, (F32(1.0) - f).astype(F32)).min(axis=-1)
    return c.astype(np.int64), (c - lean).astype(np.int64), margin.astype(F32), f


def predict_nn(grid: Grid, query, pts, r_max=None):
    """Walk the point-to-point search's certificates over each gadget's own points: (stage, slot kept or -1).  Stage: 'octant',
    'cube<rho>' (certified by that cube) or 'unmatched'.  No pruning is modelled: pruning must not change the answer."""
    r_max = int(grid.r_max if r_max is None else r_max)
    n, m = pts.shape[:2]
    c, lowc, margin, _ = _octant_low(grid, query)
    pc = cell_of(grid, pts)
    d2 = d2_f32(np.broadcast_to(query[:, None, :], pts.shape), pts)
    here = np.isfinite(pts).all(axis=-1)
    d2 = np.where(here, d2, _INF32)
    in_oct = here & ((pc >= lowc[:, None, :]) & (pc <= lowc[:, None, :] + 1)).all(axis=-1)
    cheb = np.abs(pc - c[:, None, :]).max(axis=-1)
    stage = np.full(n, "unmatched", dtype=object)
    want = np.full(n, -1)
    open_ = np.ones(n, bool)

    def settle(seen, bound_sq, name):
        nonlocal open_
        dd = np.where(seen, d2, _INF32)
        best = dd.argmin(axis=1)
        bd = dd[np.arange(n), best]
        ok = open_ & (bd <= bound_sq) & np.isfinite(bd)
        tie = (dd == bd[:, None]).sum(axis=1) > 1        # equal d2: the lower cloud index wins, which only assemble() decides
        stage[ok], want[ok] = name, np.where(tie, -1, best)[ok]
        open_ &= ~ok
    lsafe = (margin * grid.h * SAFETY).astype(F32)
    settle(in_oct, (lsafe * lsafe).astype(F32), "octant")
    for rho in grid.ladder(r_max):
        safe = F32(F32(rho) * grid.h) * SAFETY
        settle(here & (cheb <= rho), F32(safe * safe), f"cube{rho}")
    return stage, want


def _finish(grid, g: Gadgets, r_max=None):
    g.stage, g.want = predict_nn(grid, g.query, g.pts, r_max)
    return g


def _axes(n, k):
    """main axis and its two companions, cycling with the gadget number"""
    a0 = (np.arange(n) + k) % 3
    return a0, (a0 + 1) % 3, (a0 + 2) % 3


def _put(arr, axis, val):
    arr[np.arange(len(arr)), axis] = val


def make_octant(grid: Grid, centres, seed=0) -> Gadgets:
    """One gadget per centre cell.  The fractions cycle through FRAC_NAMES per axis (so all 8 orientations come up), t through
    T_SET, every second pair of copies has no B."""
    n = len(centres)
    i = np.arange(n)
    rng = np.random.default_rng(seed)
    t_code, has_b, b_first = i % 6, (i // 6) % 2 == 0, (i // 12) % 2 == 0
    # (one column stays off the faces: a margin of a whole cell would put A at t > 1 outside the octant)
    code = np.stack([(i // 3 + 3 * (i % 3)) % 8, rng.integers(2, 7, n), rng.integers(0, 8, n)], axis=1)
    code = np.stack([code[i, (a - i % 3) % 3] for a in range(3)], axis=1)   # the cycling column moves over the axes
    q = np.stack([at_fraction(grid, a, centres[:, a], code[:, a]) for a in range(3)], axis=1).astype(F32)
    c, lowc, margin, f = _octant_low(grid, q)
    assert (c == centres).all()
    ax = np.maximum(f, (F32(1.0) - f).astype(F32)).argmin(axis=1)          # the axis the margin comes from
    s = np.where(f[i, ax] < F32(0.5), 1.0, -1.0)                           # towards the octant's nearest face
    lsafe = (margin * grid.h * SAFETY).astype(F32)
    unit = margin.astype(F64) * F64(grid.h)
    A = q.copy()
    _put(A, ax, at_distance(q, ax, -s, t_code, (lsafe * lsafe).astype(F32), unit))
    B = q.copy()
    bx = (q[i, ax].astype(F64) + s * unit * (1 + 2.0 ** -12)).astype(F32)
    beyond = c[i, ax] + np.where(s > 0, 1, 0)                              # the face B has to cross (a cell boundary)
    edge = x_ge(grid, ax, beyond.astype(F64))
    bx = np.where(s > 0, np.maximum(bx, edge), np.minimum(bx, step(edge, -1)))
    _put(B, ax, bx)
    B[~has_b] = np.nan
    g = Gadgets("octant", q, np.stack([A, B], axis=1), ("A", "B"), b_first, classes=("octant", "cube1"))
    g.extra = dict(t_code=t_code, has_b=has_b, margin_axis=ax, code=code)
    return _finish(grid, g)


def _towards(grid, centres, a0, a1, a2, s, where):
    """a query one float short of the face towards `s` on the main axis (and on one / both companions for where = 1 / 2)"""
    n = len(centres)
    near = np.where(s > 0, 7, 0)
    code = np.full((n, 3), 4)
    _put(code, a0, near)
    _put(code, a1, np.where(where >= 1, near, 4))
    _put(code, a2, np.where(where >= 2, near, 4))
    return np.stack([at_fraction(grid, a, centres[:, a], code[:, a]) for a in range(3)], axis=1).astype(F32)


def _beyond_face(grid, q, c, a0, a1, a2, s, where, cells, dist):
    """B at `dist` from the query on the main axis, inside the cell `cells` + 1 cells away; where >= 1: one float into the next row"""
    n = len(q)
    i = np.arange(n)
    B = q.copy()
    bx = (q[i, a0].astype(F64) + s * dist).astype(F32)
    face = x_ge(grid, a0, (c[i, a0] + np.where(s > 0, cells + 1, -cells)).astype(F64))
    _put(B, a0, np.where(s > 0, np.maximum(bx, face), np.minimum(bx, step(face, -1))))
    for ak, lvl in ((a1, 1), (a2, 2)):
        row = x_ge(grid, ak, (c[i, ak] + np.where(s > 0, 1, 0)).astype(F64))
        _put(B, ak, np.where(where >= lvl, np.where(s > 0, row, step(row, -1)), q[i, ak]))
    return B


def make_cube(grid: Grid, centres, r_max=None) -> Gadgets:
    """rho cycles through the ladder, t through T_SET, B's place through face / edge / corner, its side through + and -."""
    n = len(centres)
    i = np.arange(n)
    ladder = np.array(grid.ladder(r_max))
    t_code, where = i % 6, (i // 6) % 3
    rho = ladder[(i // 18) % len(ladder)]
    s = np.where((i // (18 * len(ladder))) % 2 == 0, 1.0, -1.0)
    b_first = (i // (36 * len(ladder)) + i) % 2 == 0
    a0, a1, a2 = _axes(n, i // 6)
    q = _towards(grid, centres, a0, a1, a2, s, where)
    c = cell_of(grid, q)
    assert (c == centres).all()
    safe = (rho.astype(F32) * grid.h).astype(F32) * SAFETY
    unit = rho.astype(F64) * F64(grid.h)
    A = q.copy()
    _put(A, a0, at_distance(q, a0, -s, t_code, (safe * safe).astype(F32), unit))
    B = _beyond_face(grid, q, c, a0, a1, a2, s, where, rho, unit * (1 + 2.0 ** -12))
    g = Gadgets("cube", q, np.stack([A, B], axis=1), ("A", "B"), b_first,
                classes=tuple(f"cube{r}" for r in ladder) + ("unmatched",))
    g.extra = dict(t_code=t_code, rho=rho, where=where)
    return _finish(grid, g, r_max)


def make_chord(grid: Grid, centres) -> Gadgets:
    """A known at D inside the octant; B at D * (1 - 2^-10) in the row beyond the octant whose slab is tangent to the ball
    (B is the first or second float past the row's face), in the chord's only cell, its last cell or its first cell."""
    n = len(centres)
    i = np.arange(n)
    kind, second, b_first = i % 3, (i // 3) % 2, (i // 6) % 2 == 0
    a0, a1, a2 = _axes(n, i // 12)                     # a0: the chord's axis; a1: the slab's axis; a2 at the cell's middle
    q = np.empty((n, 3), F32)
    fa0 = np.choose(kind, [0.25, 0.9, 0.1])
    _put(q, a0, x_ge(grid, a0, centres[i, a0] + fa0))
    _put(q, a1, x_ge(grid, a1, centres[i, a1] + 0.25))
    _put(q, a2, x_ge(grid, a2, centres[i, a2] + 0.5))
    B = q.copy()
    _put(B, a1, _flt(_ord(x_ge(grid, a1, (centres[i, a1] + 1).astype(F64))) + second))
    _put(B, a0, (q[i, a0].astype(F64) + np.choose(kind, [0.0, 0.15, -0.15]) * F64(grid.h)).astype(F32))
    D = np.sqrt(d2_f32(q, B).astype(F64)) / (1 - 2.0 ** -10)
    A = q.copy()
    _put(A, a1, (q[i, a1].astype(F64) - D).astype(F32))
    g = Gadgets("chord", q, np.stack([A, B], axis=1), ("A", "B"), b_first, classes=("cube1",))
    g.extra = dict(kind=kind, axis=a0)
    return _finish(grid, g)


def make_gate(grid: Grid, centres, gate: float, r_max=None, with_query_point=False) -> Gadgets:
    """B alone at gate * (1 - 2^-12) (inside) or gate * (1 + 2^-12) (outside) along an axis, an edge and a diagonal; the query at
    the fraction nearest to B (the cell offset reaches r_max) and at the farthest."""
    n = len(centres)
    i = np.arange(n)
    inside, direction, nearest = i % 2 == 0, (i // 2) % 3, (i // 6) % 2 == 0
    s = np.where((i // 12) % 2 == 0, 1.0, -1.0)
    a0, a1, a2 = _axes(n, i // 24)
    code = np.where((s > 0) == nearest, 7, 0)
    q = np.stack([at_fraction(grid, a, centres[:, a], code) for a in range(3)], axis=1).astype(F32)
    comp = np.zeros((n, 3))
    _put(comp, a0, 1.0)
    _put(comp, a1, np.where(direction >= 1, 1.0, 0.0))
    _put(comp, a2, np.where(direction >= 2, 1.0, 0.0))
    comp /= np.linalg.norm(comp, axis=1, keepdims=True)
    dist = gate * np.where(inside, 1 - 2.0 ** -12, 1 + 2.0 ** -12)
    B = (q.astype(F64) + s[:, None] * comp * dist[:, None]).astype(F32)
    g = Gadgets("gate", q, B[:, None, :], ("B",), np.ones(n, bool), classes=("inside", "outside"))
    stage, want = predict_nn(grid, q, g.pts, r_max)
    if with_query_point:                                            # (self-queries: the radius outlier filter)
        g.pts, g.role = np.stack([q, B], axis=1), ("i", "B")
    d2 = d2_f32(q, B).astype(F64)
    g.stage = np.where(d2 <= gate * gate, "inside", "outside").astype(object)
    g.want = np.full(n, len(g.role) - 1)                            # ungated: B is the neighbour either way
    g.extra = dict(grid_stage=stage, offset=np.abs(cell_of(grid, B) - cell_of(grid, q)).max(axis=1), inside=inside)
    return g


def make_prev(grid: Grid, centres, shift) -> Gadgets:
    """Two poses: identity, then the translation `shift` (float32 (3,), along -y).  Designed in the frame of pose 2: the query at
    fractions (0.25 | 0.1, 0.25, 0.5); B in the octant's row below (slab at 0.25 cells), first float under the face, at D'(1 - 2^-10)
    where D' is N's distance.  kind 0: N along z (pose 2 brings the query nearer to it); kind 1: N along +y, where pose 1 had the
    query NEARER to it than pose 2 has -- a bound taken from the stale distance prunes B away.  Under pose 1 N is nearest."""
    n = len(centres)
    i = np.arange(n)
    shift = np.asarray(shift, F32)
    kind, low_x, b_first = i % 2, (i // 2) % 2, (i // 4) % 2 == 0
    q2 = np.empty((n, 3), F32)
    q2[:, 0] = x_ge(grid, 0, centres[:, 0] + np.where(low_x, 0.1, 0.25))
    q2[:, 1] = x_ge(grid, 1, centres[:, 1] + 0.25)
    q2[:, 2] = x_ge(grid, 2, centres[:, 2] + 0.5)
    src = (q2 - shift).astype(F32)
    q2 = (src + shift).astype(F32)                      # what xform_point makes of it: one rounding per axis
    B = q2.copy()
    B[:, 1] = step(x_ge(grid, 1, centres[:, 1].astype(F64)), -1)
    B[:, 0] = (q2[:, 0].astype(F64) - np.where(low_x, 0.12, 0.0) * F64(grid.h)).astype(F32)
    D = np.sqrt(d2_f32(q2, B).astype(F64)) / (1 - 2.0 ** -10)
    N = q2.copy()
    N[:, 2] = np.where(kind == 0, (q2[:, 2].astype(F64) + D).astype(F32), q2[:, 2])
    N[:, 1] = np.where(kind == 1, (q2[:, 1].astype(F64) + D).astype(F32), q2[:, 1])
    g = Gadgets("prev", q2, np.stack([N, B], axis=1), ("N", "B"), b_first, classes=("bounded", "stale"))
    stage, want = predict_nn(grid, q2, g.pts)
    d1 = d2_f32(np.broadcast_to(src[:, None, :], g.pts.shape), g.pts)
    g.stage = np.where(d1[:, 0] < d2_f32(q2, N), "stale", "bounded").astype(object)
    g.want = want
    g.extra = dict(source=src, first_pose_want=d1.argmin(axis=1), grid_stage=stage, kind=kind)
    return g


def predict_knn(grid: Grid, query, pts, k: int, shells: int):
    """search_knn_kernel's walk over each gadget's own points: 'shell<rho>' where the k-th kept distance is certified (strictly
    below (rho h 63/64)^2), 'far' when shells 0..`shells` do not certify; and the k slots kept, ascending by d2"""
    n = len(query)
    dims = np.array(grid.dims)
    c = np.clip(cell_of(grid, query), 0, dims - 1)
    pc = cell_of(grid, pts)
    here = np.isfinite(pts).all(axis=-1)
    d2 = np.where(here, d2_f32(np.broadcast_to(query[:, None, :], pts.shape), pts), _INF32)
    cheb = np.abs(pc - c[:, None, :]).max(axis=-1)
    stage = np.full(n, "far", dtype=object)
    open_ = np.ones(n, bool)
    for rho in range(shells + 1):
        kth = np.sort(np.where(here & (cheb <= rho), d2, _INF32), axis=1)[:, k - 1]
        safe = F32(F32(rho) * grid.h) * SAFETY
        ok = open_ & (kth < F32(safe * safe))
        stage[ok] = f"shell{rho}"
        open_ &= ~ok
    return stage, np.argsort(d2, axis=1, kind="stable")[:, :k]


def _inner(q, count, h, s, a1, a2):
    """`count` points around the query, all nearer than 0.45 h and on the side away from B, every distance different"""
    n = len(q)
    j = np.arange(count)
    r = (0.05 + 0.4 * (j + 1) / (count + 1)) * F64(h)
    ang = 2.399963 * j
    pts = np.repeat(q[:, None, :], count, axis=1).astype(F64)
    i = np.arange(n)[:, None]
    pts[i, j[None, :], a1[:, None]] += (r * np.cos(ang))[None, :]
    pts[i, j[None, :], a2[:, None]] += (r * np.sin(ang))[None, :] * 0.5
    return pts.astype(F32)


def make_knn(grid: Grid, centres, k: int, shells: int, with_query_point: bool) -> Gadgets:
    """The k nearest of the query: (itself, when the cloud holds it,) inner points, and A at t * rho * h as the candidate k-th;
    B, the true k-th when t > 1, at rho * h * (1 + 2^-12) in the first cell beyond shell rho.  rho = 1 .. shells + 1: the last
    is certified only by the far list."""
    n = len(centres)
    i = np.arange(n)
    t_code = i % 6
    seq = np.array([1] + list(range(1, shells + 2)))    # (rho = 1 twice: nothing is passed on to shell 1 from below)
    rho = seq[(i // 6) % len(seq)]
    s = np.where((i // (6 * len(seq))) % 2 == 0, 1.0, -1.0)
    a0, a1, a2 = _axes(n, i // 6)
    zero = np.zeros(n, int)
    q = _towards(grid, centres, a0, a1, a2, s, zero)
    c = cell_of(grid, q)
    safe = (rho.astype(F32) * grid.h).astype(F32) * SAFETY
    unit = rho.astype(F64) * F64(grid.h)
    A = q.copy()
    # (strict certificate: `63/64` itself, d2 == bound, is NOT certified; the bisection's members stay what they are)
    _put(A, a0, at_distance(q, a0, -s, t_code, (safe * safe).astype(F32), unit))
    B = _beyond_face(grid, q, c, a0, a1, a2, s, zero, rho, unit * (1 + 2.0 ** -12))
    n_inner = k - 1 - (1 if with_query_point else 0)
    parts, role = [], []
    if with_query_point:
        parts.append(q[:, None, :])
        role.append("i")
    if n_inner > 0:
        parts.append(_inner(q, n_inner, grid.h, s, a1, a2))
        role += ["i"] * n_inner
    if k > 1 or not with_query_point:
        parts += [A[:, None, :], B[:, None, :]]
        role += ["A", "B"]
    g = Gadgets(f"knn{k}", q, np.concatenate(parts, axis=1), tuple(role), (i // 3) % 2 == 0,
                classes=tuple(f"shell{r}" for r in range(1, shells + 1)) + ("far",))
    g.stage, g.want = predict_knn(grid, q, g.pts, k, shells)
    g.extra = dict(t_code=t_code, rho=rho, k=k)
    return g


def radius_for(grid: Grid, R: int) -> float:
    """a radius whose cube is R cells: (R - 1/4) * h * 63/64, so that ceil(radius / (h * 63/64)) == R"""
    return (R - 0.25) * float(grid.h) * float(SAFETY)


def make_radius(grid: Grid, centres, R: int, with_query_point: bool) -> Gadgets:
    """The query one float short of the face towards B; 63 or 64 inner points (62 / 63 and the query itself when the cloud holds
    it) and B at radius * (1 - 2^-12): rows of 64 and 65 entries whose last entry is the rim point, in the cell R cells away;
    and B at radius * (1 + 2^-12), which is no neighbour."""
    n = len(centres)
    i = np.arange(n)
    radius = radius_for(grid, R)
    inside, long_row, where = i % 2 == 0, (i // 2) % 2 == 1, (i // 4) % 3
    s = np.where((i // 12) % 2 == 0, 1.0, -1.0)
    a0, a1, a2 = _axes(n, i // 4)
    q = _towards(grid, centres, a0, a1, a2, s, where)
    c = cell_of(grid, q)
    B = _beyond_face(grid, q, c, a0, a1, a2, s, where, R - 1, radius * np.where(inside, 1 - 2.0 ** -12, 1 + 2.0 ** -12))
    n_inner = 64 - (1 if with_query_point else 0)
    inner = _inner(q, n_inner, grid.h, s, a1, a2)
    inner[~long_row, -1] = np.nan                                   # 63 + B = 64 entries; 64 + B = 65
    parts = ([q[:, None, :]] if with_query_point else []) + [inner, B[:, None, :]]
    role = (["i"] if with_query_point else []) + ["i"] * n_inner + ["B"]
    g = Gadgets(f"radius{R}", q, np.concatenate(parts, axis=1), tuple(role), np.zeros(n, bool), classes=("in64", "in65", "out64", "out65"))
    r2 = F32(radius * radius)
    d2 = d2_f32(q, B)
    g.stage = np.array([("in" if a else "out") + ("65" if b else "64") for a, b in zip(d2 < r2, long_row)], dtype=object)
    g.want = (np.isfinite(g.pts).all(axis=-1) & (d2_f32(np.broadcast_to(q[:, None, :], g.pts.shape), g.pts) < r2)).sum(axis=1)
    g.extra = dict(radius=radius, offset=np.abs(cell_of(grid, B) - c).max(axis=1), R=R, inside=inside)
    return g


# ---- mis-binned points -----------------------------------------------------------------------------------------------------
def find_misbinned(grid: Grid, axis: int, cells, fixed, reach: int = 6):
    """For each cell face `cells` on `axis` (the other coordinates from `fixed`, a point): the floats within `reach` places of
    the face whose float32 cell differs from their exact cell.  -> (coordinates, float cell, exact cell), one per face at most."""
    cells = np.asarray(cells)
    face = x_ge(grid, axis, cells.astype(F64))
    xs, fc, ec = [], [], []
    for x0, k in zip(face, cells):
        cand = _flt(_ord(x0) + np.arange(-reach, reach + 1))
        p = np.tile(np.asarray(fixed, F32), (len(cand), 1))
        p[:, axis] = cand
        cf = cell_of(grid, p)[:, axis]
        # (float64 narrows: the exact coordinate is within 2^-40 of it; Fractions decide the few that are left)
        u64 = (cand.astype(F64) - F64(grid.o[axis])) * F64(grid.inv_h)
        for j in np.flatnonzero(np.floor(u64) != cf):
            ce = cell_exact(grid, p[j])[0, axis]
            if ce != cf[j]:
                xs.append(cand[j]); fc.append(cf[j]); ec.append(ce)
                break
    return np.array(xs, F32), np.array(fc, np.int64), np.array(ec, np.int64)


def make_misbinned(grid: Grid, axis: int, found, other_cells) -> Gadgets:
    """Octant and cube gadgets around mis-binned coordinates `found` = find_misbinned's result: even copies have the QUERY on
    such a coordinate (an octant gadget on the float cell's fractions of the other axes), odd copies have B on it (a cube gadget
    of rho = 1 or 2 whose query is one float short of its own face)."""
    xs, fc, ec = found
    n = len(xs)
    i = np.arange(n)
    t_code, as_query = (i // 2) % 6, i % 2 == 0
    rho = 1 + (i // 12) % 2
    s = np.ones(n)                                                  # B beyond the face in +axis
    a0 = np.full(n, axis)
    a1, a2 = (a0 + 1) % 3, (a0 + 2) % 3
    centres = np.empty((n, 3), np.int64)
    centres[:, axis] = np.where(as_query, fc, fc - rho - 1)
    centres[:, (axis + 1) % 3], centres[:, (axis + 2) % 3] = other_cells[0], other_cells[1]
    q = _towards(grid, centres, a0, a1, a2, s, np.zeros(n, int))
    q[as_query, axis] = xs[as_query]
    c, lowc, margin, f = _octant_low(grid, q)
    unit = np.where(as_query, margin.astype(F64), rho.astype(F64)) * F64(grid.h)
    bound = np.where(as_query, (margin * grid.h * SAFETY).astype(F32), (rho.astype(F32) * grid.h).astype(F32) * SAFETY).astype(F32)
    ax = np.where(as_query, np.maximum(f, (F32(1.0) - f).astype(F32)).argmin(axis=1), axis)
    sa = np.where(as_query, np.where(f[i, ax] < F32(0.5), 1.0, -1.0), s)
    A = q.copy()
    _put(A, ax, at_distance(q, ax, -sa, t_code, (bound * bound).astype(F32), unit))
    B = q.copy()
    bq = (q[i, ax].astype(F64) + sa * unit * (1 + 2.0 ** -12)).astype(F32)
    edge = x_ge(grid, ax, (c[i, ax] + np.where(sa > 0, 1, 0)).astype(F64))
    bq = np.where(sa > 0, np.maximum(bq, edge), np.minimum(bq, step(edge, -1)))
    _put(B, ax, np.where(as_query, bq, xs))
    g = Gadgets("misbinned", q, np.stack([A, B], axis=1), ("A", "B"), (i // 4) % 2 == 0, classes=("query", "B"))
    stage, g.want = predict_nn(grid, q, g.pts)
    g.stage = np.where(as_query, "query", "B").astype(object)
    g.extra = dict(grid_stage=stage, float_cell=fc, exact_cell=ec)
    return g


# ---- scenes ----------------------------------------------------------------------------------------------------------------
@dataclass
class Scene:
    grid: Grid
    cloud: np.ndarray          # (m, 4) float32: anchors, filler, then the gadgets' points
    queries: np.ndarray        # (q, 4) float32
    family: np.ndarray         # per query
    stage: np.ndarray
    want: np.ndarray           # index into cloud the certificates keep (-1: none; radius family: the row's length)
    gadgets: list
    slots: list                # per Gadgets: (n, m) index into cloud of every point (-1: none)
    passes: int = 0

    def counts(self):
        out = {}
        for f, s in zip(self.family, self.stage):
            out[(f, s)] = out.get((f, s), 0) + 1
        return out

    def assert_classes(self, at_least=8):
        c = self.counts()
        for g in self.gadgets:
            for cls in g.classes:
                assert c.get((g.family, cls), 0) >= at_least, (g.family, cls, c)
        return c


def clumps(lo, spacing, nx, ny, size, per, seed=0):
    """filler: nx * ny clumps of `per` points within `size` of lattice sites in the plane z = lo[2], `spacing` apart"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    site = np.stack([lo[0] + spacing * (gx.ravel() + 0.5), lo[1] + spacing * (gy.ravel() + 0.5), np.full(gx.size, lo[2] + size)], axis=1)
    pts = np.repeat(site, per, axis=0) + rng.uniform(0, size, (gx.size * per, 3))
    return pts.astype(F32)


class Blocks:
    """Centre cells for gadgets: a lattice of `pitch` cells inside the grid, pitch / 2 + 2 cells clear of its faces (the anchors
    sit in the corner cells) and `pitch` cells above the filler (every cell up to z index `floor_z`)."""

    def __init__(self, grid: Grid, pitch: int, floor_z: int):
        self.grid, self.pitch = grid, int(pitch)
        clear = self.pitch // 2 + 2
        lo = np.array([clear, clear, floor_z + self.pitch])
        cnt = (np.array(grid.dims) - clear - lo) // self.pitch + 1
        assert (cnt >= 1).all(), ("the box holds no gadget block", grid.dims, pitch, floor_z)
        self.lo, self.cnt, self.used = lo, cnt, 0

    def take(self, n: int) -> np.ndarray:
        k = self.used + np.arange(n)
        assert self.used + n <= int(np.prod(self.cnt)), ("the box is too small for the gadgets", self.used + n, self.cnt, self.grid.dims)
        self.used += n
        idx = np.stack([k % self.cnt[0], (k // self.cnt[0]) % self.cnt[1], k // (self.cnt[0] * self.cnt[1])], axis=1)
        return self.lo + idx * self.pitch


def assemble(grid: Grid, fixed, gadget_sets, centred=False) -> Scene:
    """The cloud of `fixed` points (anchors, filler) and every gadget's points -- B before A where b_first says so -- and the
    queries.  centred: every gadget point at the centre of the cell it will occupy (pass 1 of build_scene)."""
    rows, queries, family, stage, want, slots = [np.asarray(fixed, F32)[:, :3]], [], [], [], [], []
    at = len(fixed)
    for g in gadget_sets:
        n, m = g.pts.shape[:2]
        order = np.tile(np.arange(m), (n, 1))
        if "A" in g.role and "B" in g.role:
            ia, ib = g.role.index("A"), g.role.index("B")
            sw = np.asarray(g.b_first, bool)
            order[sw, ia], order[sw, ib] = ib, ia
        elif "N" in g.role:
            sw = np.asarray(g.b_first, bool)
            order[sw, 0], order[sw, 1] = 1, 0
        pts = np.take_along_axis(g.pts, order[:, :, None], axis=1)
        here = np.isfinite(pts).all(axis=-1)
        pos = np.full((n, m), -1)
        pos[here] = at + np.arange(int(here.sum()))
        slot = np.full((n, m), -1)
        np.put_along_axis(slot, order, pos, axis=1)                  # slot[i, role slot] = index in the cloud
        flat = pts[here]
        if centred:
            flat = (grid.origin().astype(F64) + (cell_of(grid, flat) + 0.5) * F64(grid.h)).astype(F32)
        rows.append(flat)
        at += len(flat)
        slots.append(slot)
        queries.append(g.query)
        family += [g.family] * n
        stage += list(g.stage)
        if g.family.startswith("radius"):
            want += list(g.want)
        elif g.want.ndim == 1:
            want += [slot[i, w] if w >= 0 else -1 for i, w in enumerate(g.want)]
        else:
            want += [-2] * n
    cloud = np.ones((at, 4), F32)
    cloud[:, :3] = np.concatenate(rows)
    q = np.ones((sum(len(x) for x in queries), 4), F32)
    q[:, :3] = np.concatenate(queries) if queries else np.zeros((0, 3), F32)
    return Scene(grid, cloud, q, np.array(family, dtype=object), np.array(stage, dtype=object), np.array(want), list(gadget_sets), slots)


def build_scene(probe, fixed, plan, pitch_of, max_passes: int = 6) -> Scene:
    """probe(cloud (m, 4)) -> Grid: set the cloud in the library and read the grid it built.  plan(grid, blocks) -> [Gadgets].
    pitch_of(grid) -> cells between gadget centres (at least 2 * r_max + 2).

    Pass 0 probes the fixed points alone.  Pass 1 puts every gadget point at the centre of the cell it will occupy, on the grid
    read so far, and probes again; then the points move to their adversarial places inside the same cells, and the probe must
    show the IDENTICAL descriptor: per-cell counts, and with them pop, max and the host's plan, cannot have changed.  Where a
    plan makes the cell size a continuous function of the population (a probe between passes that differs), the scene is laid
    out again on the new grid; it has to settle within max_passes."""
    fixed = np.asarray(fixed, F32)
    cloud0 = np.ones((len(fixed), 4), F32)
    cloud0[:, :3] = fixed[:, :3]
    grid = probe(cloud0)
    for n_pass in range(1, max_passes + 1):
        floor_z = int(cell_of(grid, fixed[2:])[:, 2].max()) if len(fixed) > 2 else 0
        sets = plan(grid, Blocks(grid, pitch_of(grid), floor_z))
        centred = assemble(grid, fixed, sets, centred=True)
        g1 = probe(centred.cloud)
        if g1.descriptor() != grid.descriptor():
            grid = g1
            continue
        scene = assemble(grid, fixed, sets)
        assert (cell_of(grid, scene.cloud) == cell_of(grid, centred.cloud)).all(), "a gadget point left its cell"
        g2 = probe(scene.cloud)
        assert g2.descriptor() == grid.descriptor(), ("the adversarial positions changed the grid", g2, grid)
        assert (g2.pop, g2.max_pop, g2.attempt, g2.binned) == (g1.pop, g1.max_pop, g1.attempt, g1.binned)
        scene.grid, scene.passes = g2, n_pass
        return scene
    raise AssertionError(f"the grid did not settle in {max_passes} passes: {grid}")


def brute_force(cloud, queries):
    """(index, d2) of every query's nearest cloud point under the arithmetic contract: lowest index among equal d2"""
    idx = np.empty(len(queries), np.int64)
    d2 = np.empty(len(queries), F32)
    for lo in range(0, len(queries), 256):
        q = queries[lo:lo + 256, None, :3]
        d = d2_f32(np.broadcast_to(q, (q.shape[0], len(cloud), 3)), np.broadcast_to(cloud[None, :, :3], (q.shape[0], len(cloud), 3)))
        idx[lo:lo + 256] = d.argmin(axis=1)
        d2[lo:lo + 256] = d.min(axis=1)
    return idx, d2
