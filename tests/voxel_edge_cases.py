"""Boxes and leaves at the edges of the voxel filter's plan (icpslam_amd/csrc/icp_voxel_plan.h), shared by
tests/test_voxel_plan_host.py (no GPU) and tests/test_gpu_voxel_edges.py, and an exact restatement of the plan in Python integers
and fractions.  Nothing here calls the library."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32 = np.float32
INT32_MAX = 2**31 - 1
DIRECT, NO_FINITE, PASS_THROUGH, WRAP = 0, 1, 2, 3
FLT_MAX = float(np.finfo(F32).max)


def plan_exact(lo, hi, leaf):
    """(verdict, min_b, div_b): float32 for the six operations PCL does in float -- 1 / leaf, (hi - lo) * inv, lo * inv, hi * inv --
    and exact rational / integer arithmetic for every decision after them.  div_b is reduced modulo 2^32 to a signed int32, as
    PCL's int arithmetic leaves it; both are None unless the cloud is filtered (DIRECT, WRAP)."""
    lo, hi = [F32(v) for v in lo], [F32(v) for v in hi]
    if not all(l <= h for l, h in zip(lo, hi)):
        return NO_FINITE, None, None
    with np.errstate(all="ignore"):
        inv = F32(1.0) / F32(leaf)
        span = [F32(F32(h - l) * inv) for l, h in zip(lo, hi)]
        lo_s, hi_s = [F32(l * inv) for l in lo], [F32(h * inv) for h in hi]
    d, first, last = [], [], []
    for a in range(3):
        if not math.isfinite(span[a]) or Fraction(float(span[a])) >= 2**63:
            return PASS_THROUGH, None, None
        if not (math.isfinite(lo_s[a]) and math.isfinite(hi_s[a])):
            return PASS_THROUGH, None, None
        fl, fh = math.floor(Fraction(float(lo_s[a]))), math.floor(Fraction(float(hi_s[a])))
        if not (-2**31 <= fl <= INT32_MAX and -2**31 <= fh <= INT32_MAX):
            return PASS_THROUGH, None, None
        d.append(math.floor(Fraction(float(span[a]))) + 1)
        first.append(fl)
        last.append(fh)
    if d[0] * d[1] * d[2] > INT32_MAX:
        return PASS_THROUGH, None, None
    div = [b - a + 1 for a, b in zip(first, last)]
    as_i32 = [((v + 2**31) % 2**32) - 2**31 for v in div]
    return (WRAP if div[0] * div[1] * div[2] > INT32_MAX else DIRECT), first, as_i32


def bbox(cloud):
    xyz = np.asarray(cloud, F32)[:, :3]
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    return xyz.min(axis=0), xyz.max(axis=0)


def finding_rows():
    """The seven rows of the finding (profiles/voxel_plan_overflow_finding.txt): ordinary clouds of the suite at leaves whose int64
    product of extents wraps.  (name, cloud, leaf)."""
    from icpslam_amd import synth
    scan = synth.scan(synth.make_scene(3), np.eye(4), 20000, seed=4)
    pair = synth.make_pair(3000, 10, seed=7)[0]
    return ([(f"scan20k@{leaf:g}", scan, leaf) for leaf in (1e-5, 7e-6, 3e-6, 1e-7)] +
            [(f"pair3k@{leaf:g}", pair, leaf) for leaf in (5e-6, 3e-6, 1e-6)])


def _below(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def boundary_boxes():
    """(name, lo, hi, leaf, expected verdict): both sides of every boundary of the rule.  INT32_MAX is prime and 2^31 - 2 is no
    float32, so a product of extents of exactly INT32_MAX cannot occur: the largest products below it that can, and INT32_MAX + 1
    itself, stand on the two sides."""
    B = []

    def box(name, lo, hi, leaf, want):
        B.append((name, tuple(float(F32(v)) for v in lo), tuple(float(F32(v)) for v in hi), float(leaf), want))

    # (a) the exact product: extents (dx, dy, dz) at leaf 1 from a box [0, d - 1]
    def cells(name, d, want, leaf=1.0):
        box(name, (0, 0, 0), tuple((v - 1) * leaf for v in d), leaf, want)
    cells("2^31 cells exactly", (2048, 1024, 1024), PASS_THROUGH)
    cells("2^31 - 2^20 cells", (2047, 1024, 1024), DIRECT)
    cells("46341^2 > INT32_MAX", (46341, 46341, 1), PASS_THROUGH)
    cells("46341 * 46340 fits", (46341, 46340, 1), DIRECT)
    cells("1291^3 > INT32_MAX", (1291, 1291, 1291), PASS_THROUGH)
    cells("1290^3 fits", (1290, 1290, 1290), DIRECT)
    cells("2^21 per axis: the int64 product wraps to 0", (2**21 + 1, 2**21 + 1, 2**22 + 1), PASS_THROUGH)
    cells("2^22 per axis at leaf 0.25", (2**22, 2**22, 2**22), PASS_THROUGH, leaf=0.25)
    cells("odd extents whose int64 product wraps negative", (15321545, 1840620, 441087), PASS_THROUGH)
    # one axis: the largest float below 2^31 (2147483521 cells, more than INT32_MAX), 2^31, around 2^63
    box("one axis, 2^31 - 127 cells", (-2.0**30, 0, 0), (_below(2.0**30), 0, 0), 1.0, PASS_THROUGH)
    box("one axis, INT32_MAX - 127 cells", (-2.0**30, 0, 0), (2.0**30 - 256, 0, 0), 1.0, DIRECT)
    box("one axis, 2^31 + 1 cells", (-2.0**30, 0, 0), (2.0**30, 0, 0), 1.0, PASS_THROUGH)
    box("one axis, 2^63 cells (the cast's edge)", (0, 0, 0), (2.0**53, 0, 0), 2.0**-10, PASS_THROUGH)
    box("one axis, just below 2^63 cells", (0, 0, 0), (_below(2.0**53), 0, 0), 2.0**-10, PASS_THROUGH)
    box("one axis, 2^64 cells", (0, 0, 0), (2.0**54, 0, 0), 2.0**-10, PASS_THROUGH)
    box("three axes of 2^63 cells", (0, 0, 0), (2.0**53,) * 3, 2.0**-10, PASS_THROUGH)
    # (b) hi - lo overflows float although lo * inv and hi * inv are small
    box("hi - lo = inf, finite bounds", (-3e38, 0, 0), (3e38, 1e38, 0), 1e38, PASS_THROUGH)
    box("hi - lo just finite", (-1.7e38, 0, 0), (1.7e38, 1e38, 0), 1e38, DIRECT)
    box("+-FLT_MAX at leaf 1000", (-FLT_MAX,) * 3, (FLT_MAX,) * 3, 1000.0, PASS_THROUGH)
    # (c) the first / last cell at the edge of int32, the box one cell wide
    box("one cell at 2^31", (2.0**31, 0, 0), (2.0**31, 0, 0), 1.0, PASS_THROUGH)
    box("one cell just below 2^31", (_below(2.0**31), 0, 0), (_below(2.0**31), 0, 0), 1.0, DIRECT)
    box("one cell at -2^31", (-2.0**31, 0, 0), (-2.0**31, 0, 0), 1.0, DIRECT)
    box("one cell just below -2^31", (-2.0**31 - 256, 0, 0), (-2.0**31 - 256, 0, 0), 1.0, PASS_THROUGH)
    box("one cell at 1e19, leaf 1e-3", (1e19,) * 3, (1e19,) * 3, 1e-3, PASS_THROUGH)
    box("one cell at -1e30", (-1e30, 5, 5), (-1e30, 5, 5), 0.5, PASS_THROUGH)
    # the leaf: denormal with a finite inverse, and leaves whose inverse is inf (0 * inf = NaN at the origin)
    box("denormal leaf, finite inverse, tiny box", (0, 0, 0), (4e-38, 2e-38, 0), 1e-38, DIRECT)
    box("denormal leaf, finite inverse, ordinary box", (-1, -1, -1), (1, 1, 1), 1e-38, PASS_THROUGH)
    box("1 / leaf = inf, box at the origin", (0, 0, 0), (0, 0, 0), 1e-40, PASS_THROUGH)
    box("1 / leaf = inf, ordinary box", (-1, -2, -3), (1, 2, 3), 2e-39, PASS_THROUGH)
    box("smallest denormal leaf", (0, 0, 0), (1, 0, 0), 1.4e-45, PASS_THROUGH)
    # large coordinates at leaves 1e-3 .. 1e3
    box("1e4 m at leaf 1e-3", (-1e4,) * 3, (1e4,) * 3, 1e-3, PASS_THROUGH)
    box("1e4 m at leaf 1e3", (-1e4,) * 3, (1e4,) * 3, 1e3, DIRECT)
    box("1e10 m at leaf 1e3", (-1e10, 0, 0), (1e10, 5e5, 1e3), 1e3, PASS_THROUGH)
    box("1e10 m, one axis, leaf 1e3", (-1e10, 0, 0), (1e10, 10, 10), 1e3, DIRECT)
    box("1e19 m at leaf 1e3", (-1e19,) * 3, (1e19,) * 3, 1e3, PASS_THROUGH)
    box("1e30 m at leaf 1e-3", (-1e30,) * 3, (1e30,) * 3, 1e-3, PASS_THROUGH)
    box("1e30 m on one axis at leaf 1", (-1e30, 0, 0), (1e30, 1, 1), 1.0, PASS_THROUGH)
    box("no finite point", (1, 1, 1), (0, 2, 2), 0.2, NO_FINITE)
    return B


def random_boxes(n, seed, near_the_edge=False):
    """lo, hi (n, 3) float32 and leaves (n,).  Plain: log-uniform extents 1e-6 .. 1e38 (an axis in five has none), log-uniform
    leaves 1e-7 .. 1e3, the box placed anywhere within a few extents of the origin.  near_the_edge: extents chosen as cell counts
    whose product is within a factor 4 of 2^31, so that both verdicts and the wrapped corner come up."""
    rng = np.random.default_rng(seed)
    leaf = (10.0 ** rng.uniform(-7, 3, n)).astype(F32)
    if near_the_edge:
        split = rng.dirichlet(np.ones(3), n) * (31 + rng.uniform(-2, 2, (n, 1)))
        ext = (2.0 ** split) * leaf[:, None].astype(np.float64)
    else:
        ext = 10.0 ** rng.uniform(-6, 38, (n, 3))
    ext[rng.random((n, 3)) < 0.2] = 0.0
    lo = (rng.uniform(-3, 1, (n, 3)) * ext + rng.normal(0, 1, (n, 3)) * (rng.random((n, 1)) < 0.5)).astype(np.float64)
    with np.errstate(over="ignore"):
        lo32 = np.clip(lo, -FLT_MAX, FLT_MAX).astype(F32)
        hi32 = np.clip(lo32.astype(np.float64) + ext, -FLT_MAX, FLT_MAX).astype(F32)
    return lo32, np.maximum(hi32, lo32), leaf


def cloud_in_box(lo, hi, n_inside, seed, bad=0, pad=1.0):
    """The box's two corners (so that it is the cloud's bounding box), n_inside points inside it and `bad` non-finite points mixed
    in; pad = the fourth component (anything but 1 tells a returned input from a filtered one-point-per-cell cloud)."""
    rng = np.random.default_rng(seed)
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    u = rng.random((n_inside, 3))
    inner = np.clip((lo64 * (1 - u) + hi64 * u).astype(F32), F32(lo), F32(hi))
    xyz = np.vstack([np.asarray([lo, hi], F32), inner])
    order = rng.permutation(len(xyz))
    cloud = np.full((len(xyz), 4), pad, F32)
    cloud[:, :3] = xyz[order]
    if bad:
        rows = np.full((bad, 4), pad, F32)
        rows[:, :3] = rng.normal(0, 1, (bad, 3))
        rows[np.arange(bad), rng.integers(0, 3, bad)] = rng.choice([np.nan, np.inf, -np.inf], bad)
        at = np.sort(rng.integers(0, len(cloud) + 1, bad))
        cloud = np.insert(cloud, at, rows, axis=0)
    return np.ascontiguousarray(cloud, F32)
