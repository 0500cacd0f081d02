"""Inputs of the point-to-point solve at its edges, shared by tests/test_solve_host.py and tests/test_gpu_solve_edges.py.  Data and builders
only.  A case is (name, p, q): float64 arrays (n, 3) of float32-representable coordinates -- the same case can be a cloud on the device --
paired row by row, q ~ R p + t.  The name's part before ':' is the case's family.  sums_of() is the 17-term record, by math.fsum."""
import functools
import math

import numpy as np

F32 = np.float32


def f32(a) -> np.ndarray:
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


def sums_of(p, q) -> np.ndarray:
    """{n, sum p, sum q, sum q p^T (row = q), sum |q - p|^2}: every product of two float32 values is exact in double, fsum rounds once."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    s = np.zeros(17)
    s[0] = len(p)
    for a in range(3):
        s[1 + a] = math.fsum(p[:, a])
        s[4 + a] = math.fsum(q[:, a])
        for b in range(3):
            s[7 + 3 * a + b] = math.fsum(q[:, a] * p[:, b])
    s[16] = math.fsum(((q - p) ** 2).sum(axis=1))
    return s


def rotation(axis, angle) -> np.ndarray:
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def moved(p, R, t=(0, 0, 0), centre=(0, 0, 0)) -> np.ndarray:
    c = np.asarray(centre, np.float64)
    return f32((np.asarray(p) - c) @ np.asarray(R).T + c + np.asarray(t, np.float64))


# The small motion of the cases that also run as one-iteration alignments: 0.23 degrees and 2 cm, at least 20 times below their spacing.
SMALL_R = rotation((0.3, -0.5, 0.8), 0.004)
SMALL_T = (0.012, -0.009, 0.015)
QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])   # exact in any format
MIRROR = np.diag([1.0, 1.0, -1.0])

# ---- the cases that are also clouds of a one-iteration alignment on the device: the pairing is the identity by construction -----------------
GPU_CASES = ("three:spread", "planar:four", "planar:patch64", "slab:1e-06", "slab:0", "tie:cube", "tie:prism", "mirror:planar", "offset:3000")
GPU_GUESS_CASES = ("planar:patch64", "tie:cube")


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, p, q):
        p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
        assert p.shape == q.shape and (f32(p) == p).all() and (f32(q) == q).all(), name
        p.setflags(write=False)
        q.setflags(write=False)
        out.append((name, p, q))

    # three points: the rank-2 branch every SCP / RSAC hypothesis takes
    tri = f32([[0.0, 0.0, 0.0], [2.0, 0.25, 0.5], [0.5, 1.75, -0.25]])
    add("three:spread", tri, moved(tri, SMALL_R, SMALL_T))
    for h in (1e-2, 1e-4, 1e-6, 1e-8, 1e-12):                                     # height / base; the image is another skinny triangle, turned
        p = f32([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.375, h, 0.0]])
        p2 = f32([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.375, 1.5 * h, 0.0]])
        add(f"three:skinny{h:g}", p, f32(p2 @ QUARTER.T + (0.5, -0.25, 2.0)))
    line = f32(np.outer([0.0, 1.0, 3.0], [1.0, 2.0, -0.5]))
    add("three:collinear", line, f32(np.outer([0.0, 1.0, 3.0], [-2.0, 1.0, 0.5]) + (1.0, 1.0, 1.0)))
    add("three:coincident", f32([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [2.0, 0.0, 1.0]]), f32([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [2.0, 2.0, 1.0]]))

    # planar inputs: Sigma has rank 2 exactly (p_z is an exact combination of p_x and p_y)
    four = f32([[0.0, 0.0, 0.0], [2.0, 0.0, 1.0], [0.0, 3.0, 0.75], [2.0, 2.0, 1.5]])              # z = x / 2 + y / 4
    add("planar:four", four, moved(four, SMALL_R, SMALL_T))
    g = np.array([[a, b] for a in range(8) for b in range(8)], np.float64)
    patch = f32(np.column_stack([g[:, 0], g[:, 1], 0.5 * g[:, 0] + 0.25 * g[:, 1]]))
    add("planar:patch64", patch, moved(patch, SMALL_R, SMALL_T, centre=(3.5, 3.5, 2.6)))
    flat = np.column_stack([np.repeat(np.arange(6.0), 6), np.tile(np.arange(6.0), 6), rng.uniform(-1, 1, 36)])
    for eps in (1e-3, 1e-6, 1e-9, 1e-12, 1e-13, 1e-14, 0.0):                       # a slab: both clouds thin, s2 / s0 ~ eps^2
        p = f32(flat * (1.0, 1.0, 5.0 * eps))
        add(f"slab:{eps:g}", p, moved(p, SMALL_R, SMALL_T, centre=(2.5, 2.5, 0.0)))
    for eps in (1e-12, 1e-13, 1e-14):                                              # thin p, thick q: s2 / s0 ~ eps, either side of the 1e-13 rank cut
        p = f32(flat * (1.0, 1.0, 5.0 * eps))
        add(f"slabcut:{eps:g}", p, moved(flat * (1.0, 1.0, 5.0), rotation((1, 2, -1), 0.7), (0.5, 0.1, -0.2)))

    # the reflection branch
    cloud = rng.normal(size=(32, 3)) * (3.0, 2.0, 1.0)
    add("mirror:full", f32(cloud), f32(cloud @ (rotation((2, 1, 1), 0.4) @ MIRROR).T + rng.normal(size=(32, 3)) * 0.01 * (3.0, 2.0, 1.0)))
    x = rng.uniform(-0.015, 0.015, 16)
    ribbon = f32(np.column_stack([x, np.arange(16.0), x]))                         # in the plane z = x; mirrored about its centre line
    add("mirror:planar", ribbon, f32(ribbon * (-1.0, 1.0, -1.0)))

    # tied singular values
    cube = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    add("tie:cube", cube, moved(cube, SMALL_R, SMALL_T))
    add("tie:cube_exact", cube, cube @ QUARTER.T)
    add("tie:prism", cube * (1.0, 1.0, 2.0), moved(cube * (1.0, 1.0, 2.0), SMALL_R, SMALL_T))

    # a half turn, and none
    cloud = f32(rng.normal(size=(32, 3)) * (3.0, 2.0, 1.0))
    add("turn:pi_random_axis", cloud, moved(cloud, rotation(rng.normal(size=3), math.pi)))
    add("turn:pi_exact", cloud, cloud * (1.0, -1.0, -1.0))
    add("turn:identity", cloud, cloud)

    # unrelated clouds: Sigma is what is left of mag = |M / n| + |mu mu^T| ~ 100
    add("unrelated:64", f32(rng.normal(size=(64, 3)) + (10.0, -8.0, 6.0)), f32(rng.normal(size=(64, 3)) + (-9.0, 10.0, 7.0)))

    # far from the origin: Sigma ~ 1 is the difference of two numbers ~ offset^2
    local = np.array([[x, y, z] for x in (0.0, 2.0) for y in (0.0, 2.0) for z in (0.0, 2.0)]) + rng.uniform(-0.25, 0.25, (8, 3))
    for off in (1e3, 3e3, 1e5, 1e6):
        c = np.array([off, -0.5 * off, 0.25 * off])
        p = f32(local + c)
        add(f"offset:{off:g}", p, moved(p, SMALL_R, SMALL_T, centre=c + 1.0))

    # one scene at other scales
    scene = rng.normal(size=(32, 3)) * (30.0, 20.0, 1.5) + (5.0, -3.0, 0.2)
    image = scene @ rotation((0.1, 0.2, 1.0), 0.3).T + (0.4, -0.2, 0.05) + rng.normal(size=(32, 3)) * 0.02
    for k in (1e-6, 1e-3, 1e3, 1e6):
        add(f"scaled:{k:g}", f32(scene * k), f32(image * k))

    # one and two pairs
    add("small:n1", f32([[1.5, -2.0, 0.25]]), f32([[0.5, 3.0, -1.0]]))
    add("small:n2", f32([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]]), f32([[1.0, 1.0, 1.0], [3.0, 2.0, -1.0]]))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c[0] == name)


def families():
    return sorted({name.split(":")[0] for name, _, _ in cases()})


def rejected():
    """(name, sums) the solve must refuse: rc != 0 and the identity."""
    good = sums_of(*case("three:spread")[1:])
    out = [("n0", np.zeros(17))]
    for what, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        for k, where in ((2, "p"), (5, "q"), (11, "M")):
            s = good.copy()
            s[k] = v
            out.append((f"{what}_{where}", s))
    s = good.copy()
    s[0] = np.nan
    out.append(("nan_n", s))
    return out


# ---- matrices for svd3x3 itself ---------------------------------------------------------------------------------------------------------
HAND = {
    "zeros": np.zeros((3, 3)),
    "rank1": np.outer([1.0, -2.0, 0.5], [0.25, 1.0, -1.0]),
    "diag_3_1e-9_0": np.diag([3.0, 1e-9, 0.0]),
    "identity": np.eye(3),
    "minus_identity": -np.eye(3),
    "permutation": np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
    "dense": np.array([[4.0, -2.0, 1.0], [1.0, 3.0, -1.0], [0.5, 2.0, 5.0]]),                   # full rank: every sweep rotates
}
SCALES = tuple(range(-1000, -500, 100)) + tuple(range(-500, 501, 50)) + tuple(range(600, 1001, 100))   # (squares leave the format beyond 2^+-511)


def hand_matrices():
    """(name, A): every hand matrix at every power-of-two scale 2^k, k = -500 .. 500 in steps of 50 and on to +-1000 in steps of 100."""
    return [(f"{name}@2^{k}", np.ldexp(A, k)) for name, A in HAND.items() for k in SCALES]
