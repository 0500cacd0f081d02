"""CPU tests of the symmetric point-to-plane objective and the surface-normal rejector (include/icpgpu.h, "symmetric objective for
ICPGPU_P2PLANE", SURFACE_NORMAL): the NumPy restatement (tests/symmetric_restated.py) against a literal per-pair loop and against
Python integers, its branches on hand-made normals, the host solve against the parent's, a known answer, and the ABI."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import symmetric_restated as S
from icpslam_amd import _lib, synth
from icpslam_amd.registration import solve_point_to_plane, solve_symmetric_point_to_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icpgpu_set_source_normals", "icpgpu_set_p2plane_symmetric", "icpgpu_get_p2plane_symmetric",
               "icpgpu_reduce_symmetric_point_to_plane", "icpgpu_solve_symmetric_point_to_plane")
F = np.float32


# ---- the fma emulation ---------------------------------------------------------------------------------------------------------
def _round_f32(v: Fraction) -> np.float32:
    """v rounded to the nearest float32, ties to even, by integer arithmetic (finite, non-zero results in the normal range)"""
    sign = -1 if v < 0 else 1
    v = abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()       # 2^(e-1) <= v < 2^(e+1)
    if Fraction(2) ** e > v:
        e -= 1                                                       # 2^e <= v < 2^(e+1)
    scaled = v / Fraction(2) ** (e - 23)                             # in [2^23, 2^24)
    q, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and q & 1):
        q += 1
    return F(sign * math.ldexp(q, e - 23))


def _fma_exact(a, b, c):
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return F(0.0) if v == 0 else _round_f32(v)


def test_fma_through_float64_is_the_fma_on_random_values():
    rng = np.random.default_rng(5)
    n = 4000
    a = rng.normal(size=n).astype(F)
    b = rng.normal(size=n).astype(F)
    c = (rng.normal(size=n) * 10.0 ** rng.uniform(-8, 3, n)).astype(F)
    got = S.fma_f32(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fma_at_float32_midpoints_where_float64_rounds_twice():
    """a b = +-(1 - 2^-46) with a = 1 + 2^-23, b = 1 - 2^-23, and c = 2^24 + 2: the true sum lies 2^-46 beside the float32 midpoint
    2^24 + 3 (or 2^24 + 1), float64 rounds it ONTO the midpoint, and a plain cast then goes to the even neighbour whichever side
    the true sum lies on -- the wrong one in all four cases."""
    e = F(2.0 ** -23)
    a = np.array([F(1) + e, -(F(1) + e), F(1) + e, -(F(1) + e)], F)
    b = np.full(4, F(1) - e, F)
    c = np.array([2.0 ** 24 + 2, 2.0 ** 24 + 2, -(2.0 ** 24 + 2), -(2.0 ** 24 + 2)], F)
    got = S.fma_f32(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert list(want) == [2.0 ** 24 + 2, 2.0 ** 24 + 2, -(2.0 ** 24 + 2), -(2.0 ** 24 + 2)]
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    assert (naive != want).all()


# ---- the restatement against a literal loop --------------------------------------------------------------------------------------
def _literal_sums(X, tgt, src_nrm, tgt_nrm, T, idx, d2, max_dist, enforce):
    M = S.xform32(T)
    cols = [[] for _ in range(29)]
    for i in range(len(idx)):
        if idx[i] < 0 or not (float(d2[i]) <= max_dist * max_dist):
            continue
        cols[0].append(1.0)
        cols[1].append(float(d2[i]))
        p, q, a, n2 = X[i], tgt[idx[i]], src_nrm[i], tgt_nrm[idx[i]]
        n1 = [_fma_np(M[r, 2], a[2], _fma_np(M[r, 1], a[1], F(M[r, 0] * a[0]))) for r in range(3)]
        with np.errstate(invalid="ignore", over="ignore"):
            dot = F(F(F(n1[0] * n2[0]) + F(n1[1] * n2[1])) + F(n1[2] * n2[2]))
            flip = enforce and not (dot >= 0)
            n = [F(n1[k] - n2[k]) if flip else F(n1[k] + n2[k]) for k in range(3)]
            if not all(np.isfinite(n)):
                continue
            m = [F(p[k] + q[k]) for k in range(3)]
            c = [F(F(m[1] * n[2]) - F(m[2] * n[1])), F(F(m[2] * n[0]) - F(m[0] * n[2])), F(F(m[0] * n[1]) - F(m[1] * n[0]))]
            d = [F(q[k] - p[k]) for k in range(3)]
            r = F(F(F(d[0] * n[0]) + F(d[1] * n[1])) + F(d[2] * n[2]))
        v = [float(x) for x in c + n]
        k = 2
        for a_ in range(6):
            for b_ in range(a_, 6):
                cols[k].append(v[a_] * v[b_])
                k += 1
        for a_ in range(6):
            cols[23 + a_].append(v[a_] * float(r))
    return np.array([float(len(cols[0]))] + [math.fsum(col) for col in cols[1:]])


def _fma_np(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return S.fma_f32(np.array([a], F), np.array([b], F), np.array([c], F))[0]


def _random_case(seed, n=300):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-20, 20, (n, 4)).astype(F)
    tgt = rng.uniform(-20, 20, (n + 50, 4)).astype(F)
    sn = rng.normal(size=(n, 4)).astype(F)
    tn = rng.normal(size=(n + 50, 4)).astype(F)
    sn[:, :3] /= np.linalg.norm(sn[:, :3], axis=1, keepdims=True)
    tn[:, :3] /= np.linalg.norm(tn[:, :3], axis=1, keepdims=True)
    idx = rng.integers(-1, n + 50, n).astype(np.int32)
    d2 = rng.uniform(0, 1.5, n).astype(F)
    T = synth.pose_matrix(0.3, -0.2, 0.1, 0.02, -0.03, 0.05)
    return X, tgt, sn, tn, T, idx, d2


@pytest.mark.parametrize("enforce", [True, False])
def test_restatement_equals_a_literal_per_pair_loop(enforce):
    X, tgt, sn, tn, T, idx, d2 = _random_case(1)
    tn[::13, 1] = np.nan
    sn[::17, 2] = np.inf
    got = S.sums_from_pairs(X, tgt, sn, tn, T, idx, d2, 1.0, enforce)
    want = _literal_sums(X, tgt, sn, tn, T, idx, d2, 1.0, enforce)
    assert got[0] > 100 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    flips = (S.normal_dot(S.rotate_normals(T, sn[:, :3]), tn[np.maximum(idx, 0), :3]) < 0).sum()
    assert flips > 50                                                  # both branches of `enforce` are taken


def test_enforce_branch_on_hand_made_normals():
    X = np.array([[1, 2, 3, 1]] * 4, F)
    tgt = np.array([[1.5, 2, 3, 1]] * 4, F)
    sn = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [np.nan, 0, 0, 0]], F)
    tn = np.array([[0, 1, 0, 0], [-1, 0.5, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], F)      # dots: exactly 0, -1, 1, NaN
    idx = np.arange(4, dtype=np.int32)
    d2 = np.full(4, 0.25, F)
    n1 = S.rotate_normals(np.eye(4), sn[:, :3])
    v, r, fin = S.pair_terms(X, tgt, n1, tn, True)
    assert np.array_equal(v[0, 3:], [1, 1, 0])                         # dot == 0 keeps n1 + n2
    assert np.array_equal(v[1, 3:], [2, -0.5, 0])                      # dot < 0: n1 - n2
    assert np.array_equal(v[2, 3:], [2, 0, 0])
    assert list(fin) == [True, True, True, False]
    v_off, _, _ = S.pair_terms(X, tgt, n1, tn, False)
    assert np.array_equal(v_off[1, 3:], [0, 0.5, 0])                   # without enforce: always n1 + n2
    s = S.sums_from_pairs(X, tgt, sn, tn, np.eye(4), idx, d2, 1.0, True)
    assert s[0] == 4 and s[1] == 1.0                                   # the NaN pair counts and adds its d2 ...
    s3 = S.sums_from_pairs(X[:3], tgt[:3], sn[:3], tn[:3], np.eye(4), idx[:3], d2[:3], 1.0, True)
    assert np.array_equal(s[2:], s3[2:])                               # ... and nothing else
    # r = (q - p) . n for pair 0: (0.5, 0, 0) . (1, 1, 0)
    assert r[0] == F(0.5)


def test_rejector_rule_on_axis_aligned_normals():
    sn = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [np.nan, 0, 0, 0], [1, 0, 0, 0]], F)
    tn = np.array([[1, 0, 0, 0]] * 5, F)
    tn[4, 0] = np.nan
    idx = np.arange(5, dtype=np.int32)
    alive = np.ones(5, bool)
    kept, st = S.surface_normal(idx, alive, sn, tn, np.eye(4), 0.0)
    assert list(kept) == [True, False, False, False, False]           # dot 0 == threshold 0 is rejected; NaN on either side too
    assert (st["pairs_in"], st["pairs_out"], float(st["cut"])) == (5, 1, 0.0)
    kept, _ = S.surface_normal(idx, alive, sn, tn, np.eye(4), 1.0)
    assert not kept.any()                                              # dot 1 == threshold 1 is rejected (PCL's default keeps nothing exact)
    kept, _ = S.surface_normal(idx, alive, sn, tn, np.eye(4), -1.0)
    assert list(kept) == [True, True, False, False, False]            # dot -1 == threshold -1 is rejected
    kept, _ = S.surface_normal(idx, np.array([1, 0, 1, 1, 1], bool), sn, tn, np.eye(4), -2.0)
    assert list(kept) == [True, False, True, False, False]            # only pairs that entered can stay; NaN never does


def test_rejector_threshold_must_be_finite(built):
    L = _lib.load()
    # (no context is needed to see the refusal order: a null context is refused first -- the chain of a real context is covered on
    # the GPU; here the validity rule through the one entry point that needs no device)
    r = (_lib.Rejector * 1)(_lib.Rejector(_lib.REJECT_SURFACE_NORMAL, 0, 0.5))
    assert L.icpgpu_set_correspondence_rejectors(None, r, 1) == _lib.ERR_INVALID_ARG
    assert _lib.REJECT_SURFACE_NORMAL == 4 and _lib.MAX_REJECTORS == 4 and C.sizeof(_lib.Rejector) == 16


# ---- the host solve --------------------------------------------------------------------------------------------------------------
def _systems():
    rng = np.random.default_rng(23)
    out = []
    for _ in range(300):
        n = int(rng.integers(20, 300))
        nrm = rng.normal(size=(n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        m = rng.uniform(-20, 20, size=(n, 3))
        A = np.hstack([np.cross(m, nrm), nrm])
        r = rng.normal(scale=0.05, size=n)
        out.append(np.concatenate([[n, 1.0], (A.T @ A)[np.triu_indices(6)], A.T @ r]))
    for _ in range(200):
        out.append(rng.normal(size=29) * 10.0 ** rng.uniform(-3, 3, 29))
    return out


def test_solve_is_the_parents_x_composed_as_R_Tr_R(built):
    """x through the parent's host call on identical sums (its Tk carries Rz Ry Rx of x0..x2 term by term and x3..x5), then
    (R Tr) R by two 4x4 products: bit for bit."""
    n = 0
    for s in _systems():
        Tp, got = solve_point_to_plane(s), solve_symmetric_point_to_plane(s)
        assert (Tp is None) == (got is None)
        if Tp is None:
            continue
        want = S.solve(s)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), s
        R = Tp[:3, :3]
        assert np.abs(got[:3, :3] - R @ R).max() <= 1e-12 and np.abs(got[:3, 3] - R @ Tp[:3, 3]).max() <= 1e-12 * max(1.0, np.abs(Tp[:3, 3]).max())
        assert np.array_equal(got[3], [0, 0, 0, 1])
        n += 1
    assert n >= 400


def _construct(x):
    """tests/test_point_to_plane_host.py's NumPy construct (libm sin / cos), rotation only"""
    al, be, ga = x
    ca, sa, cb, sb, cg, sg = np.cos(al), np.sin(al), np.cos(be), np.sin(be), np.cos(ga), np.sin(ga)
    return np.array([[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca, 0.0],
                     [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca, 0.0],
                     [-sb, cb * sa, cb * ca, 0.0],
                     [0.0, 0.0, 0.0, 1.0]])


def test_solve_matches_numpy_on_random_systems(built):
    """against np.linalg.solve and libm's sin / cos: the tolerance of tests/test_point_to_plane_host.py's construct comparison"""
    worst = 0.0
    for s in _systems()[:300]:
        ata = np.zeros((6, 6))
        ata[np.triu_indices(6)] = s[2:23]
        ata = ata + np.triu(ata, 1).T
        x = np.linalg.solve(ata, s[23:29])
        R4 = _construct(x[:3])
        Tr = np.eye(4)
        Tr[:3, 3] = x[3:]
        got = solve_symmetric_point_to_plane(s)
        assert got is not None
        worst = max(worst, float(np.abs(got - R4 @ Tr @ R4).max()))
    assert worst <= 1e-12, worst


def test_singular_systems_give_identity(built):
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    rng = np.random.default_rng(3)
    # one plane z = 0 with both normals +z: c, nx, ny carry no information
    p = np.column_stack([rng.uniform(-5, 5, 300), rng.uniform(-5, 5, 300), np.zeros(300), np.ones(300)]).astype(F)
    nrm = np.tile(np.array([0, 0, 1, 0], F), (300, 1))
    plane = S.sums_from_pairs(p, p, nrm, nrm, np.eye(4), np.arange(300), np.zeros(300, F), 1.0, True)
    assert plane[0] == 300
    for s in (np.zeros(29), plane):
        Tk = np.full(16, 7.0)
        rc = L.icpgpu_solve_symmetric_point_to_plane(np.ascontiguousarray(s).ctypes.data_as(dp), Tk.ctypes.data_as(dp))
        assert rc == _lib.ERR_INVALID_ARG and np.array_equal(Tk.reshape(4, 4), np.eye(4))
        assert solve_symmetric_point_to_plane(s) is None and S.solve(s) is None
    assert L.icpgpu_solve_symmetric_point_to_plane(None, None) == _lib.ERR_INVALID_ARG


# ---- known answer ----------------------------------------------------------------------------------------------------------------
def curved_surface(n, seed):
    """points and unit normals of z = 0.3 sin(0.7 x) + 0.2 cos(0.5 y) + 0.05 x y over [-4, 4]^2"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-4, 4, n), rng.uniform(-4, 4, n)
    z = 0.3 * np.sin(0.7 * x) + 0.2 * np.cos(0.5 * y) + 0.05 * x * y
    nrm = np.column_stack([-(0.21 * np.cos(0.7 * x) + 0.05 * y), -(-0.1 * np.sin(0.5 * y) + 0.05 * x), np.ones(n)])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.column_stack([x, y, z]), nrm


def _solve_f64(p, q, n1, n2, enforce):
    """one symmetric step in float64 terms (the contract's formulas without the float32 roundings): Tk"""
    dot = (n1 * n2).sum(axis=1)
    n = np.where((enforce & ~(dot >= 0))[:, None], n1 - n2, n1 + n2)
    A = np.hstack([np.cross(p + q, n), n])
    r = ((q - p) * n).sum(axis=1)
    sums = np.concatenate([[len(p), 0.0], (A.T @ A)[np.triu_indices(6)], A.T @ r])
    return solve_symmetric_point_to_plane(sums)


@pytest.mark.parametrize("flip_target_normals", [False, True])
def test_known_answer_on_a_curved_surface(built, flip_target_normals):
    """Exact correspondences, a motion of 3 degrees and 0.37 m: the loop recovers it to 1e-6 / 1e-6 m within 5 iterations -- with
    flipped target normals too, under enforce_same_direction (the signs of the contract)."""
    q, nq = curved_surface(800, 4)
    M = synth.pose_matrix(0.3, -0.2, 0.08, np.deg2rad(1.5), np.deg2rad(-2.0), np.deg2rad(1.7))     # source -> target
    Minv = np.linalg.inv(M)
    p0 = q @ Minv[:3, :3].T + Minv[:3, 3]
    n0 = nq @ Minv[:3, :3].T
    n2 = np.where((np.arange(len(q)) % 2 == 0)[:, None] & flip_target_normals, -nq, nq)
    T = np.eye(4)
    for _ in range(5):
        p = p0 @ T[:3, :3].T + T[:3, 3]
        Tk = _solve_f64(p, q, n0 @ T[:3, :3].T, n2, True)
        assert Tk is not None
        T = Tk @ T
    assert np.abs(T[:3, :3] - M[:3, :3]).max() <= 1e-6 and np.linalg.norm(T[:3, 3] - M[:3, 3]) <= 1e-6


def test_restated_loop_recovers_the_motion_in_float32(built):
    """the float32 restatement on the same surface with fixed pairs: to float32's resolution of 4 m coordinates"""
    q, nq = curved_surface(800, 4)
    M = synth.pose_matrix(0.3, -0.2, 0.08, np.deg2rad(1.5), np.deg2rad(-2.0), np.deg2rad(1.7))
    Minv = np.linalg.inv(M)
    pad = lambda a: np.hstack([a, np.ones((len(a), 1))]).astype(F)   # noqa: E731
    src, tgt = pad(q @ Minv[:3, :3].T + Minv[:3, 3]), pad(q)
    sn, tn = pad(nq @ Minv[:3, :3].T), pad(nq)
    res = S.align(src, tgt, sn, tn, pairs=np.arange(800), max_iterations=5, transformation_epsilon=0.0,
                  max_correspondence_distance=10.0)
    assert 3 <= res["iterations"] <= 5       # (the mean squared distance reaches float32's floor: the absolute-mse test may end it)
    assert np.abs(res["T64"][:3, :3] - M[:3, :3]).max() <= 2e-6 and np.linalg.norm(res["T64"][:3, 3] - M[:3, 3]) <= 1e-5


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_version_sizes_and_new_symbols(built):
    lib = _lib.load()
    assert lib.icpgpu_version() == 1002 == _lib.HEADER_VERSION
    sizes = (C.c_size_t * 3)()
    lib.icpgpu_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(_lib.Params), C.sizeof(_lib.Result), C.sizeof(_lib.Profile)] == [56, 120, 384]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in _lib.EXPORTS


def test_null_context_refusals(built):
    L = _lib.load()
    one = (C.c_float * 4)(0, 0, 1, 0)
    on, enforce = C.c_int(5), C.c_int(5)
    sums = (C.c_double * 29)()
    T = (C.c_float * 16)()
    assert L.icpgpu_set_source_normals(None, one, 1) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_set_p2plane_symmetric(None, 1, 1) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_get_p2plane_symmetric(None, C.byref(on), C.byref(enforce)) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_reduce_symmetric_point_to_plane(None, T, 1.0, 1, sums) == _lib.ERR_INVALID_ARG
    assert (on.value, enforce.value) == (5, 5)


def test_header_compiles_as_c99_with_the_new_names(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){ icpgpu_rejector r = {ICPGPU_REJECT_SURFACE_NORMAL, 0, 0.5}; double s[29] = {0}, T[16];\n'
                   '  int a = icpgpu_set_source_normals(0, 0, 0), b = icpgpu_set_p2plane_symmetric(0, 1, 1);\n'
                   '  printf("%d %d %d %d %d %d %d\\n", (int)r.kind, ICPGPU_MAX_REJECTORS, (int)sizeof(icpgpu_rejector), ICPGPU_HEADER_VERSION,\n'
                   '         icpgpu_solve_symmetric_point_to_plane(s, T), a, b); return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [4, 4, 16, 1002, _lib.ERR_INVALID_ARG, _lib.ERR_INVALID_ARG, _lib.ERR_INVALID_ARG]


def build_demo(tmp_path):
    exe = tmp_path / "symmetric_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "symmetric_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_symmetric_shim_compiles_and_fails_loudly_without_gpu(built, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_cpp_symmetric.py")
    exe = build_demo(tmp_path)
    src, tgt, _ = synth.make_pair(100, 100, seed=1)
    a, b = tmp_path / "src.bin", tmp_path / "tgt.bin"
    src.tofile(a)
    tgt.tofile(b)
    r = subprocess.run([str(exe), str(a), "100", str(b), "100", "10", "12", "0.5"], capture_output=True, text=True)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr


def test_python_mirrors_carry_the_new_names():
    import icpslam_amd as pkg
    icp = pkg.IterativeClosestPointWithNormals.__dict__
    for name in ("setUseSymmetricObjective", "getUseSymmetricObjective", "setEnforceSameDirectionNormals", "getEnforceSameDirectionNormals"):
        assert name in icp
    for name in ("setSourceNormals", "setTargetNormals"):
        assert name in pkg.IterativeClosestPoint.__dict__
    r = pkg.CorrespondenceRejectorSurfaceNormal()
    assert r.getThreshold() == 1.0
    r.setThreshold(0.25)
    e = r._entry()
    assert (e.kind, e.value) == (pkg.REJECT_SURFACE_NORMAL, 0.25)
    for name in ("set_source_normals", "set_p2plane_symmetric", "get_p2plane_symmetric", "reduce_symmetric_point_to_plane",
                 "solve_symmetric_point_to_plane"):
        assert hasattr(pkg.Context, name)
