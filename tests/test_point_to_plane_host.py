"""CPU tests of the point-to-plane mode's boundary (ICPGPU_P2PLANE, C-ABI 1.2): the header, the exports, the shim, and the host
solve -- (AᵀA)⁻¹Aᵀr by partial-pivot LU, then PCL's constructTransformationMatrix -- against a NumPy restatement and, bit for bit,
against the oracle's (oracle/p2plane_oracle.c)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from icpslam_amd import _lib, synth
from icpslam_amd.registration import solve_point_to_plane
import oracle  # (test infrastructure: the C restatement)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icpgpu_set_target_normals", "icpgpu_normals", "icpgpu_reduce_point_to_plane", "icpgpu_solve_point_to_plane")


def test_header_compiles_as_c_with_the_method(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "icpgpu.h"\n#include <stdio.h>\n'
                   'int main(void){ icpgpu_method m = ICPGPU_P2PLANE; double s[29] = {0}, T[16];\n'
                   '  printf("%d %d %d\\n", (int)m, ICPGPU_HEADER_VERSION, icpgpu_solve_point_to_plane(s, T)); return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-licpgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    m, version, rc = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert m == 2 and version == 1002
    assert rc == _lib.ERR_INVALID_ARG          # an all-zero system is singular


def test_version_and_new_symbols(built):
    lib = _lib.load()
    assert lib.icpgpu_version() == 1002 == _lib.HEADER_VERSION
    assert _lib.P2PLANE == 2
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in _lib.EXPORTS


def _construct(x):
    """PCL 1.8 TransformationEstimationPointToPlaneLLS::constructTransformationMatrix, float64."""
    al, be, ga, tx, ty, tz = x
    ca, sa, cb, sb, cg, sg = np.cos(al), np.sin(al), np.cos(be), np.sin(be), np.cos(ga), np.sin(ga)
    return np.array([[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca, tx],
                     [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca, ty],
                     [-sb, cb * sa, cb * ca, tz],
                     [0.0, 0.0, 0.0, 1.0]])


def _sums_from(A, r, d2):
    """The 29 sums of icpgpu_reduce_point_to_plane from rows A = (a, b, c, nx, ny, nz) and residuals r."""
    ata, atr = A.T @ A, A.T @ r
    iu = np.triu_indices(6)
    return np.concatenate([[A.shape[0], d2.sum()], ata[iu], atr])


def test_solve_matches_numpy_on_random_systems(built):
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(200):
        n = int(rng.integers(20, 400))
        nrm = rng.normal(size=(n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        s = rng.uniform(-20, 20, size=(n, 3))
        abc = np.cross(s, nrm)
        A = np.hstack([abc, nrm])
        r = rng.normal(scale=0.05, size=n)
        sums = _sums_from(A, r, rng.uniform(0, 1, n))
        ata = np.zeros((6, 6))
        ata[np.triu_indices(6)] = sums[2:23]
        ata = ata + np.triu(ata, 1).T
        x = np.linalg.solve(ata, sums[23:29])
        Tk = solve_point_to_plane(sums)
        assert Tk is not None
        worst = max(worst, float(np.abs(Tk - _construct(x)).max()))
    assert worst <= 1e-12, worst


def test_solve_refuses_a_single_plane(built):
    """One plane (z = 0, normals +z) leaves c, nx, ny without information: a zero pivot -> non-zero status, Tk = identity."""
    rng = np.random.default_rng(3)
    s = np.column_stack([rng.uniform(-5, 5, 300), rng.uniform(-5, 5, 300), np.zeros(300)]).astype(np.float32)
    n = np.tile(np.array([0, 0, 1], np.float32), (300, 1))
    f = np.float32
    a = (n[:, 2] * s[:, 1] - n[:, 1] * s[:, 2]).astype(f)
    b = (n[:, 0] * s[:, 2] - n[:, 2] * s[:, 0]).astype(f)
    c = (n[:, 1] * s[:, 0] - n[:, 0] * s[:, 1]).astype(f)
    A = np.column_stack([a, b, c, n]).astype(np.float64)
    sums = _sums_from(A, rng.normal(scale=0.01, size=300), np.zeros(300))
    L = _lib.load()
    Tk = np.full(16, 7.0)
    dp = C.POINTER(C.c_double)
    rc = L.icpgpu_solve_point_to_plane(np.ascontiguousarray(sums).ctypes.data_as(dp), Tk.ctypes.data_as(dp))
    assert rc == _lib.ERR_INVALID_ARG
    assert np.array_equal(Tk.reshape(4, 4), np.eye(4))
    assert solve_point_to_plane(sums) is None


def test_public_structs_unchanged(built):
    """The structs did not change: the ctypes mirrors still match the library's sizes (a 1.1 caller keeps working)."""
    sizes = (C.c_size_t * 3)()
    _lib.load().icpgpu_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(_lib.Params), C.sizeof(_lib.Result), C.sizeof(_lib.Profile)] == [56, 120, 384]


def test_p2plane_shim_compiles_and_fails_loudly_without_gpu(built, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_point_to_plane.py")
    exe = tmp_path / "p2plane_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "p2plane_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    src, tgt, _ = synth.make_pair(100, 100, seed=1)
    a, b = tmp_path / "src.bin", tmp_path / "tgt.bin"
    src.tofile(a)
    tgt.tofile(b)
    r = subprocess.run([str(exe), str(a), "100", str(b), "100", "10"], capture_output=True, text=True)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr


# ---- the host solve against the oracle's, bit for bit (PartialPivLU, first of equal pivots, x = inv b in
# increasing j, constructTransformationMatrix with correctly rounded sin / cos) --------------------------------------------------
def _sums_of(M, b):
    M = np.asarray(M, np.float64)
    return np.concatenate([[100.0, 1.0], M[np.triu_indices(6)], b])


def _pinned_systems():
    rng = np.random.default_rng(11)
    out = []
    for _ in range(3000):                                               # random, any scale
        out.append(rng.normal(size=29) * 10.0 ** rng.uniform(-4, 4, 29))
    for _ in range(1500):                                               # small integers: equal pivot candidates at every step
        M = rng.integers(-3, 4, size=(6, 6)).astype(np.float64)
        out.append(_sums_of(M + M.T, rng.integers(-5, 6, 6)))
    for _ in range(500):                                                # the largest entry of each column below the diagonal
        M = rng.uniform(-1, 1, (6, 6))
        M = M + M.T
        M[np.arange(6), np.arange(6)[::-1]] = M[np.arange(6)[::-1], np.arange(6)] = 10.0 + rng.uniform(0, 1, 6)
        out.append(_sums_of(M, rng.normal(size=6)))
    for k in range(500):                                                # near-singular: rank 5 plus a perturbation of 1e-(8..15)
        V = rng.normal(size=(5, 6))
        M = V.T @ V + 10.0 ** -(8 + k % 8) * np.diag(rng.uniform(0.5, 1, 6))
        out.append(_sums_of(M, rng.normal(size=6) * 1e-3))
    for k in range(200):                                                # singular: one unknown without information
        M = rng.normal(size=(6, 6))
        M = M @ M.T
        M[k % 6, :] = M[:, k % 6] = 0.0
        out.append(_sums_of(M, rng.normal(size=6)))
    for seed in range(6):                                               # the per-iteration sums of real alignments
        src, tgt, _ = synth.make_pair(4000, 4000, seed=60 + seed)
        out += [t["sums"] for t in oracle.p2plane_align(src, tgt)["trace"]]
    return [s for s in out if oracle.p2plane_solve(s) is None or _angles_below_2e19(s)]


def _angles_below_2e19(s):
    """beyond |x| > 2^19 rad DESIGN.md section 3 leaves sin / cos to the platform (never a rotation angle): such systems are
    left out (a margin: the angles estimated by least squares stay below 4e5 rad)"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[2:23]
    x = np.linalg.lstsq(A + np.triu(A, 1).T, s[23:29], rcond=None)[0]
    return bool(np.abs(x[:3]).max() < 4e5)


def _lu_pivots(sums):
    """(row swaps, steps with an exact tie for the pivot) of the partial-pivot LU restated here (counts only: coverage)."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[2:23]
    A = A + np.triu(A, 1).T
    swaps = ties = 0
    for k in range(6):
        col = np.abs(A[k:, k])
        if not col.max() > 0:
            break
        p = k + int(np.argmax(col))
        ties += int((col == col.max()).sum() > 1)
        swaps += p != k
        A[[k, p]] = A[[p, k]]
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return swaps, ties


def test_solve_equals_the_oracle_bit_for_bit(built):
    systems = _pinned_systems()
    solved = singular = all_swaps = tied = 0
    for s in systems:
        ref = oracle.p2plane_solve(s)
        got = solve_point_to_plane(s)
        assert (ref is None) == (got is None), s
        if ref is None:
            singular += 1
            continue
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), s
        solved += 1
        swaps, ties = _lu_pivots(s)
        all_swaps += swaps >= 5
        tied += ties > 0
    assert solved > 5000 and singular >= 200 and all_swaps >= 200 and tied >= 500, (solved, singular, all_swaps, tied)


def test_single_plane_is_singular_on_both_sides(built):
    rng = np.random.default_rng(3)
    s = np.column_stack([rng.uniform(-5, 5, 300), rng.uniform(-5, 5, 300), np.zeros(300), np.ones(300)]).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1, 0], np.float32), (300, 1))
    sums = oracle.p2plane_sums(s, s, nrm, np.eye(4), np.arange(300), np.zeros(300, np.float32), 1.0)
    assert sums[0] == 300
    assert oracle.p2plane_solve(sums) is None and solve_point_to_plane(sums) is None
