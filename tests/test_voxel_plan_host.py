"""The voxel filter's plan without a GPU: icpgpu_voxel_plan is the ONE function (icpslam_amd/csrc/icp_voxel_plan.h) the host
and voxel_plan_kernel both call -- verdict, min_b, div_b from a bounding box and a leaf.  Against an exact Python-integer
restatement (tests/voxel_edge_cases.py) on the rows of the finding (ordinary clouds of this suite whose int64 product of extents
wraps, so that PCL's literal test misses them), on both sides of every boundary of the rule, and on random boxes; and the two
oracles (C, NumPy: each written for itself) against each other and against the verdict on the same table."""
import ctypes as C

import numpy as np
import pytest

import oracle
from oracle import icp_oracle_np as onp
from icpslam_amd import _lib

import voxel_edge_cases as vx

F32 = np.float32


def lib_plan(lo, hi, leaf):
    L = _lib.load()
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    verdict, minb, divb = C.c_int32(-1), (C.c_int32 * 3)(), (C.c_int32 * 3)()
    fp = C.POINTER(C.c_float)
    rc = L.icpgpu_voxel_plan(lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), C.c_float(leaf), C.byref(verdict), minb, divb)
    assert rc == 0
    return verdict.value, list(minb), list(divb)


def check(lo, hi, leaf, what):
    got, ref = lib_plan(lo, hi, leaf), vx.plan_exact(lo, hi, leaf)
    assert got[0] == ref[0], (what, got, ref)
    if ref[0] in (vx.DIRECT, vx.WRAP):
        assert list(got[1:]) == list(ref[1:]), (what, got, ref)
    return got[0]


def test_the_findings_rows_are_pass_through(built):
    """Each of these seven has a true product of extents far above INT32_MAX and an int64 product that wraps below it (negative,
    or small): the parent's three copies of PCL's line all skipped the pass-through and planned the direct path with a negative
    number of cells."""
    for name, cloud, leaf in vx.finding_rows():
        lo, hi = vx.bbox(cloud)
        inv = F32(1.0) / F32(leaf)
        d = [int(F32(F32(h - l) * inv)) + 1 for l, h in zip(lo, hi)]
        true = d[0] * d[1] * d[2]
        wrapped = (true + 2**63) % 2**64 - 2**63
        assert true > vx.INT32_MAX and wrapped <= vx.INT32_MAX, name          # PCL's literal test: not taken
        assert check(lo, hi, leaf, name) == vx.PASS_THROUGH, name
        assert onp.voxel_plan_np(lo, hi, leaf)[0] == onp.VOXEL_PASS_THROUGH, name
        out = oracle.voxel_grid(cloud, leaf)
        assert out.shape == cloud.shape and np.array_equal(out.view(np.uint32), cloud.view(np.uint32)), name


def test_both_sides_of_every_boundary(built):
    seen = set()
    for name, lo, hi, leaf, want in vx.boundary_boxes():
        assert vx.plan_exact(lo, hi, leaf)[0] == want, name                   # the table says what it means to say
        assert check(lo, hi, leaf, name) == want, name
        seen.add(want)
    assert seen == {vx.DIRECT, vx.NO_FINITE, vx.PASS_THROUGH}


def test_the_wrapped_index_stays_the_sort_paths(built):
    """PCL's defined corner (tests/test_gpu_voxel.py: test_voxel_index_wraps_like_pcl): float extents that pass the test, integer
    extents one cell wider whose product exceeds int32 -- filtered, never passed through."""
    rng = np.random.default_rng(9000 + 2864)
    n = int(rng.integers(1, 120000))
    leaf = float(rng.choice([0.03, 0.1, 0.2, 0.35, 0.77, 2.0, 5.0]))
    c = np.ones((n, 4), F32)
    c[:, :3] = rng.normal(0, float(rng.choice([2.0, 30.0, 300.0])), (n, 3)).astype(F32)
    lo, hi = vx.bbox(c)
    assert check(lo, hi, leaf, "seed 2864") == vx.WRAP


@pytest.mark.parametrize("near_the_edge", [False, True])
def test_random_boxes(built, near_the_edge):
    lo, hi, leaf = vx.random_boxes(4000, 11 + near_the_edge, near_the_edge)
    counts = {}
    for k in range(len(leaf)):
        v = check(lo[k], hi[k], float(leaf[k]), k)                            # zero mismatches: every box asserts
        counts[v] = counts.get(v, 0) + 1
        ref = onp.voxel_plan_np(lo[k], hi[k], float(leaf[k]))[0]
        assert (ref == onp.VOXEL_PASS_THROUGH) == (v == vx.PASS_THROUGH), k
    assert counts.get(vx.PASS_THROUGH, 0) > 200 and counts.get(vx.DIRECT, 0) > 200, counts
    if near_the_edge:
        assert counts.get(vx.WRAP, 0) > 0, counts


def test_hook_refuses_what_the_filter_refuses(built):
    L = _lib.load()
    z = (C.c_float * 3)()
    v, i3 = C.c_int32(), (C.c_int32 * 3)()
    for leaf in (0.0, -1.0, float("inf"), float("nan")):
        assert L.icpgpu_voxel_plan(z, z, C.c_float(leaf), C.byref(v), i3, i3) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_voxel_plan(None, z, C.c_float(1.0), C.byref(v), i3, i3) == _lib.ERR_INVALID_ARG


def test_oracle_c_equals_oracle_numpy_on_the_table(built):
    """Through oracle.voxel_grid with 2- to 8-point clouds that span each box (pad 7: a returned input is told from a filtered
    cloud of one point per cell), non-finite points mixed into every third: same bits from both oracles, and a returned input
    exactly where the library's plan says pass-through."""
    rows = [(name, lo, hi, leaf) for name, lo, hi, leaf, want in vx.boundary_boxes() if want != vx.NO_FINITE]
    rows += [(name,) + tuple(vx.bbox(cloud)) + (leaf,) for name, cloud, leaf in vx.finding_rows()]
    lo, hi, leaf = vx.random_boxes(300, 5, True)
    rows += [(f"random {k}", lo[k], hi[k], float(leaf[k])) for k in range(len(leaf))]
    passed = 0
    for k, (name, lo, hi, leaf) in enumerate(rows):
        cloud = vx.cloud_in_box(lo, hi, k % 7, seed=k, bad=2 if k % 3 == 0 else 0, pad=7.0)
        a, b = oracle.voxel_grid(cloud, leaf), onp.voxel_grid_np(cloud, leaf)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        verdict = lib_plan(lo, hi, leaf)[0]
        returned = a.shape == cloud.shape and np.array_equal(a.view(np.uint32), cloud.view(np.uint32))
        assert returned == (verdict == vx.PASS_THROUGH), name
        if not returned:
            assert (a[:, 3] == 1.0).all() and 0 < len(a) <= np.isfinite(cloud[:, :3]).all(axis=1).sum(), name
        passed += returned
    assert 20 < passed < len(rows) - 20
