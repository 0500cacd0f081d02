"""What answers from the search cloud's rows, at the size DESIGN.md quotes its timings for: the bench scan voxel-filtered at 0.2 m
(some 17 500 points, five tiles of the row scans, thousands of rows on the ranked scratch path at 1 m), every point its own query,
with the parameters those timings use.  Each feature against its restatement bit for bit, by its own test file's check; the
restatements take their rows from tests/search_restated.py, which answers clouds of this size through its tree-narrowed form.  Every
test here is the first of its feature above 3 000 points: row_start offsets beyond the first scan tile, compaction over more than one
tile, per-point kernels with thousands of workgroups."""
import math

import numpy as np
import pytest

import normals_restated as N
import test_gpu_boundary as BD
import test_gpu_cluster as CL
import test_gpu_fpfh as FP
import test_gpu_iss as IS
import test_gpu_iss_border as IB
import test_gpu_mls as ML
import test_gpu_normal_estimation as NE
from test_gpu_search_scale import few_rows_swept, filtered

pytestmark = pytest.mark.gpu

_NORMALS = []


def normals10(F):
    """The restatement's k = 10 normals of F (what FPFH and the boundary rule are timed on)."""
    if not _NORMALS:
        nrm = N.estimate(F, None, k=10)[0]
        nrm.setflags(write=False)
        _NORMALS.append(nrm)
    return _NORMALS[0]


@pytest.mark.parametrize("mode", [{"k": 20}, {"radius": 0.5}], ids=["k20", "r0.5"])
def test_normals(ctx, mode):
    """normals_from_rows_kernel over dense rows (k = 20) and over CSR rows whose row_start comes from five scan tiles (0.5 m)."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        normals, counts, moments = NE.check(ctx, "F", F, None, **mode)
    assert counts.min() >= 1 and np.isfinite(normals[counts >= 3]).all() and (counts >= 3).sum() > len(F) // 2


def test_fpfh(ctx):
    """spfh_from_rows_kernel / fpfh_from_rows_kernel over the 1.0 m rows (more than a million entries, thousands of rows longer than
    64) on the k = 10 normals."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        fpfh, counts, spfh = FP.check(ctx, "F", F, normals10(F), None, radius=1.0)
    assert counts.sum() > 1 << 20 and (counts > 64).sum() > 1000 and np.isfinite(fpfh).all()


def test_boundary(ctx):
    """boundary_from_rows_kernel at k = 20 on the k = 10 normals."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        got = BD.check(ctx, F, None, normals10(F), 20, 0.0, BD.HALF_PI)
    assert 500 < got["boundary"].sum() < len(F) - 500 and (got["n_neighbours"] == 20).all()


def test_iss(ctx):
    """iss_scatter / _eigen / _suppress_kernel and the keypoints' compaction at salient 1.2 m, non-max 0.8 m."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        got = IS.check(ctx, "F", F, (1.2, 0.8, 0.975, 0.975, 5))
    assert 100 < got["n_keypoints"] < (got["saliency"] > 0).sum() and got["n_salient"].max() > 128
    assert got["keypoint_index"][-1] >= 4 * 4096                                  # (the compaction's scan crossed its tiles)


def test_iss_border(ctx):
    """... with the border rule at 0.5 m (DESIGN.md's border radius for this scan), the normals computed by the call itself at 0.5 m:
    two more row sets in the search state's scratch, boundary_from_rows_kernel with min_row, iss_border_kernel."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        got = IB.check(ctx, F, (1.2, 0.8, 0.975, 0.975, 5), 0.5, math.pi / 2, None, 0.5)
    assert 500 < got["edge"].sum() < got["border"].sum() < len(F) and got["n_keypoints"] > 10


def test_euclidean_clustering(ctx):
    """The radius graph's components at tolerance 0.5 m, every cluster kept (min size 1): union-find, sizes, the sort by size and the
    gather over some 17 500 labels."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        start, indices, labels, component = CL.check(ctx, "F", F, 0.5, 1, CL.INT_MAX)
    assert start[-1] == indices.size == len(F) and 10 < len(start) - 1 < len(F) // 4 and start[1] > 4096


def test_moving_least_squares(ctx):
    """mls kernels over the 1.0 m rows at order 2, and the kept points' compaction."""
    F = filtered(ctx)
    ctx.search_set_input(F)
    with few_rows_swept():
        got = ML.check(ctx, "F", F, None, 1.0, 2)
    assert got["n_out"] > len(F) // 2 and (got["status"] == 2).sum() > len(F) // 2 and got["n_neighbours"].max() > 128
