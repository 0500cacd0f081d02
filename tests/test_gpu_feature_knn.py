"""icpgpu_feature_knn on the GPU against tests/scp_restated.py (feature_knn), bit for bit: idx, d2 and n_found at the kernel's edges --
its tile of 256 target rows, its 32 queries per workgroup, its 64-wide selection -- on exact ties, non-finite rows, overflowing
distances and real FPFH rows; every refusal; repeatability; and the history check of DESIGN.md section 9b for this call."""
import numpy as np
import pytest

import history_model as hm
import scp_restated as R
import scp_scenes as S
from icpslam_amd import Context, IcpGpuError, _lib, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE, QUERIES = 256, 32          # icp_feature.hip: FK_TILE, FK_QUERIES


rows, scan = S.descriptors, S.scan


def same(got, want):
    for g, w, name in zip(got, want, ("idx", "d2", "n_found")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name


def check(ctx, target, query, ks):
    for k in ks:
        same(ctx.feature_knn(target, query, k), R.feature_knn(target, query, k))


@pytest.mark.parametrize("n_t", [1, 2, 63, 64, 65, 255, 256, 257, 2 * TILE, 2 * TILE + 1, 1000])
def test_target_sizes(ctx, n_t):
    check(ctx, rows(n_t, 1), rows(65, 2), (1, 2, 5, 63, 64))        # (k above n_t for the small sizes)


@pytest.mark.parametrize("n_q", [1, 3, 4, 5, QUERIES - 1, QUERIES, QUERIES + 1, 63, 64, 65, 300])
def test_query_sizes(ctx, n_q):
    check(ctx, rows(257, 3), rows(n_q, 4), (5, 64))


def test_exact_ties_on_duplicated_and_integer_rows(ctx):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 4, (40, 33)).astype(F32)                 # small integers: d2 is exact and ties are common
    target = base[rng.integers(0, 40, 700)]                         # every row many times over
    query = np.concatenate([base[:20], rng.integers(0, 4, (30, 33)).astype(F32)])
    for k in (1, 5, 64):
        idx, d2, n_found = ctx.feature_knn(target, query, k)
        same((idx, d2, n_found), R.feature_knn(target, query, k))
        assert (d2[:20, 0] == 0).all()
        ties = d2[:, 1:] == d2[:, :-1]
        assert (ties.any() or k == 1) and (idx[:, 1:][ties] > idx[:, :-1][ties]).all()   # the lowest index first among equals


def test_non_finite_rows(ctx):
    target, query = rows(300, 5).copy(), rows(70, 6).copy()
    target[::7, 3] = np.nan
    target[5, 32] = np.inf
    target[299, 0] = -np.inf
    query[::9, 10] = np.nan
    query[1, 0] = np.inf
    query[69, 32] = -np.inf
    for k in (1, 5, 64):
        idx, d2, n_found = ctx.feature_knn(target, query, k)
        same((idx, d2, n_found), R.feature_knn(target, query, k))
        bad_t = np.flatnonzero(~np.isfinite(target).all(axis=1))
        assert not np.isin(idx, bad_t).any()
        bad_q = ~np.isfinite(query).all(axis=1)
        assert (n_found[bad_q] == 0).all() and (idx[bad_q] == -1).all() and np.isposinf(d2[bad_q]).all()
        assert (n_found[~bad_q] == min(k, 300 - bad_t.size)).all()
    all_bad = np.full((66, 33), np.nan, F32)
    same(ctx.feature_knn(all_bad, query, 3), R.feature_knn(all_bad, query, 3))       # no finite target row at all
    assert (ctx.feature_knn(all_bad, query, 3)[2] == 0).all()


def test_all_zero_rows(ctx):
    target = np.zeros((130, 33), F32)
    target[100:] = rows(30, 8)
    query = np.zeros((5, 33), F32)
    idx, d2, n_found = ctx.feature_knn(target, query, 64)
    same((idx, d2, n_found), R.feature_knn(target, query, 64))
    assert (idx == np.arange(64)).all() and (d2 == 0).all()


def test_distances_that_overflow_are_neighbours_at_infinity(ctx):
    rng = np.random.default_rng(9)
    target = rows(200, 10).copy()
    target[::3] *= F32(1e19)                 # squares near 1e38 .. 1e42: some sums overflow, some do not
    target[1::6, 0] = F32(3e38)
    target[4::6, 0] = F32(-3e38)             # q - t itself overflows against +3e38 queries
    query = rows(40, 11).copy()
    query[::4, 0] = F32(3e38)
    query[1::4] *= F32(1e19)
    for k in (5, 64):
        idx, d2, n_found = ctx.feature_knn(target, query, k)
        same((idx, d2, n_found), R.feature_knn(target, query, k))
        assert (n_found == k).all() and (idx >= 0).all() and not np.isnan(d2).any()
    assert np.isposinf(ctx.feature_knn(target, query, 64)[1]).any()


def test_real_fpfh_rows(ctx):
    """Descriptors of a 2k scan (normals with k = 10, FPFH with radius 2.0) matched against those of another scan of the scene."""
    tgt, src = scan(2000), scan(300, 9)
    ctx.search_set_input(tgt)
    tf = ctx.fpfh_estimation(ctx.normal_estimation(None, k=10)[0], None, radius=2.0)[0]
    ctx.search_set_input(src)
    qf = ctx.fpfh_estimation(ctx.normal_estimation(None, k=10)[0], None, radius=2.0)[0]
    assert np.isfinite(tf).all(axis=1).sum() > 1900
    check(ctx, tf, qf, (1, 5))


def test_empty_inputs_are_ok(ctx):
    idx, d2, n_found = ctx.feature_knn(np.empty((0, 33), F32), rows(5, 1), 3)
    assert (idx == -1).all() and np.isposinf(d2).all() and (n_found == 0).all()
    rc, idx, d2, n_found = ctx.feature_knn_raw(rows(5, 1), np.empty((0, 33), F32), 3)
    assert rc == 0 and idx.shape == (0, 3)
    rc, *_ = ctx.feature_knn_raw(None, None, 3)
    assert rc == 0
    rc, idx, d2, n_found = ctx.feature_knn_raw(None, rows(2, 1), 2)               # a null target with n_t = 0
    assert rc == 0 and (n_found == 0).all()


def test_refusals(ctx):
    t, q = rows(10, 1), rows(4, 2)
    for k in (0, -1, 65, 1 << 20):
        rc, idx, d2, n_found = ctx.feature_knn_raw(t, q, k)
        assert rc == _lib.ERR_INVALID_ARG and (n_found == -2).all()
    assert ctx.feature_knn_raw(None, q, 3, n_t=10)[0] == _lib.ERR_INVALID_ARG       # null target rows against n_t
    assert ctx.feature_knn_raw(t, None, 3, n_q=4)[0] == _lib.ERR_INVALID_ARG        # null query rows against n_q
    L, ip, fp = ctx._L, _lib.C.POINTER(_lib.C.c_int32), _lib.C.POINTER(_lib.C.c_float)
    idx, d2 = np.full((4, 3), -2, np.int32), np.full((4, 3), np.nan, F32)
    tp, qp = t.ctypes.data_as(fp), q.ctypes.data_as(fp)
    assert L.icpgpu_feature_knn(ctx._h, tp, 10, qp, 4, 3, None, d2.ctypes.data_as(fp), None) == _lib.ERR_INVALID_ARG
    assert L.icpgpu_feature_knn(ctx._h, tp, 10, qp, 4, 3, idx.ctypes.data_as(ip), None, None) == _lib.ERR_INVALID_ARG
    assert (idx == -2).all() and np.isnan(d2).all()
    assert L.icpgpu_feature_knn(ctx._h, tp, 10, qp, 4, 3, idx.ctypes.data_as(ip), d2.ctypes.data_as(fp), None) == 0   # n_found may be NULL
    same((idx, d2), R.feature_knn(t, q, 3)[:2])
    with pytest.raises(IcpGpuError):
        ctx.feature_knn(t, q, 0)


def test_five_identical_runs(ctx):
    t, q = rows(1000, 12), rows(300, 13)
    first = [a.tobytes() for a in ctx.feature_knn(t, q, 10)]
    for _ in range(4):
        assert [a.tobytes() for a in ctx.feature_knn(t, q, 10)] == first


# ---- the history check -----------------------------------------------------------------------------------
def answers(c):
    out = c.feature_knn(rows(1000, 12), rows(300, 13), 10) + c.feature_knn(rows(257, 3), rows(65, 4), 64) + c.feature_knn(rows(64, 1), rows(5, 2), 1)
    return [np.asarray(a).tobytes() for a in out]


def test_a_context_with_history_answers_as_a_new_one():
    with Context(0) as fresh:
        want = answers(fresh)
    src, tgt, _ = synth.make_pair(2000, 2000, seed=3)
    raw = scan(20000, 6)
    with Context(0) as c:
        for method in (hm.P2P, hm.GICP, hm.P2PLANE, hm.NDT):
            c.set_params(method=method, max_iterations=5)
            c.set_source(src)
            c.set_target(tgt)
            c.align(want_cloud=True, want_fitness=True)
        c.statistical_outlier_removal(raw, 19, 1.0)
        c.radius_outlier_removal(raw, 0.3, 5)
        c.voxel_grid(raw, 0.4)
        c.feature_knn(rows(2000, 20), rows(700, 21), 33)       # larger calls of its own first
        c.search_set_input(raw)
        c.search_knn(scan(300, 9), 20)
        normals, _ = c.normal_estimation(None, k=20)
        c.fpfh_estimation(normals, scan(300, 9), radius=0.5)
        c.euclidean_cluster_extraction(0.3, 2, 1000)
        c.sac_plane_segmentation(0.15, 100, 0.999, 5)
        assert answers(c) == want
        c.search_radius(scan(300, 9), 1.0)
        assert answers(c) == want
