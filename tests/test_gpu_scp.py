"""icpgpu_scp_align / _fetch / _stats on the GPU against tests/scp_restated.py.  Per hypothesis, status and indices are compared bit for
bit; the transforms against float32(oracle.umeyama(sums)) within one float32 ulp per entry plus 1e-10 (on samples that are not nearly
collinear), and EVERY evaluated hypothesis' transform against tests/solve_reference.py's float32 check on its own sums; count, S, error, best_t, the inliers, fitness and the aligned cloud bit for bit against the restatement FED THE DEVICE'S OWN
TRANSFORMS.  Then the end-to-end chain on the device: normals, FPFH, alignment, ICP."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import oracle
import scp_restated as R
import scp_scenes as S
import solve_reference as SR
from icpslam_amd import Context, IterativeClosestPoint, _lib

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
KW = S.GPU_KW
PER_HYPOTHESIS = ("status", "source_idx", "target_idx", "count", "sum", "error")


def device(c, source, sf, target, tf, nr, kc, similarity, distance, fraction, max_iterations, seed, set_input=True):
    """One alignment and its fetch: the restatement's dictionary, from the device."""
    if set_input:
        c.search_set_input(target)
    rc, T, n_in, fit, conv, cloud = c.scp_align_raw(source, sf, tf, nr, kc, similarity, distance, fraction, max_iterations, seed)
    assert rc == 0, c._L.icpgpu_last_error(c._h)
    out = c.scp_fetch()
    assert out["inliers"].size == n_in
    out.update(T=T, fitness=F32(fit), converged=conv, cloud=cloud, stats=c.scp_stats())
    return out


well_spread = S.well_spread


def compare(dev, source, sf, target, tf, nr, kc, similarity, distance, fraction, max_iterations, seed):
    want = R.align(source, sf, target, tf, nr, kc, similarity, distance, fraction, max_iterations, seed, transforms=dev["transforms"])
    for name in ("status", "source_idx", "target_idx"):
        assert dev[name].dtype == want[name].dtype and dev[name].tobytes() == want[name].tobytes(), name
    evaluated = np.flatnonzero(want["status"] == R.EVALUATED)
    checked = 0
    for e in evaluated:                                         # the host solve against the oracle's
        if well_spread(want["sums17"][e]):
            ref = oracle.umeyama(want["sums17"][e]).T.reshape(16)
            ref32 = ref.astype(F32)
            tol = np.spacing(np.abs(ref32)).astype(np.float64) + 1e-10
            assert (np.abs(dev["transforms"][e].astype(np.float64) - ref32.astype(np.float64)) <= tol).all(), (e, dev["transforms"][e], ref)
            checked += 1
    assert checked >= 0.90 * evaluated.size, (checked, evaluated.size)         # (tests/test_scp_host.py checks the scenes on the CPU)
    for e in evaluated:                                         # EVERY hypothesis, skinny samples included: a proper rotation that maximises the trace
        SR.check32(want["sums17"][e], dev["transforms"][e].reshape(4, 4).T)
    assert not dev["transforms"][want["status"] != R.EVALUATED].any()
    for name in ("count", "sum", "error"):                      # the scoring, bit for bit
        assert dev[name].dtype == want[name].dtype and dev[name].tobytes() == want[name].tobytes(), name
    assert dev["best_t"] == want["best_t"] and dev["converged"] == want["converged"]
    assert dev["inliers"].dtype == np.int32 and dev["inliers"].tobytes() == want["inliers"].tobytes()
    assert dev["T"].tobytes() == want["T"].tobytes() and F32(dev["fitness"]).tobytes() == F32(want["fitness"]).tobytes()
    finite = np.isfinite(want["cloud"]).all(axis=1)
    assert dev["cloud"][finite].tobytes() == want["cloud"][finite].tobytes() and not np.isfinite(dev["cloud"][~finite]).all(axis=1).any()
    assert dev["stats"]["evaluated"] == evaluated.size
    return want


def run(c, scene, **kw):
    args = {**KW, **kw}
    source, sf, target, tf = scene[:4]
    want = compare(device(c, source, sf, target, tf, **args), source, sf, target, tf, **args)
    assert c.scp_stats()["host_waits"] == expected_waits(want["status"], len(source))
    return want


def expected_waits(status, n_s) -> int:
    """One per chunk, one more where the chunk has hypotheses to score, one for the best hypothesis' pass (a source there is)."""
    if n_s == 0:
        return 0
    return sum(1 + int((status[a:a + _lib.SCP_CHUNK] == R.EVALUATED).any()) for a in range(0, len(status), _lib.SCP_CHUNK)) + 1


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s,n", [(3, 3), (4, 4), (63, 64), (64, 63), (65, 65), (257, 257), (300, 257), (1500, 1500)])
def test_cloud_sizes(ctx, n_s, n):
    want = run(ctx, S.matched(n_s, n), **(dict(max_iterations=33, kc=1) if n >= 1000 else {}))
    if n >= 63:
        assert want["converged"] == 1 and (want["status"] == R.EVALUATED).sum() > 5


@pytest.mark.parametrize("max_iterations", [0, 1, 63, 64, 65, 129])
def test_iteration_counts(ctx, max_iterations):
    run(ctx, S.matched(65, 65), max_iterations=max_iterations)


@pytest.mark.parametrize("max_iterations", [65535, 65536, 65537])
def test_the_chunk_edge(ctx, max_iterations):
    """An 8-point cloud, four candidates per point and a tight similarity: the restatement scores a few hundred hypotheses."""
    want = run(ctx, S.matched(8, 8, seed=4), max_iterations=max_iterations, similarity=0.98, kc=4, distance=0.5, fraction=0.5)
    assert 100 < (want["status"] == R.EVALUATED).sum() < 1500
    assert ctx.scp_stats()["host_waits"] in ((3,) if max_iterations <= 65536 else (4, 5))


@pytest.mark.parametrize("nr,kc", [(3, 2), (4, 2), (8, 1)])
def test_sample_counts(ctx, nr, kc):
    want = run(ctx, S.matched(257, 257), nr=nr, kc=kc, similarity=0.8)
    assert (want["status"] == R.EVALUATED).sum() > 5 and want["converged"] == 1


@pytest.mark.parametrize("n,kc", [(257, 1), (257, 2), (257, 5), (4, 5), (63, 64)])
def test_correspondence_randomness(ctx, n, kc):
    run(ctx, S.matched(n, n), kc=kc)                                                    # (k above n: the rows are short)


def test_similarity_zero_scores_everything_and_one_rejects_everything(ctx):
    scene = S.matched(64, 64)
    want = run(ctx, scene, similarity=0.0, max_iterations=129)                           # many survivors: two evaluation batches
    assert ((want["status"] == R.EVALUATED) | (want["status"] == R.INVALID)).all() and (want["status"] == R.EVALUATED).sum() > 64
    waits_zero = ctx.scp_stats()["host_waits"]
    run(ctx, scene, similarity=0.9, max_iterations=129)
    assert ctx.scp_stats()["host_waits"] == waits_zero == 3                             # the waits do not depend on how many survive
    want = run(ctx, scene, similarity=1.0, max_iterations=129)                          # noisy points: no polygon is congruent
    assert not (want["status"] == R.EVALUATED).any() and want["converged"] == 0 and want["fitness"] == FLT_MAX
    assert want["T"].tobytes() == np.eye(4, dtype=F32).tobytes() and ctx.scp_stats()["host_waits"] == 2


def test_self_match_at_similarity_one(ctx):
    """A cloud matched with itself: every polygon is congruent with itself, the edge ratios are exactly 1."""
    _, _, target, tf, _ = S.matched(65, 65)
    want = run(ctx, (target, tf, target, tf), similarity=1.0, kc=1)
    assert (want["status"] != R.PREREJECTED).all() and want["converged"] == 1 and want["inliers"].size == 65 and want["fitness"] == 0


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_in_both_clouds(ctx):
    source, sf, target, tf, _ = (a.copy() for a in S.matched(257, 257))
    source[::9, 1] = np.nan
    source[4, 0] = np.inf
    target[::7, 2] = np.nan
    target[5, 0] = -np.inf
    sf[::13] = np.nan                                                                   # FPFH's rows of non-finite points, and some more
    tf[::7] = np.nan
    want = run(ctx, (source, sf, target, tf), max_iterations=129)
    assert (want["status"] == R.INVALID).sum() > 10 and (want["status"] == R.EVALUATED).sum() > 5
    assert not np.isin(want["inliers"], np.flatnonzero(~np.isfinite(source).all(axis=1))).any()


def test_duplicated_points(ctx):
    source, sf, target, tf, _ = (a.copy() for a in S.matched(64, 64))
    source[32:], sf[32:] = source[:32], sf[:32]                                         # every source point twice: edges of length 0
    target[48:], tf[48:] = target[:16], tf[:16]
    want = run(ctx, (source, sf, target, tf), max_iterations=129, kc=3, similarity=0.5)
    assert (want["status"] == R.PREREJECTED).any()


def lattice():
    """27 + 8 source points whose images under the exact translation (2, 1, 0) are lattice points (A) or lie exactly 0.5 from the nearest
    one (B); B's descriptors match nothing well."""
    grid = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float64) * 2.0 + 3.0   # (no coordinate is 0)
    target = np.concatenate([grid, np.ones((27, 1))], axis=1).astype(F32)
    a = grid - [2.0, 1.0, 0.0]
    b = grid[:8] + [0.5, 0.0, 0.0] - [2.0, 1.0, 0.0]
    source = np.concatenate([np.concatenate([a, b]), np.ones((35, 1))], axis=1).astype(F32)
    tf = S.descriptors(27, 5)
    sf = np.concatenate([tf, S.descriptors(8, 6)]).astype(F32)
    return source, sf, target, tf


def test_images_exactly_on_the_distance_and_the_inlier_fraction_exactly_met(ctx):
    scene = lattice()
    kw = dict(kc=1, similarity=0.99, max_iterations=65, seed=3)
    want = run(ctx, scene, distance=0.5, fraction=27 / 35, **kw)                         # d2 == r2 is NOT an inlier; 27 / 35 is just enough
    assert want["converged"] == 1 and want["inliers"].tolist() == list(range(27)) and want["fitness"] == 0
    assert np.abs(want["T"] - np.array([[1, 0, 0, 2], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], F32)).max() < 1e-6
    want = run(ctx, scene, distance=0.5, fraction=float(np.nextafter(F32(27 / 35), F32(1))), **kw)
    assert want["converged"] == 0 and want["count"].max() == 27
    want = run(ctx, scene, distance=float(np.nextafter(F32(0.5), F32(1))), fraction=1.0, **kw)   # the next r2 up takes all 35, and fraction 1 holds
    assert want["converged"] == 1 and want["inliers"].size == 35
    want = run(ctx, scene, distance=0.0, fraction=0.0, **kw)                            # r2 = 0: nothing is below it
    assert want["converged"] == 0 and not want["count"].any()


def test_one_sum_over_twelve_orders_of_magnitude(ctx):
    """64 target points 1 km apart.  Half of the source points coincide with their partners; the others sit 1e-4 .. 1e2 m from theirs,
    the smallest offsets nearest the origin, where float32 resolves them.  A hypothesis sampled from coinciding points is the identity
    to rounding, and its inliers' d2 span 1e-8 .. 1e4 m^2 in one sum.  Attained (checked below): the offset points give terms from
    1.0e-8 to 6.4e3 m^2 (the largest offset that is kept is 80 m), and the coinciding points add rounding residues down to 1e-27 m^2
    -- a wider span than the header's range promises exactness for; the sums are still compared bit for bit with math.fsum."""
    rng = np.random.default_rng(2)
    grid = np.array([[x, y, z] for x in range(4) for y in range(4) for z in range(4)], np.float64) * 1000.0
    grid = grid[np.argsort(np.linalg.norm(grid, axis=1), kind="stable")]
    off = rng.normal(size=(64, 3))
    off *= (10.0 ** np.linspace(-4, 2, 64) / np.linalg.norm(off, axis=1))[:, None]
    off[1::2] = 0.0
    target = np.concatenate([grid, np.ones((64, 1))], axis=1).astype(F32)
    source = np.concatenate([grid + off, np.ones((64, 1))], axis=1).astype(F32)
    tf = S.descriptors(64, 8)
    want = run(ctx, (source, tf, target, tf), kc=1, similarity=0.9, distance=150.0, fraction=0.5, max_iterations=129)
    assert want["converged"] == 1
    exact = [e for e in np.flatnonzero(want["status"] == R.EVALUATED) if (want["source_idx"][e] % 2 == 1).all()]
    assert len(exact) >= 3
    for e in exact[:3]:
        mask, d2 = R.inlier_d2(want["transforms"][e], source, target, 150.0)
        terms = d2[mask][d2[mask] > 0]
        assert mask.sum() == want["count"][e] >= 60
        assert ((terms > 0.5e-8) & (terms < 2e-8)).any() and terms.max() > 6.4e3 and terms.min() < 1e-20     # 1e-8 .. 6.4e3 m^2, and residues


def grid_cell_size(c, cloud, monkeypatch, capfd) -> float:
    """icpgpu_search_set_input(cloud) and the cell size h of the grid it built, from the library's debug line; the grid is usable."""
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    c.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=%d binned=\d+ h=([0-9.]+) .* max=(\d+) " % len(cloud), capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found and int(found[-1][1]) <= 4096
    return float(found[-1][0])


def test_distance_beyond_the_cube_walk_on_a_usable_grid(ctx, monkeypatch, capfd):
    """A dense 300-point target whose grid is usable, and a correspondence distance of 10 cells (ASSERTED from the library's debug line):
    more than the 8 cells a cube walk takes, so every image inside the target's box grown by d sweeps the whole cloud, and the images
    far outside it -- 38 source points some 780 m away -- are settled by the box test in front of the sweep."""
    source, sf, target, tf, _ = (a.copy() for a in S.matched(300, 300))
    h = grid_cell_size(ctx, target, monkeypatch, capfd)
    distance = 10.0 * h
    assert distance > 8.0 * h > 0 and distance < 100.0
    source[::8, :3] += F32([600.0, -500.0, 50.0])                                       # (every 8th point: far outside under any sampled pose)
    args = {**KW, "kc": 1, "distance": distance, "fraction": 0.5, "max_iterations": 65}
    want = compare(device(ctx, source, sf, target, tf, set_input=False, **args), source, sf, target, tf, **args)
    near = np.ones(300, bool)
    near[::8] = False
    assert want["converged"] == 1 and want["inliers"].tolist() == np.flatnonzero(near).tolist()
    assert (want["count"][want["status"] == R.EVALUATED] <= near.sum()).all()


def clustered(n, seed):
    """The cloud tests/test_gpu_search.py builds for it: tight clusters (4 centres, sigma 0.3) in a wide sparse volume."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-50, 50, (4, 3))
    c = np.ones((n, 4), F32)
    c[:, :3] = (centres[r.integers(0, 4, n)] + r.normal(0, 0.3, (n, 3))).astype(F32)
    c[::11, :3] = r.uniform(-200, 200, (len(c[::11]), 3)).astype(F32)
    return c


def test_target_the_grid_refuses(ctx, monkeypatch, capfd):
    target = clustered(22000, 1)
    target[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(target)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    monkeypatch.delenv("ICPGPU_DEBUG")
    assert found and int(found[-1]) > 4096
    pick = np.arange(11, 22000, 11)[:48]                                                 # sparse points: their polygons are distinctive
    truth = S.rigid(0.4, 0.0, 0.0, (3.0, 1.0, 0.0))
    source = S.moved(target[pick], np.linalg.inv(truth))
    tf = S.descriptors(22000, 3)
    args = {**KW, "kc": 1, "distance": 0.2, "fraction": 0.5, "max_iterations": 33}
    dev = device(ctx, source, tf[pick], target, tf, set_input=False, **args)
    want = compare(dev, source, tf[pick], target, tf, **args)
    assert want["converged"] == 1 and want["inliers"].size >= 40


def test_empty_inputs_are_ok(ctx):
    source, sf, target, tf, _ = S.matched(65, 65)
    e4, e33 = np.empty((0, 4), F32), np.empty((0, 33), F32)
    for scene in ((e4, e33, target, tf), (source, sf, e4, e33), (e4, e33, e4, e33)):
        want = run(ctx, scene, max_iterations=9)
        assert want["converged"] == 0 and (want["status"] == R.INVALID).all() and want["best_t"] == -1
    ctx.search_set_input(e4)
    rc, T, n_in, fit, conv, _ = ctx.scp_align_raw(None, None, None, max_iterations=5)       # null arrays against zero sizes
    assert (rc, n_in, conv) == (0, 0, 0) and fit == FLT_MAX and T.tobytes() == np.eye(4, dtype=F32).tobytes()
    want = run(ctx, (source, sf, target, tf), max_iterations=0)
    assert want["converged"] == 0 and want["status"].size == 0 and ctx.scp_stats()["host_waits"] == 1


def test_refusals_and_the_fetch_capacities():
    source, sf, target, tf, _ = S.matched(65, 65)
    nan, inf = float("nan"), float("inf")
    with Context(0) as c:
        assert c.scp_align_raw(source, sf, None)[0] == _lib.ERR_INVALID_ARG                 # no search cloud
        assert c.scp_fetch_raw(0, 0, 3)[0] == _lib.ERR_INVALID_ARG                          # ... and no result
        assert c._L.icpgpu_scp_stats(c._h, None, None, None) == _lib.ERR_INVALID_ARG
        c.search_set_input(target)
        ok = dict(nr_samples=3, k_correspondences=2, similarity_threshold=0.9, max_correspondence_distance=0.3, inlier_fraction=0.25,
                  max_iterations=65, seed=7)
        for bad in (dict(nr_samples=2), dict(nr_samples=9), dict(k_correspondences=0), dict(k_correspondences=65), dict(similarity_threshold=-0.1),
                    dict(similarity_threshold=1.1), dict(similarity_threshold=nan), dict(max_correspondence_distance=-1.0),
                    dict(max_correspondence_distance=nan), dict(max_correspondence_distance=inf), dict(inlier_fraction=-0.1),
                    dict(inlier_fraction=1.5), dict(inlier_fraction=nan), dict(max_iterations=-1), dict(max_iterations=(1 << 20) + 1)):
            rc, T, n_in, fit, conv, _ = c.scp_align_raw(source, sf, tf, **{**ok, **bad})
            assert rc == _lib.ERR_INVALID_ARG and (n_in, conv) == (0, 0) and fit == FLT_MAX and T.tobytes() == np.eye(4, dtype=F32).tobytes(), bad
            assert c.scp_fetch_raw(65, 65, 3)[0] == _lib.ERR_INVALID_ARG                    # a refused call leaves no result behind
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        T16, n_in, fit, conv = np.zeros(16, F32), C.c_size_t(), C.c_float(), C.c_int32()
        ptr = lambda a: a.ctypes.data_as(fp)
        nums = (3, 2, 0.9, 0.3, 0.25, 65, 7)
        outs = [ptr(T16), C.byref(n_in), C.byref(fit), C.byref(conv)]
        for k in range(3):                                                                  # null clouds or descriptors against a size
            a = [ptr(source), ptr(sf), ptr(tf)]
            a[k] = None
            assert c._L.icpgpu_scp_align(c._h, a[0], 65, a[1], a[2], *nums, *outs, None) == _lib.ERR_INVALID_ARG
        for k in range(4):                                                                  # null outputs
            o = list(outs)
            o[k] = None
            assert c._L.icpgpu_scp_align(c._h, ptr(source), 65, ptr(sf), ptr(tf), *nums, *o, None) == _lib.ERR_INVALID_ARG
        assert c._L.icpgpu_scp_align(c._h, ptr(source), 65, ptr(sf), ptr(tf), *nums, *outs, None) == 0      # out_xyzw may be NULL
        n = int(n_in.value)
        assert conv.value == 1 and n > 30
        rc, full = c.scp_fetch_raw(65, n, 3)
        assert rc == 0 and (full["status"] >= 0).all() and (full["inliers"] >= 0).all()
        for caps in ((64, n), (65, n - 1), (0, 0)):                                         # too small: nothing is written
            rc, out = c.scp_fetch_raw(*caps, 3)
            assert rc == _lib.ERR_INVALID_ARG and (out["status"] == -2).all() and (out["inliers"] == -2).all() and out["best_t"] == -2
        rc, out = c.scp_fetch_raw(100, n + 5, 3)                                            # room to spare
        assert rc == 0 and out["status"][:65].tobytes() == full["status"].tobytes() and (out["status"][65:] == -2).all()
        assert out["inliers"][:n].tobytes() == full["inliers"].tobytes() and (out["inliers"][n:] == -2).all()
        best = C.c_int32(-2)                                                                # every output may be NULL
        assert c._L.icpgpu_scp_fetch(c._h, 0, 0, None, None, None, None, None, None, None, C.byref(best), None) == 0 and best.value == full["best_t"]
        one = np.full(n, -2, np.int32)
        assert c._L.icpgpu_scp_fetch(c._h, 0, n, None, None, None, None, None, None, None, None, one.ctypes.data_as(ip)) == 0
        assert one.tobytes() == full["inliers"].tobytes()
        assert c.scp_align_raw(source, sf, tf, **{**ok, "max_iterations": 1 << 20, "similarity_threshold": 1.0})[0] == 0   # the largest count is accepted
        assert c.scp_stats()["host_waits"] == 16 + 1 and c.scp_stats()["evaluated"] == 0
        c.search_set_input(target)                                                          # a new search cloud drops the result
        assert c.scp_fetch_raw(1 << 20, 65, 3)[0] == _lib.ERR_INVALID_ARG


def test_five_identical_runs(ctx):
    source, sf, target, tf, _ = S.matched(257, 257)
    args = {**KW, "max_iterations": 129}
    first = device(ctx, source, sf, target, tf, **args)
    for _ in range(4):
        again = device(ctx, source, sf, target, tf, **args)
        for name in PER_HYPOTHESIS + ("transforms", "inliers", "T", "cloud"):
            assert np.asarray(again[name]).tobytes() == np.asarray(first[name]).tobytes(), name
        assert again["best_t"] == first["best_t"] and again["fitness"] == first["fitness"]


def test_the_rows_inside_the_call_are_feature_knn_rows(ctx):
    source, sf, target, tf, _ = S.matched(300, 257)
    args = {**KW, "kc": 5, "max_iterations": 129}
    dev = device(ctx, source, sf, target, tf, **args)
    rows, _, found = ctx.feature_knn(tf, sf, 5)
    status, sidx, tidx, _ = R.hypotheses(source, target, rows, found, 3, args["similarity"], args["seed"], 0, 129)
    assert dev["source_idx"].tobytes() == sidx.tobytes() and dev["target_idx"].tobytes() == tidx.tobytes()
    assert (np.where(dev["status"] == R.NO_TRANSFORM, R.EVALUATED, dev["status"]) == status).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_descriptors():
    source, target, _ = S.e2e_clouds()
    out = []
    with Context(0) as c:
        for cloud in (source, target):
            c.search_set_input(cloud)
            out.append(c.fpfh_estimation(c.normal_estimation(None, k=S.E2E_NORMAL_K)[0], None, radius=S.E2E_FPFH_RADIUS)[0])
    return out


@pytest.mark.parametrize("seed", S.E2E_SEEDS)
def test_end_to_end_relocalisation(ctx, seed):
    """The host test's scene through the whole device chain -- normals, FPFH, alignment: within 2 degrees and the correspondence
    distance (0.5 m) of the truth, and compared with the restatement like everything else."""
    source, target, truth = S.e2e_clouds()
    sf, tf = device_descriptors()
    args = {**S.E2E, "seed": seed}
    dev = device(ctx, source, sf, target, tf, **args)
    compare(dev, source, sf, target, tf, **args)
    rot, trans = S.pose_error(dev["T"], truth)
    print(f"seed {seed}: {rot:.4f} degrees, {trans:.4f} m, {dev['inliers'].size} inliers, best_t {dev['best_t']}, stats {dev['stats']}")
    assert dev["converged"] == 1 and rot <= 2.0 and trans <= 0.5


def test_icp_from_the_alignment_reaches_the_truth_and_from_the_identity_does_not(ctx):
    source, target, truth = S.e2e_clouds()
    sf, tf = device_descriptors()
    ctx.search_set_input(target)
    start = ctx.scp_align(source, sf, tf, nr_samples=3, k_correspondences=5, similarity_threshold=0.9, max_correspondence_distance=0.5,
                          inlier_fraction=0.25, max_iterations=3000, seed=S.E2E_SEEDS[1])["T"]
    results = []
    for guess in (start, None):
        icp = IterativeClosestPoint()
        icp.setInputSource(source)
        icp.setInputTarget(target)
        icp.setMaximumIterations(50)
        icp.setMaxCorrespondenceDistance(1.0)
        icp.align(guess)
        T = np.asarray(icp.getFinalTransformation(), np.float64)
        results.append((float(np.abs(T[:3, :3] - truth[:3, :3]).max()), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))))
    (dR, dt), (dR0, dt0) = results
    print(f"ICP from the alignment: dR {dR:.2e} dt {dt:.2e}; from the identity: dR {dR0:.2e} dt {dt0:.2e}")
    assert dR <= 1e-4 and dt <= 1e-3
    assert not (dR0 <= 1e-4 and dt0 <= 1e-3)
