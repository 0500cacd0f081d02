"""GPU parity of the mapper's map (octree_mapper.cpp:55-90,133-172) against oracle/map_oracle.c:
map contents and order bit for bit, nn cloud bit for bit, and the refine-and-grow loop end to end."""
import numpy as np
import pytest

import oracle
from icpslam_amd import NN_BRUTE, NN_GRID, synth
from icpslam_amd.mapper import OctreeMapper, identity_pose
from icpslam_amd.sequence import pose_compose, pose_from_matrix, pose_inverse, pose_to_matrix

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_map_insert_bit_exact_over_several_batches(ctx):
    ref = oracle.VoxelMap(0.5)
    ctx.map_reset(0.5)
    rng = np.random.default_rng(0)
    for k in range(4):
        a, _, _ = synth.make_pair(30000 + 5000 * k, 10, seed=10 + k)
        T = synth.pose_matrix(0.8 * k, 0.1 * k, 0.0, 0.0, 0.0, 0.05 * k) if k else None
        a = a.copy()
        a[rng.integers(0, a.shape[0], 5), :3] = np.nan           # never inserted
        got = ctx.map_add_points(a, T)
        want = ref.add_points(a, T)
        assert got == want and ctx.map_size() == len(ref)
    assert np.array_equal(_bits(ctx.map_points()), _bits(ref.points()))
    # every voxel of the last batch is taken now
    assert ctx.map_add_points(a, T) == 0


def test_map_anchor_is_first_finite_point_and_other_resolutions(ctx):
    a, _, _ = synth.make_pair(20000, 10, seed=20)
    a = a.copy()
    a[:3, :3] = np.nan
    for res in (0.05, 0.2, 3.0):
        ref = oracle.VoxelMap(res)
        ctx.map_reset(res)
        assert ctx.map_add_points(a) == ref.add_points(a)
        assert np.array_equal(_bits(ctx.map_points()), _bits(ref.points()))


def test_map_duplicates_and_single_voxel(ctx):
    pts = np.ones((5000, 4), np.float32)
    pts[:, :3] = (1.0, 2.0, 3.0)
    ctx.map_reset(0.5)
    assert ctx.map_add_points(pts) == 1
    assert np.array_equal(ctx.map_points(), pts[:1])
    assert ctx.map_add_points(np.zeros((0, 4), np.float32)) == 0


@pytest.mark.parametrize("mode", [NN_GRID, NN_BRUTE])
def test_nn_target_bit_exact(ctx, mode):
    scan0, scan1, Tgt = synth.make_pair(40000, 40000, seed=30)
    pose = synth.pose_matrix(2.0, -1.0, 0.1, 0.01, 0.02, 0.3)
    pose_inv = np.linalg.inv(pose.astype(np.float64)).astype(np.float32)
    ref = oracle.VoxelMap(0.5)
    ref.add_points(scan1, pose)
    ctx.set_params(ctx.default_params(), nn_mode=mode)
    ctx.map_reset(0.5)
    ctx.map_add_points(scan1, pose)
    src = scan0.copy()
    src[11, :3] = np.nan                                           # dropped
    src[12, :3] = (500.0, 500.0, 50.0)                             # far from the map: brute-force completion
    ctx.set_source(src)
    nn = ctx.map_nn_target(pose, pose_inv)
    want = ref.nn_cloud(src, pose, pose_inv)
    assert nn.shape == want.shape == (src.shape[0] - 1, 4)
    assert np.array_equal(_bits(nn), _bits(want))
    # the nn cloud IS the target now: aligning against it equals aligning against the oracle's nn cloud
    r = ctx.align()
    o = oracle.icp_align(src, want, oracle.default_params())
    assert r["iterations"] == o["iterations"] and r["n_corr"] == o["n_corr"]
    assert np.abs(r["T"][:3, :3] - o["T"][:3, :3]).max() <= 1e-4   # BASELINE tolerance (R)
    assert np.linalg.norm(r["T"][:3, 3] - o["T"][:3, 3]) <= 1e-3   # BASELINE tolerance (t), metres


def test_nn_target_on_empty_map(ctx):
    a, _, _ = synth.make_pair(1000, 10, seed=31)
    ctx.map_reset(0.5)
    ctx.set_source(a)
    nn = ctx.map_nn_target(np.eye(4), np.eye(4))
    assert nn.shape == (0, 4)
    r = ctx.align()                                                 # PCL: empty target -> not converged, identity
    assert not r["converged"] and np.array_equal(r["T"], np.eye(4, dtype=np.float32))


def test_refine_and_grow_matches_the_oracle_flow(ctx):
    """octree_mapper.cpp:133-172 over five scans of a short drive, odometry = ground truth + a known error."""
    scene = synth.make_scene(seed=40)
    poses = [synth.pose_matrix(0.6 * k, 0.05 * k, 0.0, 0.0, 0.0, 0.02 * k) for k in range(5)]
    scans = [synth.scan(scene, P, 30000, seed=400 + k) for k, P in enumerate(poses)]
    err = synth.pose_matrix(0.15, -0.1, 0.02, 0.0, 0.0, 0.01)

    from icpslam_amd import P2P_SVD
    mapper = OctreeMapper(ctx, octree_resolution=0.5, method=P2P_SVD)      # (the default is GICP, as octree_mapper.cpp:104 has it)
    ref = oracle.VoxelMap(0.5)
    p_icp = oracle.default_params(max_iterations=30)
    for k, (scan, P) in enumerate(zip(scans, poses)):
        raw = pose_from_matrix((P.astype(np.float64) @ err.astype(np.float64)).astype(np.float32) if k else P)
        raw_M = pose_to_matrix(raw)
        raw_Minv = pose_to_matrix(pose_inverse(raw))
        ok, transform, refined, info = mapper.refineTransformAndGrowMap(scan, raw)
        # the same sequence on the CPU
        if len(ref) == 0:
            ref.add_points(scan, raw_M)
            assert not ok and info["seeded"]
        else:
            nn = ref.nn_cloud(scan, raw_M, raw_Minv)
            o = oracle.icp_align(scan, nn, p_icp)
            assert ok == o["converged"]
            assert info["n_nn"] == nn.shape[0]
            T_gpu = pose_to_matrix(transform)
            assert np.abs(T_gpu[:3, :3] - o["T"][:3, :3]).max() <= 1e-4
            assert np.linalg.norm(T_gpu[:3, 3] - o["T"][:3, 3]) <= 1e-3
            # the CPU map grows with the GPU's refined pose so that both maps stay comparable bit for bit
            ref.add_points(scan, pose_to_matrix(refined))
            # the refinement must undo most of the injected odometry error
            resid = np.linalg.inv(P.astype(np.float64)) @ pose_to_matrix(refined).astype(np.float64)
            assert np.linalg.norm(resid[:3, 3]) < 0.08
        assert mapper.map_size == len(ref)
    assert np.array_equal(_bits(mapper.map_cloud()), _bits(ref.points()))


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_map_against_oracle(ctx, seed):
    """Random resolutions, poses, batch sizes and shapes (clumps, sheets, duplicates, non-finite points): the map and the
    nn cloud stay bit-identical to the sequential oracle."""
    rng = np.random.default_rng(500 + seed)
    res = float(rng.choice([0.07, 0.25, 0.5, 1.3, 4.0]))
    ref = oracle.VoxelMap(res)
    ctx.set_params(ctx.default_params())
    ctx.map_reset(res)
    for k in range(int(rng.integers(2, 5))):
        n = int(rng.integers(50, 40000))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            p = rng.uniform(-25, 25, (n, 3))
        elif kind == 1:
            p = rng.uniform(-25, 25, (n, 3))
            p[:, 2] = rng.normal(0.0, 0.02, n)                    # a sheet: many points per voxel column
        else:
            c = rng.uniform(-10, 10, (8, 3))
            p = c[rng.integers(0, 8, n)] + rng.normal(0, 0.3, (n, 3))
        cloud = np.ones((n, 4), np.float32)
        cloud[:, :3] = p.astype(np.float32)
        cloud[rng.integers(0, n, 3), :3] = np.nan
        cloud[n // 2: n // 2 + 20] = cloud[n // 2]                 # exact duplicates
        pose = synth.pose_matrix(*rng.uniform(-3, 3, 3), *rng.uniform(-0.3, 0.3, 3))
        assert ctx.map_add_points(cloud, pose) == ref.add_points(cloud, pose)
    assert ctx.map_size() == len(ref)
    assert np.array_equal(_bits(ctx.map_points()), _bits(ref.points()))
    q = np.ones((3000, 4), np.float32)
    q[:, :3] = rng.uniform(-30, 30, (3000, 3)).astype(np.float32)
    q[7, :3] = np.inf
    pose = synth.pose_matrix(*rng.uniform(-1, 1, 3), *rng.uniform(-0.2, 0.2, 3))
    pinv = np.linalg.inv(pose.astype(np.float64)).astype(np.float32)
    ctx.set_source(q)
    assert np.array_equal(_bits(ctx.map_nn_target(pose, pinv)), _bits(ref.nn_cloud(q, pose, pinv)))


@pytest.mark.parametrize("seed,n_scans,res", [(7, 3, 0.5), (11, 4, 0.5), (13, 3, 0.3), (17, 2, 1.0)])
def test_pcl_approx_search_mode_returns_the_restatements_nn_cloud(built, seed, n_scans, res):
    """icpgpu_map_set_search(PCL_APPROX): the nn cloud of OctreePointCloudSearch::approxNearestSearch as the reference
    literally calls it (octree_mapper.cpp:84) -- the octree's bounding box grown point by point, the greedy descent by voxel
    centre -- equals oracle/map_approx_np.py's (the NumPy restatement of PCL 1.8's octree) bit for bit, map after map as the
    box doubles; switching back gives the exact neighbours again."""
    from icpslam_amd import Context
    from oracle.map_approx_np import ApproxOctreeMap
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(70 + seed)
    poses = [np.eye(4)]
    for _ in range(n_scans):
        poses.append(poses[-1] @ synth.pose_matrix(rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), 0.0, 0.0, 0.0,
                                                   np.deg2rad(rng.uniform(-4, 4))))
    scans = [synth.scan(scene, P, 9000, seed=900 + 10 * seed + k) for k, P in enumerate(poses)]
    scans[1][5, :3] = np.nan                                   # a non-finite query / map candidate along the way
    am = ApproxOctreeMap(res)
    with Context(0) as c:
        c.map_reset(res)
        c.map_set_search(True)
        for k in range(n_scans):
            P = poses[k].astype(np.float32)
            added = c.map_add_points(scans[k], P)
            assert added == am.add_points(oracle.transform_cloud(scans[k], P))
            assert np.array_equal(c.map_points(), am.map_points())
            raw = poses[k + 1].copy()
            raw[:3, 3] += (0.07, -0.04, 0.01)
            raw = raw.astype(np.float32)
            raw_inv = np.linalg.inv(raw.astype(np.float64)).astype(np.float32)
            q = oracle.transform_cloud(scans[k + 1], raw)
            fin = np.isfinite(q[:, :3]).all(axis=1)
            ia = am.nn_indices_approx(q[fin])
            want = oracle.transform_cloud(am.map_points()[ia], raw_inv)
            c.set_source(scans[k + 1])
            got = c.map_nn_target(raw, raw_inv)
            assert got.shape == want.shape and np.array_equal(got, want), (k, am.depth)
        assert am.depth >= 6                                   # the box has doubled a few times on the way
        c.map_set_search(False)                                # ... and the exact search still is what it was
        ie, _ = oracle.nn(scans[n_scans], am.map_points(), raw)
        got = c.map_nn_target(raw, raw_inv)
        assert np.array_equal(got, oracle.transform_cloud(am.map_points()[ie[fin]], raw_inv))


def _face_queries(cloud, rng, n=6000):
    q = np.ones((n, 4), np.float32)
    q[:, :3] = cloud[rng.integers(0, cloud.shape[0], n), :3] + rng.normal(0.0, 0.3, (n, 3)).astype(np.float32)
    q[:50, :3] *= np.float32(40.0)                              # far from the map
    q[7, :3] = np.nan                                           # dropped
    return q


@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("res", [0.2, 0.3, 0.05, 0.02, 0.25, 0.5])
def test_face_campaign_map_and_nn_cloud_equal_the_c_octree(built, res, approx):
    """~10k points on voxel faces +- 1 ulp (tests/test_map_oracle.py: face_cloud), keyed by PCL under nine boxes, inserted in
    three batches (in the map frame, so that they stay on the faces) so that the points that grow the box sit in the middle
    of a batch and the points on either side of one are keyed under different box versions: the map equals PCL's octree (oracle.PclOctreeMap) bit for bit, in
    both search modes; the approximate nn cloud equals the octree's, the exact one oracle.nn's on that map."""
    from icpslam_amd import Context
    from test_map_oracle import face_cloud
    cloud = face_cloud(res, 0)
    T = None
    octree = oracle.PclOctreeMap(res)
    with Context(0) as c:
        c.map_reset(res)
        c.map_set_search(approx)
        for part in np.array_split(cloud, 3):
            assert c.map_add_points(part, T) == octree.add_points(part, T)
        assert np.array_equal(_bits(c.map_points()), _bits(octree.points()))
        rng = np.random.default_rng(int(res * 1000))
        q = _face_queries(cloud, rng)
        P = synth.pose_matrix(0.05, 0.02, -0.01, 0.0, 0.0, 0.01)
        Pinv = np.linalg.inv(P.astype(np.float64)).astype(np.float32)
        c.set_source(q)
        got = c.map_nn_target(P, Pinv)
        if approx:
            want = octree.nn_cloud(q, P, Pinv)
        else:
            idx, _ = oracle.nn(q, octree.points(), P)
            want = oracle.transform_cloud(octree.points()[idx[idx >= 0]], Pinv)
        assert got.shape == want.shape == (q.shape[0] - 1, 4)
        assert np.array_equal(_bits(got), _bits(want))


def test_pcl_approx_interleaved_adds_and_searches_equal_a_map_built_at_once(built):
    """The node set grows incrementally between searches (and is rebuilt when the box grows or its capacity doubles): after
    every scan the nn cloud equals the C octree's, and the last one equals that of a fresh context that added everything
    first."""
    from icpslam_amd import Context
    rng = np.random.default_rng(21)
    scene = synth.make_scene(121)
    poses = [np.eye(4)]
    for _ in range(5):
        poses.append(poses[-1] @ synth.pose_matrix(rng.uniform(0.5, 1.5), rng.uniform(-0.3, 0.3), 0.0, 0.0, 0.0,
                                                   np.deg2rad(rng.uniform(-5, 5))))
    scans = [synth.scan(scene, P.astype(np.float32), 20000, seed=1210 + k) for k, P in enumerate(poses)]
    octree = oracle.PclOctreeMap(0.3)
    q = scans[-1]
    P = poses[-1].astype(np.float32)
    Pinv = np.linalg.inv(P.astype(np.float64)).astype(np.float32)
    with Context(0) as a:
        a.map_reset(0.3)
        a.map_set_search(True)
        a.set_source(q)
        for s, S in zip(scans[:-1], poses[:-1]):
            S = S.astype(np.float32)
            assert a.map_add_points(s, S) == octree.add_points(s, S)
            got = a.map_nn_target(P, Pinv)
            assert np.array_equal(_bits(got), _bits(octree.nn_cloud(q, P, Pinv))), (len(octree), octree.depth)
    with Context(0) as b:
        b.map_reset(0.3)
        b.map_set_search(True)
        for s, S in zip(scans[:-1], poses[:-1]):
            b.map_add_points(s, S.astype(np.float32))
        b.set_source(q)
        assert np.array_equal(_bits(b.map_nn_target(P, Pinv)), _bits(got))


def test_pcl_approx_depth_limits(built):
    """Depth 19 (two points ~300 m apart at res 0.001) is searched like the C octree; depth 20 (~600 m) is refused with
    ICPGPU_ERR_UNSUPPORTED on that search and on every later one, while the exact search stays correct; map_reset recovers."""
    from icpslam_amd import Context
    from icpslam_amd._lib import ERR_UNSUPPORTED, IcpGpuError
    rng = np.random.default_rng(19)
    q = np.ones((2000, 4), np.float32)
    I = np.eye(4, dtype=np.float32)
    with Context(0) as c:
        for sep, depth in ((300.0, 19), (600.0, 20)):
            pts = np.ones((2000, 4), np.float32)
            pts[0, :3] = (1.0, 2.0, 3.0)
            pts[1, :3] = (1.0 + sep, 2.0 - sep / 3, 3.0 + sep / 2)
            t = rng.uniform(0.05, 0.95, (1998, 1))              # on the segment between them: inside the box
            pts[2:, :3] = pts[0, :3] + t * (pts[1, :3] - pts[0, :3]) + rng.normal(0, 0.01, (1998, 3))
            q[:, :3] = pts[rng.integers(0, 2000, 2000), :3] + rng.normal(0, 0.1, (2000, 3)).astype(np.float32)
            octree, vm = oracle.PclOctreeMap(0.001), oracle.VoxelMap(0.001)
            c.map_reset(0.001)
            c.map_set_search(True)
            assert c.map_add_points(pts) == octree.add_points(pts) == vm.add_points(pts)
            assert octree.depth == depth
            c.set_source(q)
            if depth == 19:
                assert np.array_equal(_bits(c.map_nn_target(I, I)), _bits(octree.nn_cloud(q, I, I)))
                continue
            for _ in range(2):
                with pytest.raises(IcpGpuError) as e:
                    c.map_nn_target(I, I)
                assert e.value.code == ERR_UNSUPPORTED
            c.map_add_points(pts[:10])                          # (nothing new: the map stays 20 levels deep)
            with pytest.raises(IcpGpuError):
                c.map_nn_target(I, I)
            c.map_set_search(False)
            assert np.array_equal(_bits(c.map_nn_target(I, I)), _bits(vm.nn_cloud(q, I, I)))
            c.map_set_search(True)
            c.map_reset(0.001)
            small = oracle.PclOctreeMap(0.001)
            assert c.map_add_points(pts[:1]) == small.add_points(pts[:1]) == 1
            assert np.array_equal(_bits(c.map_nn_target(I, I)), _bits(small.nn_cloud(q, I, I)))


def test_points_beyond_the_keys_reach_are_dropped_like_the_c_octree(ctx):
    """Keys are 21 bits per axis: a point more than 2^20 - 1 voxels from the first box's minimum is dropped and does not grow
    the box; the map equals the C octree's (which applies the same rule)."""
    rng = np.random.default_rng(3)
    pts = np.ones((4000, 4), np.float32)
    pts[:, :3] = rng.uniform(-5, 5, (4000, 3))
    pts[100, :3] = (1.0e6, 0.5, 0.5)
    pts[200, :3] = (1.5e6, 0.5, 0.5)
    pts[300, :3] = (0.5, -1.2e6, 0.5)
    pts[400, :3] = (1048574.5, 1048576.9, -3.0)              # the thin shell just beyond the reach
    pts[500, :3] = (-1.0e6, 0.5, 3.5)
    octree = oracle.PclOctreeMap(1.0)
    ctx.map_reset(1.0)
    assert ctx.map_add_points(pts) == octree.add_points(pts)
    assert np.array_equal(_bits(ctx.map_points()), _bits(octree.points()))
    assert not (np.abs(octree.points()[:, :3]) > 1.1e6).any()
