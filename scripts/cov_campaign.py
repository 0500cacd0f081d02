"""Dev tool (round 6): GICP's covariances (gicp_cov_select_kernel -> gicp_cov_far_kernel -> gicp_cov_kernel -> finish) against the oracle on
many random clouds -- sizes 20..60k, gaussian / uniform / raw-scan / voxel-filtered-scan / clustered shapes, duplicates, lattices and
non-finite points -- then on the named shapes below (a plane through the origin, a wall through the sensor, a scan 3 km away).

Every point that is not bit-identical to the oracle is classified from the oracle's own 20 neighbours: its raw moments are added
again in sequential order (the oracle's, PCL's loop) and in the order of the wave butterfly the covariance kernels used until the
moment sums became sequential (xor 32, 16, 8, 4, 2, 1 over lanes 0..19: see tree_sum), each finished with the oracle's SVD and
regularisation.  "tree" = the device equals the butterfly-order covariance; "neither" = the neighbour set or the decomposition
differs.  --cpu: no device; count the points where the two orders give different covariances.

Usage: python scripts/cov_campaign.py FIRST LAST [--cpu]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import oracle
from icpslam_amd import synth

K, EPS = 20, 1e-3


def campaign_cloud(seed, scene):
    rng = np.random.default_rng(70_000 + seed)
    n = int(rng.integers(20, 60000))
    kind = seed % 6
    c = np.ones((n, 4), np.float32)
    if kind == 0:
        c[:, :3] = rng.normal(0, float(rng.choice([0.5, 5.0, 60.0])), (n, 3)).astype(np.float32)
    elif kind == 1:
        c[:, :3] = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    elif kind == 2:
        c = synth.scan(scene, np.eye(4), n, seed=seed)
    elif kind == 3:
        c = oracle.voxel_grid(synth.scan(scene, synth.pose_matrix(float(rng.uniform(-20, 20)), 0, 0, 0, 0, 0), 4 * n, seed=seed), float(rng.choice([0.1, 0.2, 0.4])))
    elif kind == 4:  # a few tight clusters in a sparse volume, far-away stragglers
        k = int(rng.integers(1, 6))
        centres = rng.uniform(-50, 50, (k, 3))
        c[:, :3] = (centres[rng.integers(0, k, n)] + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
        c[::11, :3] = rng.uniform(-200, 200, (len(c[::11]), 3)).astype(np.float32)
    else:  # a lattice with duplicates: dozens of equal distances
        m = max(3, int(round(n ** (1 / 3))))
        g = (np.arange(m, dtype=np.float32) * np.float32(rng.choice([0.1, 0.25, 1.0])))
        c = np.ones((m ** 3, 4), np.float32)
        c[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        c = np.concatenate([c, c[: len(c) // 7]])
    if len(c) > 40 and seed % 5 == 0:
        c[rng.integers(0, len(c), 3), rng.integers(0, 3, 3)] = np.nan
    return f"seed {seed} kind {kind}", c


def named_clouds(scene):
    shifted = synth.scan(scene, np.eye(4), 60000, seed=9100)
    shifted[:, :3] += np.float32(3000.0)
    yield "plane through the origin", synth.plane_through_origin(40000, seed=3)
    yield "wall through the sensor", synth.wall_through_sensor(40000, seed=2)
    yield "scan shifted 3 km", shifted


def tree_sum(v):
    """The value lane 0 of wave_sum_d (butterfly xor 32 .. 1) holds for terms v[0..19] in lanes 0..19, zeros above."""
    a = [(v[l] + 0.0) + ((v[l + 16] + 0.0) if l < 4 else 0.0) for l in range(16)]
    d = [(a[l] + a[l + 8]) + (a[l + 4] + a[l + 12]) for l in range(4)]
    return (d[0] + d[2]) + (d[1] + d[3])


def seq_sum(v):
    s = 0.0
    for t in v:
        s += t
    return s


def finish(q, summer):
    """Raw covariance of the 20 float32 points q (in key order) with the given summation, then the oracle's SVD and regularisation."""
    x, y, z = (q[:, k] for k in range(3))
    f = lambda a: [float(t) for t in a]
    m = [summer(f(x)) / K, summer(f(y)) / K, summer(f(z)) / K]
    prods = {(0, 0): x * x, (1, 0): y * x, (2, 0): z * x, (1, 1): y * y, (2, 1): z * y, (2, 2): z * z}  # float32 products
    A = np.empty((3, 3))
    for (r, c), p in prods.items():
        A[r, c] = A[c, r] = summer(f(p)) / K - m[r] * m[c]
    U, _ = oracle.svd3_eigen_u(A)
    C = np.empty((3, 3))
    for r in range(3):
        for c in range(r + 1):
            acc = 0.0
            for k in range(3):
                acc += ((EPS if k == 2 else 1.0) * U[r, k]) * U[c, k]
            C[r, c] = C[c, r] = acc
    return C


def classify(cloud, nbr, idx, got):
    """'tree' / 'sequential' / 'neither' for the points idx (indices into cloud, whose neighbours are nbr)."""
    out = {"tree": 0, "sequential": 0, "neither": 0}
    for i in idx:
        q = cloud[nbr[i], :3]
        if np.array_equal(got[i], finish(q, tree_sum)):
            out["tree"] += 1
        elif np.array_equal(got[i], finish(q, seq_sum)):
            out["sequential"] += 1
        else:
            out["neither"] += 1
    return out


def main():
    first, last = int(sys.argv[1]), int(sys.argv[2])
    cpu = "--cpu" in sys.argv[3:]
    scene = synth.make_scene(3)
    clouds = [campaign_cloud(seed, scene) for seed in range(first, last)] + list(named_clouds(scene))
    bad = refused = inexact = points = 0
    worst = 0.0
    kinds = {"tree": 0, "sequential": 0, "neither": 0}
    t0 = time.time()
    ctx = None
    if not cpu:
        from icpslam_amd import Context, GICP
        ctx = Context(0)
        ctx.set_params(ctx.default_params(), method=GICP)
    for name, c in clouds:
        fin = np.isfinite(c[:, :3]).all(axis=1)
        if fin.sum() < K:
            continue
        cf = np.ascontiguousarray(c[fin])
        ref = oracle.gicp_covariances(cf)
        if cpu:
            nbr = oracle.gicp_neighbours(cf)  # the two orders against each other, on every point
            d = [i for i in range(len(cf)) if not np.array_equal(finish(cf[nbr[i], :3], tree_sum), ref[i])] if len(cf) <= 60000 else []
            points += len(cf)
            inexact += len(d)
            if d:
                print(f"{name} n {len(c)}: {len(d)} points whose butterfly-order covariance differs from the sequential one", flush=True)
            continue
        ctx.set_source(c)
        try:
            got = ctx.gicp_covariances()[fin]
        except Exception as e:  # (a cloud the k-NN grid refuses -- thousands of points in one cell -- is an error, not a wrong answer)
            refused += 1
            print(f"refused {name} n {len(c)}: {str(e)[:100]}", flush=True)
            continue
        diff = np.abs(got - ref).reshape(len(ref), -1).max(axis=1)
        points += len(ref)
        inexact += int((diff > 0).sum())
        worst = max(worst, float(diff.max()))
        if (diff > 0).any():
            bad += 1
            cls = classify(cf, oracle.gicp_neighbours(cf), np.flatnonzero(diff > 0), got)
            for k in kinds:
                kinds[k] += cls[k]
            print(f"MISMATCH {name} n {len(c)}: {int((diff > 0).sum())} points differ, worst {diff.max():.3e}; the device equals "
                  f"butterfly order {cls['tree']}, sequential order {cls['sequential']}, neither {cls['neither']}", flush=True)
    if ctx is not None:
        ctx.close()
    if cpu:
        print(f"covariance clouds {first}..{last} + named shapes (CPU): {inexact} of {points} points have a butterfly-order covariance "
              f"that differs from the sequential one; {time.time()-t0:.0f} s")
        return
    print(f"covariance clouds {first}..{last} + named shapes: {bad} clouds with differences, {refused} refused; {inexact} of {points} points "
          f"not bit-identical to the oracle, worst difference {worst:.3e}; of those the device equals butterfly order {kinds['tree']}, "
          f"sequential order {kinds['sequential']}, neither {kinds['neither']}; {time.time()-t0:.0f} s")


if __name__ == "__main__":
    main()
