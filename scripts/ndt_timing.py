"""Dev tool: scans/s of the reference's pipeline (voxel filter 0.2 m -> registration against the previous scan -> fitness ->
promote) over a 40-scan drive, NDT (PCL's defaults at resolution 1.0, and with transformation epsilon 0.01) beside point-to-plane
and exact GICP.  Usage: ndt_timing.py [scans] [points]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from icpslam_amd import GICP, GICP_INNER_EXACT, NDT, P2PLANE, Context, synth

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 40
n_pts = int(sys.argv[2]) if len(sys.argv) > 2 else 200000
rng = np.random.default_rng(8)
scene = synth.make_scene(321)
poses = [np.eye(4)]
for _ in range(n_scans - 1):
    poses.append(poses[-1] @ synth.pose_matrix(0.3, rng.uniform(-0.03, 0.03), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-2, 2))))
scans = [synth.scan(scene, P, n_pts, seed=900 + k) for k, P in enumerate(poses)]


def drive(ctx):
    iters = accepted = 0
    for k, raw in enumerate(scans):
        ctx.set_source(ctx.voxel_grid(raw, 0.2))
        if k:
            r = ctx.align(want_fitness=True)
            iters += r["iterations"]
            ok = r["converged"] and r["fitness"] < 20.0
            accepted += ok
            if not ok:
                continue
        ctx.promote_source_to_target()
    return iters, accepted


for name, kw in (("ndt", dict(method=NDT, max_iterations=35, transformation_epsilon=0.1)),
                 ("ndt eps 0.01", dict(method=NDT, max_iterations=35, transformation_epsilon=0.01)),
                 ("p2plane", dict(method=P2PLANE)), ("gicp exact", dict(method=GICP, gicp_inner=GICP_INNER_EXACT))):
    with Context(0) as ctx:
        ctx.set_params(ctx.default_params(), **kw)
        ctx.set_ndt_params(1.0, 0.1, 0.55)
        drive(ctx)                                               # warm-up: allocations, code objects
        ctx.profile_reset()
        t0 = time.perf_counter()
        iters, accepted = drive(ctx)
        wall = time.perf_counter() - t0
        print(f"{name:15s} {n_scans / wall:8.1f} scans/s ({wall / n_scans * 1e3:.3f} ms per scan; {iters / (n_scans - 1):.1f} iterations per "
              f"registration, {accepted}/{n_scans - 1} accepted)", flush=True)
