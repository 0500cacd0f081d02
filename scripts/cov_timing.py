"""Dev tool: GICP's covariance pass on a voxel-filtered scan (0.2 m, ~19k points) and on a raw 200k-point scan, REPS times each
(set_source + gicp_covariances), for a kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/cov_timing.py [REPS]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from icpslam_amd import GICP, Context, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
with Context(0) as ctx:
    ctx.set_params(ctx.default_params(), method=GICP)
    vox = ctx.voxel_grid(raw, 0.2)
    for name, cloud in (("filtered", vox), ("raw", raw)):
        ctx.set_source(cloud)
        ctx.gicp_covariances()          # warm-up
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.set_source(cloud)
            ctx.gicp_covariances()
        print(f"{name}: {len(cloud)} points, {1e3 * (time.perf_counter() - t0) / reps:.3f} ms per set_source + covariances (host wall)")
