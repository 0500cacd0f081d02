"""Dev tool: scans/s of the reference's pipeline (voxel filter 0.2 m -> registration against the previous scan -> fitness ->
promote) over a 40-scan drive with plain point-to-plane, the symmetric objective, and the symmetric objective behind the
surface-normal rejector at 0 -- alternated in one process, `rounds` timed passes each after a warm-up pass, so that the plain
row is the yardstick of the same run.  Per-kernel times (p2plane_reduce_kernel, p2plane_sym_reduce_kernel, reject_normal_kernel)
come from a run of their own under `rocprofv3 --kernel-trace --stats`.
Usage: symmetric_timing.py [scans] [points] [rounds] [out.txt]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from icpslam_amd import P2PLANE, REJECT_SURFACE_NORMAL, Context, synth

n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 40
n_pts = int(sys.argv[2]) if len(sys.argv) > 2 else 200000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
out_path = sys.argv[4] if len(sys.argv) > 4 else None
rng = np.random.default_rng(8)
scene = synth.make_scene(321)
poses = [np.eye(4)]
for _ in range(n_scans - 1):
    poses.append(poses[-1] @ synth.pose_matrix(0.3, rng.uniform(-0.03, 0.03), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-2, 2))))
scans = [synth.scan(scene, P, n_pts, seed=900 + k) for k, P in enumerate(poses)]

# name, symmetric, chain, supply: the scan's normals are estimated once as the source's, handed back with set_source_normals
# and moved to the target by promote (the per-scan protocol of include/icpgpu.h) instead of being estimated again as the target's
SETTINGS = (("p2plane", False, (), False),
            ("symmetric", True, (), False),
            ("symmetric+normal rejector 0", True, ((REJECT_SURFACE_NORMAL, 0.0),), False),
            ("symmetric, normals supplied once", True, (), True))


def drive(ctx, symmetric, chain, supply):
    ctx.set_p2plane_symmetric(symmetric)
    ctx.set_correspondence_rejectors(chain)
    iters = accepted = 0
    for k, raw in enumerate(scans):
        ctx.set_source(ctx.voxel_grid(raw, 0.2))
        if supply:
            ctx.set_source_normals(ctx.normals(of_target=False))
        if k:
            r = ctx.align(want_fitness=True)
            iters += r["iterations"]
            ok = r["converged"] and r["fitness"] < 20.0
            accepted += ok
            if not ok:
                continue
        ctx.promote_source_to_target()
    return iters, accepted


lines = []
contexts = []
for name, symmetric, chain, supply in SETTINGS:
    ctx = Context(0)
    ctx.set_params(ctx.default_params(), method=P2PLANE)
    drive(ctx, symmetric, chain, supply)                         # warm-up: allocations, code objects
    contexts.append(ctx)
for rnd in range(rounds):
    for ctx, (name, symmetric, chain, supply) in zip(contexts, SETTINGS):
        ctx.profile_reset()
        t0 = time.perf_counter()
        iters, accepted = drive(ctx, symmetric, chain, supply)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        p = ctx.profile()
        lines.append(f"round {rnd} {name:33s} {n_scans / wall:8.1f} scans/s ({wall / n_scans * 1e3:.3f} ms per scan; "
                     f"{iters / (n_scans - 1):.2f} iterations per registration, {accepted}/{n_scans - 1} accepted; normal passes "
                     f"{p.gicp_cov_launches}; reduce launches {p.reduce_launches}, {p.reduce_bytes / max(1, p.reduce_launches) / 1e6:.3f} MB each)")
        print(lines[-1], flush=True)
for ctx in contexts:
    ctx.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
