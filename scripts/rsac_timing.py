"""Dev tool: what the sample-consensus rejector costs per ICP iteration on the reference's pipeline (voxel filter 0.2 m ->
point-to-point registration against the previous scan -> fitness -> promote) over a 40-scan drive: no chain, a MEDIAN chain (a
stage that never waits) and the sample-consensus stage at two thresholds -- alternated in one process, `rounds` timed passes each
after a warm-up pass, so that the chain-less row is the yardstick of the same run.  Host timers and the profile counters only.
Usage: rsac_timing.py [scans] [points] [rounds] [out.txt]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from icpslam_amd import P2P_SVD, REJECT_MEDIAN_DISTANCE, Context, synth
from icpslam_amd._lib import REJECT_SAMPLE_CONSENSUS

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

SETTINGS = (("no chain", ()),
            ("median 2.0", ((REJECT_MEDIAN_DISTANCE, 2.0),)),
            ("sample consensus 0.05 m, 1000", ((REJECT_SAMPLE_CONSENSUS, 0.05, 1000),)),
            ("sample consensus 0.2 m, 1000", ((REJECT_SAMPLE_CONSENSUS, 0.2, 1000),)))


def drive(ctx, chain):
    ctx.set_correspondence_rejectors(chain)
    sac = any(c[0] == REJECT_SAMPLE_CONSENSUS for c in chain)
    iters = accepted = pairs = waits = hyp = 0
    for k, raw in enumerate(scans):
        ctx.set_source(ctx.voxel_grid(raw, 0.2))
        if k:
            r = ctx.align(want_fitness=True)
            iters += r["iterations"]
            ok = r["converged"] and r["fitness"] < 20.0
            accepted += ok
            if sac:                                             # the last iteration's run of the stage
                f = ctx.rejector_sac_fetch(per_hypothesis=False)
                pairs, waits, hyp = pairs + f["m"], waits + f["host_waits"], hyp + f["iterations"]
            if not ok:
                continue
        ctx.promote_source_to_target()
    return iters, accepted, pairs, waits, hyp


lines = []
contexts = []
for name, chain in SETTINGS:
    ctx = Context(0)
    ctx.set_params(ctx.default_params(), method=P2P_SVD)
    drive(ctx, chain)                                           # warm-up: allocations, code objects
    contexts.append(ctx)
for rnd in range(rounds):
    for ctx, (name, chain) in zip(contexts, SETTINGS):
        ctx.profile_reset()
        t0 = time.perf_counter()
        iters, accepted, pairs, waits, hyp = drive(ctx, chain)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        p = ctx.profile()
        n = n_scans - 1
        lines.append(f"round {rnd} {name:30s} {wall / n_scans * 1e3:8.3f} ms per scan, {iters / n:5.2f} iterations per registration, "
                     f"{wall / max(1, iters) * 1e6:8.1f} us of wall per iteration, {accepted}/{n} accepted; reduce launches {p.reduce_launches}, "
                     f"grid launches {p.grid_launches}; last iteration's stage: {pairs / n:.0f} pairs, {hyp / n:.1f} hypotheses, {waits / n:.1f} host waits")
        print(lines[-1], flush=True)
for ctx in contexts:
    ctx.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
