"""Dev tool: scans/s of the reference's pipeline (voxel filter 0.2 m -> registration against the previous scan -> fitness ->
promote) over a 40-scan drive, NDT (PCL's defaults at resolution 1.0, and with transformation epsilon 0.01) beside point-to-plane
and exact GICP.  Usage: ndt_timing.py [scans] [points] [--line-search pcl18|mt|both]
--line-search (default pcl18): the NDT step rule; with mt or both the NDT rows also report line-search trials per registration,
the drift of the chained estimate from synth's ground truth, and a third NDT row at resolution 0.5 and transformation epsilon 1e-3;
"both" runs the NDT rows under each rule (PCL 1.8's first) and the other methods once."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from icpslam_amd import GICP, GICP_INNER_EXACT, NDT, NDT_LINE_SEARCH_MORE_THUENTE, NDT_LINE_SEARCH_PCL18, P2PLANE, Context, synth

args = sys.argv[1:]
mode = "pcl18"
if "--line-search" in args:
    i = args.index("--line-search")
    mode = args[i + 1]
    del args[i:i + 2]
assert mode in ("pcl18", "mt", "both"), mode
n_scans = int(args[0]) if len(args) > 0 else 40
n_pts = int(args[1]) if len(args) > 1 else 200000
rng = np.random.default_rng(8)
scene = synth.make_scene(321)
poses = [np.eye(4)]
for _ in range(n_scans - 1):
    poses.append(poses[-1] @ synth.pose_matrix(0.3, rng.uniform(-0.03, 0.03), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-2, 2))))
scans = [synth.scan(scene, P, n_pts, seed=900 + k) for k, P in enumerate(poses)]


def drive(ctx):
    iters = accepted = trials = 0
    P = np.eye(4)
    for k, raw in enumerate(scans):
        ctx.set_source(ctx.voxel_grid(raw, 0.2))
        if k:
            r = ctx.align(want_fitness=True)
            iters += r["iterations"]
            if ctx.get_params().method == NDT:
                trials += len(ctx.ndt_line_search_trace()["step"])
            P = P @ r["T"].astype(np.float64)
            ok = r["converged"] and r["fitness"] < 20.0
            accepted += ok
            if not ok:
                continue
        ctx.promote_source_to_target()
    return iters, accepted, trials, float(np.linalg.norm(P[:3, 3] - poses[-1][:3, 3]))


rules = {"pcl18": [("", NDT_LINE_SEARCH_PCL18)], "mt": [(" mt", NDT_LINE_SEARCH_MORE_THUENTE)],
         "both": [("", NDT_LINE_SEARCH_PCL18), (" mt", NDT_LINE_SEARCH_MORE_THUENTE)]}[mode]
rows = []
for suffix, rule in rules:
    rows += [("ndt" + suffix, dict(method=NDT, max_iterations=35, transformation_epsilon=0.1), rule, 1.0),
             ("ndt eps 0.01" + suffix, dict(method=NDT, max_iterations=35, transformation_epsilon=0.01), rule, 1.0)]
    if mode != "pcl18":
        rows.append(("ndt r0.5 e1e-3" + suffix, dict(method=NDT, max_iterations=35, transformation_epsilon=1e-3), rule, 0.5))
rows += [("p2plane", dict(method=P2PLANE), NDT_LINE_SEARCH_PCL18, 1.0),
         ("gicp exact", dict(method=GICP, gicp_inner=GICP_INNER_EXACT), NDT_LINE_SEARCH_PCL18, 1.0)]
for name, kw, rule, resolution in rows:
    with Context(0) as ctx:
        ctx.set_params(ctx.default_params(), **kw)
        ctx.set_ndt_params(resolution, 0.1, 0.55, line_search=rule)
        drive(ctx)                                               # warm-up: allocations, code objects
        ctx.profile_reset()
        t0 = time.perf_counter()
        iters, accepted, trials, drift = drive(ctx)
        wall = time.perf_counter() - t0
        extra = ""
        if mode != "pcl18" and kw["method"] == NDT:
            extra = (f"; {trials / (n_scans - 1):.1f} line-search trials per registration" if rule == NDT_LINE_SEARCH_MORE_THUENTE else "")
            extra += f"; drift {drift:.3f} m"
        print(f"{name:18s} {n_scans / wall:8.1f} scans/s ({wall / n_scans * 1e3:.3f} ms per scan; {iters / (n_scans - 1):.1f} iterations per "
              f"registration, {accepted}/{n_scans - 1} accepted{extra})", flush=True)
