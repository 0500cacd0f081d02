"""Dev tool: the normal estimation per call on a voxel-filtered scan (leaf 0.2 m, ~19k points), the search cloud's own points as
queries: icpgpu_normal_estimation at k = 20 and at radius 0.5 m, beside the search calls that produce the same rows
(icpgpu_search_knn k = 20, icpgpu_search_radius 0.5 m) and beside the point-to-plane mode's own estimate (icpgpu_normals: GICP's
plane over a fixed 20 neighbours), all in one run on one build.  A warm-up call per case, then REPS timed calls (default 200); the
median and the 10th / 90th percentiles in microseconds of HOST WALL around a call that ends in the wait for its result.
    python scripts/normals_timing.py [REPS [CASE [LIMIT_S]]]
CASE all (default): the five figures.  CASE k: normal_estimation and search_knn at k = 20 and the icpgpu_normals pass; CASE radius:
normal_estimation and search_radius at 0.5 m -- so that a kernel trace holds one mode's dispatches only.
The search cloud is set once, outside the timed calls (a query call builds nothing).  The icpgpu_normals case is a whole call with
an upload in it -- set_target with a cloud the context does not hold, then the estimate and its copy to the host -- NOT comparable
with the other figures; under
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/normals_timing.py 50 k
the per-kernel statistics hold normals_from_rows_kernel beside the search kernels that feed it (their rows average the
normal_estimation calls and the plain search calls: the same work) and beside gicp_cov_select_kernel / gicp_cov_far_kernel /
gicp_normal_finish_kernel over the same cloud: the comparison DESIGN.md section 5 quotes.  The script ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from icpslam_amd import P2PLANE, Context, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
case = sys.argv[2] if len(sys.argv) > 2 else "all"
signal.alarm(int(sys.argv[3]) if len(sys.argv) > 3 else 600)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)


def timed(call, n):
    call()  # warm-up
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        us.append(1e6 * (time.perf_counter() - t0))
    return np.percentile(us, [50, 10, 90])


with Context(0) as ctx:
    ctx.set_params(ctx.default_params(), method=P2PLANE)
    vox = ctx.voxel_grid(raw, 0.2)
    n = vox.shape[0]
    ctx.search_set_input(vox)
    # two clouds that differ in one point: set_target never recognises the one it is given, so every call estimates
    pair = [vox.copy(), vox.copy()]
    pair[1][0, 0] += np.float32(0.001)
    turn = [0]

    def p2plane_estimate():
        turn[0] ^= 1
        ctx.set_target(pair[turn[0]])
        ctx.normals(True)

    rows = {}

    def ne(**mode):
        rows["normals"], rows["counts"] = ctx.normal_estimation(None, **mode)

    cases = (("normal_estimation k 20", lambda: ne(k=20)), ("search_knn k 20 (the rows alone, copied to the host)", lambda: ctx.search_knn(None, 20)),
             ("normal_estimation radius 0.5", lambda: ne(radius=0.5)),
             ("search_radius 0.5 (the rows alone, copied to the host; two calls: the first sizes the arrays)", lambda: ctx.search_radius(None, 0.5)),
             ("set_target + icpgpu_normals (whole call: upload, GICP's plane over 20 neighbours, the copy to the host)", p2plane_estimate))
    if case == "k":
        cases = cases[:2] + cases[4:]
    elif case == "radius":
        cases = cases[2:4]
    for label, call in cases:
        p50, p10, p90 = timed(call, reps)
        extra = ""
        if label.startswith("normal_estimation"):
            c = rows["counts"]
            extra = f"; rows {int(c.min())}..{int(c.max())} entries, {int(np.isnan(rows['normals'][:, 0]).sum())} points without a normal"
        print(f"filtered ({n} points): {label}: {p50:.1f} us per call (p10 {p10:.1f}, p90 {p90:.1f}; {reps} calls{extra})", flush=True)
