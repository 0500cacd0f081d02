"""Dev tool: feature-space matching and the sample-consensus alignment per call, on a re-localisation scene.
    python scripts/scp_timing.py [REPS [CASE [LIMIT_S]]]
The target is a scan; the source is the same scan seen from a pose 1.2 rad of yaw and (4, -2, 0.1) m away.  Two sizes: the bench scan
voxel-filtered at 0.2 m (~19k points; normals k = 10, FPFH radius 0.6 m) and a 2 000-point scan of the tests' scene (normals k = 10,
FPFH radius 2.0 m).  Descriptors and the search cloud are set up outside the timed calls.  Timed, as HOST WALL around a call that ends
in the wait for its result (a warm-up call, then REPS calls: median, 10th and 90th percentile):
    icpgpu_feature_knn   the source's descriptors in the target's, k = 5 (uploads 2 x n x 132 bytes, copies n x 5 x 8 bytes back)
    icpgpu_scp_align     3 samples, randomness 5, similarity 0.9, distance 0.5 m, inlier fraction 0.25, at 3 000 and at 50 000 hypotheses
and once per size, not repeated: similarity 0 (every valid hypothesis solved on the host and scored) at 4 096 hypotheses; at 2k points
also a whole chunk of 65 536.  Each alignment line carries icpgpu_scp_stats: host waits, hypotheses scored, the host's solve time.
CASE all (default), knn, align, sim0, or setup (nothing but the set-up), so that under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/scp_timing.py 5 CASE
the kernel statistics hold one case's dispatches (feature_knn_kernel, scp_sample_kernel, scp_eval_kernel, scp_fold_kernel, ...).  The
script ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
import math
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from icpslam_amd import Context, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
case = sys.argv[2] if len(sys.argv) > 2 else "all"
signal.alarm(int(sys.argv[3]) if len(sys.argv) > 3 else 600)
ARGS = dict(nr_samples=3, k_correspondences=5, similarity_threshold=0.9, max_correspondence_distance=0.5, inlier_fraction=0.25, seed=1)


def truth():
    cz, sz = math.cos(1.2), math.sin(1.2)
    T = np.eye(4)
    T[:3, :3] = [[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]
    T[:3, 3] = (4.0, -2.0, 0.1)
    return T


def moved(cloud, T):
    out = np.ones((len(cloud), 4), np.float32)
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out


def timed(call, n):
    call()  # warm-up
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        us.append(1e6 * (time.perf_counter() - t0))
    return np.percentile(us, [50, 10, 90])


def pose_error(T, ref):
    d = np.linalg.inv(ref) @ np.asarray(T, np.float64)
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(d[:3, :3]) - 1) / 2)))), float(np.linalg.norm(T[:3, 3] - ref[:3, 3]))


def run(ctx, name, target, radius, whole_chunk):
    ref = truth()
    source = moved(target, np.linalg.inv(ref))
    feats = []
    for cloud in (source, target):                      # (the target last: it stays the search cloud)
        ctx.search_set_input(cloud)
        feats.append(ctx.fpfh_estimation(ctx.normal_estimation(None, k=10)[0], None, radius=radius)[0])
    sf, tf = feats
    n = len(target)
    if case == "setup":
        print(f"{name} ({n} points): set-up only", flush=True)
        return
    if case in ("all", "knn"):
        p50, p10, p90 = timed(lambda: ctx.feature_knn(tf, sf, 5), reps)
        print(f"{name} ({n} x {n} descriptors): feature_knn k 5: {p50:.1f} us per call (p10 {p10:.1f}, p90 {p90:.1f}; {reps} calls)", flush=True)
    got = {}

    def align(**kw):
        got["r"] = ctx.scp_align(source, sf, tf, **{**ARGS, **kw})
        got["s"] = ctx.scp_stats()

    def report(label, p50, p10, p90, n_calls, iterations):
        r, s = got["r"], got["s"]
        rot, trans = pose_error(r["T"], ref)
        chunks = (iterations + 65535) // 65536
        print(f"{name} ({n} points): scp_align {label}: {p50:.1f} us per call (p10 {p10:.1f}, p90 {p90:.1f}; {n_calls} calls; host waits {s['host_waits']}, "
              f"{s['evaluated']} hypotheses scored, host solve {s['host_solve_ms']:.3f} ms = {s['host_solve_ms'] / chunks:.3f} ms per chunk; converged "
              f"{int(r['converged'])}, {r['inliers'].size} inliers, {rot:.3f} degrees and {trans:.4f} m from the truth)", flush=True)

    if case in ("all", "align"):
        for iterations in (3000, 50000):
            report(f"{iterations} hypotheses", *timed(lambda: align(max_iterations=iterations), reps), reps, iterations)
    if case in ("all", "sim0"):
        for iterations in (4096,) + ((65536,) if whole_chunk else ()):
            t0 = time.perf_counter()
            align(max_iterations=iterations, similarity_threshold=0.0)
            us = 1e6 * (time.perf_counter() - t0)
            report(f"similarity 0, {iterations} hypotheses", us, us, us, 1, iterations)


with Context(0) as ctx:
    raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
    run(ctx, "filtered", ctx.voxel_grid(raw, 0.2), 0.6, False)
    run(ctx, "2k", synth.scan(synth.make_scene(3), np.eye(4), 2000, 5), 2.0, True)
