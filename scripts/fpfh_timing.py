"""Dev tool: the fast point feature histograms per call, beside the normal estimation over the same cloud in the same run.
    python scripts/fpfh_timing.py [REPS [CASE [LIMIT_S]]]
The bench scan voxel-filtered at 0.2 m (~19k points): icpgpu_fpfh_estimation at k = 10 and at radius 0.5 m (2.5 cells) with the
cloud's own points as queries, at k = 10 for 1 000 keypoints given as queries, and icpgpu_normal_estimation at k = 10 and radius
0.5 m as the yardstick.  The raw scan (200 000 points): icpgpu_fpfh_estimation and icpgpu_normal_estimation at k = 10.  The normals
handed in are icpgpu_normal_estimation's (k = 10), computed once outside the timed calls, as the search cloud is set outside them.  A
warm-up call per case, then REPS timed calls (default 100; a fifth of them on the raw scan): the median and the 10th / 90th
percentiles in microseconds of HOST WALL around a call that ends in the wait for its result -- the upload of the normals and the
copy of n x 33 floats to the host included.
CASE all (default): every figure.  CASE k / radius / keypoints / raw: that mode's calls only, and CASE setup: nothing but the
set-up, so that under
    rocprofv3 --kernel-trace --hip-trace --stats --output-format csv -d OUT -- python scripts/fpfh_timing.py 20 k
the kernel statistics hold one mode's dispatches (spfh_from_rows_kernel and fpfh_from_rows_kernel beside the search kernels that feed
them and normals_from_rows_kernel) and the HIP statistics count its host waits: hipStreamSynchronize calls, less those of CASE setup,
over the REPS + 1 calls of each of the case's two entry points.  The script ends itself after LIMIT_S seconds (default 600): a hang
does not outlive it."""
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from icpslam_amd import Context, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
case = sys.argv[2] if len(sys.argv) > 2 else "all"
signal.alarm(int(sys.argv[3]) if len(sys.argv) > 3 else 600)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
K, RADIUS = 10, 0.5


def timed(call, n):
    call()  # warm-up
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        us.append(1e6 * (time.perf_counter() - t0))
    return np.percentile(us, [50, 10, 90])


def run(ctx, name, cloud, cases, n_reps):
    ctx.search_set_input(cloud)
    normals, _ = ctx.normal_estimation(None, k=K)
    keypoints = np.ascontiguousarray(cloud[:: max(1, len(cloud) // 1000)][:1000])
    got = {}

    def fpfh(queries=None, **mode):
        got["fpfh"], got["counts"] = ctx.fpfh_estimation(normals, queries, **mode)

    table = {"k": ((f"fpfh_estimation k {K}", lambda: fpfh(k=K)), (f"normal_estimation k {K}", lambda: ctx.normal_estimation(None, k=K))),
             "radius": ((f"fpfh_estimation radius {RADIUS}", lambda: fpfh(radius=RADIUS)),
                        (f"normal_estimation radius {RADIUS}", lambda: ctx.normal_estimation(None, radius=RADIUS))),
             "keypoints": ((f"fpfh_estimation k {K} at {len(keypoints)} keypoints (queries)", lambda: fpfh(keypoints, k=K)),
                           (f"normal_estimation k {K} at {len(keypoints)} keypoints (queries)", lambda: ctx.normal_estimation(keypoints, k=K)))}
    for c in cases:
        for label, call in table[c]:
            p50, p10, p90 = timed(call, n_reps)
            extra = ""
            if label.startswith("fpfh"):
                cnt, f = got["counts"], got["fpfh"]
                extra = f"; rows {int(cnt.min())}..{int(cnt.max())} entries, {int(np.isnan(f).any(axis=1).sum())} NaN signatures, {int((~f.any(axis=1)).sum())} all-zero"
            print(f"{name} ({len(cloud)} points): {label}: {p50:.1f} us per call (p10 {p10:.1f}, p90 {p90:.1f}; {n_reps} calls{extra})", flush=True)


with Context(0) as ctx:
    vox = ctx.voxel_grid(raw, 0.2)
    if case == "setup":
        ctx.search_set_input(vox)
        ctx.normal_estimation(None, k=K)
        print(f"filtered ({len(vox)} points): set-up only", flush=True)
    elif case == "raw":
        run(ctx, "raw", raw, ("k",), max(1, reps // 5))
    elif case == "all":
        run(ctx, "filtered", vox, ("k", "radius", "keypoints"), reps)
        run(ctx, "raw", raw, ("k",), max(1, reps // 5))
    else:
        run(ctx, "filtered", vox, (case,), reps)
