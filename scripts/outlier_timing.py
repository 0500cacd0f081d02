"""Dev tool: the outlier filters per call, on a voxel-filtered scan (leaf 0.2 m, ~23k points) and on the raw 200k-point scan it comes
from: SOR at mean_k 20 and 50, ROR at radius 0.3 / min_pts 5.  A warm-up call per shape, then REPS timed calls (default 200); the
median and the 10th / 90th percentiles in microseconds of HOST WALL around a call that ends in the wait for its result -- upload,
grid build with its two round trips, kernels, the result's arrival.
    python scripts/outlier_timing.py [REPS [CASE [LIMIT_S]]]
CASE all (default): the six figures above, and set_source + gicp_covariances on the same clouds -- host wall too, with an upload and
the covariances' copy to the host in it: a figure for the whole call, NOT comparable with a kernel's time.
CASE yardstick: only SOR at mean_k 19 and the covariance pass, on the filtered cloud.  Under
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/outlier_timing.py 50 yardstick
the per-kernel statistics then hold sor_dist_kernel (a selection of 20) and the covariance kernels (the same selection and a Jacobi
SVD) over the same cloud, the same number of times: the comparison DESIGN.md section 5 quotes.  Only the kernel trace can make it.
The script ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from icpslam_amd import GICP, Context, synth

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
    ctx.set_params(ctx.default_params(), method=GICP)
    L, h = ctx._L, ctx._h
    vox = ctx.voxel_grid(raw, 0.2)
    for name, cloud in (("filtered", vox), ("raw", raw)):
        if case == "yardstick" and name == "raw":
            break
        ptr, n = cloud.ctypes.data_as(C.POINTER(C.c_float)), cloud.shape[0]
        view, m = C.POINTER(C.c_float)(), C.c_size_t()

        def sor(k):
            assert L.icpgpu_statistical_outlier_removal_view(h, ptr, n, k, 1.0, 0, C.byref(view), C.byref(m)) == 0

        def ror():
            assert L.icpgpu_radius_outlier_removal_view(h, ptr, n, 0.3, 5, 0, C.byref(view), C.byref(m)) == 0

        def cov():
            ctx.set_source(cloud)
            ctx.gicp_covariances()

        cov_label = "set_source + covariances (whole call: upload and the covariances' copy to the host included)"
        if case == "yardstick":
            calls = (("SOR mean_k 19", lambda: sor(19)), (cov_label, cov))
        else:
            calls = (("SOR mean_k 20", lambda: sor(20)), ("SOR mean_k 50", lambda: sor(50)), ("ROR 0.3 / 5", ror), (cov_label, cov))
        for label, call in calls:
            p50, p10, p90 = timed(call, reps)
            kept = f", {m.value} kept" if "OR" in label else ""
            print(f"{name} ({n} points): {label}: {p50:.1f} us per call (p10 {p10:.1f}, p90 {p90:.1f}; {reps} calls{kept})", flush=True)
