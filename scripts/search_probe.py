"""Dev tool: the neighbour search per call beside the outlier filters doing the nearest comparable work, on a voxel-filtered scan
(leaf 0.2 m, ~23k points) and on the raw 200k-point scan it comes from.
    search_knn(NULL, k) for k = 1, 8, 20, 64          beside  the statistical filter at mean_k = k - 1 (a distance-only selection)
    search_radius(NULL, r, 0) for r = 0.3 and 0.5 m   beside  the radius filter at the same r (a count only)
A warm-up call per shape, then REPS timed calls (default 30); the median and the 10th / 90th percentiles in microseconds of HOST WALL
around a call that ends in the wait for its result.  The two sides do not hold the same work: a search call searches a cloud that
icpgpu_search_set_input has uploaded and indexed already (timed on its own line) and copies idx / d2 rows to the host; a filter call
uploads, builds its grid, selects, and copies the kept points.  Under
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/search_probe.py 10
the per-kernel statistics hold search_knn_kernel / search_far_kernel beside sor_dist_kernel / sor_far_kernel, and
search_radius_count_kernel / search_radius_fill_kernel beside ror_count_kernel, each the same number of times per k and r: the ratio
of keyed to unkeyed selection comes from there.
    python scripts/search_probe.py [REPS [LIMIT_S]]
The script ends itself after LIMIT_S seconds (default 500): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from icpslam_amd import Context, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 500)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def timed(call, n):
    call()  # warm-up
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        us.append(1e6 * (time.perf_counter() - t0))
    return np.percentile(us, [50, 10, 90])


def line(name, n, label, p, extra=""):
    print(f"{name} ({n} points): {label}: {p[0]:.1f} us per call (p10 {p[1]:.1f}, p90 {p[2]:.1f}; {reps} calls{extra})", flush=True)


with Context(0) as ctx:
    L, h = ctx._L, ctx._h
    vox = ctx.voxel_grid(raw, 0.2)
    for name, cloud in (("filtered", vox), ("raw", raw)):
        ptr, n = cloud.ctypes.data_as(fp), cloud.shape[0]
        view, m = fp(), C.c_size_t()
        line(name, n, "search_set_input (upload + k-NN grid)", timed(lambda: ctx.search_set_input(cloud), reps))
        idx, d2, nf = np.empty((n, 64), np.int32), np.empty((n, 64), np.float32), np.empty(n, np.int32)
        for k in (1, 8, 20, 64):
            def knn():
                assert L.icpgpu_search_knn(h, None, n, k, idx.ctypes.data_as(ip), d2.ctypes.data_as(fp), nf.ctypes.data_as(ip)) == 0

            def sor():
                assert L.icpgpu_statistical_outlier_removal_view(h, ptr, n, k - 1, 1.0, 0, C.byref(view), C.byref(m)) == 0

            line(name, n, f"search_knn k {k}", timed(knn, reps), f", {n * k * 8} result bytes")
            if k > 1:  # (mean_k = 0 does not exist)
                line(name, n, f"SOR mean_k {k - 1}", timed(sor, reps))
        for r in (0.3, 0.5):
            row_start, total = np.empty(n + 1, np.int64), C.c_size_t()
            L.icpgpu_search_radius(h, None, n, r, 0, 0, row_start.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(total))
            ridx, rd2 = np.empty(total.value, np.int32), np.empty(total.value, np.float32)

            def radius():
                assert L.icpgpu_search_radius(h, None, n, r, 0, total.value, row_start.ctypes.data_as(C.POINTER(C.c_int64)), ridx.ctypes.data_as(ip),
                                              rd2.ctypes.data_as(fp), C.byref(total)) == 0

            def ror():
                assert L.icpgpu_radius_outlier_removal_view(h, ptr, n, r, 5, 0, C.byref(view), C.byref(m)) == 0

            line(name, n, f"search_radius r {r}", timed(radius, reps), f", {total.value} neighbours, longest row {int(np.diff(row_start).max())}")
            line(name, n, f"ROR r {r}", timed(ror, reps))
