"""Dev tool: the ground filter per call on the voxel-filtered scan of the reference pipeline (leaf 0.2 m, ~19k points), the search
cloud set once outside the timed calls.
    python scripts/pmf_timing.py [REPS [LIMIT_S]]
The default schedule (windows 3, 5, 9, 17, 33) as one call, and the schedules cut after 1 .. 5 passes (max_window_size 3, 4, 6, 10,
18), whose differences are the passes' times; beside them icpgpu_search_knn at k = 30 on the same cloud, the yardstick
profiles/boundary.txt uses, and icpgpu_morphological_operator OPEN at the first and the last window.  With every filter call the exact
point tests its rim scans made (icpgpu_pmf_stats), against the sum over the passes of (ground points before the pass)^2 x 2 that
testing every pair would make.  A warm-up of 3 calls per case, then REPS timed calls (default 100).  Per call two clocks: HIP events
recorded on the context's own stream in front of the call and behind it, and the host's wall clock around the same call.  Median, 10th
and 90th percentile in microseconds.  The script ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icpslam_amd import MORPH_OPEN, Context, _lib, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 600)
print(f"library: {_lib.LIB_PATH}", flush=True)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
K = 30


def timed(stream, call):
    for _ in range(3):
        call()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        call()
        wall.append(1e6 * (time.perf_counter() - t0))
        b.record(stream)
        b.synchronize()
        ev.append(1e3 * a.elapsed_time(b))
    return np.percentile(ev, [50, 10, 90]), np.percentile(wall, [50, 10, 90])


with Context(0) as ctx:
    handle = C.c_void_p()
    ctx._check(ctx._L.icpgpu_get_stream(ctx._h, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    cloud = ctx.voxel_grid(raw, 0.2).copy()
    ctx.search_set_input(cloud)
    full = ctx.progressive_morphological_filter()
    before = np.concatenate([[ctx.search_size()[1]], full["ground_after"][:-1]]).astype(np.int64)
    print(f"filtered ({cloud.shape[0]} points): windows {full['windows'].tolist()}, thresholds {[round(float(t), 3) for t in full['thresholds']]}, "
          f"ground after each pass {full['ground_after'].tolist()}", flush=True)
    note = {}

    def filter_call(max_window_size):
        rc, note["ground"], note["passes"] = ctx.pmf_filter_raw(max_window_size=max_window_size)
        assert rc == 0
        note["waits"], note["point tests"] = ctx.pmf_stats()
        note["pairs x 2"] = int(2 * (before[: note["passes"]] ** 2).sum())

    cases = [(f"progressive_morphological_filter, {p} pass{'es' if p > 1 else ''} (max_window_size {m})", lambda m=m: filter_call(m))
             for p, m in ((5, 33), (1, 3), (2, 4), (3, 6), (4, 10), (5, 18))]
    cases += [(f"morphological_operator OPEN, window {w}", lambda w=w: ctx.morphological_operator(w, MORPH_OPEN)) for w in (3.0, 33.0)]
    cases += [(f"search_knn k {K} (rows copied to the host)", lambda: ctx.search_knn(None, K))]
    for label, call in cases:
        note.clear()
        ev, wall = timed(stream, call)
        extra = ", ".join(f"{k} {v}" for k, v in sorted(note.items()))
        print(f"filtered ({cloud.shape[0]} points): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), host wall {wall[0]:.1f} us "
              f"(p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {reps} calls; {extra}", flush=True)
