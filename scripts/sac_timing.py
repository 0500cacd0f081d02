"""Dev tool: the plane segmentation per call and per batch of 64 hypotheses.  Two inputs: the voxel-filtered scan of the reference
pipeline (leaf 0.2 m, ~20k points) and the raw 200 000-point scan, both at a distance threshold of 0.2 m.  The search cloud is set
once, outside the timed calls.
    python scripts/sac_timing.py [REPS [LIMIT_S]]
Cases per cloud: the call as a pipeline makes it (PCL's defaults: 50 iterations, probability 0.99, the refinement on) and without the
refinement; the same followed by icpgpu_sac_extract_view(negative); and, to price a batch (model kernel + counting kernel + its wait),
a threshold of 0.5 mm -- so few inliers that the loop runs to max_iterations -- with the refinement off at 64 and at 640 iterations:
(t640 - t64) / 9 is one batch.  Every line names the iterations, the inliers and the host waits (icpgpu_sac_stats).
A warm-up of 3 calls per case, then REPS timed calls (default and minimum 100).  Per call two clocks: HIP events recorded on the
context's own stream in front of the call and behind it, and the host's wall clock around the same call.  Median, 10th and 90th
percentile in microseconds.  The script ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icpslam_amd import Context, _lib, synth

reps = max(100, int(sys.argv[1])) if len(sys.argv) > 1 else 100
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 600)
print(f"library: {_lib.LIB_PATH}", flush=True)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)


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
    vox = ctx.voxel_grid(raw, 0.2).copy()
    for name, cloud in (("filtered", vox), ("raw", raw)):
        ctx.search_set_input(cloud)
        note = {}

        def segment(threshold=0.2, max_iterations=50, optimize=True, extract=False):
            rc, _, note["inliers"], note["iterations"], note["found"] = ctx.sac_segment_raw(threshold, max_iterations, 0.99, 1, optimize)
            assert rc == 0
            note["waits"] = ctx.sac_host_waits()
            if extract:
                note["left"] = len(ctx.sac_extract(True, view=True))

        cases = (("segmentation, PCL's defaults", lambda: segment()),
                 ("segmentation without the refinement", lambda: segment(optimize=False)),
                 ("segmentation + extract_view(negative)", lambda: segment(extract=True)),
                 ("one batch (0.5 mm, 64 iterations, no refinement)", lambda: segment(0.0005, 64, False)),
                 ("ten batches (0.5 mm, 640 iterations, no refinement)", lambda: segment(0.0005, 640, False)))
        walls = {}
        for label, call in cases:
            note.clear()
            ev, wall = timed(stream, call)
            walls[label] = wall[0]
            extra = ", ".join(f"{k} {v}" for k, v in sorted(note.items()))
            print(f"{name} ({cloud.shape[0]} points): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), "
                  f"host wall {wall[0]:.1f} us (p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {reps} calls; {extra}", flush=True)
        print(f"{name}: one batch of 64 hypotheses (model + counting launch + its wait) = (ten batches - one batch) / 9 = "
              f"{(walls[cases[4][0]] - walls[cases[3][0]]) / 9:.1f} us of host wall", flush=True)
