"""Dev tool: the segmentation from normals per call and per batch of 64 hypotheses, beside the plane segmentation on the same clouds.
Two inputs: the voxel-filtered scan of the reference pipeline (leaf 0.2 m, ~19k points) and the raw 200 000-point scan; the normals
are icpgpu_normal_estimation's over 12 neighbours.  The search cloud is set once, outside the timed calls; the normals travel with
every call (they are an argument).
    python scripts/sac_normals_timing.py [REPS [LIMIT_S]]
Cases per cloud and model (plane = icpgpu_sac_plane_segmentation, NORMAL_PLANE, CYLINDER), all without the refinement:
  idle batches     a threshold of 0.5 mm -- so few inliers that the loop runs to max_iterations and nearly every wave takes the
                   short-cut -- at 64 and at 640 iterations: (t640 - t64) / 9 is one batch
  loaded batches   a threshold of 0.2 m and a probability of 1 - 1e-15, at 64 and at 256 iterations: the difference divided by the
                   difference in host waits is one batch in which the angle is evaluated for the waves near a hypothesis
and the call as a pipeline makes it (50 iterations, 0.2 m, probability 0.99, the refinement on).  Every line names the iterations,
the inliers and the host waits.  A warm-up of 3 calls per case, then REPS timed calls (default and minimum 100).  Per call two clocks:
HIP events on the context's own stream around the call, and the host's wall clock.  Median, 10th and 90th percentile in microseconds.
The script ends itself after LIMIT_S seconds (default 500): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icpslam_amd import SACMODEL_CYLINDER, SACMODEL_NORMAL_PLANE, Context, _lib, synth

reps = max(100, int(sys.argv[1])) if len(sys.argv) > 1 else 100
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 500)
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
        normals = np.ascontiguousarray(ctx.normal_estimation(None, k=12)[0])
        note = {}

        def run(model, threshold, max_iterations, probability, optimize):
            if model == "plane":
                rc, _, note["inliers"], note["iterations"], _ = ctx.sac_segment_raw(threshold, max_iterations, probability, 1, optimize)
                assert rc == 0
                note["waits"] = ctx.sac_host_waits()
            else:
                rc, _, _, note["inliers"], note["iterations"], _ = ctx.sac_segmentation_from_normals_raw(model, normals, threshold, 0.1, 0.0, 0.0,
                                                                                                        max_iterations, probability, 1, optimize)
                assert rc == 0
                note["waits"] = ctx.sac_normals_host_waits()

        for label, model in (("plane", "plane"), ("NORMAL_PLANE", SACMODEL_NORMAL_PLANE), ("CYLINDER", SACMODEL_CYLINDER)):
            got = {}
            for case, args in (("default call", (0.2, 50, 0.99, True)), ("idle 64", (0.0005, 64, 0.99, False)), ("idle 640", (0.0005, 640, 0.99, False)),
                               ("loaded 64", (0.2, 64, 1 - 1e-15, False)), ("loaded 256", (0.2, 256, 1 - 1e-15, False))):
                note.clear()
                ev, wall = timed(stream, lambda: run(model, *args))
                got[case] = (wall[0], note["waits"])
                extra = ", ".join(f"{k} {v}" for k, v in sorted(note.items()))
                print(f"{name} ({cloud.shape[0]} points) {label}: {case}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), "
                      f"host wall {wall[0]:.1f} us (p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {reps} calls; {extra}", flush=True)
            print(f"{name} {label}: one idle batch = {(got['idle 640'][0] - got['idle 64'][0]) / 9:.1f} us of host wall", flush=True)
            dw = got["loaded 256"][1] - got["loaded 64"][1]
            if dw > 0:
                print(f"{name} {label}: one loaded batch = {(got['loaded 256'][0] - got['loaded 64'][0]) / dw:.1f} us of host wall "
                      f"({dw} batches apart)", flush=True)
