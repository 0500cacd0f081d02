"""Dev tool: region growing per call on the voxel-filtered scan of the reference pipeline (leaf 0.2 m), the search cloud set and the
normals estimated (the device's own, k = 30) once outside the timed calls.
    python scripts/region_timing.py [REPS [LIMIT_S]]
icpgpu_region_growing at k = 30 and k = 10 with PCL's defaults (30 degrees, curvature 0.05), alone and with icpgpu_region_fetch; beside
them, from the same build on the same cloud, icpgpu_search_knn at the same k (its rows copied to the host: the call a user has) and
icpgpu_euclidean_cluster_extraction at 0.5 m.  A warm-up of 3 calls per case, then REPS timed calls (default 100).  Per call two
clocks: HIP events recorded on the context's own stream in front of the call and behind it, and the host's wall clock around the same
call.  Median, 10th and 90th percentile in microseconds.  The script ends itself after LIMIT_S seconds (default 600): a hang does not
outlive it."""
import ctypes as C
import math
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icpslam_amd import Context, _lib, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 600)
print(f"library: {_lib.LIB_PATH}", flush=True)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
COS30 = np.float32(math.cos(math.radians(30.0)))
INT_MAX = 2**31 - 1


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
    normals, _ = ctx.normal_estimation(None, k=30)
    note = {}

    def grow(k, fetch):
        rc, note["regions"], note["points in them"] = ctx.region_growing_raw(normals, k, COS30, 0.05, 1, INT_MAX)
        assert rc == 0
        if fetch:
            rc, _, _, _, _, kind, _ = ctx.region_fetch_raw(note["regions"], note["points in them"])
            assert rc == 0
            note["core / border / single / none"] = "/".join(str(int((kind == v).sum())) for v in (2, 1, 0, -1))

    cases = []
    for k in (30, 10):
        cases += [(f"region_growing k {k}", lambda k=k: grow(k, False)), (f"region_growing k {k} + region_fetch", lambda k=k: grow(k, True)),
                  (f"search_knn k {k} (rows copied to the host)", lambda k=k: ctx.search_knn(None, k))]
    cases += [("euclidean_cluster_extraction 0.5 m", lambda: ctx.cluster_extract_raw(0.5, 1, INT_MAX))]
    for label, call in cases:
        note.clear()
        ev, wall = timed(stream, call)
        extra = ", ".join(f"{k} {v}" for k, v in sorted(note.items()))
        print(f"filtered ({cloud.shape[0]} points): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), host wall {wall[0]:.1f} us "
              f"(p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {reps} calls; {extra}", flush=True)
