"""Dev tool: euclidean clustering per call, beside the radius search a user had to buy before a host breadth-first search could start.
Two inputs: the voxel-filtered scan of the reference pipeline (leaf 0.2 m, ~20k points) at tolerance 0.5 m, and the raw
200 000-point scan at 0.25 m.  The search cloud is set once, outside the timed calls.
    python scripts/cluster_timing.py WHAT [REPS [LIMIT_S]]
WHAT cluster: icpgpu_euclidean_cluster_extraction (the call alone: it ends in the wait for its two counts) and the same followed by
icpgpu_cluster_fetch of all four arrays.  WHAT radius: icpgpu_search_radius(NULL, the same radius, max_nn 0) as a caller uses it
-- the sizing call, then the call that fills the rows -- and its sizing call alone (the count pass and the scans: the same walk as
the clustering's, no rows written).  WHAT radius uses nothing the commit before the clustering lacks: copy this file into a
checkout and build of that commit and run it there, so that the figure does not come from moved code; the first line printed names
the library in use.
A warm-up of 3 calls per case, then REPS timed calls (default and minimum 100; a case whose warm-up call takes more than 0.25 s is
timed over 10 calls, and says so).  Per call two clocks: HIP events recorded on the context's own stream in front of the call and
behind it (the call waits for the stream itself, so the second event is behind all of its device work), and the host's wall clock
around the same call.  Median, 10th and 90th percentile in microseconds.  The script ends itself after LIMIT_S seconds (default
900): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icpslam_amd import Context, _lib, synth

what = sys.argv[1] if len(sys.argv) > 1 else "cluster"
reps = max(100, int(sys.argv[2])) if len(sys.argv) > 2 else 100
signal.alarm(int(sys.argv[3]) if len(sys.argv) > 3 else 900)
assert what in ("cluster", "radius"), what
print(f"library: {_lib.LIB_PATH}", flush=True)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)


def timed(stream, call):
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        once = time.perf_counter() - t0
    n = reps if once <= 0.25 else 10
    ev, wall = [], []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        call()
        wall.append(1e6 * (time.perf_counter() - t0))
        b.record(stream)
        b.synchronize()
        ev.append(1e3 * a.elapsed_time(b))
    return n, np.percentile(ev, [50, 10, 90]), np.percentile(wall, [50, 10, 90])


with Context(0) as ctx:
    handle = C.c_void_p()
    ctx._check(ctx._L.icpgpu_get_stream(ctx._h, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    vox = ctx.voxel_grid(raw, 0.2).copy()
    for name, cloud, radius in (("filtered", vox, 0.5), ("raw", raw, 0.25)):
        ctx.search_set_input(cloud)
        note = {}
        if what == "cluster":
            def extract():
                rc, note["clusters"], note["clustered"] = ctx.cluster_extract_raw(radius, 1, 2**31 - 1)
                assert rc == 0

            def extract_and_fetch():
                start, _, _, component = ctx.euclidean_cluster_extraction(radius)
                note["largest"] = int(np.diff(start).max())

            cases = (("euclidean_cluster_extraction (the call alone)", extract), ("euclidean_cluster_extraction + cluster_fetch (four arrays)", extract_and_fetch))
        else:
            def sizing():
                rc, _, _, _, note["neighbours"] = ctx.search_radius_raw(None, radius, 0, 0)
                assert rc in (0, _lib.ERR_INVALID_ARG)

            cases = (("search_radius, the sizing call alone (count pass + scans, no rows)", sizing),
                     ("search_radius as a caller uses it (sizing call + filling call, rows copied to the host)", lambda: ctx.search_radius(None, radius)))
        for label, call in cases:
            n, ev, wall = timed(stream, call)
            extra = ", ".join(f"{k} {v}" for k, v in sorted(note.items()))
            print(f"{name} ({cloud.shape[0]} points, {radius} m): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), "
                  f"host wall {wall[0]:.1f} us (p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {n} calls; {extra}", flush=True)
