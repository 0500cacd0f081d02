"""Dev tool: the ISS keypoints per call, beside the radius search's sizing pass over the same cloud at the salient radius -- the count
kernel walks the very candidates the scatter kernel walks and is what its time is to be read against.  Two inputs: the
voxel-filtered scan of the reference pipeline (leaf 0.2 m, ~19k points) at salient 1.2 m / non-max 0.8 m, and the raw 200 000-point
scan at 0.3 / 0.2 m.  The search cloud is set once, outside the timed calls.
    python scripts/iss_timing.py [WHAT [REPS [LIMIT_S]]]
WHAT iss: icpgpu_iss_keypoints (the call alone: it ends in the wait for its count) and the same followed by icpgpu_iss_fetch of all six
arrays.  WHAT radius: icpgpu_search_radius(NULL, the salient radius, max_nn 0), its sizing call alone (the count pass and the scans,
no rows written) and as a caller uses it (the sizing call, then the call that fills the rows and copies them to the host).  WHAT
radius uses nothing the commit before the keypoints lacks, and icp_search.hip has not changed since: the first line printed names the
library in use.  WHAT all (default): both.  Under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/iss_timing.py all 20
the kernel statistics put iss_scatter_kernel and iss_suppress_kernel beside search_radius_count_kernel.
A warm-up of 3 calls per case, then REPS timed calls (default and minimum 100 unless REPS is given below that for a profiler run; a
case whose warm-up call takes more than 0.25 s is timed over 10 calls, and says so).  Per call two clocks: HIP events recorded on the
context's own stream in front of the call and behind it (the call waits for the stream itself, so the second event is behind all of
its device work), and the host's wall clock around the same call.  Median, 10th and 90th percentile in microseconds.  The script
ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icpslam_amd import Context, _lib, synth

what = sys.argv[1] if len(sys.argv) > 1 else "all"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
signal.alarm(int(sys.argv[3]) if len(sys.argv) > 3 else 600)
assert what in ("iss", "radius", "all"), what
print(f"library: {_lib.LIB_PATH}", flush=True)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)


def timed(stream, call):
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        once = time.perf_counter() - t0
    n = reps if once <= 0.25 else min(reps, 10)
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
    for name, cloud, salient, non_max in (("filtered", vox, 1.2, 0.8), ("raw", raw, 0.3, 0.2)):
        ctx.search_set_input(cloud)
        note = {}
        cases = []
        if what in ("iss", "all"):
            def compute():
                rc, note["keypoints"] = ctx.iss_keypoints_raw(salient, non_max)
                assert rc == 0

            def compute_and_fetch():
                got = ctx.iss_keypoints(salient, non_max)
                note["largest ball"], note["salient points"] = int(got["n_salient"].max()), int((got["saliency"] > 0).sum())

            cases += [("iss_keypoints (the call alone)", compute), ("iss_keypoints + iss_fetch (six arrays)", compute_and_fetch)]
        if what in ("radius", "all"):
            def sizing():
                rc, _, _, _, note["neighbours"] = ctx.search_radius_raw(None, salient, 0, 0)
                assert rc in (0, _lib.ERR_INVALID_ARG)

            cases += [("search_radius at the salient radius, the sizing call alone (count pass + scans, no rows)", sizing),
                      ("search_radius at the salient radius as a caller uses it (sizing + filling call, rows copied to the host)",
                       lambda: ctx.search_radius(None, salient))]
        for label, call in cases:
            if "as a caller" in label and note.get("neighbours", 0) > 50_000_000:
                print(f"{name}: {label}: skipped, {note['neighbours']} neighbours in all", flush=True)
                continue
            n, ev, wall = timed(stream, call)
            extra = ", ".join(f"{k} {v}" for k, v in sorted(note.items()))
            print(f"{name} ({cloud.shape[0]} points, salient {salient} m, non-max {non_max} m): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, "
                  f"p90 {ev[2]:.1f}), host wall {wall[0]:.1f} us (p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {n} calls; {extra}", flush=True)
