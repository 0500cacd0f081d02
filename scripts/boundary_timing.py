"""Dev tool: the boundary estimation and ISS with border estimation per call on the voxel-filtered scan of the reference pipeline
(leaf 0.2 m, ~19k points), the search cloud set once outside the timed calls.
    python scripts/boundary_timing.py [WHAT [REPS [LIMIT_S]]]
WHAT boundary: icpgpu_boundary_estimation at k = 30 and at radius 0.5 m (the radius the FPFH timing uses) with the cloud's own points
as queries, each beside icpgpu_normal_estimation at the same arguments -- the two calls search the same rows and differ in the kernel
that reads them -- and beside the row search alone (icpgpu_search_knn delivered; icpgpu_search_radius' sizing call).  WHAT iss:
icpgpu_iss_keypoints (salient 1.2 m / non-max 0.8 m) beside icpgpu_iss_keypoints_border at border radius 0.5 m, with the normals
given and with the normals computed from radius 0.5 m.  WHAT all (default): both.  Under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/boundary_timing.py all 20
the kernel statistics put boundary_from_rows_kernel beside the search kernels that feed it, and iss_border_kernel beside the walks.
A warm-up of 3 calls per case, then REPS timed calls (default 100).  Per call two clocks: HIP events recorded on the context's own
stream in front of the call and behind it, and the host's wall clock around the same call.  Median, 10th and 90th percentile in
microseconds.  The script ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
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

what = sys.argv[1] if len(sys.argv) > 1 else "all"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
signal.alarm(int(sys.argv[3]) if len(sys.argv) > 3 else 600)
assert what in ("boundary", "iss", "all"), what
print(f"library: {_lib.LIB_PATH}", flush=True)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
K, RADIUS, ANGLE = 30, 0.5, math.pi / 2
SALIENT, NON_MAX, BORDER = 1.2, 0.8, 0.5


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
    normals, _ = ctx.normal_estimation(None, k=10)
    note = {}
    cases = []
    if what in ("boundary", "all"):
        def boundary(k, radius):
            got = ctx.boundary_estimation(normals, None, k, radius, ANGLE)
            note["boundary points"], note["neighbours"] = int(got["boundary"].sum()), int(got["n_neighbours"].sum())
            note["largest row"] = int(got["n_neighbours"].max())

        def sizing():
            rc, _, _, _, note["neighbours"] = ctx.search_radius_raw(None, RADIUS, 0, 0)
            assert rc in (0, _lib.ERR_INVALID_ARG)

        cases += [(f"boundary_estimation k {K}", lambda: boundary(K, 0.0)),
                  (f"normal_estimation k {K}", lambda: ctx.normal_estimation(None, k=K)),
                  (f"search_knn k {K} (rows copied to the host)", lambda: ctx.search_knn(None, K)),
                  (f"boundary_estimation radius {RADIUS}", lambda: boundary(0, RADIUS)),
                  (f"normal_estimation radius {RADIUS}", lambda: ctx.normal_estimation(None, radius=RADIUS)),
                  (f"search_radius {RADIUS}, the sizing call alone (count pass + scans, no rows)", sizing)]
    if what in ("iss", "all"):
        def plain():
            rc, note["keypoints"] = ctx.iss_keypoints_raw(SALIENT, NON_MAX)
            assert rc == 0

        def border(given):
            rc, note["keypoints"] = ctx.iss_keypoints_border_raw(SALIENT, NON_MAX, 0.975, 0.975, 5, BORDER, ANGLE, normals if given else None, RADIUS)
            assert rc == 0
            note["waits"] = ctx.iss_stats()

        def border_and_fetch():
            got = ctx.iss_keypoints_border(SALIENT, NON_MAX, 0.975, 0.975, 5, BORDER, ANGLE, normals)
            note["edge points"], note["border points"] = int(got["edge"].sum()), int(got["border"].sum())

        cases += [("iss_keypoints (the call alone)", plain),
                  (f"iss_keypoints_border, border {BORDER}, normals given (the call alone)", lambda: border(True)),
                  (f"iss_keypoints_border, border {BORDER}, normals computed at {RADIUS} (the call alone)", lambda: border(False)),
                  ("iss_keypoints_border, normals given + iss_fetch + iss_fetch_border", border_and_fetch)]
    for label, call in cases:
        note.clear()
        ev, wall = timed(stream, call)
        extra = ", ".join(f"{k} {v}" for k, v in sorted(note.items()))
        print(f"filtered ({cloud.shape[0]} points): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), host wall {wall[0]:.1f} us "
              f"(p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {reps} calls; {extra}", flush=True)
