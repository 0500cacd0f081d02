"""Dev tool: the cropping and sampling filters per call, on the voxel-filtered scan of the reference pipeline (leaf 0.2 m, ~19k points) and
on the raw 200k scan.
    python scripts/sampling_timing.py [REPS [LIMIT_S]]
PassThrough on z, CropBox (negative, the vehicle's box; with and without a transform), UniformSampling at leaf 0.5 and 1.0, and
FarthestPointSampling at 256 and 1024 samples -- on the filtered scan through the one-workgroup shape (its prefix of
ICPGPU_FPS_ONE_WORKGROUP_MAX rows) and the many-workgroup shape, on the raw scan through the latter.  With every call its kernel launches,
host waits and path (icpgpu_subset_stats).  A warm-up of 3 calls per case, then REPS timed calls (default 50).  Per call two clocks: HIP
events recorded on the context's own stream in front of the call and behind it, and the host's wall clock around the same call (it
includes the host's scan of the cloud and the upload).  Median, 10th and 90th percentile in microseconds.  The script ends itself after
LIMIT_S seconds (default 400): a hang does not outlive it."""
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icpslam_amd import Context, _lib, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 400)
print(f"library: {_lib.LIB_PATH}", flush=True)
raw = synth.scan(synth.make_scene(321), np.eye(4), 200000, seed=900)
EGO = ((-1.5, -1.0, -2.0), (2.5, 1.0, 0.5))
T = synth.pose_matrix(0.4, -0.2, 0.1, 0.02, -0.03, 0.3)


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
    filtered = ctx.voxel_grid(raw, 0.2).copy()
    one = filtered[: _lib.FPS_ONE_WORKGROUP_MAX]
    for name, cloud in (("filtered", filtered), ("raw", raw)):
        cases = [("pass_through z in [-1.5, 3]", lambda c=cloud: ctx.pass_through(c, 2, -1.5, 3.0, view=True)),
                 ("crop_box negative, the vehicle's box", lambda c=cloud: ctx.crop_box(c, *EGO, None, True, view=True)),
                 ("crop_box negative, with a transform", lambda c=cloud: ctx.crop_box(c, *EGO, T, True, view=True))]
        cases += [(f"uniform_sampling leaf {leaf}", lambda c=cloud, leaf=leaf: ctx.uniform_sampling(c, leaf, view=True)) for leaf in (0.5, 1.0)]
        for k in (256, 1024):
            if name == "filtered":
                cases.append((f"farthest_point_sampling {k} of the first {len(one)} rows", lambda k=k: ctx.farthest_point_sampling(one, k, view=True)))
            cases.append((f"farthest_point_sampling {k}", lambda c=cloud, k=k: ctx.farthest_point_sampling(c, k, view=True)))
        for label, call in cases:
            ev, wall = timed(stream, call)
            st = ctx.subset_stats()
            n_kept = len(ctx.subset_fetch()["kept"])
            print(f"{name} ({cloud.shape[0]} points): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), host wall {wall[0]:.1f} us "
                  f"(p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {reps} calls; kept {n_kept}, launches {st['launches']}, host waits {st['host_waits']}, "
                  f"path {st['path']}", flush=True)
