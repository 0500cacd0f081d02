"""Dev tool: the segment moments per call on the voxel-filtered scan of the reference pipeline (leaf 0.2 m, ~19k points), the search
cloud set, the clusters extracted (0.5 m) and the regions grown (k = 30, the device's own normals) once outside the timed calls.
    python scripts/segment_timing.py [REPS [LIMIT_S]]
icpgpu_segment_moments over the clusters and over the regions where they lie on the device, over the clusters' fetched CSR handed back
as a HOST source, and over one segment that holds the whole cloud; beside them, from the same build on the same cloud,
icpgpu_search_knn at k = 30 (its rows copied to the host: the yardstick profiles/boundary.txt uses) and the host alternative the call
replaces: icpgpu_cluster_fetch plus a NumPy loop over the clusters that computes the same fields (count, centroid, covariance,
eigen-decomposition, both boxes).  A warm-up of 3 calls per case, then REPS timed calls (default 100).  Per call two clocks: HIP events
recorded on the context's own stream in front of the call and behind it, and the host's wall clock around the same call.  Median, 10th
and 90th percentile in microseconds.  The script ends itself after LIMIT_S seconds (default 600): a hang does not outlive it."""
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
K = 30


def timed(stream, call, n_reps):
    for _ in range(3):
        call()
    ev, wall = [], []
    for _ in range(n_reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        call()
        wall.append(1e6 * (time.perf_counter() - t0))
        b.record(stream)
        b.synchronize()
        ev.append(1e3 * a.elapsed_time(b))
    return np.percentile(ev, [50, 10, 90]), np.percentile(wall, [50, 10, 90])


def numpy_loop(cloud, start, indices):
    """What a user writes today behind cluster_fetch: per cluster the count, centroid, normalised covariance, eigen-decomposition and
    both boxes, in float64 NumPy."""
    out = []
    xyz = cloud[:, :3].astype(np.float64)
    for a, b in zip(start[:-1], start[1:]):
        p = xyz[indices[a:b]]
        p = p[np.isfinite(p).all(axis=1)]
        c = p.mean(axis=0)
        d = p - c
        lam, vec = np.linalg.eigh(d.T @ d / len(p))
        u = d @ vec
        lo, hi = u.min(axis=0), u.max(axis=0)
        out.append((len(p), c, lam, vec, p.min(axis=0), p.max(axis=0), hi - lo, c + vec @ ((hi + lo) / 2)))
    return out


with Context(0) as ctx:
    handle = C.c_void_p()
    ctx._check(ctx._L.icpgpu_get_stream(ctx._h, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    cloud = ctx.voxel_grid(raw, 0.2).copy()
    ctx.search_set_input(cloud)
    normals, _ = ctx.normal_estimation(None, k=K)
    rc, n_clusters, n_clustered = ctx.cluster_extract_raw(0.5, 1, INT_MAX)
    rc2, n_regions, n_in = ctx.region_growing_raw(normals, K, COS30, 0.05, 1, INT_MAX)
    assert rc == rc2 == 0
    rc, start, indices, _, _ = ctx.cluster_fetch_raw(n_clusters, n_clustered)
    assert rc == 0
    sizes = np.diff(start)
    print(f"filtered ({cloud.shape[0]} points): {n_clusters} clusters of {n_clustered} points at 0.5 m (largest {sizes.max()}, {int((sizes <= 5).sum())} of "
          f"5 or fewer), {n_regions} regions of {n_in} points at k {K}", flush=True)
    whole = (np.array([0, len(cloud)], np.int64), np.arange(len(cloud), dtype=np.int32))

    def host_alternative():
        rc, s, i, _, _ = ctx.cluster_fetch_raw(n_clusters, n_clustered, want_labels=False, want_component=False)
        assert rc == 0
        numpy_loop(cloud, s, i)

    cases = [(f"segment_moments over the {n_clusters} clusters on the device", lambda: ctx.segment_moments(source="clusters", n_segments=n_clusters), reps),
             (f"segment_moments over the {n_regions} regions on the device", lambda: ctx.segment_moments(source="regions", n_segments=n_regions), reps),
             (f"segment_moments over the {n_clusters} clusters as a HOST source", lambda: ctx.segment_moments(start, indices), reps),
             ("segment_moments over one segment holding the whole cloud", lambda: ctx.segment_moments(*whole), reps),
             (f"search_knn k {K} (rows copied to the host)", lambda: ctx.search_knn(None, K), reps),
             (f"cluster_fetch + a NumPy loop over the {n_clusters} clusters", host_alternative, max(3, reps // 10))]
    for label, call, n_reps in cases:
        ev, wall = timed(stream, call, n_reps)
        print(f"filtered ({cloud.shape[0]} points): {label}: events {ev[0]:.1f} us (p10 {ev[1]:.1f}, p90 {ev[2]:.1f}), host wall {wall[0]:.1f} us "
              f"(p10 {wall[1]:.1f}, p90 {wall[2]:.1f}); {n_reps} calls; host waits {ctx.segment_stats()['host_waits']}", flush=True)
