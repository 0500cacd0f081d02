"""Generates tests/golden/rows_f/region_2k.npz, region growing's fixture.  Run here:
python tests/golden/make_golden_region.py

A 2 000-point scan with two non-finite rows, its normals from the normal estimation's restatement at k = 12 (tests/normals_restated.py)
with three of them made non-finite, grown at k = 12, 30 degrees, curvature threshold 0.05 with the window 3 .. 400: the restatement's
six arrays (tests/region_restated.py) -- region_start, indices, labels, region, kind, anchor.  The window cuts on both sides, every
kind of point occurs, and many emitted regions tie in size.  tests/test_region_host.py checks that the restatement still reproduces
the file; tests/test_gpu_region.py compares the device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import normals_restated as N  # noqa: E402
import region_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "region_2k.npz")
K, THETA_DEG, THRESHOLD, MIN_SIZE, MAX_SIZE = 12, 30.0, 0.05, 3, 400


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    normals = N.estimate(cloud, None, k=K)[0].copy()
    normals[[7, 333, 1200], [0, 3, 2]] = [np.nan, np.inf, np.nan]
    cos = R.smoothness_cos(np.radians(THETA_DEG))
    out = R.grow(cloud, normals, K, cos, THRESHOLD, MIN_SIZE, MAX_SIZE)
    data = {"cloud": cloud, "normals": normals, "k": np.int64(K), "smoothness_cos": np.float32(cos), "curvature_threshold": np.float32(THRESHOLD),
            "min_size": np.int64(MIN_SIZE), "max_size": np.int64(MAX_SIZE)}
    data.update(zip(R.NAMES, out))
    return data


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    sizes = np.diff(data["region_start"])
    all_sizes = np.unique(data["region"][data["region"] >= 0], return_counts=True)[1]
    print("regions", all_sizes.size, "largest", all_sizes.max(), "emitted", sizes.size, "sizes", sizes[:5], "...", sizes[-3:],
          "tied", int(sizes.size - np.unique(sizes).size), "points", data["indices"].size,
          "kinds", {v: int((data["kind"] == v).sum()) for v in (-1, 0, 1, 2)})
    print(os.path.getsize(OUT), "bytes")
