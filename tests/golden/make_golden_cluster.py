"""Generates tests/golden/rows_f/cluster_2k.npz, euclidean clustering's fixture.  Run here:
python tests/golden/make_golden_cluster.py

A 2 000-point scan with three isolated returns and two non-finite rows, clustered at tolerance 0.5 m with the window 3 .. 400: the
restatement's four arrays (tests/cluster_restated.py) -- cluster_start, indices, labels, component.  The window cuts on both sides:
singletons and pairs are dropped and so is the one component of more than 400 points, and dozens of the emitted clusters tie in
size.  tests/test_cluster_host.py checks that the restatement still reproduces the file; tests/test_gpu_cluster.py compares the device
with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cluster_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "cluster_2k.npz")
TOLERANCE, MIN_SIZE, MAX_SIZE = 0.5, 3, 400


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[[10, 900, 1999], :3] = np.float32([[300, 0, 0], [0, -700, 4], [1000, 10, 0]])
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    start, indices, labels, component = R.extract(cloud, TOLERANCE, MIN_SIZE, MAX_SIZE)
    return {"cloud": cloud, "tolerance": np.float64(TOLERANCE), "min_size": np.int64(MIN_SIZE), "max_size": np.int64(MAX_SIZE),
            "cluster_start": start, "indices": indices, "labels": labels, "component": component}


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    sizes = np.diff(data["cluster_start"])
    all_sizes = np.unique(data["component"][data["component"] >= 0], return_counts=True)[1]
    print("components", all_sizes.size, "largest", all_sizes.max(), "clusters", sizes.size, "sizes", sizes[:5], "...", sizes[-3:],
          "tied", int(sizes.size - np.unique(sizes).size), "points", data["indices"].size)
    print(os.path.getsize(OUT), "bytes")
