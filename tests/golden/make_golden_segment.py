"""Generates tests/golden/rows_f/segment_2k.npz, the segment moments' fixture.  Run here:
python tests/golden/make_golden_segment.py

A 2 000-point scan with three non-finite rows, cut into the clusters of the clustering's restatement at a tolerance of 0.6 (sizes from 1
to several hundred), followed by five segments of the caller's kind: an empty one, one of only non-finite rows, one that starts with a
non-finite row, one with repeats that overlaps the largest cluster, and the whole cloud in reverse order.  records: the restatement's
(tests/segment_restated.py).  tests/test_segment_host.py checks that the restatement still reproduces the file;
tests/test_gpu_segment.py compares the device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cluster_restated as CR  # noqa: E402
import segment_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "segment_2k.npz")
TOLERANCE = 0.6
BAD = (64, 700, 1500)


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[BAD[0], 0], cloud[BAD[1], 1], cloud[BAD[2], 2] = np.nan, np.inf, -np.inf
    start, idx, _, _ = CR.extract(cloud, TOLERANCE, 1)
    segments = [idx[a:b].tolist() for a, b in zip(start[:-1], start[1:])]
    largest = segments[0]
    segments += [[], list(BAD), [BAD[0]] + largest[:40], largest[:10] * 3 + largest[5:15], list(range(len(cloud) - 1, -1, -1))]
    segment_start, indices = R.csr(segments)
    return {"cloud": cloud, "segment_start": segment_start, "indices": indices, "records": R.records(cloud, segment_start, indices)}


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    sizes = np.diff(data["segment_start"])
    print("segments", sizes.size, "entries", data["indices"].size, "largest", sizes.max(), "of one", int((sizes == 1).sum()),
          "empty", int((data["records"]["status"] == R.EMPTY).sum()))
    print(os.path.getsize(OUT), "bytes")
