"""Generates tests/golden/rows_f/outlier_2k.npz, the outlier filters' fixture.  Run here:
python tests/golden/make_golden_outlier.py

A 2 000-point scan with three isolated returns and two non-finite rows; for the statistical filter at three mean_k and the radius
filter at three radii: the per-point measure, the statistics' bits and the removed indices, all from the NumPy restatement
(tests/outlier_restated.py).  tests/test_outlier_host.py checks that the restatement still reproduces the file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import outlier_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "outlier_2k.npz")
SOR_CASES = [(1, 0.0), (19, 1.0), (50, 0.25)]
ROR_CASES = [(0.05, 1), (0.3, 5), (2.0, 40)]


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[[10, 900, 1999], :3] = np.float32([[300, 0, 0], [0, -700, 4], [1000, 10, 0]])
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    out = {"cloud": cloud, "sor_cases": np.array(SOR_CASES, np.float64), "ror_cases": np.array(ROR_CASES, np.float64)}
    for i, (k, mult) in enumerate(SOR_CASES):
        r = R.statistical_outlier_removal(cloud, k, mult)
        out[f"sor{i}_dist"] = r["measure"]
        out[f"sor{i}_stats"] = np.array([r["mean"], r["stddev"], r["threshold"]], np.float64).view(np.uint64)
        out[f"sor{i}_n_valid"] = np.int64(r["n_valid"])
        out[f"sor{i}_removed"] = r["removed"]
    for i, (radius, min_pts) in enumerate(ROR_CASES):
        r = R.radius_outlier_removal(cloud, radius, int(min_pts))
        out[f"ror{i}_k"] = r["k"].astype(np.int32)
        out[f"ror{i}_removed"] = r["removed"]
    return out


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    for k in sorted(data):
        if k.endswith("_removed"):
            print(k, len(data[k]))
