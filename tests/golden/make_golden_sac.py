"""Generates tests/golden/rows_f/sac_2k.npz, the plane segmentation's fixture.  Run here:
python tests/golden/make_golden_sac.py

A 2 000-point scan with two non-finite rows and three far returns, segmented at a threshold of 0.12 m with PCL's defaults (50
iterations, probability 0.99, the refinement on): what the restatement (tests/sac_restated.py) computes at every stage -- the counts of
every iteration, the best hypothesis and its sample, the unrefined coefficients and inlier count, the refinement's nine sums, the
refined coefficients and the final inliers.  tests/test_sac_host.py checks that the restatement still reproduces the file;
tests/test_gpu_sac.py compares the device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sac_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "sac_2k.npz")
THRESHOLD, MAX_ITERATIONS, PROBABILITY, SEED = 0.12, 50, 0.99, 2


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[[10, 900, 1999], :3] = np.float32([[300, 0, 0], [0, -700, 4], [1000, 10, 0]])
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    r = R.segment(cloud, THRESHOLD, MAX_ITERATIONS, PROBABILITY, SEED, True)
    out = {"cloud": cloud, "threshold": np.float64(THRESHOLD), "max_iterations": np.int64(MAX_ITERATIONS), "probability": np.float64(PROBABILITY),
           "seed": np.int64(SEED)}
    for name in ("counts", "sample", "coeff_unrefined", "moments", "coeff", "inliers"):
        out[name] = r[name]
    for name in ("iterations", "best_t", "n_unrefined", "found"):
        out[name] = np.int64(r[name])
    return out


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    print("iterations", int(data["iterations"]), "best_t", int(data["best_t"]), "unrefined inliers", int(data["n_unrefined"]), "inliers",
          data["inliers"].size, "coefficients", data["coeff_unrefined"], "->", data["coeff"], "invalid", int((data["counts"] < 0).sum()))
    print(os.path.getsize(OUT), "bytes")
