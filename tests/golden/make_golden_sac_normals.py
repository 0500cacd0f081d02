"""Generates tests/golden/rows_f/sac_normals_2k.npz, the fixture of the segmentation from normals.  Run here:
python tests/golden/make_golden_sac_normals.py

2 000 points of the synthetic street of tests/sac_normals_cases.py (a crowned ground, boxes, three poles) with a NaN point, an infinite
point and a NaN normal planted in them, and the normals of tests/normals_restated.py over 12 neighbours: what the restatement
(tests/sac_normals_restated.py) computes at every stage for SACMODEL_NORMAL_PLANE and for SACMODEL_CYLINDER with a vertical axis and
radius limits -- the counts of every iteration, the best hypothesis and its sample, the unrefined coefficients and inlier count, the
refinement's sums, the refined coefficients and the final inliers.  tests/test_sac_normals_host.py checks that the restatement still
reproduces the file; tests/test_gpu_sac_normals.py compares the device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import normals_restated as NR  # noqa: E402
import sac_normals_cases as CS  # noqa: E402
import sac_normals_restated as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "sac_normals_2k.npz")
# threshold, weight, radius_min, radius_max, max_iterations, probability, seed, eps_angle
ARGS = {"plane": (0.08, 0.1, 0.0, 0.0, 100, 0.99, 2, 0.0), "cyl": (0.03, 0.1, 0.05, 0.3, 400, 0.99, 2, 0.1)}
NAMES = ("counts", "sample", "coeff_unrefined", "moments", "cylinder_sums", "coeff", "inliers")


def fixture():
    full = CS.street(1)[0]
    keep = np.sort(np.random.default_rng(3).choice(full.shape[0], 2000, replace=False))
    cloud = full[keep].copy()
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    normals = NR.estimate(cloud, None, k=12, viewpoint=(0.0, 0.0, 3.0))[0]
    normals[700, 1] = np.nan
    out = {"cloud": cloud, "normals": normals}
    for tag, model in (("plane", R.NORMAL_PLANE), ("cyl", R.CYLINDER)):
        a = ARGS[tag]
        r = R.segment(model, cloud, normals, a[0], a[1], a[2], a[3], a[4], a[5], a[6], True, None if tag == "plane" else (0.0, 0.0, 1.0), a[7])
        out[tag + "_args"] = np.array(a, np.float64)
        for name in NAMES:
            out[f"{tag}_{name}"] = r[name]
        for name in ("iterations", "best_t", "n_unrefined", "found", "cylinder_stop"):
            out[f"{tag}_{name}"] = np.int64(r[name])
    return out


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    for tag in ("plane", "cyl"):
        print(tag, "iterations", int(data[tag + "_iterations"]), "best_t", int(data[tag + "_best_t"]), "unrefined", int(data[tag + "_n_unrefined"]),
              "inliers", data[tag + "_inliers"].size, data[tag + "_coeff_unrefined"], "->", data[tag + "_coeff"], "invalid",
              int((data[tag + "_counts"] < 0).sum()), "stop", int(data[tag + "_cylinder_stop"]), "passes", data[tag + "_cylinder_sums"].shape[0])
    print(os.path.getsize(OUT), "bytes")
