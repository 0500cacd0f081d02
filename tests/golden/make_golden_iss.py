"""Generates tests/golden/rows_f/iss_2k.npz, the ISS keypoints' fixture.  Run here:
python tests/golden/make_golden_iss.py

A 2 000-point scan with two non-finite rows, three isolated returns and ten duplicated points, at salient and non-max radius
1.5 m, PCL's default gammas (0.975) and 52 neighbours: the restatement's outputs (tests/iss_restated.py) -- the keypoint indices and
points, n_salient, scatter6, eigenvalues3 and saliency.  min_neighbors sits above the median ball size (40), so the threshold cuts
through the middle of the cloud, on both the salient and the non-max ball, and the skipped half's zeros keep the file within the size
of the other fixtures here.  tests/test_iss_host.py checks that the restatement still reproduces the file;
tests/test_gpu_iss.py compares the device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import iss_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "iss_2k.npz")
SALIENT, NON_MAX, GAMMA_21, GAMMA_32, MIN_NEIGHBORS = 1.5, 1.5, 0.975, 0.975, 52


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[[10, 900, 1999], :3] = np.float32([[300, 0, 0], [0, -700, 4], [1000, 10, 0]])
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    cloud[100:110] = cloud[1200:1210]
    got = R.keypoints(cloud, SALIENT, NON_MAX, GAMMA_21, GAMMA_32, MIN_NEIGHBORS)
    data = {"cloud": cloud, "salient_radius": np.float64(SALIENT), "non_max_radius": np.float64(NON_MAX), "gamma_21": np.float64(GAMMA_21),
            "gamma_32": np.float64(GAMMA_32), "min_neighbors": np.int64(MIN_NEIGHBORS), "n_keypoints": np.int64(got["n_keypoints"])}
    data.update({f: got[f] for f in R.FIELDS})
    return data


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    print("keypoints", int(data["n_keypoints"]), "salient points", int((data["saliency"] > 0).sum()), "ball sizes", data["n_salient"].min(),
          "..", data["n_salient"].max(), "below min_neighbors", int((data["n_salient"] < MIN_NEIGHBORS).sum()))
    print(os.path.getsize(OUT), "bytes")
