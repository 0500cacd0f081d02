"""Generates tests/golden/rows_f/mls_1k.npz, the moving least squares' fixture.  Run here:
python tests/golden/make_golden_mls.py

A 4 000-point scan reduced to about 1 000 points by voxel centroids (NumPy: the centroid of every occupied 0.65 m cell, in the order
of the cells' first points), with one non-finite row, two isolated returns and five duplicated points, at radius 1.5 m and PCL's
default weights: every output of the restatement (tests/mls_restated.py) for orders 2 and 3 -- the kept points, normals and
indices, and per query status, n_neighbours, plane7 and coeff10.  The rows run from one entry to several dozen, so all of status 0,
1 and 2 occur.  tests/test_mls_host.py checks that the restatement still reproduces the file; tests/test_gpu_mls.py compares the
device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mls_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "mls_1k.npz")
LEAF, RADIUS, SQR_GAUSS_PARAM = 0.65, 1.5, 0.0


def voxel_centroids(cloud, leaf):
    xyz = cloud[:, :3].astype(np.float64)
    cell = np.floor(xyz / leaf).astype(np.int64)
    _, first, inverse = np.unique(cell, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    sums = np.zeros((len(first), 3))
    np.add.at(sums, inverse, xyz)
    out = np.ones((len(first), 4), np.float32)
    out[:, :3] = (sums / np.bincount(inverse)[:, None]).astype(np.float32)
    return out[np.argsort(first)]


def fixture():
    cloud = voxel_centroids(synth.scan(synth.make_scene(3), np.eye(4), 4000, 9), LEAF)
    cloud[[10, 700], :3] = np.float32([[300, 0, 0], [0, -700, 4]])
    cloud[64, 0] = np.nan
    cloud[100:105] = cloud[600:605]
    data = {"cloud": cloud, "radius": np.float64(RADIUS), "sqr_gauss_param": np.float64(SQR_GAUSS_PARAM)}
    for order in (2, 3):
        got = R.project(cloud, None, RADIUS, order, SQR_GAUSS_PARAM)
        data[f"n_out_{order}"] = np.int64(got["n_out"])
        data.update({f"{f}_{order}": got[f] for f in R.FIELDS})
    return data


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    for order in (2, 3):
        print("order", order, "kept", int(data[f"n_out_{order}"]), "of", len(data["cloud"]), "status", np.bincount(data[f"status_{order}"], minlength=4),
              "rows", data[f"n_neighbours_{order}"].min(), "..", data[f"n_neighbours_{order}"].max())
    print(os.path.getsize(OUT), "bytes")
