"""Generates tests/golden/rows_f/normals_2k.npz, the normal estimation's fixture.  Run here:
python tests/golden/make_golden_normals.py

A 2 000-point scan with three isolated returns and two non-finite rows; at k = 20 and at radius 0.8 m, towards the viewpoint
(0.5, -0.25, 1.0): the neighbour counts of every point, the normals {nx, ny, nz, curvature} of every second point and the moments of
every eighth (float noise does not compress: the whole arrays would make the file three times the size of the largest fixture
beside it), all from the NumPy restatement (tests/normals_restated.py).  tests/test_normals_host.py checks that the restatement still
reproduces the file; tests/test_gpu_normal_estimation.py compares the device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import normals_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "normals_2k.npz")
K, RADIUS, VIEWPOINT = 20, 0.8, (0.5, -0.25, 1.0)


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[[10, 900, 1999], :3] = np.float32([[300, 0, 0], [0, -700, 4], [1000, 10, 0]])
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    out = {"cloud": cloud, "k": np.int64(K), "radius": np.float64(RADIUS), "viewpoint": np.array(VIEWPOINT, np.float32)}
    for name, kw in (("k", dict(k=K)), ("r", dict(radius=RADIUS))):
        normals, counts, moments = R.estimate(cloud, None, viewpoint=VIEWPOINT, **kw)
        out[f"{name}_normals"], out[f"{name}_counts"], out[f"{name}_moments"] = normals[::2], counts, moments[::8]
    return out


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    for name in ("k", "r"):
        c = data[f"{name}_counts"]
        print(name, "rows", c.min(), np.median(c), c.max(), "NaN normals", int(np.isnan(data[f"{name}_normals"][:, 0]).sum()))
    print(os.path.getsize(OUT), "bytes")
