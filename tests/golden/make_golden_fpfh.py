"""Generates tests/golden/rows_f/fpfh_512.npz, the fast point feature histograms' fixture.  Run here:
python tests/golden/make_golden_fpfh.py

A 512-point scan with two isolated returns, a duplicated point and one non-finite row, its normals (k = 12, from
tests/normals_restated.py, with one NaN normal of their own); at k = 10 and at radius 0.9 m: the neighbour counts, the SPFH and the
FPFH of every point, all from the NumPy restatement (tests/fpfh_restated.py).
tests/test_fpfh_host.py checks that the restatement still reproduces the file; tests/test_gpu_fpfh.py compares the device with it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fpfh_restated as R  # noqa: E402
import normals_restated as N  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "fpfh_512.npz")
K, RADIUS, NORMALS_K = 10, 0.9, 12


def fixture():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 512, 9).copy()
    cloud[[10, 511], :3] = np.float32([[300, 0, 0], [0, -700, 4]])
    cloud[100] = cloud[37]
    cloud[64, 0] = np.nan
    normals = N.estimate(cloud, None, k=NORMALS_K)[0].copy()
    normals[200, 1] = np.nan
    out = {"cloud": cloud, "normals": normals, "k": np.int64(K), "radius": np.float64(RADIUS)}
    for name, kw in (("k", dict(k=K)), ("r", dict(radius=RADIUS))):
        fpfh, counts, spfh = R.estimate(cloud, normals, None, **kw)
        out[f"{name}_fpfh"], out[f"{name}_counts"], out[f"{name}_spfh"] = fpfh, counts, spfh
    return out


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    for name in ("k", "r"):
        c = data[f"{name}_counts"]
        print(name, "rows", c.min(), np.median(c), c.max(), "NaN fpfh", int(np.isnan(data[f"{name}_fpfh"][:, 0]).sum()))
    print(os.path.getsize(OUT), "bytes")
