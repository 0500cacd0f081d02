"""Generates tests/golden/rows_f/boundary_2k.npz and iss_border_2k.npz, the fixtures of the boundary estimation and of ISS with
border estimation.  Run here: python tests/golden/make_golden_boundary.py

boundary_2k: a 2 000-point scan with two non-finite rows, three isolated returns and ten duplicated points; its restated normals
from 12 neighbours, one of them zeroed and one NaN; the restatement's outputs (tests/boundary_restated.py) for k = 30 at pi / 2 and
for a radius of 1.5 m at 2.5 rad.
iss_border_2k: the same cloud at salient radius 1.5, non-max radius 1.0, PCL's default gammas, 20 neighbours, border radius 1.2, the
threshold 2.5 rad and the normals above: the outputs of tests/iss_border_restated.py.  min_neighbors and the border keep most
scatter rows zero, and the file small.
tests/test_boundary_host.py checks that the restatements still reproduce the files; tests/test_gpu_boundary.py and
tests/test_gpu_iss_border.py compare the device with them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import boundary_restated as B  # noqa: E402
import iss_border_restated as IB  # noqa: E402
import normals_restated as N  # noqa: E402
from icpslam_amd import synth  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f")
K, K_ANGLE, RADIUS, RADIUS_ANGLE = 30, np.pi / 2, 1.5, 2.5
ISS = dict(salient_radius=1.5, non_max_radius=1.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=20, border_radius=1.2, angle_threshold=2.5)


def cloud_and_normals():
    cloud = synth.scan(synth.make_scene(3), np.eye(4), 2000, 9).copy()
    cloud[[10, 900, 1999], :3] = np.float32([[300, 0, 0], [0, -700, 4], [1000, 10, 0]])
    cloud[64, 0] = np.nan
    cloud[1500, 2] = np.inf
    cloud[100:110] = cloud[1200:1210]
    normals = N.estimate(cloud, None, 12, 0.0)[0].copy()
    normals[300, :3] = 0.0
    normals[301, 1] = np.nan
    return cloud, normals


def fixtures():
    cloud, normals = cloud_and_normals()
    a = B.estimate(cloud, None, normals, K, 0.0, K_ANGLE)
    b = B.estimate(cloud, None, normals, 0, RADIUS, RADIUS_ANGLE)
    boundary = {"cloud": cloud, "normals": normals, "k": np.int64(K), "k_angle": np.float64(K_ANGLE), "radius": np.float64(RADIUS),
                "radius_angle": np.float64(RADIUS_ANGLE)}
    boundary.update({f"k_{f}": a[f] for f in B.FIELDS})
    boundary.update({f"radius_{f}": b[f] for f in B.FIELDS})
    got = IB.keypoints_border(cloud, normals=normals, **ISS)
    iss = {"cloud": cloud, "normals": normals, "n_keypoints": np.int64(got["n_keypoints"])}
    iss.update({name: np.float64(v) if isinstance(v, float) else np.int64(v) for name, v in ISS.items()})
    iss.update({f: got[f] for f in IB.FIELDS})
    return boundary, iss


if __name__ == "__main__":
    boundary, iss = fixtures()
    for name, data in (("boundary_2k.npz", boundary), ("iss_border_2k.npz", iss)):
        np.savez_compressed(os.path.join(HERE, name), **data)
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")
    print("boundary points", int(boundary["k_boundary"].sum()), int(boundary["radius_boundary"].sum()), "edge", int(iss["edge"].sum()), "border",
          int(iss["border"].sum()), "keypoints", int(iss["n_keypoints"]))
