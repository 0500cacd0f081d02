"""Generates tests/golden/rows_f/sampling_2k.npz, the cropping and sampling filters' fixture.  Run here:
python tests/golden/make_golden_sampling.py

A 2 000-return scan with three non-finite rows and forty duplicated ones; PassThrough on z in both modes, CropBox of 18 m x 12 m x 3 m
with and without a transform in both modes, UniformSampling at three leaves and FarthestPointSampling at 1, 64 and 300 samples: the
kept indices and the measures, all from the NumPy restatement (tests/sampling_restated.py).  tests/test_sampling_host.py checks that
the restatement still reproduces the file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sampling_cases as SC  # noqa: E402
import sampling_restated as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "sampling_2k.npz")
Z_LIMITS = (-1.2, 2.0)
CROP_MIN, CROP_MAX = (-8.0, -6.0, -2.0), (10.0, 6.0, 1.0)
CROP_POSE = dict(translation=(0.4, -0.2, 0.1), rotation=(0.02, -0.03, 0.3))
LEAVES = (0.25, 1.0, 8.0)
FPS_CASES = ((1, -1), (64, -1), (300, 1234))


def cloud():
    c = SC.scan(2000, 5).copy()
    c[[7, 64, 1999], :3] = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf]])
    c[1000:1040, :3] = c[100:140, :3]
    return c


def fixture():
    c = cloud()
    T = R.crop_box_matrix(None, **CROP_POSE)
    out = {"cloud": c, "z_limits": np.float32(Z_LIMITS), "crop_T": T, "crop_min": np.float32(CROP_MIN), "crop_max": np.float32(CROP_MAX),
           "leaves": np.float32(LEAVES), "fps_cases": np.int64(FPS_CASES)}
    for neg in (0, 1):
        out[f"pass{neg}_kept"] = R.pass_through(c, 2, *Z_LIMITS, negative=neg)
        out[f"crop{neg}_kept"] = R.crop_box(c, CROP_MIN, CROP_MAX, None, neg)
        out[f"cropT{neg}_kept"] = R.crop_box(c, CROP_MIN, CROP_MAX, T, neg)
    for i, leaf in enumerate(LEAVES):
        out[f"uniform{i}_kept"], out[f"uniform{i}_measure"] = R.uniform_sampling(c, leaf)
    for i, (k, first) in enumerate(FPS_CASES):
        out[f"fps{i}_kept"], out[f"fps{i}_measure"] = R.farthest_point_sampling(c, k, first)
    return out


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    for k in sorted(data):
        if k.endswith("_kept"):
            print(k, len(data[k]))
