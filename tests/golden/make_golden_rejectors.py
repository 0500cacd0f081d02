"""Generates tests/golden/rows_f/rejectors_1k5.npz, the correspondence rejectors' fixture.  Run here:
python tests/golden/make_golden_rejectors.py

A 1.5k-point pair; for each rejector alone and two chains: the kept correspondences at a fixed transform and the whole alignments
of both methods, all from the NumPy restatement (tests/rejectors_restated.py) over the oracle's pinned primitives.
tests/test_rejectors_host.py checks that the restatement still reproduces the file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rejectors_restated as R  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "rejectors_1k5.npz")
CHAINS = {
    "median": [(R.MEDIAN, 1.0, 0)],
    "trimmed": [(R.TRIMMED, 0.5, 0)],
    "one_to_one": [(R.ONE_TO_ONE, 0.0, 0)],
    "median_one_to_one": [(R.MEDIAN, 2.0, 0), (R.ONE_TO_ONE, 0.0, 0)],
    "one_to_one_trimmed": [(R.ONE_TO_ONE, 0.0, 0), (R.TRIMMED, 0.75, 10)],
}
SEED = 41


def fixture():
    src, tgt, _ = synth.make_pair(1500, 1500, seed=SEED)
    T_fixed = synth.pose_matrix(0.05, -0.02, 0.01, 0.0, 0.0, 0.01).astype(np.float32)
    out = {"src": src, "tgt": tgt, "T_fixed": T_fixed}
    for name, chain in CHAINS.items():
        idx, d2, stats = R.correspondences(src, tgt, T_fixed, 1.0, chain)
        out[f"{name}_chain"] = np.array(chain, np.float64)
        out[f"{name}_idx"] = idx
        out[f"{name}_stats"] = np.array([[s["pairs_in"], s["pairs_out"], np.float32(s["cut"]).view(np.uint32)] for s in stats], np.int64)
        for method in ("p2p", "p2plane"):
            r = R.align(src, tgt, chain, method=method)
            out[f"{name}_{method}_T"] = r["T"]
            out[f"{name}_{method}_result"] = np.array([r["iterations"], r["state"], r["n_corr"], int(r["converged"])], np.int64)
    return out


if __name__ == "__main__":
    data = fixture()
    np.savez_compressed(OUT, **data)
    for k in sorted(data):
        if k.endswith("_result"):
            print(k, data[k])
