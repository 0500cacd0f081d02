"""Generates tests/golden/rows_f/p2plane_1k5.npz, the point-to-plane fixture.  Run here (needs scipy, mpmath):
python tests/golden/make_golden_p2plane.py

Expected values come from the NumPy restatement (oracle/icp_oracle_np.py: p2plane_align), with the normals from the C oracle's
estimate (oracle.gicp_normals, itself pinned to gicp_oracle_np.normals) and a second, supplied set.  tests/test_oracle.py checks
the C restatement (oracle/p2plane_oracle.c) against it.  (Beside, not in, tests/golden/*.npz: those are the point-to-point set.)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from icpslam_amd import synth  # noqa: E402
from oracle import icp_oracle_np as onp  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows_f", "p2plane_1k5.npz")


def main():
    src, tgt, _ = synth.make_pair(1500, 1500, seed=31)
    guess = synth.pose_matrix(0.05, -0.02, 0.01, 0.0, 0.0, 0.01).astype(np.float32)
    est = oracle.gicp_normals(tgt)
    sup = est.copy()
    sup[::7, :3] *= np.float32(3.0)                                   # not unit length
    sup[::11, 1] = np.nan                                             # one NaN component: the pair is skipped
    out = {"src": src, "tgt": tgt, "guess": guess}
    for name, nrm in (("est", est), ("sup", sup)):
        r = onp.p2plane_align(src, tgt, nrm, guess=guess, want_fitness=True)
        out.update({f"{name}_nrm": nrm, f"{name}_T": r["T"], f"{name}_iterations": r["iterations"], f"{name}_state": r["state"],
                    f"{name}_n_corr": r["n_corr"], f"{name}_mse": r["mse"], f"{name}_fitness": r["fitness"],
                    f"{name}_sums": np.array([t["sums"] for t in r["trace"]]).reshape(-1, 29)})
        print(name, "iters", r["iterations"], "state", r["state"], "n_corr", r["n_corr"])
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    main()
