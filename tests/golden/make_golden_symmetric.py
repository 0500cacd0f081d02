"""Generates tests/golden/rows_f/symmetric_1k5.npz, the fixture of the symmetric point-to-plane objective and the surface-normal
rejector.  Run here (needs scipy, mpmath and the built library, whose host solve the restatement calls):
python tests/golden/make_golden_symmetric.py

Expected values come from the NumPy restatement (tests/symmetric_restated.py) over the C oracle's search and normals
(oracle.nn, oracle.gicp_normals): a plain symmetric alignment from a guess, and one with the surface-normal rejector at 0.5 in its
chain.  The generator refuses to write a fixture whose deciding quantities sit at a threshold (symmetric_restated.decisions_clear).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
import symmetric_restated as S  # noqa: E402
from icpslam_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "rows_f", "symmetric_1k5.npz")


def main():
    src, tgt, _ = synth.make_pair(1500, 1500, seed=31)
    guess = synth.pose_matrix(0.05, -0.02, 0.01, 0.0, 0.0, 0.01).astype(np.float32)
    sn, tn = oracle.gicp_normals(src), oracle.gicp_normals(tgt)
    out = {"src": src, "tgt": tgt, "guess": guess, "src_nrm": sn, "tgt_nrm": tn}
    for name, chain in (("plain", ()), ("rej", ((S.SURFACE_NORMAL, 0.5),))):
        r = S.align(src, tgt, sn, tn, chain=chain, guess=guess)
        assert S.decisions_clear(r), name
        out.update({f"{name}_T": r["T"], f"{name}_iterations": r["iterations"], f"{name}_state": r["state"],
                    f"{name}_n_corr": r["n_corr"], f"{name}_mse": r["mse"],
                    f"{name}_sums": np.array([t["sums"] for t in r["trace"]]).reshape(-1, 29)})
        if chain:
            out[f"{name}_stats"] = np.array([[s["pairs_in"], s["pairs_out"]] for s in r["stats"]], np.int64)
        print(name, "iters", r["iterations"], "state", r["state"], "n_corr", r["n_corr"], "stats", [(s["pairs_in"], s["pairs_out"]) for s in r["stats"]])
    np.savez_compressed(OUT, **out)
    print(os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
