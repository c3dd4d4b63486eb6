#!/usr/bin/env python3
"""Generate tests/golden/calib/*.npz: whole runs of the essential-matrix kinds
recorded from the CPU oracle (its run loop around the product's host solvers,
tests/oracle_ffi.find_essential / find_gravity_essential).

No reference exists for these kinds, so the files are recorded results: they
pin the oracle and the product together against drifting in step.  Each holds
the pixel rows, K1 / K2 (G1 / G2 for the gravity kind), the parameters, the
packed mask, the model and the run statistics.  Needs no GPU.

usage: python tools/gen_calib_golden.py   (rewrites tests/golden/calib/)
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "graph-cut-ransac_amd"))

import calibrated_cases as CC  # noqa: E402
import oracle_ffi as O  # noqa: E402


def main():
    O.build()
    os.makedirs(CC.CALIB_DIR, exist_ok=True)
    for name in CC.CALIB_NAMES:
        p, kw = CC.calib_problem(name), CC.CALIB_PARAMS[name]
        r = CC.run_oracle(p, **kw)
        d = dict(correspondences=p["corr"], thr=np.float64(p["thr"]), K1=p["K"], K2=p["K"],
                 params=np.array([kw[k] for k in CC.PARAM_KEYS], dtype=np.int64),
                 confidence=np.float64(kw["confidence"]), lam=np.float64(kw["lam"]),
                 image_size=np.array(CC.SIZE), num_inliers=np.int64(r["num_inliers"]), M=r["H"],
                 mask=np.packbits(r["mask"].astype(np.uint8)), score=np.float64(r["stats"]["score"]),
                 stats=np.array([r["stats"][k] for k in CC.COUNTS], dtype=np.int64))
        if p["kind"] == "G":
            d.update(G1=p["G1"], G2=p["G2"])
        np.savez_compressed(os.path.join(CC.CALIB_DIR, name + ".npz"), **d)
        print(name, int(d["num_inliers"]), d["stats"])


if __name__ == "__main__":
    main()
