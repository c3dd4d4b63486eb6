#!/usr/bin/env python3
"""Generate tests/golden/samplers/*.npz: whole runs under PROSAC (with and
without its own stop) and NAPSAC sampling, and of the homography from two SIFT
correspondences, recorded from the CPU oracle (its run loop and its
restatements of csrc/prosac.h, csrc/prosac_stop.h and csrc/napsac.h;
tests/sampler_run_cases.run_oracle).

No reference exists for these modes, so the files are recorded results: they
pin the oracle and the product together against drifting in step.  Each holds
the rows in the caller's order, the quality scores of a PROSAC run, the
calibration of an essential-matrix run, the parameters, the packed mask (in the
caller's order), the model and the run statistics.  Needs no GPU.

usage: python tools/gen_sampler_golden.py   (rewrites tests/golden/samplers/)
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "graph-cut-ransac_amd"))

import oracle_ffi as O  # noqa: E402
import sampler_run_cases as SR  # noqa: E402


def main():
    O.build()
    for name in SR.GOLDEN_NAMES:
        p, scores = SR.golden_problem(name)
        kw = SR.GOLDEN_PARAMS[name]
        r = SR.run_oracle(p, scores=scores, **kw)
        SR.save_golden(name, p, scores, kw, r)
        print(name, r["num_inliers"], {k: r["stats"][k] for k in SR.COUNTS}, r.get("prosac_star"))


if __name__ == "__main__":
    main()
