#!/usr/bin/env python3
"""The split small-batch scorer (k_lo_resid + k_lo_fold through gcr_debug_score,
GCR_DEBUG_SCORER=small) on the bench's M2 problem (5000 + 5000 features) for
128 and 256 generated hypotheses with a valid model -- what a list of the
bound path holds.  Run it under `rocprofv3 --kernel-trace --stats` and read the
two kernels' mean dispatch per model count from the trace (two warm-up calls,
then REPS calls per count; the dispatches come in that order).  It prints the
wall time per call as well."""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "graph-cut-ransac_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
os.environ["GCR_DEBUG_SCORER"] = "small"

import numpy as np  # noqa: E402

from gcr_testutil import Problem  # noqa: E402
from pygcransac import _native as N  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

REPS = int(os.environ.get("REPS", "10"))
fs, fo, _, _, t0, t1 = S.problem_m2(5000, 5000, seed=20251121)
prob = Problem(N.SOLVER_SIFT22, fs, fo)
inc, models = prob.generate(20251121, 0, 4096)
ok = (inc <= 101) & (np.maximum(np.abs(models[:, 3]), np.abs(models[:, 4])) < 1e-3)    # valid_model_sift22
live = models[ok]
print("valid models:", len(live), flush=True)
for nm in (256, 128):
    ms = live[:nm]
    for _ in range(2):
        n0, n1, _, _, _ = prob.score_raw(ms, t0, t1)
    ts = []
    for _ in range(REPS):
        a = time.perf_counter()
        prob.score_raw(ms, t0, t1)
        ts.append((time.perf_counter() - a) * 1e6)
    print(f"models {nm:3d}: inliers a model {float((n0 + n1).mean()):7.1f}  wall median {statistics.median(ts):8.1f} us",
          flush=True)
