#!/usr/bin/env python3
"""Descriptor matching at the shape of a real image pair: n1 = n2 = 10 000
uint8 descriptors of dim 128 (uniform random bytes, seeded).

  1  gcr_match_descriptors: the kernels' time (HIP events, ms_kernel_out) and
     the whole call's (host clock; upload, kernels, download), each the median
     of --calls calls after a warm-up call; the kernels' int8 MAC/s
     (n1 * n2 * dim over the kernel time) beside the matrix cores' dense int8
     peak; the same with the column split pinned (--splits, GCR_MATCH_SPLIT)
  2  the host twin (gcr_host_match_descriptors) on --threads threads and
     whether the two agree bit for bit
  3  the numpy float32 formulation |a|^2 + |b|^2 - 2 a.b on the BLAS (exact
     for dim <= 258: every value below 2^24), in row blocks, with its top-2;
     whether it agrees
  4  end to end on problem_match(10 000, 4000): match_descriptors(ratio=None,
     mutual=False) + findHomography(sampler=1, probabilities=-ratios) beside
     the estimator call alone, the median of --calls calls each, alternating

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "graph-cut-ransac_amd"))
ap.add_argument("--n", type=int, default=10_000)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--calls", type=int, default=11)
ap.add_argument("--threads", type=int, default=16, help="host twin's threads")
ap.add_argument("--host-runs", type=int, default=3)
ap.add_argument("--splits", default="0,1,2,4,7,16", help="column splits to time (GCR_MATCH_SPLIT), 0 = the planner's")
ap.add_argument("--no-pipeline", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.pkg)
import pygcransac  # noqa: E402
from pygcransac import _native as N  # noqa: E402
from pygcransac import features as F  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

# dense int8 matrix-core peak: twice the BF16 rate per clock (~2.5 PFLOP/s dense), in MAC/s
PEAK_I8_MAC_PER_S = 2.5e15
SEED = 20260305
n, dim = args.n, args.dim
rng = np.random.default_rng(SEED)
d1 = rng.integers(0, 256, (n, dim), dtype=np.uint8)
d2 = rng.integers(0, 256, (n, dim), dtype=np.uint8)
ctx = N.context(0)
out = {"pkg": args.pkg, "build_id": N.lib.gcr_kernel_build_id().decode(), "n1": n, "n2": n, "dim": dim,
       "calls": args.calls}


def quart(v):
    qs = statistics.quantiles(v, n=4) if len(v) > 1 else [v[0]] * 3
    return {"median_ms": round(statistics.median(v), 4), "q1_ms": round(qs[0], 4), "q3_ms": round(qs[2], 4),
            "ms": [round(x, 4) for x in v]}


def gpu_call(res, ms):
    t0 = time.perf_counter()
    N.check(N.lib.gcr_match_descriptors(ctx, d1.ctypes.data, n, d2.ctypes.data, n, dim,
                                        *[r.ctypes.data for r in res], C.byref(ms)))
    return (time.perf_counter() - t0) * 1e3           # the call ends in a stream synchronisation


# ---- leg 1 ---------------------------------------------------------------------
gpu = [np.empty(n, dtype=np.uint32) for _ in range(4)]
ms = C.c_double()
legs = {}
for s in [int(v) for v in args.splits.split(",")]:
    if s:
        os.environ["GCR_MATCH_SPLIT"] = str(s)
    else:
        os.environ.pop("GCR_MATCH_SPLIT", None)
    res = [np.empty(n, dtype=np.uint32) for _ in range(4)]
    gpu_call(res, ms)                                 # warm-up
    kern, whole = [], []
    for _ in range(args.calls):
        whole.append(gpu_call(res, ms))
        kern.append(ms.value)
    if s == 0:
        gpu = res
    k = quart(kern)
    legs[f"split{s}"] = {"kernel": k, "call": quart(whole),
                         "mac_per_s": round(n * n * dim / (k["median_ms"] * 1e-3)),
                         "share_of_i8_peak": round(n * n * dim / (k["median_ms"] * 1e-3) / PEAK_I8_MAC_PER_S, 4),
                         "equals_planner_split_bitwise": all(np.array_equal(a, b) for a, b in zip(res, gpu))}
os.environ.pop("GCR_MATCH_SPLIT", None)
out["gpu"] = legs
out["i8_peak_mac_per_s"] = PEAK_I8_MAC_PER_S

# ---- leg 2 ---------------------------------------------------------------------
host = [np.empty(n, dtype=np.uint32) for _ in range(4)]
hs = []
for _ in range(args.host_runs):
    t0 = time.perf_counter()
    N.check(N.lib.gcr_host_match_descriptors(d1.ctypes.data, n, d2.ctypes.data, n, dim, args.threads,
                                             *[h.ctypes.data for h in host]))
    hs.append((time.perf_counter() - t0) * 1e3)
out["host_twin"] = {"threads": args.threads, **quart(hs),
                    "equals_gpu_bitwise": all(np.array_equal(a, b) for a, b in zip(host, gpu))}

# ---- leg 3 ---------------------------------------------------------------------
if dim <= 258:
    t0 = time.perf_counter()
    a, b = d1.astype(np.float32), d2.astype(np.float32)
    na, nb = (a * a).sum(1), (b * b).sum(1)
    ref = [np.empty(n, dtype=np.uint32) for _ in range(4)]
    for lo in range(0, n, 1000):
        d = na[lo:lo + 1000, None] + nb[None, :] - 2.0 * (a[lo:lo + 1000] @ b.T)
        rows = np.arange(len(d))
        j1 = d.argmin(1)                              # the first minimum: the lower index on a tie
        ref[0][lo:lo + 1000], ref[1][lo:lo + 1000] = j1, d[rows, j1]
        d[rows, j1] = np.inf
        j2 = d.argmin(1)
        ref[2][lo:lo + 1000], ref[3][lo:lo + 1000] = j2, d[rows, j2]
    out["numpy_float32"] = {"ms": round((time.perf_counter() - t0) * 1e3, 2),
                            "equals_gpu_bitwise": all(np.array_equal(x, y) for x, y in zip(ref, gpu))}

# ---- leg 4 ---------------------------------------------------------------------
if not args.no_pipeline:
    kp1, e1, kp2, e2, pairs, _ = S.problem_match(n, int(0.4 * n), seed=SEED, dim=dim)
    size = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)
    truth = set(map(tuple, pairs.tolist()))
    m, r = F.match_descriptors(e1, e2, ratio=None, mutual=False)
    corr = F.correspondences_from_matches(kp1, kp2, m)
    true = np.array([tuple(x) in truth for x in m.tolist()])
    kw = dict(threshold=2.0, conf=0.99, max_iters=10**6, min_iters=50, sampler=1)

    def estimator(seed):
        return pygcransac.findHomography(corr, *size, probabilities=-r, seed=seed, **kw)

    def pipeline(seed):
        mm, rr = F.match_descriptors(e1, e2, ratio=None, mutual=False)
        cc = F.correspondences_from_matches(kp1, kp2, mm)
        return pygcransac.findHomography(cc, *size, probabilities=-rr, seed=seed, **kw)

    acc = {"estimator_alone": ([], []), "match_and_estimator": ([], [])}
    for k in range(-1, args.calls):                   # call -1 warms up
        for name, fn in (("estimator_alone", estimator), ("match_and_estimator", pipeline)):
            t0 = time.perf_counter()
            H, mask = fn(100 + k)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 0:
                acc[name][0].append(dt)
                acc[name][1].append(int((np.asarray(mask).astype(bool) & true).sum()))
    out["pipeline"] = {name: {**quart(v[0]), "truth_inliers_found": v[1], "truth_pairs": len(pairs)}
                       for name, v in acc.items()}
    out["pipeline"]["matches"] = len(m)
print(json.dumps(out))
