#!/usr/bin/env python3
"""The essential-matrix estimator with known gravity at the configs[3] shape:
problem_g (problem_e's scene seen by cameras whose relative rotation is about
the vertical), N = 10 000, 80 % outliers, 14 848 slots per launch.

  1  the gravity generator's time per launch (HIP events,
     gcr_measure_generate_h) beside the 5-point and the 7-point generators' on
     the same pixels, for the lanes-per-slot settings of --groups (GCR_GEN_G;
     0 = the engine's choice); attempts and live models per slot; the host twin
     of the generator (gcr_host_generate_g) on --threads host threads, its
     slots/s beside the GPU's, and whether the two agree bit for bit
  2  hypotheses/s of gcr_problem_verify_batches for the three estimators
  3  wall time and iterations to 0.99 confidence through
     findGravityEssentialMatrix, findEssentialMatrix and findFundamentalMatrix
     on the same data, the median of --calls calls, the lines alternating call
     by call; truth inliers found

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
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--batches", type=int, default=200, help="launches per timed run")
ap.add_argument("--slots", type=int, default=14848)
ap.add_argument("--calls", type=int, default=11, help="leg 3: timed calls per estimator")
ap.add_argument("--gen-reps", type=int, default=50, help="generator launches per HIP-event window")
ap.add_argument("--groups", default="0,1,2,4,8", help="lanes per slot to time (GCR_GEN_G), 0 = the engine's choice")
ap.add_argument("--threads", type=int, default=16, help="host twin's threads")
ap.add_argument("--no-latency", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.pkg)
import pygcransac  # noqa: E402
from pygcransac import _native as N  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

SEED = 20251121
thr = 1.0
corr, truth, K, G1, G2, E_gt = S.problem_g(10_000, 0.8, seed=SEED)
corr, K, G1, G2 = (np.ascontiguousarray(v) for v in (corr, K, G1, G2))
n = corr.shape[0]
ctx = N.context(0)
dp = C.POINTER(C.c_double)
hg, he, hf = C.c_void_p(), C.c_void_p(), C.c_void_p()
N.check(N.lib.gcr_problem_create_gravity_essential(ctx, corr.ctypes.data, n, K.ctypes.data, K.ctypes.data,
                                                   G1.ctypes.data, G2.ctypes.data, C.byref(hg)))
N.check(N.lib.gcr_problem_create_essential(ctx, corr.ctypes.data, n, K.ctypes.data, K.ctypes.data, C.byref(he)))
N.check(N.lib.gcr_problem_create(ctx, N.SOLVER_FUNDAMENTAL7, corr.ctypes.data_as(dp), n, None, 0, C.byref(hf)))
p = N.default_params()
p.scale_residual_thresh = thr
p.seed = SEED
out = {"pkg": args.pkg, "build_id": N.lib.gcr_kernel_build_id().decode(), "n": n, "slots": args.slots,
       "batches": args.batches, "runs": args.runs}


def gen_ms(h, g):
    if g:
        os.environ["GCR_GEN_G"] = str(g)
    else:
        os.environ.pop("GCR_GEN_G", None)
    ms = C.c_double()
    vals = []
    for _ in range(args.runs):
        N.check(N.lib.gcr_measure_generate_h(h, SEED, 0, args.slots, args.gen_reps, C.byref(ms)))
        vals.append(ms.value)
    os.environ.pop("GCR_GEN_G", None)
    return {"ms_per_launch": [round(v, 5) for v in vals], "median_ms": round(statistics.median(vals), 5)}


# ---- leg 1 ---------------------------------------------------------------------
groups = [int(g) for g in args.groups.split(",")]
out["generator_g"] = {f"G{g}": gen_ms(hg, g) for g in groups}
out["generator_e"] = {"G0": gen_ms(he, 0)}
out["generator_f"] = {"G0": gen_ms(hf, 0)}
inc = np.zeros(args.slots * 4, dtype=np.uint8)
models = np.zeros(args.slots * 36)
N.check(N.lib.gcr_debug_generate_h(hg, SEED, 0, args.slots, inc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   models.ctypes.data_as(dp)))
inc2 = inc.reshape(-1, 4)
ok = inc2[:, 0] <= 101
out["slots_with_a_model"] = int(ok.sum())
out["attempts_per_slot"] = round(float(np.minimum(inc2[:, 0], 101).mean()), 4)
out["live_models_per_slot"] = round(float((ok + (inc2[:, 1:] == 0).sum(axis=1)).mean()), 4)
norm = np.zeros_like(corr)
N.check(N.lib.gcr_host_essential_normalise(corr.ctypes.data, n, K.ctypes.data, K.ctypes.data, thr, norm.ctypes.data,
                                           None))
hinc = np.zeros_like(inc)
hmodels = np.zeros_like(models)
host_s = []
for _ in range(args.runs):
    t0 = time.perf_counter()
    N.check(N.lib.gcr_host_generate_g(norm.ctypes.data, n, G1.ctypes.data, G2.ctypes.data, None, SEED, 0, args.slots,
                                      args.threads, hinc.ctypes.data, hmodels.ctypes.data))
    host_s.append(time.perf_counter() - t0)
gpu_ms = out["generator_g"][f"G{groups[0]}"]["median_ms"]
out["host_twin"] = {"threads": args.threads, "ms_per_launch": [round(v * 1e3, 3) for v in host_s],
                    "slots_per_s": round(args.slots / statistics.median(host_s)),
                    "equals_gpu_bitwise": bool(np.array_equal(hinc, inc) and
                                               np.array_equal(hmodels.view(np.uint64), models.view(np.uint64)))}
out["gpu_slots_per_s"] = round(args.slots / (gpu_ms * 1e-3))


# ---- leg 2 ---------------------------------------------------------------------
def hyps_per_s(h, k0, nb):
    res = (N.BatchResult * nb)()
    st = N.Stats()
    t0 = time.perf_counter()
    N.check(N.lib.gcr_problem_verify_batches(h, C.byref(p), k0 * args.slots, args.slots, nb, res, C.byref(st)))
    dt = time.perf_counter() - t0                 # the call ends in a host synchronisation
    return sum(r.models for r in res) / dt, dt / nb * 1e3


handles = (("g", hg), ("e", he), ("f", hf))
for name, h in handles:
    hyps_per_s(h, 0, 20)                          # warm-up
rates = {name: [] for name, _ in handles}
step = {name: [] for name, _ in handles}
for r in range(args.runs):
    for name, h in handles:
        v, ms = hyps_per_s(h, 1000 + r * args.batches, args.batches)
        rates[name].append(v)
        step[name].append(ms)
for name, _ in handles:
    out["verify_" + name] = {"hyps_per_s": [round(v) for v in rates[name]],
                             "median_hyps_per_s": round(statistics.median(rates[name])),
                             "ms_per_launch": [round(v, 5) for v in step[name]]}
for _, h in handles:
    N.lib.gcr_problem_destroy(h)

# ---- leg 3 ---------------------------------------------------------------------
if not args.no_latency:
    size = (960, 1280, 960, 1280)
    lines = (("gravity_essential", lambda **kw: pygcransac.findGravityEssentialMatrix(corr, K, K, G1, G2, *size, **kw)),
             ("essential", lambda **kw: pygcransac.findEssentialMatrix(corr, K, K, *size, **kw)),
             ("fundamental", lambda **kw: pygcransac.findFundamentalMatrix(corr, *size, **kw)))
    acc = {name: ([], [], []) for name, _ in lines}
    for r in range(-1, args.calls):               # call -1 warms up
        for name, fn in lines:
            t0 = time.perf_counter()
            M, mask, st = fn(threshold=thr, conf=0.99, min_iters=0, max_iters=10**7, seed=100 + r, return_stats=True)
            dt = (time.perf_counter() - t0) * 1e3
            if r >= 0:
                acc[name][0].append(dt)
                acc[name][1].append(st["iteration_number"])
                acc[name][2].append(int(mask[truth].sum()))
    lat = {}
    for name, (ms, its, inl) in acc.items():
        qs = statistics.quantiles(ms, n=4) if len(ms) > 1 else [ms[0]] * 3
        lat[name] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(qs[0], 4), "q3_ms": round(qs[2], 4),
                     "ms": [round(v, 4) for v in ms], "median_iterations": statistics.median(its), "iterations": its,
                     "truth_inliers_found": inl, "truth_inliers": int(truth.sum())}
    out["latency_to_0.99"] = lat
print(json.dumps(out))
