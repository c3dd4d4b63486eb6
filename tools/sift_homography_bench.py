#!/usr/bin/env python3
"""The homography from two SIFT correspondences beside the 4-point estimator on
the same points: problem_hs, N = 10 000, at each outlier share of --outliers
(default 80 % and 95 %), 14 848 slots per launch.

  1  the SIFT generator's time per launch (HIP events,
     gcr_measure_generate_h) beside k_generate<3, G>'s on the same points, for
     the lanes-per-slot settings of --groups (GCR_GEN_G; 0 = the engine's
     choice) at the launch sizes of --sweep-slots; attempts and live models per
     slot; whether the host twin (gcr_host_generate_s) agrees bit for bit
  2  hypotheses/s of gcr_problem_verify_batches for both estimators
  3  wall time and iterations to 0.99 confidence through findHomographySIFT and
     findHomography on the same points, the median of --calls calls, the lines
     alternating call by call; truth inliers found

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
ap.add_argument("--batches", type=int, default=100, help="launches per timed run")
ap.add_argument("--slots", type=int, default=14848)
ap.add_argument("--calls", type=int, default=11, help="leg 3: timed calls per estimator")
ap.add_argument("--gen-reps", type=int, default=50, help="generator launches per HIP-event window")
ap.add_argument("--groups", default="0,1,2,4,8,16,32", help="lanes per slot to time (GCR_GEN_G), 0 = the engine's choice")
ap.add_argument("--sweep-slots", default="1024,3712,14848,65536", help="launch sizes of the G sweep")
ap.add_argument("--outliers", default="0.8,0.95")
ap.add_argument("--threads", type=int, default=16, help="host twin's threads")
ap.add_argument("--no-latency", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.pkg)
import pygcransac  # noqa: E402
from pygcransac import _native as N  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

SEED = 20251121
ctx = N.context(0)
dp = C.POINTER(C.c_double)
out = {"pkg": args.pkg, "build_id": N.lib.gcr_kernel_build_id().decode(), "slots": args.slots,
       "batches": args.batches, "runs": args.runs, "shapes": {}}


def gen_ms(h, g, slots):
    if g:
        os.environ["GCR_GEN_G"] = str(g)
    else:
        os.environ.pop("GCR_GEN_G", None)
    ms = C.c_double()
    vals = []
    for _ in range(args.runs):
        N.check(N.lib.gcr_measure_generate_h(h, SEED, 0, slots, args.gen_reps, C.byref(ms)))
        vals.append(ms.value)
    os.environ.pop("GCR_GEN_G", None)
    return round(statistics.median(vals), 5)


for share in (float(v) for v in args.outliers.split(",")):
    rows, truth, H_gt, thr = S.problem_hs(10_000, share, seed=SEED)
    corr, sift = np.ascontiguousarray(rows[:, :4]), np.ascontiguousarray(rows[:, 4:])
    n = len(corr)
    hs, hh = C.c_void_p(), C.c_void_p()
    N.check(N.lib.gcr_problem_create_sift_homography(ctx, corr.ctypes.data, sift.ctypes.data, n, C.byref(hs)))
    N.check(N.lib.gcr_problem_create(ctx, N.SOLVER_HOMOGRAPHY4, corr.ctypes.data_as(dp), n, None, 0, C.byref(hh)))
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.seed = SEED
    o = {"n": n, "outlier_share": share, "threshold": thr}

    # ---- leg 1 -----------------------------------------------------------------
    groups = [int(g) for g in args.groups.split(",")]
    sweep = [int(v) for v in args.sweep_slots.split(",")]
    o["generator_s_median_ms"] = {str(sl): {f"G{g}": gen_ms(hs, g, sl) for g in groups} for sl in sweep}
    o["generator_h4_median_ms"] = {str(sl): {"G0": gen_ms(hh, 0, sl)} for sl in sweep}
    per = 3
    inc = np.zeros(args.slots * per, dtype=np.uint8)
    models = np.zeros(args.slots * per * 9)
    N.check(N.lib.gcr_debug_generate_h(hs, SEED, 0, args.slots, inc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       models.ctypes.data_as(dp)))
    inc2 = inc.reshape(-1, per)
    ok = inc2[:, 0] <= 101
    o["slots_with_a_model"] = int(ok.sum())
    o["attempts_per_slot"] = round(float(np.minimum(inc2[:, 0], 101).mean()), 4)
    o["live_models_per_slot"] = round(float((ok + (inc2[:, 1:] == 0).sum(axis=1)).mean()), 6)
    hinc, hmodels = np.zeros_like(inc), np.zeros_like(models)
    t0 = time.perf_counter()
    N.check(N.lib.gcr_host_generate_s(corr.ctypes.data, sift.ctypes.data, n, None, SEED, 0, args.slots, args.threads,
                                      hinc.ctypes.data, hmodels.ctypes.data))
    o["host_twin"] = {"threads": args.threads, "ms_per_launch": round((time.perf_counter() - t0) * 1e3, 3),
                      "equals_gpu_bitwise": bool(np.array_equal(hinc, inc) and
                                                 np.array_equal(hmodels.view(np.uint64), models.view(np.uint64)))}

    # ---- leg 2 -----------------------------------------------------------------
    def hyps_per_s(h, k0, nb):
        res = (N.BatchResult * nb)()
        st = N.Stats()
        t0 = time.perf_counter()
        N.check(N.lib.gcr_problem_verify_batches(h, C.byref(p), k0 * args.slots, args.slots, nb, res, C.byref(st)))
        dt = time.perf_counter() - t0                 # the call ends in a host synchronisation
        return sum(r.models for r in res) / dt, dt / nb * 1e3

    handles = (("sift", hs), ("h4", hh))
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
        o["verify_" + name] = {"median_hyps_per_s": round(statistics.median(rates[name])),
                               "median_ms_per_launch": round(statistics.median(step[name]), 5)}
    for _, h in handles:
        N.lib.gcr_problem_destroy(h)

    # ---- leg 3 -----------------------------------------------------------------
    if not args.no_latency:
        size = (960, 1280, 960, 1280)
        lines = (("sift_homography", lambda **kw: pygcransac.findHomographySIFT(rows, *size, **kw)),
                 ("homography", lambda **kw: pygcransac.findHomography(corr, *size, **kw)))
        acc = {name: ([], [], []) for name, _ in lines}
        for r in range(-1, args.calls):               # call -1 warms up
            for name, fn in lines:
                t0 = time.perf_counter()
                M, mask, st = fn(threshold=thr, conf=0.99, min_iters=0, max_iters=10**7, seed=100 + r,
                                 spatial_coherence_weight=0.0, return_stats=True)
                dt = (time.perf_counter() - t0) * 1e3
                if r >= 0:
                    acc[name][0].append(dt)
                    acc[name][1].append(st["iteration_number"])
                    acc[name][2].append(int(mask[truth].sum()))
        lat = {}
        for name, (ms, its, inl) in acc.items():
            qs = statistics.quantiles(ms, n=4) if len(ms) > 1 else [ms[0]] * 3
            lat[name] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(qs[0], 4),
                         "q3_ms": round(qs[2], 4), "ms": [round(v, 4) for v in ms],
                         "median_iterations": statistics.median(its), "iterations": its,
                         "truth_inliers_found": inl, "truth_inliers": int(truth.sum())}
        o["latency_to_0.99"] = lat
    out["shapes"][str(share)] = o
print(json.dumps(out))
