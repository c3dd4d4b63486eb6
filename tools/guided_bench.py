#!/usr/bin/env python3
"""Guided (importance) sampling at the configs[3] shape: problem_f, N = 10 000,
80 % outliers, 14 848 slots per launch.

  1  hypotheses/s of gcr_problem_verify_batches with uniform sampling
  2  the same with guided sampling and all-ones weights (the sampler's pure
     cost: the same distribution, drawn through the CDF), with the two-level
     search and with GCR_GUIDED_FLAT=1 (one flat binary search per draw);
     and the generator's own time per launch (HIP events, gcr_measure_generate_h)
  3  wall time to 0.99 confidence through findFundamentalMatrix, the median of
     --calls calls: uniform against weights 1 / 0.05 on truth inliers / outliers
     with the adaptive stop of the uniform sampler, and those weights with the
     stop on the inlier mass (guided_stop=True); the same three lines at the H
     shape (problem_h, N = 10 000, 80 % outliers); the cost of the stop's mass
     launches (all-ones weights, flag set against clear: the same iterations);
     and the F calls on a fixed budget of --budget iterations: time and truth
     inliers found

The legs of 1 and 2 alternate run by run inside one process.  --pkg points at
another tree's graph-cut-ransac_amd (e.g. the parent commit's, with its own
libgcr.so): a library without the guided entry points runs leg 1 only, a tree
without the guided stop leaves its lines out.
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
ap.add_argument("--batches", type=int, default=2000, help="launches per timed run")
ap.add_argument("--slots", type=int, default=14848)
ap.add_argument("--calls", type=int, default=11, help="leg 3: timed calls per sampler")
ap.add_argument("--gen-reps", type=int, default=200, help="generator launches per HIP-event window")
ap.add_argument("--budget", type=int, default=1000, help="leg 3: the fixed budget's iterations")
ap.add_argument("--no-latency", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.pkg)
import pygcransac  # noqa: E402
from pygcransac import _native as N  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

SEED = 20251121
corr, truth, _, thr = S.problem_f(10_000, 0.8, seed=SEED)
corr = np.ascontiguousarray(corr)
n = corr.shape[0]
guided_lib = hasattr(N.lib, "gcr_problem_set_probabilities")
ctx = N.context(0)
h = C.c_void_p()
N.check(N.lib.gcr_problem_create(ctx, N.SOLVER_FUNDAMENTAL7, corr.ctypes.data_as(C.POINTER(C.c_double)), n, None, 0,
                                 C.byref(h)))
p = N.default_params()
p.scale_residual_thresh = thr
p.seed = SEED
ones = np.ones(n)


def set_w(w):
    if guided_lib:
        N.check(N.lib.gcr_problem_set_probabilities(h, None if w is None else w.ctypes.data, 0 if w is None else n))


def hyps_per_s(k0, nb):
    res = (N.BatchResult * nb)()
    st = N.Stats()
    t0 = time.perf_counter()
    N.check(N.lib.gcr_problem_verify_batches(h, C.byref(p), k0 * args.slots, args.slots, nb, res, C.byref(st)))
    dt = time.perf_counter() - t0                 # the call ends in a host synchronisation
    return sum(r.models for r in res) / dt, dt / nb * 1e3


def gen_ms():
    ms = C.c_double()
    N.check(N.lib.gcr_measure_generate_h(h, SEED, 0, args.slots, args.gen_reps, C.byref(ms)))
    return ms.value


legs = [("uniform", None, "0")]
if guided_lib:
    legs += [("guided_ones", ones, "0"), ("guided_ones_flat", ones, "1")]
out = {"pkg": args.pkg, "build_id": N.lib.gcr_kernel_build_id().decode(), "n": n, "slots": args.slots,
       "batches": args.batches, "runs": args.runs}
rates = {name: [] for name, _, _ in legs}
step_ms = {name: [] for name, _, _ in legs}
gen = {name: [] for name, _, _ in legs}
for name, w, flat in legs:                        # warm-up of every leg's kernels
    os.environ["GCR_GUIDED_FLAT"] = flat
    set_w(w)
    hyps_per_s(0, 200)
for r in range(args.runs):
    for name, w, flat in legs:
        os.environ["GCR_GUIDED_FLAT"] = flat
        set_w(w)
        v, ms = hyps_per_s(1000 + r * args.batches, args.batches)
        rates[name].append(v)
        step_ms[name].append(ms)
        if guided_lib:
            gen[name].append(gen_ms())
os.environ["GCR_GUIDED_FLAT"] = "0"
set_w(None)
for name, _, _ in legs:
    out[name] = {"hyps_per_s": [round(v) for v in rates[name]],
                 "median_hyps_per_s": round(statistics.median(rates[name])),
                 "ms_per_launch": [round(v, 5) for v in step_ms[name]],
                 "generator_ms_per_launch": [round(v, 5) for v in gen[name]]}
if guided_lib:
    u = statistics.median(rates["uniform"])
    out["ratio_guided_ones_to_uniform"] = round(statistics.median(rates["guided_ones"]) / u, 4)
    out["ratio_guided_ones_flat_to_uniform"] = round(statistics.median(rates["guided_ones_flat"]) / u, 4)
N.lib.gcr_problem_destroy(h)

stop_lib = hasattr(N, "FLAG_GUIDED_STOP")        # the guided stop (GCR_FLAG_GUIDED_STOP) exists in this tree


def latency_leg(fn, c, tr, t, lines, lo, hi):
    """--calls timed calls of every line, the lines alternating call by call
    (call -1 warms up); per line the median, the quartiles and what was found"""
    acc = {name: ([], [], [], []) for name, _ in lines}
    for r in range(-1, args.calls):
        for name, kw in lines:
            t0 = time.perf_counter()
            M, mask, st = fn(c, 960, 1280, 960, 1280, threshold=t, conf=0.99, min_iters=lo, max_iters=hi,
                             seed=100 + r, return_stats=True, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            if r >= 0:
                ms, its, inl, launches = acc[name]
                ms.append(dt)
                its.append(st["iteration_number"])
                inl.append(int(mask[tr].sum()))
                launches.append(st["launches"])
    lat = {}
    for name, (ms, its, inl, launches) in acc.items():
        qs = statistics.quantiles(ms, n=4) if len(ms) > 1 else [ms[0]] * 3
        lat[name] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(qs[0], 4), "q3_ms": round(qs[2], 4),
                     "ms": [round(v, 4) for v in ms], "median_iterations": statistics.median(its),
                     "iterations": its, "launches": launches, "truth_inliers_found": inl,
                     "truth_inliers": int(tr.sum())}
    return lat


def replayed_chunks(fn, c, t, kw, lo, hi):
    """chunks one call replays (the exchange log's `collected` events)"""
    os.environ["GCR_EXCHANGE_LOG"] = "1"
    try:
        fn(c, 960, 1280, 960, 1280, threshold=t, conf=0.99, min_iters=lo, max_iters=hi, seed=100, **kw)
        return sum(1 for e in N.exchange_log() if e[0] == 3)
    finally:
        del os.environ["GCR_EXCHANGE_LOG"]


if guided_lib and not args.no_latency:
    # leg 3 at the F shape (above) and the H shape: problem_h, N = 10 000, 80 % outliers
    corr_h, truth_h, _, thr_h = S.problem_h(10_000, 0.8, seed=SEED)
    corr_h = np.ascontiguousarray(corr_h)
    shapes = (("", pygcransac.findFundamentalMatrix, corr, truth, thr),
              ("h_", pygcransac.findHomography, corr_h, truth_h, thr_h))
    for tag, fn, c, tr, t in shapes:
        w = np.where(tr, 1.0, 0.05)
        lines = [("uniform", {}), ("guided", dict(probabilities=w, sampler=3))]
        if stop_lib:
            lines.append(("guided_stop", dict(probabilities=w, sampler=3, guided_stop=True)))
        out[tag + "latency_to_0.99"] = latency_leg(fn, c, tr, t, lines, 0, 10**7)
        if tag == "":
            out[f"budget_{args.budget}"] = latency_leg(fn, c, tr, t, lines[:2], args.budget, args.budget)
        if stop_lib:
            # the mass launches' cost: all-ones weights stop where the uniform
            # bound stops them with the flag set or clear (the same iterations),
            # so the difference is the launches
            w1 = np.ones(len(c))
            cost = latency_leg(fn, c, tr, t, [("ones_clear", dict(probabilities=w1, sampler=3)),
                                              ("ones_stop", dict(probabilities=w1, sampler=3, guided_stop=True))],
                               0, 10**7)
            a, b = cost["ones_clear"], cost["ones_stop"]
            chunks = replayed_chunks(fn, c, t, dict(probabilities=w1, sampler=3, guided_stop=True), 0, 10**7)
            cost["same_iterations"] = a["iterations"] == b["iterations"]
            cost["mass_launches_per_run"] = statistics.median(y - x for x, y in zip(a["launches"], b["launches"]))
            cost["replayed_chunks_seed_100"] = chunks
            cost["ms_per_run"] = round(b["median_ms"] - a["median_ms"], 4)
            cost["ms_per_replayed_chunk"] = round((b["median_ms"] - a["median_ms"]) / max(chunks, 1), 4)
            out[tag + "mass_launch_cost"] = cost
print(json.dumps(out))
