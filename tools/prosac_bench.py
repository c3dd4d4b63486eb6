#!/usr/bin/env python3
"""PROSAC sampling (csrc/prosac.h) at the H and F shapes: problem_h /
problem_f, N = 10 000, 14 848 slots per launch.

  1  the generator's own time per launch (HIP events, gcr_measure_generate_h),
     80 % outliers, rows in their shuffled order (every pool holds the same
     share of inliers, so the attempts per slot are the uniform sampler's and
     the difference is the sampler's cost):
       uniform        no table
       prosac_growth  convergence 2^40: every launch of the window is in the
                      growth phase (the window's launches cover consecutive
                      slot ranges; with the default 100 000 they would leave
                      the growth phase after 7 launches)
       prosac_past    convergence 100 000 from slot 2^30: past g[N], the launch
                      is the uniform kernel itself
       uniform_far    no table, from slot 2^30: prosac_past's slots, the
                      like-for-like comparison
       guided_ones    all-ones weights, the guided sampler's pure cost
     The legs alternate run by run inside one process.
  2  wall time to 0.99 confidence, the median of --calls calls, at 95 %
     outliers with informative scores (truth inliers N(2, 1), outliers
     N(0, 1)): uniform against sampler=1 on the same data, iterations capped
     at --cap.  The stop is the uniform bound for both, so the iteration counts
     agree by construction; what PROSAC buys shows on a fixed budget of
     --budget iterations: time and truth inliers found.  Where the tree has
     the PROSAC stop (csrc/prosac_stop.h), a third line: sampler=1 with
     prosac_stop=True.
  3  (trees with the PROSAC stop) what the stop costs:
       stop_launch_cost  H shape, rows in shuffled order (scores that rank
                      nothing), a fixed budget of --cost-budget iterations with
                      the flag clear and set: the loop runs to the budget either
                      way, so the difference is the stop launches
       qmin_build     gcr_debug_prosac_stop_h on one model at N = 10 000 with
                      the confidence alternating call by call (the table is
                      rebuilt and uploaded every call) against a constant one
                      (cached on the problem), and the host entry that builds
                      both tables

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
ap.add_argument("--slots", type=int, default=14848)
ap.add_argument("--gen-reps", type=int, default=200, help="generator launches per HIP-event window")
ap.add_argument("--calls", type=int, default=11, help="leg 2: timed calls per sampler")
ap.add_argument("--cap", type=int, default=10**6, help="leg 2: max_iters of the calls to 0.99")
ap.add_argument("--budget", type=int, default=1000, help="leg 2: the fixed budget's iterations")
ap.add_argument("--cost-budget", type=int, default=200000, help="leg 3: the stop-launch cost's iterations")
ap.add_argument("--no-latency", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.pkg)
import pygcransac  # noqa: E402
from pygcransac import _native as N  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

SEED = 20251121
ctx = N.context(0)
out = {"pkg": args.pkg, "build_id": N.lib.gcr_kernel_build_id().decode(), "slots": args.slots, "runs": args.runs,
       "gen_reps": args.gen_reps}


def generator_leg(solver, corr):
    n = corr.shape[0]
    h = C.c_void_p()
    N.check(N.lib.gcr_problem_create(ctx, solver, corr.ctypes.data_as(C.POINTER(C.c_double)), n, None, 0,
                                     C.byref(h)))
    ones = np.ones(n)

    def setup(convergence, w):
        N.check(N.lib.gcr_problem_set_prosac(h, 0))
        N.check(N.lib.gcr_problem_set_probabilities(h, None if w is None else w.ctypes.data, 0 if w is None else n))
        N.check(N.lib.gcr_problem_set_prosac(h, convergence))

    def gen_ms(slot0):
        ms = C.c_double()
        N.check(N.lib.gcr_measure_generate_h(h, SEED, slot0, args.slots, args.gen_reps, C.byref(ms)))
        return ms.value

    legs = (("uniform", 0, None, 0), ("prosac_growth", 1 << 40, None, 0), ("prosac_past", 100000, None, 1 << 30),
            ("uniform_far", 0, None, 1 << 30), ("guided_ones", 0, ones, 0))
    ms = {name: [] for name, _, _, _ in legs}
    try:
        for r in range(-1, args.runs):                # run -1 warms every leg's kernels up
            for name, convergence, w, slot0 in legs:
                setup(convergence, w)
                v = gen_ms(slot0)
                if r >= 0:
                    ms[name].append(v)
    finally:
        N.lib.gcr_problem_destroy(h)
    res = {name: {"generator_ms_per_launch": [round(v, 5) for v in vs], "median_ms": round(statistics.median(vs), 5)}
           for name, vs in ms.items()}
    u = res["uniform"]["median_ms"]
    for name in ("prosac_growth", "prosac_past", "guided_ones"):
        res[f"ratio_uniform_to_{name}"] = round(u / res[name]["median_ms"], 4)
    res["ratio_uniform_far_to_prosac_past"] = round(res["uniform_far"]["median_ms"] / res["prosac_past"]["median_ms"], 4)
    return res


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


stop_lib = hasattr(N, "FLAG_PROSAC_STOP")        # the PROSAC stop (GCR_FLAG_PROSAC_STOP) exists in this tree


def stop_launch_cost(fn, c, tr, t):
    ranks_nothing = -np.arange(len(c), dtype=np.float64)          # the rows as they come: shuffled
    kw = dict(probabilities=ranks_nothing, sampler=1)
    cost = latency_leg(fn, c, tr, t, [("clear", kw), ("stop", dict(kw, prosac_stop=True))], args.cost_budget,
                       args.cost_budget)
    a, b = cost["clear"], cost["stop"]
    launches = statistics.median(y - x for x, y in zip(a["launches"], b["launches"]))
    cost["same_iterations"] = a["iterations"] == b["iterations"]
    cost["stop_launches_per_run"] = launches
    cost["ms_per_run"] = round(b["median_ms"] - a["median_ms"], 4)
    cost["ms_per_stop_launch"] = round((b["median_ms"] - a["median_ms"]) / max(launches, 1), 4)
    return cost


def qmin_build(solver, corr, t, reps=101):
    n = corr.shape[0]
    h = C.c_void_p()
    N.check(N.lib.gcr_problem_create(ctx, solver, corr.ctypes.data_as(C.POINTER(C.c_double)), n, None, 0,
                                     C.byref(h)))
    u32p = C.POINTER(C.c_uint32)
    model = np.eye(3).reshape(9)
    res = [np.zeros(1, dtype=np.uint32) for _ in range(3)]
    p = N.default_params()
    p.scale_residual_thresh = t

    def call_ms(conf):
        p.confidence = conf
        t0 = time.perf_counter()
        N.check(N.lib.gcr_debug_prosac_stop_h(h, C.byref(p), model.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                              *(r.ctypes.data_as(u32p) for r in res)))
        return (time.perf_counter() - t0) * 1e3

    try:
        N.check(N.lib.gcr_problem_set_prosac(h, 100000))
        call_ms(0.99)
        cached = [call_ms(0.99) for _ in range(reps)]
        rebuilt = [call_ms(0.98 if k % 2 else 0.99) for k in range(reps)]
    finally:
        N.lib.gcr_problem_destroy(h)
    imin, qmin = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        N.check(N.lib.gcr_host_prosac_stop_tables(n, 4, 100000, 0.99, imin.ctypes.data_as(u32p),
                                                  qmin.ctypes.data_as(C.POINTER(C.c_double))))
        host.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median
    return {"n": n, "kernel_call_cached_ms": round(med(cached), 4), "kernel_call_rebuilt_ms": round(med(rebuilt), 4),
            "qmin_build_and_upload_ms": round(med(rebuilt) - med(cached), 4),
            "host_growth_imin_qmin_ms": round(med(host), 4)}


shapes = (("h", N.SOLVER_HOMOGRAPHY4, S.problem_h, pygcransac.findHomography),
          ("f", N.SOLVER_FUNDAMENTAL7, S.problem_f, pygcransac.findFundamentalMatrix))
for tag, solver, make, fn in shapes:
    corr = np.ascontiguousarray(make(10_000, 0.8, seed=SEED)[0])
    out[tag + "_generator"] = generator_leg(solver, corr)
    if args.no_latency:
        continue
    c, tr, _, t = make(10_000, 0.95, seed=SEED)
    c = np.ascontiguousarray(c)
    scores = np.random.default_rng(SEED).normal(0.0, 1.0, len(c)) + np.where(tr, 2.0, 0.0)
    lines = [("uniform", {}), ("prosac", dict(probabilities=scores, sampler=1))]
    if stop_lib:
        lines.append(("prosac_stop", dict(probabilities=scores, sampler=1, prosac_stop=True)))
    out[tag + "_latency_to_0.99"] = latency_leg(fn, c, tr, t, lines, 0, args.cap)
    out[tag + f"_budget_{args.budget}"] = latency_leg(fn, c, tr, t, lines[:2], args.budget, args.budget)
    if stop_lib and tag == "h":
        c80, tr80, _, t80 = make(10_000, 0.8, seed=SEED)
        c80 = np.ascontiguousarray(c80)
        out["h_stop_launch_cost"] = stop_launch_cost(fn, c80, tr80, t80)
        out["h_qmin_build"] = qmin_build(solver, c80, t80)
print(json.dumps(out))
