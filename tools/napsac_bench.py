#!/usr/bin/env python3
"""NAPSAC sampling (csrc/napsac.h) at the H and F shapes: N = 10 000, 14 848
slots per launch.

  1  the generator's own time per launch (HIP events, gcr_measure_generate_h),
     problem_h / problem_f at 80 % outliers:
       uniform        no table
       napsac_q0..q3  local length 2^40, the window's launches inside the
                      first .. fourth quarter (finest admissible layer 16, 8,
                      4, 2 cells): the record load, the layer choice and the
                      member loads on top of the uniform attempt, and whatever
                      the local samples change in the attempts per slot
       napsac_past    local length 1000 from slot 2^30: past T, the launch is
                      the uniform kernel itself
       uniform_far    no table, from slot 2^30: napsac_past's slots
     The legs alternate run by run inside one process.
  2  host time of gcr_problem_set_napsac at N = 10 000 (the four layers built
     and uploaded), the median of --calls calls, and of clearing it: on
     problem_h's rows (some x2 / y2 are negative: their keys wrap, and the
     grid's grouping takes its comparison sort) and on problem_h_local's (all
     inside the images: the counting sort).
  3  problem_h_local (N = 10 000, 95 % outliers, the inliers in a quarter x
     quarter window): truth inliers found and wall time on fixed budgets of
     --budgets iterations, sampler=2 against uniform on the same rows, the
     median of --calls calls alternating call by call.

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
ap.add_argument("--calls", type=int, default=11, help="legs 2 and 3: timed calls")
ap.add_argument("--budgets", type=int, nargs="+", default=[100, 1000], help="leg 3: the fixed budgets' iterations")
ap.add_argument("--no-latency", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.pkg)
import pygcransac  # noqa: E402
from pygcransac import _native as N  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

SEED = 20251121
EXTENT = (C.c_double * 4)(S.IMG_W, S.IMG_H, S.IMG_W, S.IMG_H)
ctx = N.context(0)
out = {"pkg": args.pkg, "build_id": N.lib.gcr_kernel_build_id().decode(), "slots": args.slots, "runs": args.runs,
       "gen_reps": args.gen_reps}


def create(solver, corr):
    h = C.c_void_p()
    N.check(N.lib.gcr_problem_create(ctx, solver, corr.ctypes.data_as(C.POINTER(C.c_double)), corr.shape[0], None, 0,
                                     C.byref(h)))
    return h


def generator_leg(solver, corr):
    h = create(solver, corr)

    def gen_ms(slot0):
        ms = C.c_double()
        N.check(N.lib.gcr_measure_generate_h(h, SEED, slot0, args.slots, args.gen_reps, C.byref(ms)))
        return ms.value

    big = 1 << 40
    legs = [("uniform", 0, 0)] + [(f"napsac_q{k}", big, k * (big >> 2)) for k in range(4)] + \
           [("napsac_past", 1000, 1 << 30), ("uniform_far", 0, 1 << 30)]
    ms = {name: [] for name, _, _ in legs}
    try:
        for r in range(-1, args.runs):                # run -1 warms every leg's kernels up
            for name, T, slot0 in legs:
                N.check(N.lib.gcr_problem_set_napsac(h, EXTENT, T))
                v = gen_ms(slot0)
                if r >= 0:
                    ms[name].append(v)
    finally:
        N.lib.gcr_problem_destroy(h)
    res = {name: {"generator_ms_per_launch": [round(v, 5) for v in vs], "median_ms": round(statistics.median(vs), 5)}
           for name, vs in ms.items()}
    u = res["uniform"]["median_ms"]
    for k in range(4):
        res[f"ratio_uniform_to_napsac_q{k}"] = round(u / res[f"napsac_q{k}"]["median_ms"], 4)
    res["ratio_uniform_far_to_napsac_past"] = round(res["uniform_far"]["median_ms"] / res["napsac_past"]["median_ms"], 4)
    return res


def set_napsac_leg(solver, corr):
    h = create(solver, corr)
    on, off = [], []
    try:
        for r in range(-1, args.calls):
            t0 = time.perf_counter()
            N.check(N.lib.gcr_problem_set_napsac(h, EXTENT, 5000))
            t1 = time.perf_counter()
            N.check(N.lib.gcr_problem_set_napsac(h, EXTENT, 0))
            t2 = time.perf_counter()
            if r >= 0:
                on.append((t1 - t0) * 1e3)
                off.append((t2 - t1) * 1e3)
    finally:
        N.lib.gcr_problem_destroy(h)
    return {"n": corr.shape[0], "set_ms": [round(v, 4) for v in on], "set_median_ms": round(statistics.median(on), 4),
            "clear_median_ms": round(statistics.median(off), 4)}


def budget_leg(c, tr, t, budget):
    lines = (("uniform", dict(sampler=0)), ("napsac", dict(sampler=2)))
    acc = {name: ([], [], []) for name, _ in lines}
    for r in range(-1, args.calls):
        for name, kw in lines:
            t0 = time.perf_counter()
            M, mask, st = pygcransac.findHomography(c, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, threshold=t, conf=0.99,
                                                    min_iters=budget, max_iters=budget, seed=100 + r,
                                                    return_stats=True, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            if r >= 0:
                ms, its, inl = acc[name]
                ms.append(dt)
                its.append(st["iteration_number"])
                inl.append(int(mask[tr].sum()) if M is not None else 0)
    res = {}
    for name, (ms, its, inl) in acc.items():
        res[name] = {"median_ms": round(statistics.median(ms), 4), "ms": [round(v, 4) for v in ms], "iterations": its,
                     "truth_inliers_found": inl, "median_truth_inliers_found": statistics.median(inl),
                     "truth_inliers": int(tr.sum())}
    return res


shapes = (("h", N.SOLVER_HOMOGRAPHY4, S.problem_h), ("f", N.SOLVER_FUNDAMENTAL7, S.problem_f))
for tag, solver, make in shapes:
    corr = np.ascontiguousarray(make(10_000, 0.8, seed=SEED)[0])
    out[tag + "_generator"] = generator_leg(solver, corr)
    if tag == "h":
        out["set_napsac"] = set_napsac_leg(solver, corr)
        local = np.ascontiguousarray(S.problem_h_local(10_000, 0.95, seed=SEED)[0])
        out["set_napsac_rows_inside"] = set_napsac_leg(solver, local)
        out["rows_outside_the_images"] = [int(((corr < 0) | (corr >= np.array(EXTENT[:]))).any(axis=1).sum()),
                                          int(((local < 0) | (local >= np.array(EXTENT[:]))).any(axis=1).sum())]
if not args.no_latency:
    c, tr, _, t = S.problem_h_local(10_000, 0.95, seed=SEED)
    for budget in args.budgets:
        out[f"h_local_budget_{budget}"] = budget_leg(c, tr, t, budget)
print(json.dumps(out))
