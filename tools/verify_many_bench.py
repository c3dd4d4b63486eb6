#!/usr/bin/env python3
"""gcr_verify_many against the ways the same work is done without it, on one GPU.

Workload: --problems (1 024) problems from synthetic.problem_h / problem_f at
50 % outliers, S = --slots (1 024) slots each.  Shapes: "mixed" (the headline:
n_p drawn uniformly from 200 .. 2 000 with a fixed seed), "n100" and "n4000"
(every problem that many rows).  Per kind (H, F) and shape, the legs alternate
call by call, medians of --calls (11) with quartiles and every sample printed:

  (a) loop_verify_batch  a loop of gcr_problem_verify_batch(prob, params, 0, S)
                         over resident problems created outside the timed
                         region: the same computation without verify_many
  (b) solve_batch        gcr_solve_batch on the same rows, 8 host threads
                         (informational: whole runs with LO and the stop,
                         min 50 / max S iterations, its uploads included)
  (c) verify_many        the whole gcr_verify_many call, upload and masks included
  (d) kernels            its three kernels alone, by HIP events (ms_kernel_out
                         of the same calls)

(a) and (c) must give the same records: "equal_records".  The hypothesis rate
is P * S * per / time (per = 1 for H, 3 for F: slots times hypothesis
positions, as bench.py counts hypotheses_computed).

  (e) pairs              features.verify_pairs beside features.match_pairs
                         alone on 120 pairs: 16 resident sets of 2 000 ..
                         10 000 rows cut from one synthetic image pair
                         (synthetic.problem_match), so that the pairs have
                         matches to verify (match_bench.py --sets uses random
                         descriptors, which leave nothing to verify)

Prints one JSON line.
usage: verify_many_bench.py [--problems 1024] [--slots 1024] [--calls 11] [--shapes mixed,n100,n4000] [--no-pairs]"""
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
ap.add_argument("--problems", type=int, default=1024)
ap.add_argument("--slots", type=int, default=1024)
ap.add_argument("--calls", type=int, default=11)
ap.add_argument("--shapes", default="mixed,n100,n4000")
ap.add_argument("--kinds", default="H,F")
ap.add_argument("--batch-calls", type=int, default=3, help="timed gcr_solve_batch calls (informational leg)")
ap.add_argument("--no-pairs", action="store_true")
args = ap.parse_args()

sys.path.insert(0, args.pkg)
import pygcransac  # noqa: E402,F401
from pygcransac import _native as N  # noqa: E402
from pygcransac import features as F  # noqa: E402
from pygcransac import synthetic as S  # noqa: E402

SEED = 20260611
P, SLOTS = args.problems, args.slots
ctx = N.context(0)
out = {"pkg": args.pkg, "build_id": N.lib.gcr_kernel_build_id().decode(), "problems": P, "slots": SLOTS,
       "calls": args.calls}
KINDS = {"H": (N.SOLVER_HOMOGRAPHY4, 1, S.problem_h), "F": (N.SOLVER_FUNDAMENTAL7, 3, S.problem_f)}


def quart(v):
    qs = statistics.quantiles(v, n=4) if len(v) > 1 else [v[0]] * 3
    return {"median_ms": round(statistics.median(v), 4), "q1_ms": round(qs[0], 4), "q3_ms": round(qs[2], 4),
            "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "ms": [round(x, 4) for x in v]}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def alternate(legs, calls):
    """name -> list of ms; call -1 warms up; the legs alternate call by call"""
    acc, last = {name: [] for name in legs}, {}
    for k in range(-1, calls):
        for name, fn in legs.items():
            ms, last[name] = timed(fn)
            if k >= 0:
                acc[name].append(ms)
    return acc, last


def sizes(shape):
    if shape == "mixed":
        return np.random.default_rng(SEED).integers(200, 2001, P).tolist()
    return [int(shape[1:])] * P


def one(kind, shape):
    solver, per, make = KINDS[kind]
    ns = sizes(shape)
    # one large synthetic problem per distinct size class would repeat rows: every problem has its own seed
    probs, thr = [], []
    for p, n_p in enumerate(ns):
        rows, _, _, t = make(n_p, 0.5, seed=SEED + p)
        probs.append(np.ascontiguousarray(rows))
        thr.append(float(t))
    off = np.zeros(P + 1, dtype=np.uint64)
    off[1:] = np.cumsum(ns)
    rows = np.ascontiguousarray(np.concatenate(probs))
    thr_a = np.array(thr)
    seeds = np.arange(1, P + 1, dtype=np.uint64)
    total = int(off[-1])
    g = {"rows_total": total, "rows_min": min(ns), "rows_max": max(ns)}

    # (a): resident problems, created outside the timed region
    handles, params = [], []
    for p in range(P):
        h = C.c_void_p()
        N.check(N.lib.gcr_problem_create(ctx, solver, probs[p].ctypes.data_as(C.POINTER(C.c_double)), ns[p], None, 0,
                                         C.byref(h)))
        handles.append(h.value)
        q = N.default_params()
        q.scale_residual_thresh = thr[p]
        q.seed = int(seeds[p])
        params.append(q)
    recs_a = (N.BatchResult * P)()

    def loop():
        vb = N.lib.gcr_problem_verify_batch
        for p in range(P):
            if vb(handles[p], C.byref(params[p]), 0, SLOTS, C.byref(recs_a[p]), None) < 0:
                raise RuntimeError(N.last_error())

    # (c), (d)
    recs_c = (N.ManyResult * P)()
    masks = np.zeros(total, dtype=np.uint8)
    kms = C.c_double()
    kernel_ms = []

    def many():
        N.check(N.lib.gcr_verify_many(ctx, solver, rows.ctypes.data, off.ctypes.data, P, thr_a.ctypes.data,
                                      seeds.ctypes.data, SLOTS, recs_c, masks.ctypes.data, C.byref(kms)))
        kernel_ms.append(kms.value)

    acc, _ = alternate({"loop_verify_batch": loop, "verify_many": many}, args.calls)
    for name, v in acc.items():
        g[name] = quart(v)
    g["kernels"] = quart(kernel_ms[1:])
    a = np.frombuffer(recs_a, dtype=np.dtype(N.BatchResult))
    c = np.frombuffer(recs_c, dtype=N.MANY_DT)
    g["equal_records"] = bool(all(np.array_equal(a[k], c[k]) for k in ("models", "iterations", "best_slot")) and
                              a["best_score"].tobytes() == c["best_score"].tobytes() and
                              np.array_equal(a["best_inliers"][:, 0], c["best_inliers"]))
    g["with_a_best"] = int((c["best_slot"] >= 0).sum())
    g["mask_sums_equal_inliers"] = bool(all(int(masks[int(off[p]):int(off[p + 1])].sum()) == int(c["best_inliers"][p])
                                            for p in range(P)))
    ma, mc, mk = (g[k]["median_ms"] for k in ("loop_verify_batch", "verify_many", "kernels"))
    g["loop_over_many"] = round(ma / mc, 3)
    # the spread of the two alternating legs: the worst verify_many call against the best loop
    g["loop_min_over_many_max"] = round(g["loop_verify_batch"]["min_ms"] / g["verify_many"]["max_ms"], 3)
    hyp = P * SLOTS * per
    g["hypotheses"] = hyp
    g["hyp_per_s"] = {"loop_verify_batch": round(hyp / (ma * 1e-3)), "verify_many": round(hyp / (mc * 1e-3)),
                      "kernels": round(hyp / (mk * 1e-3))}
    g["problems_per_s"] = {"loop_verify_batch": round(P / (ma * 1e-3)), "verify_many": round(P / (mc * 1e-3))}
    for h in handles:
        N.lib.gcr_problem_destroy(h)

    # (b): whole runs on host threads, informational
    if args.batch_calls > 0:
        items = (N.BatchItem * P)()
        keep = []
        for p in range(P):
            it = items[p]
            it.solver = solver
            it.f0 = probs[p].ctypes.data_as(C.POINTER(C.c_double))
            it.n0 = ns[p]
            it.params = N.default_params()
            it.params.scale_residual_thresh = thr[p]
            it.params.min_iteration_number = 50
            it.params.max_iteration_number = SLOTS
            it.params.confidence = 0.99
            it.params.seed = int(seeds[p])
            m = np.zeros(ns[p], dtype=np.uint8)
            keep.append(m)
            it.mask0_out = m.ctypes.data_as(C.POINTER(C.c_uint8))
        v = []
        for k in range(-1, args.batch_calls):
            ms, rc = timed(lambda: N.lib.gcr_solve_batch(0, items, P, 8))
            N.check(rc)
            if k >= 0:
                v.append(ms)
        g["solve_batch"] = quart(v)
        g["problems_per_s"]["solve_batch"] = round(P / (g["solve_batch"]["median_ms"] * 1e-3))
    return g


def pairs_mode():
    n = 10_000
    kp1, e1, kp2, e2, _, _ = S.problem_match(n, int(0.4 * n), seed=SEED, dim=128)
    ns = np.linspace(2000, 10000, 16).astype(int).tolist()
    sets = [F.DescriptorSet((e1, e2)[k % 2][:ns[k]], (kp1, kp2)[k % 2][:ns[k]]) for k in range(len(ns))]
    pr = [(i, j) for i in range(len(ns)) for j in range(i + 1, len(ns))]
    acc, last = alternate({"match_pairs": lambda: F.match_pairs(sets, pr),
                           "verify_pairs": lambda: F.verify_pairs(sets, pr, "homography", 2.0, iterations=SLOTS)},
                          min(args.calls, 5))
    g = {name: {**quart(v), "pairs_per_s": round(len(pr) / (statistics.median(v) * 1e-3), 1)}
         for name, v in acc.items()}
    m = [len(x[0]) for x in last["verify_pairs"]]
    g.update({"pairs": len(pr), "rows": ns, "matches_min": min(m), "matches_max": max(m), "matches_total": sum(m),
              "verified": sum(1 for x in last["verify_pairs"] if x[2]["model"] is not None),
              "verify_over_match": round(g["verify_pairs"]["median_ms"] / g["match_pairs"]["median_ms"], 3)})
    for s_ in sets:
        s_.close()
    return g


for kind in args.kinds.split(","):
    for shape in args.shapes.split(","):
        out[f"{kind}_{shape}"] = one(kind, shape)
if not args.no_pairs:
    out["pairs"] = pairs_mode()
print(json.dumps(out))
