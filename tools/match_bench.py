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

With --guided only the guided matcher runs (gcr_match_descriptors_guided) on
problem_match(n, 0.4 n)'s keypoints and descriptors at a 3 px bound: under
H_GT and under F = [e']x H_GT, forward and mutual (forward + reverse), kernels
and whole calls, interleaved call by call with the unguided matcher on the
same descriptors; whether the host twin agrees bit for bit; the admissible
share of the pairs, and the share of the kernel's 32 x 32 tiles and of its
128-row x 64-column steps without an admissible pair (numpy, from the
definition), which the kernel skips.

With --sets only the resident-set legs run (features.DescriptorSet) on
problem_match(n, 0.4 n): the array call match_descriptors(ratio=0.8,
mutual=True), the set call a.match(b) with both sets resident (with the pinned
and, under GCR_MATCH_SETS_PAGEABLE=1, the pageable download), set creation on
its own, the C entry with its HIP-event breakdown (forward search, reverse
search, select launches), the same for match_guided under H_GT and F against
match_descriptors_guided, and match_pairs over --pair-sets sets of 2 000 ..
10 000 rows in all unordered pairs against a loop of array calls and a loop of
a.match(b).  The legs of a group alternate call by call; medians of --calls
after a warm-up, quartiles beside them; every set result is compared with the
array function's byte for byte.

With --knn only the k-nearest-neighbour legs run (gcr_knn_descriptors) on the
uniform random descriptors: the kernels' time (HIP events) of the 2-NN matcher
(k_match) and of the k-NN kernels at k = 2, 4 and 8, the legs alternating call
by call in one process, under the planner's column split and each pinned split
of --knn-splits; the whole-call times of the array entry and of the set entry
(DescriptorSet.knn, both sets resident) with the set entry's kernel time; the
ratio of every k-NN kernel time to k_match's of the same run; whether k = 2
equals the matcher's arrays, the set entry the array entry and k = 8 the host
twin.

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
ap.add_argument("--guided", action="store_true", help="the guided matcher's legs only")
ap.add_argument("--threshold", type=float, default=3.0, help="guided: the bound in pixels")
ap.add_argument("--sets", action="store_true", help="the resident descriptor sets' legs only")
ap.add_argument("--pair-sets", type=int, default=16, help="sets: the number of sets of the match_pairs leg")
ap.add_argument("--pair-calls", type=int, default=5, help="sets: timed repetitions of the match_pairs legs")
ap.add_argument("--knn", action="store_true", help="the k-nearest-neighbour legs only")
ap.add_argument("--knn-splits", default="0,1", help="knn: column splits to time (GCR_MATCH_SPLIT), 0 = the planner's")
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


# ---- guided mode ---------------------------------------------------------------
def guided_mode():
    kp1, e1, kp2, e2, pairs, Hgt = S.problem_match(n, int(0.4 * n), seed=SEED, dim=dim)
    p1, p2 = np.ascontiguousarray(kp1[:, :2]), np.ascontiguousarray(kp2[:, :2])
    e = (2.0 * S.IMG_W, S.IMG_H / 2.0, 1.0)
    skew = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
    models = {"H": (3, np.ascontiguousarray(Hgt)), "F": (4, np.ascontiguousarray(skew @ Hgt))}
    T = args.threshold * args.threshold
    ms = C.c_double()

    def unguided(res):
        t0 = time.perf_counter()
        N.check(N.lib.gcr_match_descriptors(ctx, e1.ctypes.data, n, e2.ctypes.data, n, dim,
                                            *[r.ctypes.data for r in res], C.byref(ms)))
        return (time.perf_counter() - t0) * 1e3, ms.value

    def guided(kind, model, reverse, res, host=False):
        a = (e1.ctypes.data, n, p1.ctypes.data, e2.ctypes.data, n, p2.ctypes.data, dim, kind, model.ctypes.data, T,
             reverse)
        t0 = time.perf_counter()
        if host:
            N.check(N.lib.gcr_host_match_descriptors_guided(*a, args.threads, *[r.ctypes.data for r in res]))
        else:
            N.check(N.lib.gcr_match_descriptors_guided(ctx, *a, *[r.ctypes.data for r in res], C.byref(ms)))
        return (time.perf_counter() - t0) * 1e3, ms.value

    names = ["unguided"] + [f"{k}_{d}" for k in models for d in ("forward", "reverse")]
    res = {name: [np.empty(n, dtype=np.uint32) for _ in range(4)] for name in names}
    acc = {name: ([], []) for name in names}
    for k in range(-1, args.calls):                   # call -1 warms up; the legs alternate call by call
        for name in names:
            if name == "unguided":
                whole, kern = unguided(res[name])
            else:
                kind, model = models[name[0]]
                whole, kern = guided(kind, model, int(name.endswith("reverse")), res[name])
            if k >= 0:
                acc[name][0].append(kern)
                acc[name][1].append(whole)
    g = {name: {"kernel": quart(v[0]), "call": quart(v[1])} for name, v in acc.items()}
    for k in models:
        g[f"{k}_mutual"] = {"kernel": quart([a + b for a, b in zip(acc[f"{k}_forward"][0], acc[f"{k}_reverse"][0])]),
                            "call": quart([a + b for a, b in zip(acc[f"{k}_forward"][1], acc[f"{k}_reverse"][1])])}
    truth = set(map(tuple, pairs.tolist()))
    for k, (kind, model) in models.items():
        for d in ("forward", "reverse"):
            host = [np.empty(n, dtype=np.uint32) for _ in range(4)]
            host_ms, _ = guided(kind, model, int(d == "reverse"), host, host=True)
            g[f"{k}_{d}"]["host_twin_ms"] = round(host_ms, 2)
            g[f"{k}_{d}"]["equals_host_twin_bitwise"] = all(np.array_equal(a, b)
                                                            for a, b in zip(host, res[f"{k}_{d}"]))
        m, _ = F.match_descriptors_guided(e1, e2, kp1, kp2, model, {"H": "homography", "F": "fundamental"}[k],
                                          args.threshold)
        g[f"{k}_mutual"]["matches"] = len(m)
        g[f"{k}_mutual"]["truth_pairs_found"] = len(set(map(tuple, m.tolist())) & truth)
    # the admissible share and what the kernel skips, from the definition (forward: rows are image 1)
    x2, y2 = p2[:, 0][None, :], p2[:, 1][None, :]
    ct = (n + 31) // 32
    for k, (kind, model) in models.items():
        h = model.reshape(9)
        adm_pairs = tiles = empty_tiles = steps = empty_steps = 0
        for lo in range(0, n, 128):
            x1, y1 = p1[lo:lo + 128, 0][:, None], p1[lo:lo + 128, 1][:, None]
            if kind == 3:
                w = (h[6] * x1 + h[7] * y1) + h[8]
                du = ((h[0] * x1 + h[1] * y1) + h[2]) / w - x2
                dv = ((h[3] * x1 + h[4] * y1) + h[5]) / w - y2
                r = du * du + dv * dv
            else:
                fx0, fx1 = (h[0] * x1 + h[1] * y1) + h[2], (h[3] * x1 + h[4] * y1) + h[5]
                fx2 = (h[6] * x1 + h[7] * y1) + h[8]
                ft0, ft1 = (h[0] * x2 + h[3] * y2) + h[6], (h[1] * x2 + h[4] * y2) + h[7]
                num = (x2 * fx0 + y2 * fx1) + fx2
                r = (num * num) / (((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1)
            adm = np.zeros((128, ct * 32), dtype=bool)
            adm[:r.shape[0], :n] = r <= T
            adm_pairs += int(adm.sum())
            t = adm.reshape(4, 32, ct, 32).any(axis=(1, 3))[:(r.shape[0] + 31) // 32]
            tiles += t.size
            empty_tiles += int((~t).sum())
            st = adm.any(axis=0)
            st = np.concatenate([st, np.zeros(-len(st) % 64, dtype=bool)]).reshape(-1, 64).any(axis=1)
            steps += st.size
            empty_steps += int((~st).sum())
        g[f"{k}_forward"].update({"admissible_share": adm_pairs / (n * n), "tiles": tiles,
                                  "tile_skip_rate": round(empty_tiles / tiles, 6), "steps": steps,
                                  "step_skip_rate": round(empty_steps / steps, 6)})
    out["guided"] = g
    out["threshold_px"] = args.threshold
    print(json.dumps(out))


# ---- sets mode -----------------------------------------------------------------
def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def alternate(legs, calls):
    """name -> list of ms; call -1 warms up; the legs alternate call by call.  Also the last results."""
    acc, last = {name: [] for name in legs}, {}
    for k in range(-1, calls):
        for name, fn in legs.items():
            ms, last[name] = timed(fn)
            if k >= 0:
                acc[name].append(ms)
    return acc, last


def same(a, b):
    return bool(a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes())


def sets_mode():
    kp1, e1, kp2, e2, pairs, Hgt = S.problem_match(n, int(0.4 * n), seed=SEED, dim=dim)
    e = (2.0 * S.IMG_W, S.IMG_H / 2.0, 1.0)
    skew = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
    models = {"H": ("homography", np.ascontiguousarray(Hgt)), "F": ("fundamental", np.ascontiguousarray(skew @ Hgt))}
    a, b = F.DescriptorSet(e1, kp1), F.DescriptorSet(e2, kp2)
    g = {}

    def pageable():
        os.environ["GCR_MATCH_SETS_PAGEABLE"] = "1"
        try:
            return a.match(b)
        finally:
            os.environ.pop("GCR_MATCH_SETS_PAGEABLE", None)

    def create():
        F.DescriptorSet(e1, kp1).close()

    # the C entry with its event breakdown (four doubles) and without events
    mbuf, rbuf, mo = np.empty((n, 2), np.uint32), np.empty(n), C.c_size_t()
    opt = F._match_options(0.8, True)
    ms4 = np.zeros(4)
    events = []

    def c_entry_events():
        N.check(N.lib.gcr_match_sets(ctx, a._handle, b._handle, opt, mbuf.ctypes.data, rbuf.ctypes.data, n,
                                     C.byref(mo), ms4.ctypes.data))
        events.append(ms4.copy())

    def c_entry():
        N.check(N.lib.gcr_match_sets(ctx, a._handle, b._handle, opt, mbuf.ctypes.data, rbuf.ctypes.data, n,
                                     C.byref(mo), None))

    # three groups, each alternating call by call: the array call frees its buffers at its end, which the
    # call after it pays for, so the set call is timed both right after an array call and among set calls only
    acc, last = alternate({"array_call": lambda: F.match_descriptors(e1, e2, ratio=0.8, mutual=True),
                           "set_call": lambda: a.match(b)}, args.calls)
    acc2, last2 = alternate({"set_call_among_set_calls": lambda: a.match(b),
                             "set_call_pageable_download": pageable,
                             "set_c_entry": c_entry,
                             "set_c_entry_with_events": c_entry_events}, args.calls)
    acc3, _ = alternate({"set_create": create}, args.calls)
    acc.update(acc2)
    acc.update(acc3)
    last.update(last2)
    g["match"] = {name: quart(v) for name, v in acc.items()}
    ev = np.array(events[1:])                             # without the warm-up call
    g["match"]["kernels"] = {name: quart(ev[:, k].tolist()) for k, name in
                             enumerate(("all", "forward_search", "reverse_search", "select_launches"))}
    med = lambda name: g["match"][name]["median_ms"]
    g["match"]["set_over_array"] = round(med("set_call") / med("array_call"), 4)
    g["match"]["set_call_not_above_array_call"] = med("set_call") <= med("array_call")
    g["match"]["c_entry_minus_kernels_ms"] = round(med("set_c_entry") - g["match"]["kernels"]["all"]["median_ms"], 4)
    g["match"]["python_over_c_entry_ms"] = round(med("set_call") - med("set_c_entry"), 4)
    g["match"]["matches"] = len(last["set_call"][0])
    g["match"]["equal_bytes"] = same(last["set_call"], last["array_call"]) and \
        same(last["set_call_pageable_download"], last["array_call"])
    g["match"]["workspace"] = list(map(int, workspace()))

    for k, (kind, model) in models.items():
        acc, last = alternate({
            "array_call": lambda: F.match_descriptors_guided(e1, e2, kp1, kp2, model, kind, args.threshold),
            "set_call": lambda: a.match_guided(b, model, kind, args.threshold)}, args.calls)
        g[f"guided_{k}"] = {name: quart(v) for name, v in acc.items()}
        code = {"homography": 3, "fundamental": 4}[kind]
        gopt = F._match_options(None, True)
        ev = []
        for _ in range(args.calls + 1):
            N.check(N.lib.gcr_match_sets_guided(ctx, a._handle, b._handle, code, model.ctypes.data,
                                                args.threshold * args.threshold, gopt, mbuf.ctypes.data,
                                                rbuf.ctypes.data, n, C.byref(mo), ms4.ctypes.data))
            ev.append(ms4.copy())
        ev = np.array(ev[1:])
        g[f"guided_{k}"]["kernels"] = {name: quart(ev[:, q].tolist()) for q, name in
                                       enumerate(("all", "forward_search", "reverse_search", "select_launches"))}
        sm, am = g[f"guided_{k}"]["set_call"]["median_ms"], g[f"guided_{k}"]["array_call"]["median_ms"]
        g[f"guided_{k}"].update({"set_over_array": round(sm / am, 4), "set_call_not_above_array_call": sm <= am,
                                 "matches": len(last["set_call"][0]),
                                 "equal_bytes": same(last["set_call"], last["array_call"])})
    a.close()
    b.close()

    # match_pairs: sets of 2 000 .. 10 000 rows, every unordered pair
    ns = np.linspace(2000, 10000, args.pair_sets).astype(int).tolist()
    prng = np.random.default_rng(SEED + 1)
    ds = [prng.integers(0, 256, (k, dim), dtype=np.uint8) for k in ns]
    sets = [F.DescriptorSet(d) for d in ds]
    pr = [(i, j) for i in range(len(ns)) for j in range(i + 1, len(ns))]
    acc, last = alternate({
        "array_loop": lambda: [F.match_descriptors(ds[i], ds[j], ratio=0.8, mutual=True) for i, j in pr],
        "set_loop": lambda: [sets[i].match(sets[j]) for i, j in pr],
        "match_pairs": lambda: F.match_pairs(sets, pr)}, args.pair_calls)
    g["pairs"] = {name: {**quart(v), "pairs_per_s": round(len(pr) / (statistics.median(v) * 1e-3), 1)}
                  for name, v in acc.items()}
    g["pairs"].update({"sets": len(ns), "rows": ns, "pairs": len(pr),
                       "equal_bytes": all(same(x, y) and same(x, z) for x, y, z in
                                          zip(last["match_pairs"], last["set_loop"], last["array_loop"])),
                       "workspace": list(map(int, workspace()))})
    for s_ in sets:
        s_.close()
    out["sets"] = g
    print(json.dumps(out))


# ---- knn mode ------------------------------------------------------------------
def knn_mode():
    ks = (2, 4, 8)
    ms = C.c_double()
    two = [np.empty(n, dtype=np.uint32) for _ in range(4)]
    res = {k: (np.empty((n, k), np.uint32), np.empty((n, k), np.uint32)) for k in ks}
    sres = {k: (np.empty((n, k), np.uint32), np.empty((n, k), np.uint32)) for k in ks}
    a, b = F.DescriptorSet(d1), F.DescriptorSet(d2)

    def match_leg():
        whole = gpu_call(two, ms)
        return whole, ms.value

    def knn_leg(k):
        t0 = time.perf_counter()
        N.check(N.lib.gcr_knn_descriptors(ctx, d1.ctypes.data, n, d2.ctypes.data, n, dim, k, res[k][0].ctypes.data,
                                          res[k][1].ctypes.data, C.byref(ms)))
        return (time.perf_counter() - t0) * 1e3, ms.value

    def set_leg(k):
        t0 = time.perf_counter()
        N.check(N.lib.gcr_knn_sets(ctx, a._handle, b._handle, k, sres[k][0].ctypes.data, sres[k][1].ctypes.data,
                                   C.byref(ms)))
        return (time.perf_counter() - t0) * 1e3, ms.value

    legs = {"k_match": match_leg}
    for k in ks:
        legs[f"knn_k{k}"] = lambda k=k: knn_leg(k)
        legs[f"knn_set_k{k}"] = lambda k=k: set_leg(k)
    g = {}
    for s in [int(v) for v in args.knn_splits.split(",")]:
        if s:
            os.environ["GCR_MATCH_SPLIT"] = str(s)
        else:
            os.environ.pop("GCR_MATCH_SPLIT", None)
        acc = {name: ([], []) for name in legs}
        for c in range(-1, args.calls):                   # call -1 warms up; the legs alternate call by call
            for name, fn in legs.items():
                whole, kern = fn()
                if c >= 0:
                    acc[name][0].append(kern)
                    acc[name][1].append(whole)
        r = {name: {"kernel": quart(v[0]), "call": quart(v[1])} for name, v in acc.items()}
        base = r["k_match"]["kernel"]["median_ms"]
        for k in ks:
            r[f"knn_k{k}"]["kernel_over_k_match"] = round(r[f"knn_k{k}"]["kernel"]["median_ms"] / base, 3)
            r[f"knn_k{k}"]["mac_per_s"] = round(n * n * dim / (r[f"knn_k{k}"]["kernel"]["median_ms"] * 1e-3))
        r["k2_equals_match_descriptors"] = bool(
            np.array_equal(res[2][0][:, 0], two[0]) and np.array_equal(res[2][1][:, 0], two[1]) and
            np.array_equal(res[2][0][:, 1], two[2]) and np.array_equal(res[2][1][:, 1], two[3]))
        r["set_equals_array_entry"] = all(np.array_equal(res[k][q], sres[k][q]) for k in ks for q in (0, 1))
        r["k4_is_a_prefix_of_k8"] = bool(np.array_equal(res[8][0][:, :4], res[4][0]) and
                                         np.array_equal(res[8][1][:, :4], res[4][1]))
        g[f"split{s}"] = r
    os.environ.pop("GCR_MATCH_SPLIT", None)
    hi, hd = np.empty((n, 8), np.uint32), np.empty((n, 8), np.uint32)
    t0 = time.perf_counter()
    N.check(N.lib.gcr_host_knn_descriptors(d1.ctypes.data, n, d2.ctypes.data, n, dim, 8, args.threads, hi.ctypes.data,
                                           hd.ctypes.data))
    g["host_twin_k8"] = {"threads": args.threads, "ms": round((time.perf_counter() - t0) * 1e3, 2),
                         "equals_gpu_bitwise": bool(np.array_equal(hi, res[8][0]) and np.array_equal(hd, res[8][1]))}
    a.close()
    b.close()
    out["knn"] = g
    print(json.dumps(out))


def workspace():
    w = (C.c_uint64 * 2)()
    N.check(N.lib.gcr_debug_match_workspace(ctx, w))
    return w[0], w[1]


if args.guided:
    guided_mode()
    sys.exit(0)
if args.knn:
    knn_mode()
    sys.exit(0)
if args.sets:
    sets_mode()
    sys.exit(0)

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
