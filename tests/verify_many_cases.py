"""Shared by tests/test_verify_many.py and tests/test_gpu_verify_many.py: the
callers of gcr_verify_many / gcr_host_verify_many, an independent numpy
restatement of csrc/verify_many.h's rule, and the problems."""
import ctypes as C
import functools
import os

import numpy as np

from pygcransac import _native as N
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
H4, F7 = N.SOLVER_HOMOGRAPHY4, N.SOLVER_FUNDAMENTAL7
M_OF = {H4: 4, F7: 7}
PER_OF = {H4: 1, F7: 3}
DEFAULT_MODEL = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])


def pack(problems):
    off = np.zeros(len(problems) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in problems])
    rows = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 4) for p in problems]))
    return rows, off


def run(solver, problems, thr, seeds, slots, *, ctx=None, host=False, threads=4, masks=True):
    """(records, [mask per problem]) of one call; host=True: the twin"""
    P = len(problems)
    rows, off = pack(problems)
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, dtype=np.float64), (P,)))
    seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (P,)))
    out = (N.ManyResult * P)()
    mk = np.full(int(off[-1]), 7, dtype=np.uint8)
    mp = mk.ctypes.data if masks else None
    if host:
        N.check(N.lib.gcr_host_verify_many(solver, rows.ctypes.data, off.ctypes.data, P, thr.ctypes.data,
                                           seeds.ctypes.data, slots, threads, out, mp))
    else:
        N.check(N.lib.gcr_verify_many(ctx, solver, rows.ctypes.data, off.ctypes.data, P, thr.ctypes.data,
                                      seeds.ctypes.data, slots, out, mp, None))
    rec = np.frombuffer(out, dtype=N.MANY_DT).copy()
    return rec, [mk[int(off[p]):int(off[p + 1])].copy() for p in range(P)]


def same(a, b):
    """two (records, masks) results, byte for byte"""
    return a[0].tobytes() == b[0].tobytes() and len(a[1]) == len(b[1]) and \
        all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


# ------------------------------------------------------ numpy restatement --
def sq_residual(solver, rows, h):
    """h_sq_residual / f_sq_sampson in their operation order; numpy's
    elementwise operations round once each"""
    x1, y1, x2, y2 = (rows[:, k] for k in range(4))
    if solver == H4:
        w = (h[6] * x1 + h[7] * y1) + h[8]
        u = ((h[0] * x1 + h[1] * y1) + h[2]) / w
        v = ((h[3] * x1 + h[4] * y1) + h[5]) / w
        du, dv = u - x2, v - y2
        return du * du + dv * dv
    fx0 = (h[0] * x1 + h[1] * y1) + h[2]
    fx1 = (h[3] * x1 + h[4] * y1) + h[5]
    fx2 = (h[6] * x1 + h[7] * y1) + h[8]
    ft0 = (h[0] * x2 + h[3] * y2) + h[6]
    ft1 = (h[1] * x2 + h[4] * y2) + h[7]
    num = (x2 * fx0 + y2 * fx1) + fx2
    den = ((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1
    return (num * num) / den


def restate(solver, rows, thr, seed, slots, scores=None):
    """one problem by the rule: a dict of the record's fields and the mask;
    scores (a list, optional) takes every live hypothesis' (index, score)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n, m, per = len(rows), M_OF[solver], PER_OF[solver]
    thr = float(thr)
    T = (2.25 * thr) * thr
    dp, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    idx = np.zeros(m, dtype=np.uint32)
    models = np.zeros(27)
    cnt = C.c_uint32()
    r = dict(models=0, iterations=0, best_slot=-1, best_hypothesis=0, best_inliers=0, best_score=0.0,
             best_model=DEFAULT_MODEL.copy())
    best = 0.0
    with np.errstate(all="ignore"):
        for s in range(slots):
            inc, found = 102, 0
            for a in range(101):
                if N.lib.gcr_host_sample(int(seed), s, a, 0, 0, n, m, idx.ctypes.data_as(u32p)) != 0:
                    continue
                assert N.lib.gcr_host_solve_minimal(solver, rows.ctypes.data_as(dp), n, idx.ctypes.data_as(u32p),
                                                    models.ctypes.data_as(dp), C.byref(cnt)) == 0
                if cnt.value:
                    inc, found = a + 1, cnt.value
                    break
            r["iterations"] += inc
            for k in range(found):
                r["models"] += 1
                h = models[9 * k:9 * k + 9].copy()
                r2 = sq_residual(solver, rows, h)
                inl = r2 <= T
                n0, v0 = int(inl.sum()), 0.0
                for x in r2[inl].tolist():
                    v0 += -x
                total = v0
                if n0 < m:
                    total = 0.0
                else:
                    msac = v0 / T + float(n0)
                    total -= v0
                    total += msac
                if scores is not None:
                    scores.append((s * per + k, total))
                if best < total:
                    best = total
                    r.update(best_slot=s, best_hypothesis=k, best_inliers=n0, best_score=total, best_model=h)
        mask = np.zeros(n, dtype=np.uint8)
        if r["best_slot"] >= 0:
            mask = (sq_residual(solver, rows, r["best_model"]) <= T).astype(np.uint8)
    return r, mask


def record_equals(rec, r):
    return all(rec[k] == r[k] for k in ("models", "iterations", "best_slot", "best_hypothesis", "best_inliers")) and \
        np.float64(rec["best_score"]).tobytes() == np.float64(r["best_score"]).tobytes() and \
        np.asarray(rec["best_model"]).tobytes() == np.asarray(r["best_model"], dtype=np.float64).tobytes()


# ---------------------------------------------------------------- problems --
@functools.lru_cache(maxsize=None)
def golden_f(n):
    with np.load(os.path.join(HERE, "golden", "corr", f"f_n{n}.npz"), allow_pickle=False) as z:
        return np.ascontiguousarray(z["correspondences"]), float(z["thr"])


def _first_rows(problem, n):
    """n rows of a synthetic problem at 50 % outliers; fewer than 16: inliers
    only, so that a problem of a minimal sample's size has a model"""
    rows, truth = problem[0], problem[1]
    return np.ascontiguousarray(rows[truth][:n] if n < 16 else rows[:n])


@functools.lru_cache(maxsize=None)
def rows_h(n, seed=3):
    return _first_rows(S.problem_h(max(n, 40), 0.5, seed=seed), n)


@functools.lru_cache(maxsize=None)
def rows_f(n, seed=5):
    return _first_rows(S.problem_f(max(n, 40), 0.5, seed=seed), n)


def one_point(n):
    return np.tile(np.array([[100.0, 200.0, 110.0, 190.0]]), (n, 1))
