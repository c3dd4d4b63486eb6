"""PROSAC sampling (csrc/prosac.h): the growth table restated in Python, the
host twins' wrappers and the whole-run problems shared by test_prosac.py (CPU)
and test_gpu_prosac.py."""
import ctypes as C
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import guided_cases as G
from pygcransac import _native as N
from pygcransac import pygcransac as P
from pygcransac import synthetic as S

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
ALL_ONES = 0xFFFFFFFF

H4, F7, E5, G3, S2 = (N.SOLVER_HOMOGRAPHY4, N.SOLVER_FUNDAMENTAL7, N.SOLVER_ESSENTIAL5,
                      N.SOLVER_ESSENTIAL3_GRAVITY, N.SOLVER_HOMOGRAPHY2_SIFT)
M_OF = {H4: 4, F7: 7, E5: 5, G3: 3, S2: 2}
DEFAULT_CONVERGENCE = 100000


# ---- the definition, restated -------------------------------------------------
def growth_ref(n, m, convergence):
    """g[0 .. n] of prosac.h: Python floats are IEEE doubles, every operation
    rounds once."""
    g = [0] * (n + 1)
    T = float(convergence)
    for i in range(m):
        T = T * float(m - i) / float(n - i)
    g[m] = 1
    for k in range(m, n):
        T1 = T * float(k + 1) / float(k + 1 - m)
        g[k + 1] = g[k] + int(math.ceil(T1 - T))
        T = T1
    return np.array(g, dtype=np.uint64)


def pool_ref(g, n, m, slot):
    """n(slot + 1): the smallest n in [m, N] with g[n] >= slot + 1; 0 past g[N]."""
    t = slot + 1
    if t > int(g[n]):
        return 0
    return m + int(np.searchsorted(g[m:], t, side="left"))


# ---- host twins ---------------------------------------------------------------
def host_growth(n, m, convergence):
    g = np.zeros(n + 1, dtype=np.uint64)
    N.check(N.lib.gcr_host_prosac_growth(n, m, convergence, g.ctypes.data_as(u64p)))
    return g


def host_pool(n, m, convergence, slot):
    out = C.c_uint32()
    N.check(N.lib.gcr_host_prosac_pool(n, m, convergence, slot, C.byref(out)))
    return out.value


def host_sample_prosac(seed, slot, attempt, n, m, convergence):
    """gcr_host_sample_prosac: (rc, indices)"""
    out = np.zeros(m, dtype=np.uint32)
    rc = N.lib.gcr_host_sample_prosac(seed, slot, attempt, n, m, convergence, out.ctypes.data_as(u32p))
    return rc, out


def host_sample_uniform(seed, slot, attempt, n, m):
    """gcr_host_sample on the main stream, class 0: (rc, indices)"""
    out = np.zeros(m, dtype=np.uint32)
    rc = N.lib.gcr_host_sample(seed, slot, attempt, 0, 0, n, m, out.ctypes.data_as(u32p))
    return rc, out


def composed_sample(g, seed, slot, attempt, n, m):
    """The PROSAC sample built from the existing primitives: gcr_host_sample
    over the pool's first n - 1 rows with m - 1 indices plus [n - 1] in the
    growth phase, the uniform sample past g[N]."""
    pool = pool_ref(g, n, m, slot)
    if pool == 0:
        return host_sample_uniform(seed, slot, attempt, n, m)
    rc, head = host_sample_uniform(seed, slot, attempt, pool - 1, m - 1)
    return rc, np.append(head, np.uint32(pool - 1)).astype(np.uint32)


def host_samples_prosac(seed, slot0, nslots, attempt, n, m, convergence, threads=8):
    """(nslots, m) uint32: the definition's sample of every slot's attempt
    (composed_sample; one growth table for all), all-ones rows where the budget
    ran out."""
    g = host_growth(n, m, convergence)
    out = np.zeros((nslots, m), dtype=np.uint32)

    def work(lo, hi):
        for s in range(lo, hi):
            rc, idx = composed_sample(g, seed, slot0 + s, attempt, n, m)
            out[s] = idx if rc == 0 else ALL_ONES

    step = (nslots + threads - 1) // threads
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda lo: work(lo, min(nslots, lo + step)), range(0, nslots, step)))
    return out


# ---- whole runs ---------------------------------------------------------------
# H and F at N = 2000 and 95 % outliers under a budget of 32 iterations; noisy
# quality scores: truth inliers N(MU, 1), outliers N(0, 1).  MU and the data
# seed are chosen so that (test_prosac.py asserts both on the CPU)
#   - the first m ordered rows contain an outlier: slot 0 alone does not solve it;
#   - every tested seed draws an all-truth-inlier sample within the run's budget.
E2E_N = 2000
E2E_OUTLIERS = 0.95
E2E_BUDGET = 32
E2E_SEEDS = (0, 1, 2, 3, 4)
E2E_MU = {H4: 1.5, F7: 2.25}
E2E_DATA_SEED = {H4: 29, F7: 6}


def e2e_problem(solver):
    """corr, truth, thr, scores -- in the caller's (shuffled) order"""
    seed = E2E_DATA_SEED[solver]
    make = S.problem_h if solver == H4 else S.problem_f
    corr, truth, _, thr = make(n=E2E_N, outlier_ratio=E2E_OUTLIERS, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    scores = rng.normal(0.0, 1.0, E2E_N) + np.where(truth, E2E_MU[solver], 0.0)
    return corr, truth, thr, scores


def budget_walk(solver, corr_sorted, truth_sorted, seed, convergence=DEFAULT_CONVERGENCE, budget=E2E_BUDGET):
    """The main loop's slots under `budget` iterations, on the CPU: a slot's
    winning attempt is the first that yields a model (host sampler + host
    minimal solver) and costs attempt + 1 iterations; the loop ends once the
    budget is spent.  Returns [(slot, attempt, all_truth_inliers)]."""
    n, m = len(corr_sorted), M_OF[solver]
    out = []
    it = slot = 0
    while it < budget:
        won = None
        for a in range(101):
            rc, idx = host_sample_prosac(seed, slot, a, n, m, convergence)
            if rc == 0 and len(G.solve_minimal(solver, corr_sorted, idx)) > 0:
                won = (slot, a, bool(truth_sorted[idx].all()))
                break
        it += (won[1] + 1) if won else 102
        if won:
            out.append(won)
        slot += 1
    return out


def order_of(scores):
    return P.prosac_order(scores)
