"""The PROSAC stop (GCR_FLAG_PROSAC_STOP, csrc/prosac_stop.h): the definition
restated in Python (floats are IEEE doubles, integers exact), the host entries'
wrappers and the whole-run problems shared by test_prosac_stop.py (CPU) and
test_gpu_prosac_stop.py."""
import ctypes as C
import math

import numpy as np

import prosac_cases as PC
from pygcransac import _native as N

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
f64p = C.POINTER(C.c_double)
U64_MAX = 2 ** 64 - 1

MIN_LENGTH = 20                          # kProsacStopMinLength
BETA = 0.05                              # kProsacStopBeta
Z = 1.6448536269514722                   # kProsacStopZ
B = 256                                  # kScoreBlock (csrc/kernels.hip): the stop kernel's tile


# ---- the definition, restated -------------------------------------------------
def imin_ref(n, m):
    nb = float(n) * BETA
    v = nb * (1.0 - BETA)
    s = math.sqrt(v)
    zs = Z * s
    t = nb + zs
    return m + int(math.ceil(t))


def tables_ref(n, m, convergence, conf):
    """(Imin, qmin), n + 1 entries each, those below m are 0"""
    g = PC.growth_ref(n, m, convergence)
    log_prob = math.log(1.0 - conf)
    imin = [0] * (n + 1)
    qmin = [0.0] * (n + 1)
    for k in range(m, n + 1):
        imin[k] = imin_ref(k, m)
        qmin[k] = 1.0 - math.exp(log_prob / float(int(g[k])))
    return np.array(imin, dtype=np.uint32), np.array(qmin, dtype=np.float64)


def feasible_ref(I, n, m, imin, qmin):
    """(non-randomness, coverage) of prefix length n holding I inliers"""
    r = float(I) / float(n)
    q = r
    for _ in range(m - 1):
        q = q * r
    return I >= int(imin[n]), q >= float(qmin[n])


def better_ref(Ia, na, Ib, nb):
    l, r = Ia * nb, Ib * na
    return l > r or (l == r and na > nb)


def choose_ref(mask, m, imin, qmin):
    """(I*, n*) of the mask in row order"""
    n = len(mask)
    cum = np.cumsum(np.asarray(mask) != 0)
    best = (int(cum[-1]), n)
    for k in range(max(m, MIN_LENGTH), n):
        I = int(cum[k - 1])
        if all(feasible_ref(I, k, m, imin, qmin)) and better_ref(I, k, *best):
            best = (I, k)
    return best


def iteration_number_ref(inliers, n, m, conf):
    """GCRANSAC::getIterationNumber (GCRANSAC.h:738-757) for one class on the
    ratio inliers / n"""
    ratio = inliers / n                         # int / int: correctly rounded
    q = 1.0 * math.pow(ratio, float(m))
    lg = math.log(1 - q) if 1 - q > 0 else -math.inf
    if abs(lg) < np.finfo(np.float64).eps:
        return U64_MAX
    return int(math.ceil(math.log(1 - conf) / lg))


# ---- host entries ---------------------------------------------------------------
def host_tables(n, m, convergence, conf):
    imin = np.zeros(n + 1, dtype=np.uint32)
    qmin = np.zeros(n + 1, dtype=np.float64)
    N.check(N.lib.gcr_host_prosac_stop_tables(n, m, convergence, conf, imin.ctypes.data_as(u32p),
                                              qmin.ctypes.data_as(f64p)))
    return imin, qmin


def host_choose(mask, m, imin, qmin):
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    imin = np.ascontiguousarray(imin, dtype=np.uint32)
    qmin = np.ascontiguousarray(qmin, dtype=np.float64)
    bi, bn = C.c_uint32(), C.c_uint32()
    N.check(N.lib.gcr_host_prosac_stop(mask.ctypes.data_as(u8p), len(mask), m, imin.ctypes.data_as(u32p),
                                       qmin.ctypes.data_as(f64p), C.byref(bi), C.byref(bn)))
    return bi.value, bn.value


def host_stop_number(best_i, best_n, m, conf):
    out = C.c_uint64()
    N.check(N.lib.gcr_host_prosac_stop_number(best_i, best_n, m, conf, C.byref(out)))
    return out.value


def host_uniform_number(inliers, n, m, conf):
    """the uniform stop through the existing host entry: equal quanta of 1 give
    the ratio inliers / n exactly (test_guided_stop.py pins that identity)"""
    out = C.c_uint64()
    N.check(N.lib.gcr_host_guided_iterations(inliers, n, m, conf, C.byref(out)))
    return out.value


# ---- crafted masks ----------------------------------------------------------------
def mask_of(n, inlier_rows):
    mk = np.zeros(n, dtype=np.uint8)
    mk[np.asarray(list(inlier_rows), dtype=np.int64)] = 1
    return mk


def prefix_mask(n, k, tail=()):
    """the first k rows inliers, then outliers but for the rows in `tail`"""
    return mask_of(n, list(range(k)) + list(tail))


# ---- whole runs ---------------------------------------------------------------------
# prosac_cases.e2e_problem's data (N = 2000, 95 % outliers, noisy scores) at
# min_iters = 50, max_iters = 5000, confidence 0.99.  test_prosac_stop.py
# asserts on the CPU that the stop of the truth-inlier set in score order has
# n* < N and a stop number <= min_iters, so a flag-set run that finds the truth
# model ends at the iteration floor.
E2E_MIN_ITERS = 50
E2E_MAX_ITERS = 5000
E2E_CONF = 0.99
E2E_SEEDS = PC.E2E_SEEDS


def e2e_problem(solver):
    return PC.e2e_problem(solver)
