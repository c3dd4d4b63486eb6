"""Shared by the guided-sampling tests: the weight patterns, an independent
numpy restatement of csrc/guided.h's definition (Philox words from the
oracle, np.searchsorted on a CDF summed by a Python loop), and thin wrappers
of the host entry points."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_ffi as O
from pygcransac import _native as N

u32p = C.POINTER(C.c_uint32)
NS = (7, 8, 255, 256, 257, 1000, 10007)
PATTERNS = ("ones", "loguniform", "zero_runs", "exactly_m", "heavy", "heavy90")
K_MAX_DRAWS = 4096                     # philox.h kMaxSampleDraws
ALL_ONES = 0xFFFFFFFF


def weights(pattern, n, m, seed=11):
    """fp64 weights of length n; may hold fewer than m positive entries (then
    the engine must refuse them)."""
    rng = np.random.default_rng(seed + 1000 * n + m)
    if pattern == "ones":
        return np.ones(n)
    if pattern == "loguniform":         # 1e-300 .. 1e300, scaled so the sum stays finite
        return 10.0 ** rng.uniform(-300.0, 300.0, n) / n
    if pattern == "zero_runs":          # half zeros in runs (they straddle bucket boundaries, one ends the CDF)
        run = max(1, min(37, n // 4))
        w = rng.uniform(0.5, 2.0, n)
        w[(np.arange(n) // run) % 2 == 1] = 0.0
        return w
    if pattern == "exactly_m":
        w = np.zeros(n)
        w[rng.choice(n, m, replace=False)] = rng.uniform(0.5, 2.0, m)
        return w
    if pattern == "heavy":              # one entry holds 1 - 1e-12 of the mass
        w = np.full(n, 1e-12 / (n - 1))
        w[n // 2] = 1.0 - 1e-12
        return w
    if pattern == "heavy90":            # repeats are common, samples still complete
        w = np.full(n, 0.1 / (n - 1))
        w[n // 2] = 0.9
        return w
    raise ValueError(pattern)


def cdf_of(w):
    """c[i] = c[i-1] + w[i], sequentially in index order in fp64."""
    c = np.empty(len(w))
    acc = 0.0
    for i, wi in enumerate(w):
        acc = acc + float(wi)
        c[i] = acc
    return c


def words(seed, index, sub, stream=0, cls=0):
    """The WordStream of philox.h's counter layout: key = {seed lo, seed hi},
    ctr = {index lo, index hi, sub, stream << 24 | cls << 16 | block}; each
    block yields two 64-bit words."""
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    block = 0
    while True:
        o = O.philox([index & 0xFFFFFFFF, (index >> 32) & 0xFFFFFFFF, sub,
                      (stream << 24) | ((cls & 0xFF) << 16) | (block & 0xFFFF)], key)
        yield o[0] | (o[1] << 32)
        yield o[2] | (o[3] << 32)
        block += 1


def ref_sample(c, seed, index, sub, m):
    """The definition, restated: m distinct indices in draw order, or None when
    the draw budget runs out."""
    n = len(c)
    total = float(c[-1])
    out = []
    for k, W in enumerate(words(seed, index, sub)):
        if k >= K_MAX_DRAWS:
            return None
        r = float(W >> 11) * 2.0 ** -53          # exact: a 53-bit integer times a power of two
        u = r * total                            # one rounding
        i = int(np.searchsorted(c, u, side="right"))
        if i == n:                               # u rounded up to total
            i = int(np.searchsorted(c, total, side="left"))
        if i not in out:
            out.append(i)
            if len(out) == m:
                return out


def host_sample_guided(seed, index, sub, w, m):
    """gcr_host_sample_guided: (rc, indices)."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.zeros(m, dtype=np.uint32)
    rc = N.lib.gcr_host_sample_guided(seed, index, sub, 0, 0, w.ctypes.data, len(w), m, out.ctypes.data_as(u32p))
    return rc, out


def host_samples(seed, slot0, nslots, attempt, w, m, threads=8):
    """(nslots, m) uint32: gcr_host_sample_guided of every slot's attempt,
    all-ones rows where the budget ran out (the calls release the GIL)."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.zeros((nslots, m), dtype=np.uint32)

    def work(lo, hi):
        row = np.zeros(m, dtype=np.uint32)
        p = row.ctypes.data_as(u32p)
        for s in range(lo, hi):
            rc = N.lib.gcr_host_sample_guided(seed, slot0 + s, attempt, 0, 0, w.ctypes.data, len(w), m, p)
            out[s] = row if rc == 0 else ALL_ONES

    step = (nslots + threads - 1) // threads
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda lo: work(lo, min(nslots, lo + step)), range(0, nslots, step)))
    return out


def host_samples_uniform(seed, slot0, nslots, attempt, n, m):
    out = np.zeros((nslots, m), dtype=np.uint32)
    row = np.zeros(m, dtype=np.uint32)
    for s in range(nslots):
        rc = N.lib.gcr_host_sample(seed, slot0 + s, attempt, 0, 0, n, m, row.ctypes.data_as(u32p))
        out[s] = row if rc == 0 else ALL_ONES
    return out


def solve_minimal(solver, corr, idx):
    """gcr_host_solve_minimal: the models (k, 9), k = 0 .. 3."""
    c = np.ascontiguousarray(corr, dtype=np.float64)
    i = np.ascontiguousarray(idx, dtype=np.uint32)
    models = np.zeros(27)
    cnt = C.c_uint32()
    N.check(N.lib.gcr_host_solve_minimal(solver, c.ctypes.data_as(C.POINTER(C.c_double)), c.shape[0],
                                         i.ctypes.data_as(u32p), models.ctypes.data_as(C.POINTER(C.c_double)),
                                         C.byref(cnt)))
    return models.reshape(3, 9)[:cnt.value].copy()
