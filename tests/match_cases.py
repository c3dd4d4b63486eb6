"""Descriptor matching: an independent numpy restatement of csrc/match.h's
definition, the shapes and the crafted inputs the host and GPU tests share,
and thin ctypes wrappers of the two C entries."""
import ctypes as C

import numpy as np

from pygcransac import _native as N

NONE = 0xFFFFFFFF
SHAPES = [(1, 1), (1, 2), (2, 1), (31, 33), (33, 31), (128, 128), (129, 257), (1000, 257)]
DIMS = [32, 128, 512]


def restate(d1, d2):
    """idx, dist, idx2, dist2 (uint32): int64 brute force, then a stable
    argsort of the distances (stable = ties by the lower index, the order
    (d, j))."""
    a = d1.astype(np.int64)
    b = d2.astype(np.int64)
    n1, n2 = len(a), len(b)
    out = [np.full(n1, NONE, dtype=np.uint32) for _ in range(4)]
    for lo in range(0, n1, 256):                       # row blocks: bounded memory
        blk = a[lo:lo + 256]
        d = (blk * blk).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (blk @ b.T)
        order = np.argsort(d, axis=1, kind="stable")
        rows = np.arange(len(blk))
        out[0][lo:lo + 256] = order[:, 0]
        out[1][lo:lo + 256] = d[rows, order[:, 0]]
        if n2 > 1:
            out[2][lo:lo + 256] = order[:, 1]
            out[3][lo:lo + 256] = d[rows, order[:, 1]]
    return out


def random_pair(n1, n2, dim, seed=0):
    rng = np.random.default_rng([20260301, n1, n2, dim, seed])
    return rng.integers(0, 256, (n1, dim), dtype=np.uint8), rng.integers(0, 256, (n2, dim), dtype=np.uint8)


def crafted(dim=128):
    """name -> (D1, D2): the inputs aimed at one mistake each."""
    rng = np.random.default_rng([20260302, dim])
    cases = {}
    # only the values around the sign shift x - 128 (0, 127, 128, 255); many ties
    vals = np.array([0, 127, 128, 255], dtype=np.uint8)
    cases["sign_shift"] = (vals[rng.integers(0, 4, (70, dim))], vals[rng.integers(0, 4, (97, dim))])
    # a padded (zero) column would be nearer than every real one: dist = dim * 255^2
    cases["padding"] = (np.zeros((5, dim), np.uint8), np.full((33, dim), 255, np.uint8))
    # duplicate rows in D2: best and second at equal distance, lower index first
    d2 = rng.integers(0, 256, (40, dim), dtype=np.uint8)
    d2 = np.concatenate([d2, d2[::-1], d2[:7]])
    cases["duplicates"] = (np.clip(d2[:40].astype(np.int64) + rng.integers(-3, 4, (40, dim)), 0, 255).astype(np.uint8),
                           d2)
    # D2 a permutation of D1: dist 0, idx the inverse permutation
    d1 = rng.integers(0, 256, (150, dim), dtype=np.uint8)
    cases["permutation"] = (d1, d1[rng.permutation(150)])
    return cases


def _call(fn, d1, d2, extra_front=(), extra_mid=(), extra_back=()):
    d1 = np.ascontiguousarray(d1, dtype=np.uint8)
    d2 = np.ascontiguousarray(d2, dtype=np.uint8)
    out = [np.empty(len(d1), dtype=np.uint32) for _ in range(4)]
    N.check(fn(*extra_front, d1.ctypes.data, len(d1), d2.ctypes.data, len(d2), d1.shape[1], *extra_mid,
               *[o.ctypes.data for o in out], *extra_back))
    return out


def host(d1, d2, threads=1):
    return _call(N.lib.gcr_host_match_descriptors, d1, d2, extra_mid=(threads,))


def gpu(d1, d2, device=None):
    return _call(N.lib.gcr_match_descriptors, d1, d2, extra_front=(N.context(device),), extra_back=(None,))


def tiling():
    """rows per workgroup, columns per step, least columns per split"""
    t = (C.c_uint32 * 3)()
    N.lib.gcr_match_tiling(t)
    return tuple(t)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))
