"""k-nearest-neighbour search: an independent numpy restatement of
csrc/match_knn.h's definition, the crafted inputs the host and GPU tests share,
and thin ctypes wrappers of the C entries."""
import numpy as np

import match_cases as MC
from pygcransac import _native as N

NONE = MC.NONE
KS = [1, 2, 3, 4, 5, 8]


def restate(d1, d2, k):
    """idx, dist (uint32, n1 x k): int64 brute force, a stable argsort of the
    distances (stable = ties by the lower index, the order (d, j)), the first
    k; NONE from position n2 on."""
    a = d1.astype(np.int64)
    b = d2.astype(np.int64)
    n1, n2 = len(a), len(b)
    idx = np.full((n1, k), NONE, dtype=np.uint32)
    dist = np.full((n1, k), NONE, dtype=np.uint32)
    m = min(k, n2)
    for lo in range(0, n1, 256):                       # row blocks: bounded memory
        blk = a[lo:lo + 256]
        d = (blk * blk).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (blk @ b.T)
        order = np.argsort(d, axis=1, kind="stable")[:, :m]
        idx[lo:lo + 256, :m] = order
        dist[lo:lo + 256, :m] = np.take_along_axis(d, order, axis=1)
    return idx, dist


def crafted():
    """name -> (D1, D2), dim 32: the inputs aimed at the selection and the merges."""
    rng = np.random.default_rng(20260915)
    cases = {}
    # a two-letter alphabet: distances take at most 33 values, so ties run across lane halves, tiles and splits
    letters = np.array([3, 250], dtype=np.uint8)
    cases["alphabet"] = (letters[rng.integers(0, 2, (130, 32))], letters[rng.integers(0, 2, (515, 32))])
    # every column equal: idx[i] = 0 .. k - 1
    cases["all_equal"] = (rng.integers(0, 256, (37, 32), dtype=np.uint8), np.full((300, 32), 77, np.uint8))
    # distances fall strictly with j: every column is a new best, no tile is skipped
    ramp = np.repeat((255 - np.arange(256)).astype(np.uint8)[:, None], 32, axis=1)
    cases["descending"] = (np.zeros((70, 32), np.uint8), ramp)
    # the mirror image: only the first k columns ever insert
    cases["ascending"] = (np.zeros((70, 32), np.uint8), np.ascontiguousarray(ramp[::-1]))
    return cases


def all_crafted():
    """crafted() and match_cases.crafted's four cases (dim 128)"""
    cases = dict(crafted())
    cases.update(MC.crafted(128))
    return cases


def _out(n1, k):
    return np.empty((n1, k), dtype=np.uint32), np.empty((n1, k), dtype=np.uint32)


def host(d1, d2, k, threads=1):
    d1 = np.ascontiguousarray(d1, dtype=np.uint8)
    d2 = np.ascontiguousarray(d2, dtype=np.uint8)
    idx, dist = _out(len(d1), k)
    N.check(N.lib.gcr_host_knn_descriptors(d1.ctypes.data, len(d1), d2.ctypes.data, len(d2), d1.shape[1], k, threads,
                                           idx.ctypes.data, dist.ctypes.data))
    return idx, dist


def gpu(d1, d2, k, device=None, ms=None):
    d1 = np.ascontiguousarray(d1, dtype=np.uint8)
    d2 = np.ascontiguousarray(d2, dtype=np.uint8)
    idx, dist = _out(len(d1), k)
    N.check(N.lib.gcr_knn_descriptors(N.context(device), d1.ctypes.data, len(d1), d2.ctypes.data, len(d2),
                                      d1.shape[1], k, idx.ctypes.data, dist.ctypes.data, ms))
    return idx, dist


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))
