"""Descriptor sets: what the host and GPU tests of the set entries share -- an
independent numpy statement of csrc/match_select.h's rule, thin ctypes wrappers
of gcr_host_match_select, gcr_match_select_tiling and
gcr_debug_match_workspace, and the option grid."""
import ctypes as C

import numpy as np

import match_cases as MC
from pygcransac import _native as N
from pygcransac import features as F

NONE = MC.NONE
RATIOS = [None, 0.8, 1e-9, 1e9]
KIND_NAMES = {3: "homography", 4: "fundamental"}


def numpy_rule(search, back, guided, ratio=None, max_distance=None):
    """(matches int64 (M, 2), ratios float64 (M,)) from a search's idx, dist,
    idx2, dist2 and the reverse search's idx (or None): match_select.h's text
    in whole-array numpy, rule by rule."""
    idx, dist, idx2, dist2 = search
    rows_all = np.arange(len(idx))
    found = (idx != NONE) if guided else np.ones(len(idx), dtype=bool)
    none2 = idx2 == NONE
    fd, fd2 = dist.astype(np.float64), dist2.astype(np.float64)
    ratios = np.ones(len(idx), dtype=np.float64)
    ok = found & ~none2 & (dist2 > 0)
    ratios[ok] = np.sqrt(fd[ok] / fd2[ok])
    keep = found.copy()
    if ratio is not None:
        below = fd < (float(ratio) * float(ratio)) * fd2
        keep &= (none2 | below) if guided else (~none2 & below)
    if guided and max_distance is not None:
        keep &= fd <= float(max_distance)
    if back is not None:
        mutual = np.zeros(len(idx), dtype=bool)
        mutual[found] = back[idx[found]] == rows_all[found]          # only where found: back[NONE] does not exist
        keep &= mutual
    rows = np.nonzero(keep)[0]
    return np.stack([rows.astype(np.int64), idx[rows].astype(np.int64)], axis=1), ratios[rows]


def options(ratio, mutual, max_distance=None):
    return F._match_options(ratio, mutual, max_distance)


def host_select(search, back, guided, ratio=None, max_distance=None, cap=None):
    """gcr_host_match_select on a search's four arrays: (matches uint32 (M, 2), ratios float64 (M,))"""
    idx, dist, idx2, dist2 = (np.ascontiguousarray(a, dtype=np.uint32) for a in search)
    n = len(idx)
    cap = n if cap is None else cap
    matches = np.full((cap, 2), 0xABABABAB, dtype=np.uint32)
    ratios = np.full(cap, -1.0)
    m = C.c_size_t()
    b = None if back is None else np.ascontiguousarray(back, dtype=np.uint32)
    N.check(N.lib.gcr_host_match_select(idx.ctypes.data, dist.ctypes.data, idx2.ctypes.data, dist2.ctypes.data, n,
                                        None if b is None else b.ctypes.data, 0 if b is None else len(b), int(guided),
                                        options(ratio, back is not None, max_distance), matches.ctypes.data,
                                        ratios.ctypes.data, cap, C.byref(m)))
    assert (ratios[m.value:] == -1.0).all() and (matches[m.value:] == 0xABABABAB).all(), "written past M"
    return matches[:m.value], ratios[:m.value]


def same_result(got, exp):
    """both arrays equal byte for byte, dtypes included"""
    return (got[0].dtype == exp[0].dtype and got[1].dtype == exp[1].dtype and got[0].shape == exp[0].shape
            and np.array_equal(got[0], exp[0]) and got[1].tobytes() == exp[1].tobytes())


def as_front_end(picked):
    """the C entry's uint32 pairs as the Python front end returns them"""
    return picked[0].astype(np.int64), picked[1]


def select_rows():
    """rows per workgroup of the select kernels"""
    t = (C.c_uint32 * 1)()
    N.lib.gcr_match_select_tiling(t)
    return int(t[0])


def workspace(device=None):
    """(device allocations made for the matching workspace, bytes held now)"""
    out = (C.c_uint64 * 2)()
    N.check(N.lib.gcr_debug_match_workspace(N.context(device), out))
    return int(out[0]), int(out[1])
