"""Guided descriptor matching: an independent numpy restatement of
csrc/match_geo.h's definition, the input families and the crafted inputs the
host and GPU tests share, and thin ctypes wrappers of the two C entries.

A case is the tuple (d1, d2, p1, p2, kind, h, T): uint8 descriptors, (n, 2)
float64 positions, the kind's code (H or F), the model as 9 doubles and the
squared bound."""
import ctypes as C
import functools

import numpy as np

import match_cases as MC
from pygcransac import _native as N
from pygcransac import synthetic as S

NONE = MC.NONE
H, F = 3, 4                                    # GCR_SOLVER_HOMOGRAPHY4, GCR_SOLVER_FUNDAMENTAL7
KINDS = (H, F)
NAMES = ("idx", "dist", "idx2", "dist2")
INF = float("inf")


def residuals(kind, p1, p2, h):
    """(n1, n2) float64: geo.h's h_sq_residual / fund.h's f_sq_sampson of every
    pair, each operation in their order (numpy rounds every ufunc result to
    float64: no fused multiply-add)."""
    h = np.asarray(h, dtype=np.float64).reshape(9)
    x1, y1 = p1[:, 0][:, None], p1[:, 1][:, None]
    x2, y2 = p2[:, 0][None, :], p2[:, 1][None, :]
    with np.errstate(all="ignore"):
        if kind == H:
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


def admissible(kind, p1, p2, h, T):
    """(n1, n2) bool; NaN <= T is False"""
    with np.errstate(invalid="ignore"):
        return residuals(kind, p1, p2, h) <= T


def restate(d1, d2, p1, p2, kind, h, T, reverse=0):
    """idx, dist, idx2, dist2 (uint32): all distances in int64, the
    inadmissible entries pushed to the end of a stable argsort."""
    a, b = d1.astype(np.int64), d2.astype(np.int64)
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    adm = admissible(kind, p1, p2, h, T)
    if reverse:
        d, adm = d.T, adm.T
    key = np.where(adm, d, np.int64(1) << 40)
    order = np.argsort(key, axis=1, kind="stable")
    count = adm.sum(1)
    rows = np.arange(len(d))
    out = [np.full(len(d), NONE, dtype=np.uint32) for _ in range(4)]
    for k in range(min(2, d.shape[1])):
        has = count > k
        out[2 * k][has] = order[has, k]
        out[2 * k + 1][has] = d[rows[has], order[has, k]]
    return out


def skew(e):
    return np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])


IDENTITY = np.eye(3)
E_GENERIC = (2.0 * S.IMG_W, S.IMG_H / 2.0, 1.0)
F_GENERIC = skew(E_GENERIC) @ S.H_GT           # consistent with the plane of H_GT
# lattice models: integer translation, and [e']x of it with small integers
H_SHIFT = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]])
F_LATTICE = skew((3.0, -2.0, 1.0)) @ H_SHIFT
# integer squared bounds for a low and a middle admissible share: 9 % and 44 % under H, 19 % and 50 % under F
# (T = 0 gives 1 % under F, T = 1 is the next integer); held to 5..20 % and 40..60 % in test_match_guided.py
LATTICE_T = {H: (9.0, 64.0), F: (1.0, 9.0)}


def lattice_positions(n1, n2, seed=0):
    rng = np.random.default_rng([20261001, n1, n2, seed])
    return (rng.integers(0, 16, (n1, 2)).astype(np.float64), rng.integers(0, 16, (n2, 2)).astype(np.float64))


@functools.lru_cache(maxsize=None)
def _problem_positions(n):
    kp1, _, kp2, _, _, _ = S.problem_match(n=n, shared=(2 * n) // 5)
    return np.ascontiguousarray(kp1[:, :2]), np.ascontiguousarray(kp2[:, :2])


def generic_positions(n1, n2):
    """problem_match's keypoints: two fifths of the larger image's are shared scene points"""
    a, b = _problem_positions(max(n1, n2))
    return np.ascontiguousarray(a[:n1]), np.ascontiguousarray(b[:n2])


def lattice_case(n1, n2, dim, kind, share=0, shift=True):
    """share 0: near 10 % admissible, 1: near 50 %.  Under H with shift=False the model is the identity."""
    d1, d2 = MC.random_pair(n1, n2, dim)
    p1, p2 = lattice_positions(n1, n2)
    h = (H_SHIFT if shift else IDENTITY) if kind == H else F_LATTICE
    return d1, d2, p1, p2, kind, np.ascontiguousarray(h).reshape(9), LATTICE_T[kind][share]


def generic_case(n1, n2, dim, kind):
    d1, d2 = MC.random_pair(n1, n2, dim)
    p1, p2 = generic_positions(n1, n2)
    h = S.H_GT if kind == H else F_GENERIC
    return d1, d2, p1, p2, kind, np.ascontiguousarray(h, dtype=np.float64).reshape(9), 9.0


def family_cases(n1, n2, dim):
    """name -> case: both families, both kinds; the lattice at both shares"""
    out = {}
    for kind, k in ((H, "H"), (F, "F")):
        out[f"lattice10-{k}"] = lattice_case(n1, n2, dim, kind, 0)
        out[f"lattice50-{k}"] = lattice_case(n1, n2, dim, kind, 1)
        out[f"generic-{k}"] = generic_case(n1, n2, dim, kind)
    out["lattice50-H-identity"] = lattice_case(n1, n2, dim, H, 1, shift=False)
    return out


# the skip case's layout: rows per workgroup 128, rows per wave 32, columns per step 64, per tile 32
SKIP_FAR_ROWS = [(32, 64), (128, 256)]         # a whole wave, a whole workgroup
SKIP_FAR_COLS = [(0, 64), (96, 128)]           # a whole step, one tile of a step


def crafted(dim=128):
    """name -> case: the inputs aimed at one mistake each."""
    rng = np.random.default_rng([20261002, dim])
    ident = IDENTITY.reshape(9).copy()
    cases = {}
    # nothing admissible: the model moves image 1 far from image 2
    d1, d2 = MC.random_pair(70, 97, dim, seed=1)
    p1, p2 = lattice_positions(70, 97, seed=1)
    far = np.array([1.0, 0.0, 100.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    cases["nothing"] = (d1, d2, p1, p2, H, far, 1.0)
    # exactly one admissible column per row (and, in reverse, rows with one and with none)
    p1 = np.column_stack([10.0 * np.arange(70), np.zeros(70)])
    p2 = np.column_stack([10.0 * rng.permutation(97), np.zeros(97)])
    cases["single"] = (d1, d2, p1, p2, H, ident, 1.0)
    # T = +inf, identity: every pair admissible, the unguided matcher's bytes
    d1, d2 = MC.random_pair(129, 257, dim, seed=2)
    p1, p2 = lattice_positions(129, 257, seed=2)
    cases["inf_identity"] = (d1, d2, p1, p2, H, ident, INF)
    cases["inf_identity_F"] = (d1, d2, p1 + 1.0, p2 + 1.0, F, F_LATTICE.reshape(9).copy(), INF)
    # w = 0 under H for the rows with x1 = 5: u = x / 0 = inf, v = y / 0 = inf or NaN (y = 0)
    wz = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, -5.0])
    d1, d2 = MC.random_pair(70, 97, dim, seed=3)
    p1, p2 = lattice_positions(70, 97, seed=3)
    p1[::7, 0] = 5.0
    p1[::14, 1] = 0.0
    cases["w_zero"] = (d1, d2, p1, p2, H, wz, 4.0)
    cases["w_zero_inf"] = (d1, d2, p1, p2, H, wz, INF)
    # match_cases' padding and duplicates descriptor sets, every column admissible: all keypoints on one
    # point and T = 0 (r == T is admissible)
    for name in ("padding", "duplicates"):
        d1, d2 = MC.crafted(dim)[name]
        cases[name] = (d1, d2, np.full((len(d1), 2), 3.0), np.full((len(d2), 2), 3.0), H, ident, 0.0)
    # the skip path: whole tiles, whole steps and whole workgroups' rows without an admissible column
    # next to tiles that have some
    d1, d2 = MC.random_pair(300, 200, dim, seed=4)
    p1, p2 = lattice_positions(300, 200, seed=4)
    for lo, hi in SKIP_FAR_ROWS:
        p1[lo:hi] += 5000.0
    for lo, hi in SKIP_FAR_COLS:
        p2[lo:hi] -= 5000.0
    cases["skip"] = (d1, d2, p1, p2, H, ident, 2.0)
    return cases


def _call(fn, case, reverse, front=(), mid=(), back=()):
    d1, d2, p1, p2, kind, h, T = case
    d1 = np.ascontiguousarray(d1, dtype=np.uint8)
    d2 = np.ascontiguousarray(d2, dtype=np.uint8)
    p1 = np.ascontiguousarray(p1, dtype=np.float64)
    p2 = np.ascontiguousarray(p2, dtype=np.float64)
    h = np.ascontiguousarray(h, dtype=np.float64).reshape(9)
    assert p1.shape == (len(d1), 2) and p2.shape == (len(d2), 2)
    out = [np.empty(len(d2) if reverse else len(d1), dtype=np.uint32) for _ in range(4)]
    N.check(fn(*front, d1.ctypes.data, len(d1), p1.ctypes.data, d2.ctypes.data, len(d2), p2.ctypes.data, d1.shape[1],
               int(kind), h.ctypes.data, float(T), int(reverse), *mid, *[o.ctypes.data for o in out], *back))
    return out


def host(case, reverse=0, threads=1):
    return _call(N.lib.gcr_host_match_descriptors_guided, case, reverse, mid=(threads,))


def gpu(case, reverse=0, device=None, ms=None):
    return _call(N.lib.gcr_match_descriptors_guided, case, reverse, front=(N.context(device),),
                 back=(None if ms is None else C.byref(ms),))


def transposed(case):
    """The problem with the images swapped (F^T; the inverse of a translation H):
    forward on it is reverse on the original.  The residuals of the two agree
    as real numbers only; on the lattice every intermediate is an exact
    integer, so there they agree bit for bit."""
    d1, d2, p1, p2, kind, h, T = case
    m = np.asarray(h, dtype=np.float64).reshape(3, 3)
    if kind == F:
        return d2, d1, p2, p1, kind, np.ascontiguousarray(m.T).reshape(9), T
    if not np.array_equal(m[:, :2], IDENTITY[:, :2]) or m[2, 2] != 1.0:
        raise ValueError("a homography other than a translation has another residual after the swap")
    inv = IDENTITY.copy()
    inv[:2, 2] = -m[:2, 2]
    return d2, d1, p2, p1, kind, inv.reshape(9), T


def differences(got, exp):
    """'' or a description of the first differing output"""
    for g, e, name in zip(got, exp, NAMES):
        bad = np.nonzero(g != e)[0]
        if bad.size:
            return f"{name}: {bad.size} rows differ, first {bad[:5]}: {g[bad[:5]]} != {e[bad[:5]]}"
    return ""
