"""Shared by the essential-matrix tests: seeded two-view cases, an independent
numpy restatement of the 5-point solver (null space by SVD, the ten cubic
constraints by generic polynomial products, roots by numpy.roots) and thin
wrappers of the host entry points."""
from __future__ import annotations

import ctypes as C

import numpy as np

from pygcransac import _native as N

dpt = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)

# step 3's monomial order, as exponents of (x, y, z)
MONO = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
        (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def scene(rng, n):
    """Rotation vector components ~ N(0, 0.2) rad, unit baseline, depths 4..8,
    lateral coordinates in +-2, noise-free.  Returns normalised rows (n, 4)
    and E_gt at unit Frobenius norm."""
    R = rodrigues(rng.normal(0.0, 0.2, 3))
    t = rng.normal(0.0, 1.0, 3)
    t /= np.linalg.norm(t)
    T = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = T @ R
    P = np.column_stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 8, n)])
    Q = P @ R.T + t
    rows = np.column_stack([P[:, 0] / P[:, 2], P[:, 1] / P[:, 2], Q[:, 0] / Q[:, 2], Q[:, 1] / Q[:, 2]])
    return np.ascontiguousarray(rows), E / np.linalg.norm(E)


def dist_pm(A, B):
    return min(np.linalg.norm(A - B), np.linalg.norm(A + B))


def closest(models, E):
    return min((dist_pm(np.reshape(m, (3, 3)), E) for m in models), default=np.inf)


def epipolar_rows(rows):
    x1, y1, x2, y2 = rows.T
    return np.column_stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(len(rows))])


# ---- polynomials in (x, y, z) of degree <= 3 as (4, 4, 4) exponent arrays ----
def _pmul(a, b):
    out = np.zeros((4, 4, 4))
    for i, j, k in np.argwhere(a != 0.0):
        out[i:, j:, k:] += a[i, j, k] * b[:4 - i, :4 - j, :4 - k]
    return out


def _lin(x, y, z, w):
    p = np.zeros((4, 4, 4))
    p[1, 0, 0], p[0, 1, 0], p[0, 0, 1], p[0, 0, 0] = x, y, z, w
    return p


def ref_models(basis):
    """The restatement's steps 3-7 on a (4, 9) basis (X, Y, Z, W): models for
    every real root of numpy.roots, x and y by least squares on B(z)."""
    X, Y, Z, W = (np.reshape(b, (3, 3)) for b in basis)
    E = [[_lin(X[r, c], Y[r, c], Z[r, c], W[r, c]) for c in range(3)] for r in range(3)]
    det = (_pmul(E[0][0], _pmul(E[1][1], E[2][2]) - _pmul(E[1][2], E[2][1]))
           - _pmul(E[0][1], _pmul(E[1][0], E[2][2]) - _pmul(E[1][2], E[2][0]))
           + _pmul(E[0][2], _pmul(E[1][0], E[2][1]) - _pmul(E[1][1], E[2][0])))
    EEt = [[sum(_pmul(E[r][k], E[c][k]) for k in range(3)) for c in range(3)] for r in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    cons = [det]
    for r in range(3):
        for c in range(3):
            cons.append(sum(_pmul(2.0 * EEt[r][k] - (tr if r == k else 0.0), E[k][c]) for k in range(3)))
    M = np.array([[p[e] for e in MONO] for p in cons])
    red = np.linalg.solve(M[:, :10], M[:, 10:])           # rows led by the first ten monomials
    P = np.polynomial.polynomial
    rows = []
    for a, b in ((4, 5), (6, 7), (8, 9)):
        A, B = red[a], red[b]
        # ascending powers of z; columns: xz^2 xz x yz^2 yz y z^3 z^2 z 1
        bx = P.polysub([A[2], A[1], A[0]], [0.0, B[2], B[1], B[0]])
        by = P.polysub([A[5], A[4], A[3]], [0.0, B[5], B[4], B[3]])
        b1 = P.polysub([A[9], A[8], A[7], A[6]], [0.0, B[9], B[8], B[7], B[6]])
        rows.append((bx, by, b1))
    mul, sub = P.polymul, P.polysub

    def minor(i, j):
        return sub(mul(rows[i][0], rows[j][1]), mul(rows[j][0], rows[i][1]))

    n = P.polyadd(sub(mul(rows[0][2], minor(1, 2)), mul(rows[1][2], minor(0, 2))), mul(rows[2][2], minor(0, 1)))
    n = np.concatenate([n, np.zeros(11 - len(n))])[:11]
    models = []
    for z in np.roots(n[::-1]):
        if abs(z.imag) > 1e-9 * max(1.0, abs(z.real)):
            continue
        z = z.real
        Bz = np.array([[P.polyval(z, r[0]), P.polyval(z, r[1]), P.polyval(z, r[2])] for r in rows])
        xy = np.linalg.lstsq(Bz[:, :2], -Bz[:, 2], rcond=None)[0]
        Em = xy[0] * X + xy[1] * Y + z * Z + W
        models.append(Em / np.linalg.norm(Em))
    return models, n


def ref_solve(rows):
    """The restated minimal solver (no oriented test): models of five rows."""
    _, _, vt = np.linalg.svd(epipolar_rows(rows))
    return ref_models(vt[5:9])[0]


# ---- host entry points --------------------------------------------------------
def solve_minimal(rows, idx=None):
    """gcr_host_solve_minimal(5): models (k, 9), k = 0 .. 10."""
    c = np.ascontiguousarray(rows, dtype=np.float64)
    i = np.ascontiguousarray(np.arange(5) if idx is None else idx, dtype=np.uint32)
    models = np.zeros(90)
    cnt = C.c_uint32()
    N.check(N.lib.gcr_host_solve_minimal(N.SOLVER_ESSENTIAL5, c.ctypes.data_as(dpt), c.shape[0],
                                         i.ctypes.data_as(u32p), models.ctypes.data_as(dpt), C.byref(cnt)))
    assert cnt.value <= 10
    return models.reshape(10, 9)[:cnt.value].copy()


def host_fit(rows, idx):
    c = np.ascontiguousarray(rows, dtype=np.float64)
    i = np.ascontiguousarray(idx, dtype=np.uint32)
    E = np.zeros(9)
    rc = N.check(N.lib.gcr_host_fit_e(c.ctypes.data_as(dpt), c.shape[0], i.ctypes.data_as(u32p), len(i),
                                      E.ctypes.data_as(dpt)))
    return E if rc == 1 else None


def normalise(corr, K1, K2, thr):
    """gcr_host_essential_normalise: (normalised rows, normalised threshold)."""
    c = np.ascontiguousarray(corr, dtype=np.float64)
    k1 = np.ascontiguousarray(K1, dtype=np.float64)
    k2 = np.ascontiguousarray(K2, dtype=np.float64)
    out = np.zeros_like(c)
    t = C.c_double()
    N.check(N.lib.gcr_host_essential_normalise(c.ctypes.data, c.shape[0], k1.ctypes.data, k2.ctypes.data, thr,
                                               out.ctypes.data, C.byref(t)))
    return out, t.value


# ---- a device-resident essential-matrix problem (GPU tests) ------------------
u8p = C.POINTER(C.c_uint8)


class EssProblem:
    """gcr_problem_create_essential on device 0: pixel rows, K1, K2."""

    def __init__(self, corr, K1, K2):
        self.c = np.ascontiguousarray(corr, dtype=np.float64)
        self.k1 = np.ascontiguousarray(K1, dtype=np.float64)
        self.k2 = np.ascontiguousarray(K2, dtype=np.float64)
        h = C.c_void_p()
        N.check(N.lib.gcr_problem_create_essential(N.context(0), self.c.ctypes.data, self.c.shape[0],
                                                   self.k1.ctypes.data, self.k2.ctypes.data, C.byref(h)))
        self.h = h.value

    def close(self):
        if self.h:
            N.lib.gcr_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_probabilities(self, w):
        if w is None:
            return N.check(N.lib.gcr_problem_set_probabilities(self.h, None, 0))
        w = np.ascontiguousarray(w, dtype=np.float64)
        return N.check(N.lib.gcr_problem_set_probabilities(self.h, w.ctypes.data, len(w)))

    def generate(self, seed, slot0, n):
        """inc (n, 10) bytes, models (n, 10, 9)"""
        inc = np.zeros(n * 10, dtype=np.uint8)
        H = np.zeros((n * 10, 9))
        N.check(N.lib.gcr_debug_generate_h(self.h, seed, slot0, n, inc.ctypes.data_as(u8p), H.ctypes.data_as(dpt)))
        return inc.reshape(n, 10), H.reshape(n, 10, 9)

    def sample(self, seed, slot0, n, attempt):
        out = np.zeros((n, 5), dtype=np.uint32)
        N.check(N.lib.gcr_debug_sample_h(self.h, seed, slot0, n, attempt, out.ctypes.data_as(u32p)))
        return out

    def _params(self, thr, lam=0.0):
        p = N.default_params()
        p.scale_residual_thresh = thr
        p.spatial_coherence_weight = lam
        return p

    def score(self, models, thr):
        models = np.ascontiguousarray(models, dtype=np.float64)
        n = len(models)
        p = self._params(thr)
        n0 = np.zeros(n, dtype=np.uint32)
        v0, tot = np.zeros(n), np.zeros(n)
        N.check(N.lib.gcr_debug_score_h(self.h, C.byref(p), models.ctypes.data_as(dpt), n, n0.ctypes.data_as(u32p),
                                        v0.ctypes.data_as(dpt), tot.ctypes.data_as(dpt)))
        return n0, v0, tot

    def mask(self, model, rule, thr, lam=0.0):
        p = self._params(thr, lam)
        out = np.zeros(self.c.shape[0], dtype=np.uint8)
        m = np.ascontiguousarray(model, dtype=np.float64).reshape(9)
        N.check(N.lib.gcr_debug_mask_h(self.h, C.byref(p), m.ctypes.data_as(dpt), rule, out.ctypes.data_as(u8p)))
        return out.astype(bool)

    def run(self, **fields):
        """gcr_problem_run: (E or None, mask, stats dict)"""
        p = N.default_params()
        for k, v in fields.items():
            setattr(p, k, v)
        mask = np.zeros(self.c.shape[0], dtype=np.uint8)
        E = np.zeros(9)
        st = N.Stats()
        n = N.check(N.lib.gcr_problem_run(self.h, C.byref(p), mask.ctypes.data_as(u8p), None, E.ctypes.data_as(dpt),
                                          None, C.byref(st)))
        return (E.reshape(3, 3) if n > 0 else None), mask.astype(bool), st.as_dict()
