"""Shared by the tests of the essential matrix with known gravity: seeded
3-point cases from synthetic.problem_g, an independent numpy restatement of
csrc/grav.h's solver (the sextic by numpy.polynomial products, polydiv by
1 + s^2, numpy.roots, the translation as the null vector by SVD) and thin
wrappers of the host entry points."""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.polynomial import polynomial as P

from essential_cases import dist_pm, normalise
from pygcransac import _native as N
from pygcransac import synthetic as S

dpt = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)

# A case is kept when the restatement itself is well posed:
ROOT_GAP = 1e-3         # every two roots of the quartic (complex ones too) differ by more than this, relative
ROW_COND = 1e-3         # sigma_2 / sigma_1 of M(s) at every real root: the null vector is well defined
SIGN_GAP = 1e-6         # the oriented test's three values, relative: no sign is a matter of rounding
LEAD_MIN = 1e-6         # |leading coefficient| / max |coefficient| of the quartic (theta away from pi)


def aligned(rows, G1, G2):
    """p = G1 (x1, y1, 1)^T and q = G2 (x2, y2, 1)^T of normalised rows, (k, 3) each"""
    k = len(rows)
    p = np.column_stack([rows[:, 0], rows[:, 1], np.ones(k)]) @ np.asarray(G1).T
    q = np.column_stack([rows[:, 2], rows[:, 3], np.ones(k)]) @ np.asarray(G2).T
    return p, q


def _pcross(a, b):
    """cross product of two 3-vectors of polynomials (ascending coefficients)"""
    return [P.polysub(P.polymul(a[1], b[2]), P.polymul(a[2], b[1])),
            P.polysub(P.polymul(a[2], b[0]), P.polymul(a[0], b[2])),
            P.polysub(P.polymul(a[0], b[1]), P.polymul(a[1], b[0]))]


def ry(c, sn):
    return np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def ref_quartic(rows, G1, G2):
    """(quartic, remainder, sextic), ascending coefficients, and the rows of M(s) as polynomials"""
    p, q = aligned(rows, G1, G2)
    Mrows = []
    for i in range(3):
        px, py, pz = p[i]
        Rp = [np.array([px, 2 * pz, -px]), np.array([py, 0.0, py]), np.array([pz, -2 * px, -pz])]
        Mrows.append(_pcross(Rp, [np.array([v]) for v in q[i]]))
    w = _pcross(Mrows[1], Mrows[2])
    det = P.polyadd(P.polyadd(P.polymul(Mrows[0][0], w[0]), P.polymul(Mrows[0][1], w[1])),
                    P.polymul(Mrows[0][2], w[2]))
    det = np.concatenate([det, np.zeros(7 - len(det))])[:7]
    quo, rem = P.polydiv(det, [1.0, 0.0, 1.0])
    quo = np.concatenate([quo, np.zeros(5 - len(quo))])[:5]
    return quo, rem, det, Mrows


def ref_solve(rows, G1, G2):
    """The restated minimal solver on three normalised rows.  Returns (models
    in ascending root order, well_posed, relative remainder of the division)."""
    quo, rem, det, Mrows = ref_quartic(rows, G1, G2)
    scale = np.abs(det).max()
    rel_rem = np.abs(rem).max() / scale if scale > 0 else 0.0
    if not np.all(np.isfinite(quo)) or not scale > 0 or abs(quo[4]) <= LEAD_MIN * np.abs(quo).max():
        return [], False, rel_rem
    rts = np.roots(quo[::-1])
    well = True
    for i in range(len(rts)):
        for j in range(i + 1, len(rts)):
            if abs(rts[i] - rts[j]) <= ROOT_GAP * max(1.0, abs(rts[i]), abs(rts[j])):
                well = False
    real = sorted(z.real for z in rts if abs(z.imag) <= 1e-9 * max(1.0, abs(z.real)))
    G1, G2 = np.asarray(G1), np.asarray(G2)
    h1 = np.column_stack([rows[:, :2], np.ones(3)])
    h2 = np.column_stack([rows[:, 2:], np.ones(3)])
    models = []
    for s in real:
        M = np.array([[P.polyval(s, Mrows[i][k]) for k in range(3)] for i in range(3)])
        _, sv, vt = np.linalg.svd(M)
        if not sv[1] > ROW_COND * sv[0]:
            well = False
            continue
        t = vt[2]
        E = G2.T @ skew(t) @ ry((1 - s * s) / (1 + s * s), 2 * s / (1 + s * s)) @ G1
        E /= np.linalg.norm(E)
        # the oriented epipolar constraint on the sample (fund.h oriented_ok)
        e2 = np.linalg.svd(E.T)[2][2]                   # E^T e2 = 0
        sg = np.array([np.cross(e2, h2[i]) @ (E @ h1[i]) for i in range(3)])
        ref = np.array([np.linalg.norm(np.cross(e2, h2[i])) * np.linalg.norm(E @ h1[i]) for i in range(3)])
        if np.any(np.abs(sg) <= SIGN_GAP * np.maximum(ref, 1e-300)):
            well = False
        if np.all(sg > 0) or np.all(sg < 0):
            models.append(E)
    return models, well, rel_rem


def constrained_form(E, G1, G2):
    """The four structure figures of E' = G2 E G1^T: |E'[1][1]|, |E'[0][0] - E'[2][2]|,
    |E'[0][2] + E'[2][0]| and the singular values' distance from (s, s, 0), E at unit norm."""
    Ep = np.asarray(G2) @ np.reshape(E, (3, 3)) @ np.asarray(G1).T
    sv = np.linalg.svd(Ep, compute_uv=False)
    return max(abs(Ep[1, 1]), abs(Ep[0, 0] - Ep[2, 2]), abs(Ep[0, 2] + Ep[2, 0]), abs(sv[0] - sv[1]), abs(sv[2]))


def scene(seed, n=60, noise=0.0):
    """problem_g(n, no outliers, seed): normalised rows (n, 4), G1, G2, E_gt"""
    corr, _, K, G1, G2, E = S.problem_g(n, 0.0, seed=seed, noise=noise)
    rows, _ = normalise(corr, K, K, 1.0)
    return rows, np.ascontiguousarray(G1), np.ascontiguousarray(G2), E


def sampson(rows, E):
    E = np.reshape(E, (3, 3))
    h1 = np.column_stack([rows[:, :2], np.ones(len(rows))])
    h2 = np.column_stack([rows[:, 2:], np.ones(len(rows))])
    Ex1, Etx2 = h1 @ E.T, h2 @ E
    num = np.einsum("ij,ij->i", h2, Ex1) ** 2
    return num / (Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2)


# ---- host entry points --------------------------------------------------------
def _rot(G):
    return np.ascontiguousarray(G, dtype=np.float64)


def solve_g3(rows, G1, G2, idx=None):
    """gcr_host_solve_g3: models (k, 9), k = 0 .. 4"""
    c = np.ascontiguousarray(rows, dtype=np.float64)
    i = np.ascontiguousarray(np.arange(3) if idx is None else idx, dtype=np.uint32)
    g1, g2 = _rot(G1), _rot(G2)
    models = np.zeros(36)
    cnt = C.c_uint32()
    N.check(N.lib.gcr_host_solve_g3(c.ctypes.data, c.shape[0], i.ctypes.data, g1.ctypes.data, g2.ctypes.data,
                                    models.ctypes.data, C.byref(cnt)))
    assert cnt.value <= 4
    return models.reshape(4, 9)[:cnt.value].copy()


def host_fit(rows, idx, G1, G2):
    c = np.ascontiguousarray(rows, dtype=np.float64)
    i = np.ascontiguousarray(idx, dtype=np.uint32)
    g1, g2 = _rot(G1), _rot(G2)
    E = np.zeros(9)
    rc = N.check(N.lib.gcr_host_fit_g(c.ctypes.data, c.shape[0], i.ctypes.data, len(i), g1.ctypes.data,
                                      g2.ctypes.data, E.ctypes.data))
    return E if rc == 1 else None


def host_generate(rows, G1, G2, w, seed, slot0, nslots, threads=3):
    """gcr_host_generate_g: inc (nslots, 4), models (nslots, 4, 9)"""
    c = np.ascontiguousarray(rows, dtype=np.float64)
    g1, g2 = _rot(G1), _rot(G2)
    inc = np.zeros((nslots, 4), dtype=np.uint8)
    models = np.zeros((nslots, 4, 9))
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    N.check(N.lib.gcr_host_generate_g(c.ctypes.data, c.shape[0], g1.ctypes.data, g2.ctypes.data,
                                      None if wv is None else wv.ctypes.data, seed, slot0, nslots, threads,
                                      inc.ctypes.data, models.ctypes.data))
    return inc, models


# ---- a device-resident problem (GPU tests) -----------------------------------
class GravProblem:
    """gcr_problem_create_gravity_essential on device 0: pixel rows, K1, K2, G1, G2."""

    def __init__(self, corr, K1, K2, G1, G2):
        self.c = np.ascontiguousarray(corr, dtype=np.float64)
        self.k1, self.k2 = _rot(K1), _rot(K2)
        self.g1, self.g2 = _rot(G1), _rot(G2)
        h = C.c_void_p()
        N.check(N.lib.gcr_problem_create_gravity_essential(N.context(0), self.c.ctypes.data, self.c.shape[0],
                                                           self.k1.ctypes.data, self.k2.ctypes.data,
                                                           self.g1.ctypes.data, self.g2.ctypes.data, C.byref(h)))
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
        """inc (n, 4) bytes, models (n, 4, 9)"""
        inc = np.zeros(n * 4, dtype=np.uint8)
        H = np.zeros((n * 4, 9))
        N.check(N.lib.gcr_debug_generate_h(self.h, seed, slot0, n, inc.ctypes.data_as(u8p), H.ctypes.data_as(dpt)))
        return inc.reshape(n, 4), H.reshape(n, 4, 9)

    def sample(self, seed, slot0, n, attempt):
        out = np.zeros((n, 3), dtype=np.uint32)
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
