"""Shared by the tests of the homography from two SIFT correspondences:
the distance to H_GT, the eight constraints of csrc/sifth.h restated in numpy
on pixel data (no normalisation, no chart), thin wrappers of the host entry
points and a device-resident problem (SIFT kind, or the plain homography kind
over the same rows)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from pygcransac import _native as N

dpt = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)

PER = 3                 # models per sample (csrc/sifth.h kSModels)


# Two rows (random SIFT columns, no homography behind them) whose cubic has two
# nearby real roots that both pass the solver's tests, in either order of the
# rows: such samples are about 1e-5 of those that yield a model (both models
# are nearly rank-one), so the tests that need a many-model slot use this pair.
TWO_MODEL_PAIR = np.array([
    [1241.247582900181, 100.5522514955808, 809.7073057395933, 143.05636654422432,
     3.510625737713387, 13.639743957139997, -0.9546383473008753, -1.3634523594980958],
    [836.9986600117601, 671.456265699656, 86.94670303874929, 484.55087733329555,
     20.651333815004374, 5.065096680620867, 1.3418688079400622, -2.032695491256679]])


def h_distance(H, H_gt):
    """max-abs over the entries of H / H22 - H_gt / H_gt22, divided by 35 (H_GT's largest entry)"""
    H = np.reshape(H, (3, 3))
    return float(np.abs(H / H[2, 2] - H_gt / H_gt[2, 2]).max() / 35.0)


def constraint_residuals(H, rows8):
    """The four constraints of each row of rows8 (k, 8) under H, each relative
    to the sum of the magnitudes of its terms: DLT x, DLT y, orientation
    (n2^T B d1), size (det B - r s^2).  (k, 4)."""
    H = np.reshape(H, (3, 3))
    out = np.zeros((len(rows8), 4))
    for i, (x1, y1, x2, y2, q1, q2, a1, a2) in enumerate(rows8):
        X = np.array([x1, y1, 1.0])
        s = H[2] @ X
        t0, t1 = H[0] @ X, H[1] @ X
        out[i, 0] = abs(t0 - x2 * s) / (np.abs(H[0] * X).sum() + abs(x2) * np.abs(H[2] * X).sum())
        out[i, 1] = abs(t1 - y2 * s) / (np.abs(H[1] * X).sum() + abs(y2) * np.abs(H[2] * X).sum())
        B = np.array([[H[0, 0] - x2 * H[2, 0], H[0, 1] - x2 * H[2, 1]],
                      [H[1, 0] - y2 * H[2, 0], H[1, 1] - y2 * H[2, 1]]])
        d1 = np.array([np.cos(a1), np.sin(a1)])
        n2 = np.array([-np.sin(a2), np.cos(a2)])
        out[i, 2] = abs(n2 @ B @ d1) / (np.abs(n2) @ np.abs(B) @ np.abs(d1))
        r = (q2 / q1) ** 2
        out[i, 3] = abs(np.linalg.det(B) - r * s * s) / (abs(B[0, 0] * B[1, 1]) + abs(B[0, 1] * B[1, 0]) + r * s * s)
    return out


def orientation_maps_forward(H, rows8):
    """(d2^T B d1) / s > 0 for every row: the first orientation maps onto the second, not its opposite"""
    H = np.reshape(H, (3, 3))
    ok = True
    for x1, y1, x2, y2, q1, q2, a1, a2 in rows8:
        s = H[2] @ np.array([x1, y1, 1.0])
        B = np.array([[H[0, 0] - x2 * H[2, 0], H[0, 1] - x2 * H[2, 1]],
                      [H[1, 0] - y2 * H[2, 0], H[1, 1] - y2 * H[2, 1]]])
        ok = ok and (np.array([np.cos(a2), np.sin(a2)]) @ B @ np.array([np.cos(a1), np.sin(a1)])) / s > 0
    return ok


def _split(rows8):
    r = np.asarray(rows8, dtype=np.float64)
    return np.ascontiguousarray(r[:, :4]), np.ascontiguousarray(r[:, 4:8])


# ---- host entry points --------------------------------------------------------
def check_sift(sift):
    s = np.ascontiguousarray(sift, dtype=np.float64)
    return N.check(N.lib.gcr_host_check_sift(s.ctypes.data, len(s)))


def solve_s2(rows8, idx=None):
    """gcr_host_solve_s2: models (k, 9), k = 0 .. 3"""
    c, s = _split(rows8)
    i = np.ascontiguousarray(np.arange(2) if idx is None else idx, dtype=np.uint32)
    models = np.zeros(9 * PER)
    cnt = C.c_uint32()
    N.check(N.lib.gcr_host_solve_s2(c.ctypes.data, s.ctypes.data, len(c), i.ctypes.data, models.ctypes.data,
                                    C.byref(cnt)))
    assert cnt.value <= PER
    return models.reshape(PER, 9)[:cnt.value].copy()


def host_generate(rows8, w, seed, slot0, nslots, threads=3):
    """gcr_host_generate_s: inc (nslots, PER), models (nslots, PER, 9)"""
    c, s = _split(rows8)
    inc = np.zeros((nslots, PER), dtype=np.uint8)
    models = np.zeros((nslots, PER, 9))
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    N.check(N.lib.gcr_host_generate_s(c.ctypes.data, s.ctypes.data, len(c), None if wv is None else wv.ctypes.data,
                                      seed, slot0, nslots, threads, inc.ctypes.data, models.ctypes.data))
    return inc, models


# ---- a device-resident problem (GPU tests) -----------------------------------
class HProblem:
    """A problem over the rows of rows8 on device 0: sift=True the SIFT homography
    kind (gcr_problem_create_sift_homography), sift=False the plain homography kind
    (gcr_problem_create(3)) over the same x1, y1, x2, y2."""

    def __init__(self, rows8, sift=True):
        self.c, self.s = _split(rows8)
        self.per = PER if sift else 1
        self.m = 2 if sift else 4
        h = C.c_void_p()
        if sift:
            N.check(N.lib.gcr_problem_create_sift_homography(N.context(0), self.c.ctypes.data, self.s.ctypes.data,
                                                             len(self.c), C.byref(h)))
        else:
            N.check(N.lib.gcr_problem_create(N.context(0), N.SOLVER_HOMOGRAPHY4, self.c.ctypes.data_as(dpt),
                                             len(self.c), None, 0, C.byref(h)))
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
        """inc (n, per) bytes, models (n, per, 9)"""
        inc = np.zeros(n * self.per, dtype=np.uint8)
        H = np.zeros((n * self.per, 9))
        N.check(N.lib.gcr_debug_generate_h(self.h, seed, slot0, n, inc.ctypes.data_as(u8p), H.ctypes.data_as(dpt)))
        return inc.reshape(n, self.per), H.reshape(n, self.per, 9)

    def sample(self, seed, slot0, n, attempt):
        out = np.zeros((n, self.m), dtype=np.uint32)
        N.check(N.lib.gcr_debug_sample_h(self.h, seed, slot0, n, attempt, out.ctypes.data_as(u32p)))
        return out

    def params(self, thr, lam=0.0):
        p = N.default_params()
        p.scale_residual_thresh = thr
        p.spatial_coherence_weight = lam
        return p

    def score(self, models, thr):
        models = np.ascontiguousarray(models, dtype=np.float64)
        n = len(models)
        p = self.params(thr)
        n0 = np.zeros(n, dtype=np.uint32)
        v0, tot = np.zeros(n), np.zeros(n)
        N.check(N.lib.gcr_debug_score_h(self.h, C.byref(p), models.ctypes.data_as(dpt), n, n0.ctypes.data_as(u32p),
                                        v0.ctypes.data_as(dpt), tot.ctypes.data_as(dpt)))
        return n0, v0, tot

    def mask(self, model, rule, thr, lam=0.0):
        p = self.params(thr, lam)
        out = np.zeros(len(self.c), dtype=np.uint8)
        m = np.ascontiguousarray(model, dtype=np.float64).reshape(9)
        N.check(N.lib.gcr_debug_mask_h(self.h, C.byref(p), m.ctypes.data_as(dpt), rule, out.ctypes.data_as(u8p)))
        return out.astype(bool)

    def verify_batches(self, thr, seed, slot0, nslots, nbatches):
        p = self.params(thr)
        p.seed = seed
        res = (N.BatchResult * nbatches)()
        N.check(N.lib.gcr_problem_verify_batches(self.h, C.byref(p), slot0, nslots, nbatches, res, None))
        return res

    def run(self, **fields):
        """gcr_problem_run: (H or None, mask, stats dict)"""
        p = N.default_params()
        for k, v in fields.items():
            setattr(p, k, v)
        mask = np.zeros(len(self.c), dtype=np.uint8)
        H = np.zeros(9)
        st = N.Stats()
        n = N.check(N.lib.gcr_problem_run(self.h, C.byref(p), mask.ctypes.data_as(u8p), None, H.ctypes.data_as(dpt),
                                          None, C.byref(st)))
        return (H.reshape(3, 3) if n > 0 else None), mask.astype(bool), st.as_dict()
