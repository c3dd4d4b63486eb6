"""ctypes bindings to the CPU oracle (oracle/_build/liboracle.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg as the checker, never by the product package.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")
LIB_PATH = os.path.join(ORACLE_DIR, "_build", "liboracle.so")

MATH_GLIBC, MATH_TWIN, MATH_PURE_TWIN = 0, 1, 2
SAMPLER_PHILOX, SAMPLER_FAITHFUL = 0, 1
KIND_SCALE3, KIND_SCALE3_ORIGINAL, KIND_SIFT22 = 0, 1, 2


class OracleParams(C.Structure):
    _fields_ = [
        ("thr0", C.c_double), ("thr1", C.c_double), ("spatial_coherence_weight", C.c_double),
        ("min_iteration_number", C.c_uint64), ("max_iteration_number", C.c_uint64),
        ("max_local_optimization_number", C.c_uint64), ("confidence", C.c_double),
        ("seed", C.c_uint64), ("math_mode", C.c_int32), ("sampler", C.c_int32),
        ("cell_size", C.c_double * 4), ("cell_number", C.c_uint64),
    ]


class OracleStats(C.Structure):
    _fields_ = [
        ("iteration_number", C.c_uint64), ("local_optimization_number", C.c_uint64),
        ("graph_cut_number", C.c_uint64), ("slots", C.c_uint64), ("hypotheses", C.c_uint64),
        ("score", C.c_double), ("seconds", C.c_double),
        ("near_ties", C.c_uint64), ("near_tie_flips", C.c_uint64),
    ]


class OracleSampling(C.Structure):
    """mode 0: uniform or guided (by weights), 1: PROSAC, 2: NAPSAC; star_i /
    star_n: (I*, n*) of the last stop update of a prosac_stop run (out)."""
    _fields_ = [
        ("mode", C.c_int32), ("prosac_stop", C.c_int32), ("prosac_convergence", C.c_uint64),
        ("napsac_iterations", C.c_uint64), ("napsac_extent", C.c_double * 4),
        ("star_i", C.c_uint64), ("star_n", C.c_uint64),
    ]


_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        dp, u8p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
        L.oracle_rect_scale_only.argtypes = [dp, C.c_size_t, C.POINTER(OracleParams), C.c_int, u8p, dp, dp,
                                             C.POINTER(OracleStats)]
        L.oracle_rect_sift.argtypes = [dp, C.c_size_t, dp, C.c_size_t, C.POINTER(OracleParams), u8p, u8p, dp, dp,
                                       C.POINTER(OracleStats)]
        L.oracle_slot.argtypes = [C.c_int, dp, C.c_size_t, dp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, dp]
        L.oracle_score.argtypes = [C.c_int, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_double, C.c_double, C.c_int,
                                   u64p, dp, dp, u8p, u8p]
        L.oracle_residuals.argtypes = [C.c_int, C.c_int, dp, C.c_size_t, dp, C.c_int, dp]
        L.oracle_slots_scored.argtypes = [C.c_int, dp, C.c_size_t, dp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_size_t,
                                          C.c_int, dp, C.c_size_t, C.POINTER(C.c_int), dp, u64p, dp, dp]
        L.oracle_sample.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                    C.c_uint32, u64p]
        L.oracle_philox.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.oracle_philox.restype = None
        L.oracle_fit_nonminimal.argtypes = [C.c_int, dp, C.c_size_t, dp, C.c_size_t, u64p, C.c_size_t, u64p,
                                            C.c_size_t, C.c_int, dp]
        L.oracle_hot_batch.argtypes = [C.c_int, dp, C.c_size_t, dp, C.c_size_t, C.c_double, C.c_double, C.c_uint64,
                                       C.c_uint64, C.c_uint64, C.c_int, C.c_int, dp, dp]
        L.oracle_hot_batch.restype = C.c_int64
        L.oracle_find_homography.argtypes = [dp, C.c_size_t, C.POINTER(OracleParams), u8p, dp,
                                             C.POINTER(OracleStats)]
        L.oracle_h_slot.argtypes = [dp, C.c_size_t, C.c_uint64, C.c_uint64, dp]
        L.oracle_h_score.argtypes = [dp, C.c_size_t, dp, C.c_double, u64p, dp, u8p]
        L.oracle_h_residuals.argtypes = [dp, C.c_size_t, dp, dp]
        L.oracle_find_fundamental.argtypes = L.oracle_find_homography.argtypes
        u32p = C.POINTER(C.c_uint32)
        L.oracle_bk_energy.argtypes = [C.c_size_t, dp, u32p, dp, C.c_size_t, u8p, dp]
        L.oracle_grid_edges.argtypes = [dp, C.c_size_t, C.c_size_t, dp, C.c_uint64, u32p, C.c_size_t]
        L.oracle_grid_edges.restype = C.c_size_t
        L.oracle_f_slot.argtypes = [dp, C.c_size_t, C.c_uint64, C.c_uint64, dp, C.POINTER(C.c_int)]
        L.oracle_f_score.argtypes = L.oracle_h_score.argtypes
        L.oracle_f_residuals.argtypes = L.oracle_h_residuals.argtypes
        L.oracle_f_fit.argtypes = L.oracle_h_fit.argtypes
        L.oracle_h_fit.argtypes = [dp, C.c_size_t, u64p, C.c_size_t, dp]
        for name in ["oracle_clip_angle", "oracle_deg2rad", "oracle_rad2deg"]:
            getattr(L, name).argtypes = [C.c_double]
            getattr(L, name).restype = C.c_double
        for name in ["oracle_min_angle_diff", "oracle_lines_angles_diff"]:
            getattr(L, name).argtypes = [C.c_double, C.c_double]
            getattr(L, name).restype = C.c_double
        L.oracle_nchoose2.argtypes = [C.c_uint64]
        L.oracle_nchoose2.restype = C.c_uint64
        L.oracle_are_collinear.argtypes = [C.c_double] * 7
        L.oracle_line_from_point_angle.argtypes = [C.c_double, C.c_double, C.c_double, dp]
        L.oracle_line_from_point_angle.restype = None
        L.oracle_convex_hull.argtypes = [dp, C.c_size_t, dp]
        L.oracle_point_in_polygon.argtypes = [C.c_double, C.c_double, dp, C.c_size_t]
        L.oracle_model_op.argtypes = [dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]
        L.oracle_model_op.restype = C.c_double
        L.oracle_model_point.argtypes = [dp, C.c_int, C.c_double, C.c_double, dp]
        L.oracle_model_point.restype = None
        L.oracle_get_homography.argtypes = [dp, dp]
        L.oracle_get_homography.restype = None
        L.oracle_gauss3.argtypes = [dp, dp]
        L.oracle_lstsq3.argtypes = [dp, C.c_size_t, dp, dp]
        L.oracle_weighted_mode.argtypes = [dp, dp, C.c_size_t, C.c_double]
        L.oracle_weighted_mode.restype = C.c_double
        L.oracle_set_qr_order.argtypes = [C.c_int]
        _lib = L
    return _lib


QR_BLOCKED, QR_FROZEN = 0, 1


class qr_order:
    """Context manager: run the oracle's least-squares fits in `order`
    (QR_FROZEN = the frozen sequential reduction order, never changed to follow
    the product; QR_BLOCKED = the engine's blocked order, the default)."""

    def __init__(self, order):
        self.order = order

    def __enter__(self):
        self.prev = lib().oracle_set_qr_order(self.order)
        return self

    def __exit__(self, *exc):
        lib().oracle_set_qr_order(self.prev)
        return False


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def params(thr0, thr1=0.0, lam=0.0, min_it=10000, max_it=10000, lo=50, confidence=0.95, seed=0,
           math_mode=MATH_TWIN, sampler=SAMPLER_PHILOX, cell_size=(0.0, 0.0, 0.0, 0.0), cell_number=0):
    """cell_size / cell_number: the H / F neighbourhood grid over (x1, y1, x2,
    y2) (0 cells = the empty grid of the reference's entry points)."""
    return OracleParams(thr0, thr1, lam, min_it, max_it, lo, confidence, seed, math_mode, sampler,
                        (C.c_double * 4)(*map(float, cell_size)), int(cell_number))


def model7(m):
    return np.array([m["x0"], m["y0"], m["s"], m["h7"], m["h8"], m["alpha"], m["phi"]], dtype=np.float64)


def _model_dict(v):
    return dict(x0=v[0], y0=v[1], s=v[2], h7=v[3], h8=v[4], alpha=v[5], phi=v[6])


def _stats_dict(st):
    return {k: getattr(st, k) for k, _ in OracleStats._fields_}


def rect_scale_only(features, thr, original=False, **kw):
    f = _f64(features)
    n = f.shape[0]
    mask = np.zeros(n, dtype=np.uint8)
    H = np.zeros(9)
    m = np.zeros(7)
    st = OracleStats()
    p = params(thr, **kw)
    r = lib().oracle_rect_scale_only(_dp(f), n, C.byref(p), int(original),
                                     mask.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(H), _dp(m), C.byref(st))
    if r < 0:
        raise RuntimeError("oracle failed")
    return dict(num_inliers=r, mask=mask.astype(bool), H=H.reshape(3, 3), model=_model_dict(m),
                stats=_stats_dict(st))


def rect_sift(scale_features, orientation_features, thr_s, thr_o, **kw):
    fs, fo = _f64(scale_features), _f64(orientation_features)
    ms = np.zeros(fs.shape[0], dtype=np.uint8)
    mo = np.zeros(fo.shape[0], dtype=np.uint8)
    H = np.zeros(9)
    m = np.zeros(7)
    st = OracleStats()
    p = params(thr_s, thr_o, **kw)
    r = lib().oracle_rect_sift(_dp(fs), fs.shape[0], _dp(fo), fo.shape[0], C.byref(p),
                               ms.ctypes.data_as(C.POINTER(C.c_uint8)), mo.ctypes.data_as(C.POINTER(C.c_uint8)),
                               _dp(H), _dp(m), C.byref(st))
    if r < 0:
        raise RuntimeError("oracle failed")
    return dict(num_inliers=r, scale_mask=ms.astype(bool), orientation_mask=mo.astype(bool),
                H=H.reshape(3, 3), model=_model_dict(m), stats=_stats_dict(st))


def slot(kind, f0, f1, seed, slot_index, math_mode=MATH_TWIN):
    f0 = _f64(f0)
    f1 = _f64(f1) if f1 is not None else None
    m = np.zeros(7)
    inc = lib().oracle_slot(kind, _dp(f0), f0.shape[0], _dp(f1) if f1 is not None else None,
                            0 if f1 is None else f1.shape[0], seed, slot_index, math_mode, _dp(m))
    return inc, m


def score(kind, f0, f1, model, thr0, thr1=0.0, math_mode=MATH_TWIN, want_masks=False):
    f0 = _f64(f0)
    f1 = _f64(f1) if f1 is not None else None
    counts = np.zeros(2, dtype=np.uint64)
    values = np.zeros(2)
    value = np.zeros(1)
    m0 = np.zeros(f0.shape[0], dtype=np.uint8) if want_masks else None
    m1 = np.zeros(f1.shape[0], dtype=np.uint8) if (want_masks and f1 is not None) else None
    u8 = C.POINTER(C.c_uint8)
    lib().oracle_score(kind, _dp(f0), f0.shape[0], _dp(f1) if f1 is not None else None,
                       0 if f1 is None else f1.shape[0], _dp(_f64(model)), thr0, thr1, math_mode,
                       counts.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(values), _dp(value),
                       m0.ctypes.data_as(u8) if m0 is not None else None,
                       m1.ctypes.data_as(u8) if m1 is not None else None)
    out = dict(counts=counts, values=values, value=float(value[0]))
    if want_masks:
        out["masks"] = (m0.astype(bool), None if m1 is None else m1.astype(bool))
    return out


def slots_scored(kind, f0, f1, seed, slot0, nslots, thresholds, math_mode=MATH_TWIN):
    """slot() and score() of nslots consecutive slots under every (thr0, thr1)
    of `thresholds`, in one call (the GIL is released for all of it): inc
    (n,), models (n, 7), counts (t, n, 2), values (t, n, 2), value (t, n);
    zeros for a slot without a model."""
    f0 = _f64(f0)
    f1 = _f64(f1) if f1 is not None else None
    thr = _f64(thresholds).reshape(-1, 2)
    t = thr.shape[0]
    inc = np.zeros(nslots, dtype=np.int32)
    models = np.zeros((nslots, 7))
    counts = np.zeros((t, nslots, 2), dtype=np.uint64)
    values = np.zeros((t, nslots, 2))
    value = np.zeros((t, nslots))
    lib().oracle_slots_scored(kind, _dp(f0), f0.shape[0], _dp(f1) if f1 is not None else None,
                              0 if f1 is None else f1.shape[0], seed, slot0, nslots, math_mode, _dp(thr), t,
                              inc.ctypes.data_as(C.POINTER(C.c_int)), _dp(models),
                              counts.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(values), _dp(value))
    return inc, models, counts, values, value


def residuals(kind, cls, f, model, math_mode=MATH_TWIN):
    f = _f64(f)
    r2 = np.zeros(f.shape[0])
    lib().oracle_residuals(kind, cls, _dp(f), f.shape[0], _dp(_f64(model)), math_mode, _dp(r2))
    return r2


def sample(seed, index, sub, stream, cls, n, m):
    out = np.zeros(m, dtype=np.uint64)
    r = lib().oracle_sample(seed, index, sub, stream, cls, n, m, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if r != 0:
        raise RuntimeError("sample budget exhausted")
    return out


def philox(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    lib().oracle_philox(c, k, o)
    return list(o)


def fit_nonminimal(kind, f0, f1, idx0, idx1=None, math_mode=MATH_TWIN):
    f0 = _f64(f0)
    f1 = _f64(f1) if f1 is not None else None
    i0 = np.ascontiguousarray(np.asarray(idx0, dtype=np.uint64))
    i1 = np.ascontiguousarray(np.asarray(idx1 if idx1 is not None else [], dtype=np.uint64))
    m = np.zeros(7)
    u64 = C.POINTER(C.c_uint64)
    ok = lib().oracle_fit_nonminimal(kind, _dp(f0), f0.shape[0], _dp(f1) if f1 is not None else None,
                                     0 if f1 is None else f1.shape[0], i0.ctypes.data_as(u64), len(i0),
                                     i1.ctypes.data_as(u64), len(i1), math_mode, _dp(m))
    return (m if ok else None)


def find_homography(corr, thr, **kw):
    c = _f64(corr)
    n = c.shape[0]
    mask = np.zeros(n, dtype=np.uint8)
    H = np.zeros(9)
    st = OracleStats()
    p = params(thr, **kw)
    r = lib().oracle_find_homography(_dp(c), n, C.byref(p), mask.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(H),
                                     C.byref(st))
    if r < 0:
        raise RuntimeError("oracle failed")
    return dict(num_inliers=r, mask=mask.astype(bool), H=H.reshape(3, 3), stats=_stats_dict(st))


def h_slot(corr, seed, slot):
    c = _f64(corr)
    m = np.zeros(9)
    inc = lib().oracle_h_slot(_dp(c), c.shape[0], seed, slot, _dp(m))
    return inc, m


def h_score(corr, model9, thr, want_mask=False):
    c = _f64(corr)
    cnt = C.c_uint64()
    val = C.c_double()
    mask = np.zeros(c.shape[0], dtype=np.uint8) if want_mask else None
    lib().oracle_h_score(_dp(c), c.shape[0], _dp(_f64(model9)), thr, C.byref(cnt), C.byref(val),
                         mask.ctypes.data_as(C.POINTER(C.c_uint8)) if want_mask else None)
    out = dict(count=int(cnt.value), value=val.value)
    if want_mask:
        out["mask"] = mask.astype(bool)
    return out


def h_residuals(corr, model9):
    c = _f64(corr)
    r2 = np.zeros(c.shape[0])
    lib().oracle_h_residuals(_dp(c), c.shape[0], _dp(_f64(model9)), _dp(r2))
    return r2


def h_fit(corr, idx):
    c = _f64(corr)
    i = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
    m = np.zeros(9)
    ok = lib().oracle_h_fit(_dp(c), c.shape[0], i.ctypes.data_as(C.POINTER(C.c_uint64)), len(i), _dp(m))
    return m if ok else None


def find_fundamental(corr, thr, **kw):
    c = _f64(corr)
    n = c.shape[0]
    mask = np.zeros(n, dtype=np.uint8)
    H = np.zeros(9)
    st = OracleStats()
    p = params(thr, **kw)
    r = lib().oracle_find_fundamental(_dp(c), n, C.byref(p), mask.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(H),
                                     C.byref(st))
    if r < 0:
        raise RuntimeError("oracle failed")
    return dict(num_inliers=r, mask=mask.astype(bool), H=H.reshape(3, 3), stats=_stats_dict(st))


def f_slot(corr, seed, slot):
    """(inc, models (k, 9)) of one outer-iteration slot of the 7-point solver."""
    c = _f64(corr)
    m = np.zeros(27)
    k = C.c_int()
    inc = lib().oracle_f_slot(_dp(c), c.shape[0], seed, slot, _dp(m), C.byref(k))
    return inc, m.reshape(3, 9)[:k.value].copy()


def f_score(corr, model9, thr, want_mask=False):
    c = _f64(corr)
    cnt = C.c_uint64()
    val = C.c_double()
    mask = np.zeros(c.shape[0], dtype=np.uint8) if want_mask else None
    lib().oracle_f_score(_dp(c), c.shape[0], _dp(_f64(model9)), thr, C.byref(cnt), C.byref(val),
                         mask.ctypes.data_as(C.POINTER(C.c_uint8)) if want_mask else None)
    out = dict(count=int(cnt.value), value=val.value)
    if want_mask:
        out["mask"] = mask.astype(bool)
    return out


def f_residuals(corr, model9):
    c = _f64(corr)
    r2 = np.zeros(c.shape[0])
    lib().oracle_f_residuals(_dp(c), c.shape[0], _dp(_f64(model9)), _dp(r2))
    return r2


def f_fit(corr, idx):
    c = _f64(corr)
    i = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
    m = np.zeros(9)
    ok = lib().oracle_f_fit(_dp(c), c.shape[0], i.ctypes.data_as(C.POINTER(C.c_uint64)), len(i), _dp(m))
    return m if ok else None


def hot_batch(kind, f0, f1, thr0, thr1, seed, slot0, nslots, sampler=SAMPLER_FAITHFUL, math_mode=MATH_GLIBC):
    """Single-thread CPU hot path (sample+solve+score) over nslots slots."""
    f0 = _f64(f0)
    f1 = _f64(f1) if f1 is not None else None
    sec = np.zeros(1)
    best = np.zeros(1)
    n = lib().oracle_hot_batch(kind, _dp(f0), f0.shape[0], _dp(f1) if f1 is not None else None,
                               0 if f1 is None else f1.shape[0], thr0, thr1, seed, slot0, nslots, sampler,
                               math_mode, _dp(sec), _dp(best))
    return int(n), float(sec[0]), float(best[0])


def bk_energy(unary, edges, pair):
    """BK restatement over an energy: unary (n, 2) = E_i(0), E_i(1); edges
    (m, 2); pair (m, 4) = E(00), E(01), E(10), E(11).  Returns (seg (n,) bool,
    True = SINK, flow)."""
    u = _f64(np.asarray(unary).reshape(-1, 2))
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.uint32).reshape(-1, 2))
    pr = _f64(np.asarray(pair).reshape(-1, 4))
    seg = np.zeros(u.shape[0], dtype=np.uint8)
    flow = C.c_double()
    lib().oracle_bk_energy(u.shape[0], _dp(u), e.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(pr), e.shape[0],
                           seg.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(flow))
    return seg.astype(bool), flow.value


def grid_edges(points, cell_size, cell_number):
    """The neighbourhood grid's edge list in labeling()'s order, (m, 2)."""
    pts = _f64(points)
    cs = _f64(np.asarray(cell_size, dtype=np.float64))
    n, d = pts.shape
    m = lib().oracle_grid_edges(_dp(pts), n, d, _dp(cs), int(cell_number), None, 0)
    out = np.zeros((max(m, 1), 2), dtype=np.uint32)
    lib().oracle_grid_edges(_dp(pts), n, d, _dp(cs), int(cell_number), out.ctypes.data_as(C.POINTER(C.c_uint32)), m)
    return out[:m]


def score_less(kind, f0, f1, ma, mb, thr0, thr1=0.0, math_mode=MATH_TWIN):
    """The run loop's `score(ma) < score(mb)` (GCRANSAC.h:440) in math_mode:
    (decision, near_tie, value_order) -- GLIBC compares glibc scores, TWIN the
    value scores with the near-tie rule (csrc/exact.h ScoreBound)."""
    f0 = _f64(f0)
    f1 = _f64(f1) if f1 is not None else None
    L = lib()
    dp = C.POINTER(C.c_double)
    L.oracle_score_less.restype = C.c_int
    L.oracle_score_less.argtypes = [C.c_int, dp, C.c_size_t, dp, C.c_size_t, dp, dp, C.c_double, C.c_double, C.c_int]
    r = L.oracle_score_less(kind, _dp(f0), f0.shape[0], _dp(f1) if f1 is not None else None,
                            0 if f1 is None else f1.shape[0], _dp(_f64(ma)), _dp(_f64(mb)), thr0, thr1, math_mode)
    return bool(r & 1), bool(r & 2), bool(r & 4)


# ---------------------------------------- calibrated and guided whole runs ----
_DP, _U32P, _U64P, _U8P = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
MINIMAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _DP, C.c_size_t, _U32P, _DP)
FIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _DP, C.c_size_t, _U32P, C.c_size_t, _DP)
_calib_ready = False


def _calib_lib():
    global _calib_ready
    L = lib()
    if not _calib_ready:
        pp, sp = C.POINTER(OracleParams), C.POINTER(OracleStats)
        smp = C.POINTER(OracleSampling)
        L.oracle_find_calibrated.argtypes = [_DP, _DP, C.c_size_t, pp, C.c_uint32, C.c_uint32, MINIMAL_FN, FIT_FN,
                                             C.c_void_p, _DP, C.c_int, _U8P, _DP, sp, smp]
        L.oracle_find_homography_guided.argtypes = [_DP, C.c_size_t, pp, _DP, C.c_int, _U8P, _DP, sp, smp]
        L.oracle_find_fundamental_guided.argtypes = L.oracle_find_homography_guided.argtypes
        L.oracle_find_homography_sift.argtypes = [_DP, C.c_size_t, pp, C.c_uint32, MINIMAL_FN, C.c_void_p, _DP,
                                                  C.c_int, _U8P, _DP, sp, smp]
        L.oracle_prosac_growth.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, _U64P]
        L.oracle_sample_prosac.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                           C.c_uint32, C.c_uint64, _U64P, _U64P]
        L.oracle_prosac_stop_tables.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_double, _U32P, _DP]
        L.oracle_prosac_stop_choice.argtypes = [_U8P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_double, _U64P, _U64P]
        L.oracle_prosac_stop_number.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_double]
        L.oracle_prosac_stop_number.restype = C.c_uint64
        L.oracle_napsac_layers.argtypes = [_DP, C.c_uint64, _DP, _U32P, _U32P, _U32P, _U32P]
        L.oracle_samples_napsac.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _DP, C.c_uint64,
                                            C.c_uint32, _DP, C.c_uint64, _U32P]
        L.oracle_sample_guided.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _DP,
                                           C.c_uint64, C.c_uint32, _U64P]
        L.oracle_guided_pick.argtypes = [_DP, C.c_uint64, C.c_uint64]
        L.oracle_guided_pick.restype = C.c_uint64
        L.oracle_guided_quanta.argtypes = [_DP, C.c_uint64, _U64P, _U64P]
        L.oracle_guided_quanta.restype = None
        L.oracle_guided_iterations.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_double]
        L.oracle_guided_iterations.restype = C.c_uint64
        _calib_ready = True
    return L


def sample_guided(seed, index, sub, stream, cls, weights, m):
    """One guided sample (the definition of csrc/guided.h restated): m distinct
    indices in draw order, or None when the 4096-word budget runs out."""
    w = _f64(weights)
    out = np.zeros(m, dtype=np.uint64)
    r = _calib_lib().oracle_sample_guided(seed, index, sub, stream, cls, _dp(w), len(w), m, out.ctypes.data_as(_U64P))
    return out if r == 0 else None


def guided_pick(weights, word):
    """The index the 64-bit word `word` selects."""
    w = _f64(weights)
    return int(_calib_lib().oracle_guided_pick(_dp(w), len(w), word))


def guided_quanta(weights):
    """(q, Q) of csrc/guided_stop.h, restated."""
    w = _f64(weights)
    q = np.zeros(len(w), dtype=np.uint64)
    Q = C.c_uint64()
    _calib_lib().oracle_guided_quanta(_dp(w), len(w), q.ctypes.data_as(_U64P), C.byref(Q))
    return q, Q.value


def guided_iterations(mass, Q, m, confidence):
    return int(_calib_lib().oracle_guided_iterations(mass, Q, m, confidence))


def _weights(weights, n):
    if weights is None:
        return None
    w = _f64(weights)
    if w.shape != (n,):
        raise ValueError("one weight per row")
    return w


SAMPLING_KEYS = ("sampler", "prosac_convergence", "prosac_stop", "napsac_iterations", "napsac_extent")


def _sampling(kw):
    """(kw without the sampler arguments, OracleSampling or None).  sampler: 0
    (uniform, or guided by weights), 1 (PROSAC: the rows are in quality order)
    or 2 (NAPSAC: napsac_extent = (w1, h1, w2, h2), napsac_iterations = T)."""
    kw = dict(kw)
    got = {k: kw.pop(k) for k in SAMPLING_KEYS if k in kw}
    mode = int(got.get("sampler", 0) or 0)
    if mode == 0 and not got.get("prosac_stop"):
        return kw, None
    s = OracleSampling()
    s.mode = mode
    s.prosac_stop = int(bool(got.get("prosac_stop", False)))
    s.prosac_convergence = int(got.get("prosac_convergence", 100000))
    if mode == 2:
        s.napsac_iterations = int(got["napsac_iterations"])
        s.napsac_extent[:] = [float(v) for v in got["napsac_extent"]]
    return kw, s


def _result(r, mask, M, st, sampling, **more):
    if r < 0:
        raise RuntimeError("oracle failed")
    out = dict(num_inliers=r, mask=mask.astype(bool), H=M.reshape(3, 3), stats=_stats_dict(st), **more)
    if sampling is not None and sampling.prosac_stop:
        out["prosac_star"] = (int(sampling.star_i), int(sampling.star_n))
    return out


def _guided_corr(entry, corr, thr, weights, guided_stop, kw):
    c = _f64(corr)
    n = c.shape[0]
    w = _weights(weights, n)
    mask = np.zeros(n, dtype=np.uint8)
    M = np.zeros(9)
    st = OracleStats()
    kw, smp = _sampling(kw)
    p = params(thr, **kw)
    r = entry(_dp(c), n, C.byref(p), None if w is None else _dp(w), int(bool(guided_stop)),
              mask.ctypes.data_as(_U8P), _dp(M), C.byref(st), None if smp is None else C.byref(smp))
    return _result(r, mask, M, st, smp)


def find_homography_guided(corr, thr, weights=None, guided_stop=False, **kw):
    """find_homography with the main loop's samples drawn by the guided
    sampler (weights None: the uniform run) and, with guided_stop, the stop on
    the inlier mass; or, by the sampler arguments of _sampling, by PROSAC
    (prosac_stop: its own stop) or NAPSAC."""
    return _guided_corr(_calib_lib().oracle_find_homography_guided, corr, thr, weights, guided_stop, kw)


def find_fundamental_guided(corr, thr, weights=None, guided_stop=False, **kw):
    return _guided_corr(_calib_lib().oracle_find_fundamental_guided, corr, thr, weights, guided_stop, kw)


def find_homography_sift(corr8, thr, weights=None, guided_stop=False, **kw):
    """findHomographySIFT through the oracle's run loop: the 2-point solver
    reaches it as a callback over gcr_host_solve_s2 (the SIFT columns stay
    here; the callback gets the run's own x1, y1, x2, y2 rows), everything
    else is the oracle's homography solver."""
    from pygcransac import _native as N

    c8 = _f64(corr8)
    c = np.ascontiguousarray(c8[:, :4])
    sift = np.ascontiguousarray(c8[:, 4:8])
    n = c.shape[0]
    cnt = C.c_uint32()

    def minimal(user, rows, nrows, idx, out):
        rc = N.lib.gcr_host_solve_s2(C.cast(rows, C.c_void_p), sift.ctypes.data, nrows, C.cast(idx, C.c_void_p),
                                     C.cast(out, C.c_void_p), C.byref(cnt))
        return int(cnt.value) if rc == 0 else -1

    w = _weights(weights, n)
    mask = np.zeros(n, dtype=np.uint8)
    M = np.zeros(9)
    st = OracleStats()
    kw, smp = _sampling(kw)
    p = params(thr, **kw)
    cb = MINIMAL_FN(_guarded(minimal))
    r = _calib_lib().oracle_find_homography_sift(_dp(c), n, C.byref(p), 3, cb, None, None if w is None else _dp(w),
                                                 int(bool(guided_stop)), mask.ctypes.data_as(_U8P), _dp(M),
                                                 C.byref(st), None if smp is None else C.byref(smp))
    return _result(r, mask, M, st, smp)


# ---- the sampler restatements alone ---------------------------------------------
def prosac_growth(n, m, convergence):
    g = np.zeros(n + 1, dtype=np.uint64)
    if _calib_lib().oracle_prosac_growth(n, m, convergence, g.ctypes.data_as(_U64P)) != 0:
        raise ValueError("need 1 <= m <= n")
    return g


def sample_prosac(seed, slot, attempt, n, m, convergence):
    """(indices or None when the budget ran out, the slot's pool; 0 = uniform phase)"""
    out = np.zeros(m, dtype=np.uint64)
    pool = C.c_uint64()
    r = _calib_lib().oracle_sample_prosac(seed, slot, attempt, 0, 0, n, m, convergence, out.ctypes.data_as(_U64P),
                                          C.byref(pool))
    if r == -2:
        raise ValueError("need 1 <= m <= n")
    return (out if r == 0 else None), int(pool.value)


def prosac_stop_tables(n, m, convergence, confidence):
    imin = np.zeros(n + 1, dtype=np.uint32)
    qmin = np.zeros(n + 1)
    if _calib_lib().oracle_prosac_stop_tables(n, m, convergence, confidence, imin.ctypes.data_as(_U32P),
                                              _dp(qmin)) != 0:
        raise ValueError("need 1 <= m <= n")
    return imin, qmin


def prosac_stop_choice(mask, m, convergence, confidence):
    """(I*, n*) of the mask in row order"""
    mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    bi, bn = C.c_uint64(), C.c_uint64()
    if _calib_lib().oracle_prosac_stop_choice(mk.ctypes.data_as(_U8P), len(mk), m, convergence, confidence,
                                              C.byref(bi), C.byref(bn)) != 0:
        raise ValueError("need 1 <= m <= n")
    return int(bi.value), int(bn.value)


def prosac_stop_number(best_i, best_n, m, confidence):
    return int(_calib_lib().oracle_prosac_stop_number(best_i, best_n, m, confidence))


def napsac_layers(rows, extent):
    """per layer (members, start, count, pos), napsac_cases.host_layers' layout"""
    r = _f64(rows)
    n = len(r)
    e = _f64(extent)
    mem, start, count, pos = (np.zeros((4, n), dtype=np.uint32) for _ in range(4))
    _calib_lib().oracle_napsac_layers(_dp(r), n, _dp(e), *[a.ctypes.data_as(_U32P) for a in (mem, start, count, pos)])
    return [(mem[l], start[l], count[l], pos[l]) for l in range(4)]


def samples_napsac(seed, slot0, nslots, attempt, rows, m, extent, T):
    """(nslots, m) uint32, all-ones rows where the budget ran out"""
    r = _f64(rows)
    e = _f64(extent)
    out = np.zeros((nslots, m), dtype=np.uint32)
    if _calib_lib().oracle_samples_napsac(seed, slot0, nslots, attempt, _dp(r), len(r), m, _dp(e), T,
                                          out.ctypes.data_as(_U32P)) != 0:
        raise ValueError("need 1 <= m <= n and T >= 1")
    return out


def _guarded(fn):
    """A callback that answers -1 (the oracle then fails the run) where fn
    raises: ctypes would print the exception and return 0, "no model", and the
    run would go on as a silently different one."""
    def call(*args):
        try:
            return fn(*args)
        except Exception:
            import traceback

            traceback.print_exc()
            return -1

    return call


def _find_calibrated(corr, K1, K2, thr, m, per, minimal, fit, weights, guided_stop, image_size, neighborhood_size,
                     kw):
    """The oracle's run loop around the product's host solvers: rows and
    threshold from gcr_host_essential_normalise, the grid over the pixels."""
    from pygcransac import _native as N
    from pygcransac import pygcransac as P

    c = _f64(corr)
    n = c.shape[0]
    k1, k2 = _f64(K1), _f64(K2)
    norm = np.zeros_like(c)
    thr_n = C.c_double()
    N.check(N.lib.gcr_host_essential_normalise(c.ctypes.data, n, k1.ctypes.data, k2.ctypes.data, float(thr),
                                               norm.ctypes.data, C.byref(thr_n)))
    if neighborhood_size:
        kw = dict(kw, cell_size=P.grid_cell_sizes(c, *image_size, neighborhood_size), cell_number=neighborhood_size)
    w = _weights(weights, n)
    mask = np.zeros(n, dtype=np.uint8)
    E = np.zeros(9)
    st = OracleStats()
    kw, smp = _sampling(kw)
    p = params(thr_n.value, **kw)
    cb_min, cb_fit = MINIMAL_FN(_guarded(minimal)), FIT_FN(_guarded(fit))
    r = _calib_lib().oracle_find_calibrated(_dp(norm), _dp(c), n, C.byref(p), m, per, cb_min, cb_fit, None,
                                            None if w is None else _dp(w), int(bool(guided_stop)),
                                            mask.ctypes.data_as(_U8P), _dp(E), C.byref(st),
                                            None if smp is None else C.byref(smp))
    return _result(r, mask, E, st, smp, rows=norm, thr=thr_n.value)


IMAGE_SIZE = (960.0, 1280.0, 960.0, 1280.0)          # h1, w1, h2, w2 of pygcransac.synthetic


def find_essential(corr, K1, K2, thr, weights=None, guided_stop=False, image_size=IMAGE_SIZE, neighborhood_size=8,
                   **kw):
    """findEssentialMatrix through the oracle's run loop: the 5-point solver
    and its fit reach it as callbacks over gcr_host_solve_minimal(5) and
    gcr_host_fit_e.  thr in pixels.  Also returns the normalised rows and
    threshold the run used ("rows", "thr")."""
    from pygcransac import _native as N

    cnt = C.c_uint32()

    def minimal(user, rows, n, idx, out):
        rc = N.lib.gcr_host_solve_minimal(N.SOLVER_ESSENTIAL5, rows, n, idx, out, C.byref(cnt))
        return int(cnt.value) if rc == 0 else -1

    def fit(user, rows, n, idx, k, out):
        return N.lib.gcr_host_fit_e(rows, n, idx, k, out)

    return _find_calibrated(corr, K1, K2, thr, 5, 10, minimal, fit, weights, guided_stop, image_size,
                            neighborhood_size, kw)


def find_gravity_essential(corr, K1, K2, G1, G2, thr, weights=None, guided_stop=False, image_size=IMAGE_SIZE,
                           neighborhood_size=8, **kw):
    """findGravityEssentialMatrix through the oracle's run loop, the callbacks
    over gcr_host_solve_g3 and gcr_host_fit_g."""
    from pygcransac import _native as N

    g1, g2 = _f64(G1), _f64(G2)
    cnt = C.c_uint32()

    def minimal(user, rows, n, idx, out):
        rc = N.lib.gcr_host_solve_g3(rows, n, idx, g1.ctypes.data, g2.ctypes.data, out, C.byref(cnt))
        return int(cnt.value) if rc == 0 else -1

    def fit(user, rows, n, idx, k, out):
        return N.lib.gcr_host_fit_g(rows, n, idx, k, g1.ctypes.data, g2.ctypes.data, out)

    return _find_calibrated(corr, K1, K2, thr, 3, 4, minimal, fit, weights, guided_stop, image_size,
                            neighborhood_size, kw)
