"""pygcransac -- drop-in Python API of yuvalnis/graph-cut-ransac, MI355X engine.

Surface mirrors ``src/pygcransac/src/bindings.cpp:315-396`` of the reference:
three functions with the same positional/keyword arguments, defaults, input
validation messages and return tuples, and the five model classes with the
same names, inheritance, attributes and methods.  Extensions are keyword-only
(``seed``, ``confidence``, ``device``, ``batch_slots``, ``return_stats``).

Compute goes through the C ABI in ``include/gcr.h`` (libgcr.so: HIP kernels for
gfx950 plus the host engine).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from . import _native as N

__all__ = [
    "NormalizingTransform",
    "RectifyingHomography",
    "ScaleBasedRectifyingHomography",
    "OrientationBasedRectifyingHomography",
    "SIFTRectifyingHomography",
    "findRectifyingHomographyScaleOnly",
    "findRectifyingHomographyScaleOnlyOriginal",
    "findRectifyingHomographySIFT",
    "findHomography",
    "findFundamentalMatrix",
    "findEssentialMatrix",
    "findGravityEssentialMatrix",
    "findHomographySIFT",
]

_TWO_PI = 2.0 * math.pi


# ----------------------------------------------------------- model classes --
class _F64:
    """double data member with pybind11 def_readwrite semantics."""

    def __set_name__(self, owner, name):
        self.name = "_" + name

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        return obj.__dict__[self.name]

    def __set__(self, obj, value):
        if type(value) is float:                     # the common case, no ABC checks
            obj.__dict__[self.name] = value
            return
        if isinstance(value, (str, bytes)) or not isinstance(value, (numbers.Real, np.floating, np.integer)):
            raise TypeError(f"incompatible type for double attribute: {type(value).__name__}")
        obj.__dict__[self.name] = float(value)


def _cpow(x, y):
    """glibc pow() itself (numpy's SIMD power is not glibc, math.pow raises)."""
    return _libm.pow(x, y)


def _clip_angle(a):
    # math_utils.hpp:78-88 (std::fmod, then + 2pi if negative)
    if math.isinf(a) or math.isnan(a):
        return math.nan
    a = math.fmod(a, _TWO_PI)
    if a < 0.0:
        a += _TWO_PI
    return a


def _atan2(y, x):
    return math.atan2(y, x)


_libm = C.CDLL("libm.so.6")
_libm.pow.argtypes = [C.c_double, C.c_double]
_libm.pow.restype = C.c_double
_libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_libm.sincos.restype = None


def _sincos(t):
    """glibc sincos: the reference (GCC -O3) fuses model.h's adjacent
    std::cos/std::sin calls into sincos, which differs from separate sin/cos
    in ~0.1% of arguments."""
    s, c = C.c_double(), C.c_double()
    _libm.sincos(t, C.byref(s), C.byref(c))
    return s.value, c.value


class NormalizingTransform:
    """model.h:42-120"""
    x0 = _F64()
    y0 = _F64()
    s = _F64()

    def __init__(self):
        self.x0 = 0.0
        self.y0 = 0.0
        self.s = 1.0

    def _fields(self):
        return {k: getattr(self, k) for k in ("x0", "y0", "s")}

    def __repr__(self):
        inner = ", ".join(f"{k}={v!r}" for k, v in self._fields().items())
        return f"{type(self).__name__}({inner})"


class RectifyingHomography(NormalizingTransform):
    """model.h:122-227 (+ the pybind11 lambdas at bindings.cpp:335-353)."""
    h7 = _F64()
    h8 = _F64()

    def __init__(self):
        super().__init__()
        self.h7 = 0.0
        self.h8 = 0.0

    def _fields(self):
        d = super()._fields()
        d.update(h7=self.h7, h8=self.h8)
        return d

    def rectifiedScale(self, dx, dy, ds):
        return float(ds) * _cpow(-self.h7 * float(dx) - self.h8 * float(dy) + 1.0, -3.0)

    def unrectifiedScale(self, udx, udy, uds):
        return float(uds) * _cpow(self.h7 * float(udx) + self.h8 * float(udy) + 1.0, -3.0)

    def rectifiedAngle(self, x, y, angle):
        x, y, angle = float(x), float(y), float(angle)
        st, ct = _sincos(angle)
        numer = (-x * st + y * ct) * self.h7 + st
        denom = (x * st - y * ct) * self.h8 + ct
        return _clip_angle(_atan2(numer, denom))

    def unrectifiedAngle(self, x, y, angle):
        x, y, angle = float(x), float(y), float(angle)
        st, ct = _sincos(angle)
        numer = (x * st - y * ct) * self.h7 + st
        denom = (-x * st + y * ct) * self.h8 + ct
        return _clip_angle(_atan2(numer, denom))

    def rectifiedPoint(self, x, y):
        x, y = float(x), float(y)
        w = -self.h7 * x - self.h8 * y + 1.0
        with np.errstate(all="ignore"):
            return (float(np.float64(x) / w), float(np.float64(y) / w))

    def unrectifiedPoint(self, x, y):
        x, y = float(x), float(y)
        w = self.h7 * x + self.h8 * y + 1.0
        with np.errstate(all="ignore"):
            return (float(np.float64(x) / w), float(np.float64(y) / w))

    def getHomography(self):
        # N.inverse() * [[1,0,0],[0,1,0],[h7,h8,1]] * N / H22 with Eigen's
        # 3x3 cofactor inverse, evaluated in IEEE double like the C++ code.
        s, x0, y0 = self.s, self.x0, self.y0
        Nm = [s, 0.0, -s * x0, 0.0, s, -s * y0, 0.0, 0.0, 1.0]
        Hn = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, self.h7, self.h8, 1.0]

        def cof(i, j):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            return Nm[i1 * 3 + j1] * Nm[i2 * 3 + j2] - Nm[i1 * 3 + j2] * Nm[i2 * 3 + j1]

        with np.errstate(all="ignore"):
            det = (cof(0, 0) * Nm[0] + cof(1, 0) * Nm[3]) + cof(2, 0) * Nm[6]
            invdet = float(np.float64(1.0) / det)
            Ni = [cof(c, r) * invdet for r in range(3) for c in range(3)]
            T = [(Ni[i * 3] * Hn[j] + Ni[i * 3 + 1] * Hn[3 + j]) + Ni[i * 3 + 2] * Hn[6 + j]
                 for i in range(3) for j in range(3)]
            R = [(T[i * 3] * Nm[j] + T[i * 3 + 1] * Nm[3 + j]) + T[i * 3 + 2] * Nm[6 + j]
                 for i in range(3) for j in range(3)]
            d = np.float64(R[8])
            return np.array([np.float64(v) / d for v in R], dtype=np.float64).reshape(3, 3)


class ScaleBasedRectifyingHomography(RectifyingHomography):
    """model.h:229-234"""
    alpha = _F64()

    def __init__(self):
        super().__init__()
        self.alpha = 1.0

    def _fields(self):
        d = super()._fields()
        d.update(alpha=self.alpha)
        return d


class OrientationBasedRectifyingHomography(RectifyingHomography):
    """model.h:236-241"""
    phi = _F64()

    def __init__(self):
        super().__init__()
        self.phi = 0.0

    def _fields(self):
        d = super()._fields()
        d.update(phi=self.phi)
        return d


class SIFTRectifyingHomography(ScaleBasedRectifyingHomography, OrientationBasedRectifyingHomography):
    """model.h:243-246"""


# --------------------------------------------------------------- helpers ---
def _as_features(arr):
    """py::array_t<double> conversion (forcecast) + flat C-contiguous buffer."""
    try:
        a = np.asarray(arr, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise TypeError(f"incompatible function arguments: cannot convert to float64 array ({exc})") from None
    return a


def _as_size_t(v, name):
    if type(v) is int and 0 <= v <= 0xFFFFFFFFFFFFFFFF:
        return v
    if isinstance(v, (bool, np.bool_)):
        v = int(v)
    if not isinstance(v, (numbers.Integral, np.integer)) or v < 0:
        raise TypeError(f"incompatible function arguments: {name} must be a non-negative integer")
    if int(v) > 0xFFFFFFFFFFFFFFFF:
        raise TypeError(f"incompatible function arguments: {name} does not fit size_t")
    return int(v)


def _as_double(v, name):
    if type(v) is float:
        return v
    if isinstance(v, (str, bytes)) or not isinstance(v, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f"incompatible function arguments: {name} must be a float")
    return float(v)


def _params(thr0, thr1, lam, min_it, max_it, lo, seed, confidence, batch_slots):
    p = N.default_params()
    p.scale_residual_thresh = _as_double(thr0, "scale_residual_thresh")
    p.orientation_residual_thresh = _as_double(thr1, "orientation_residual_thresh")
    p.spatial_coherence_weight = _as_double(lam, "spatial_coherence_weight")
    p.min_iteration_number = _as_size_t(min_it, "min_iteration_number")
    p.max_iteration_number = _as_size_t(max_it, "max_iteration_number")
    p.max_local_optimization_number = _as_size_t(lo, "max_local_optimization_number")
    p.seed = _as_size_t(seed, "seed")
    p.confidence = _as_double(confidence, "confidence")
    p.batch_slots = _as_size_t(batch_slots, "batch_slots") & 0xFFFFFFFF
    return p


_DP, _U8P = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def _dp(a):
    return C.cast(a.ctypes.data, _DP)


def _u8(a):
    return C.cast(a.ctypes.data, _U8P)


def _fill(model, m: N.RectModel, sift: bool):
    # the engine's doubles straight into the model's slots (_F64 stores
    # Python floats under "_" + name; ctypes double fields read as floats)
    d = model.__dict__
    d["_x0"], d["_y0"], d["_s"] = m.x0, m.y0, m.s
    d["_h7"], d["_h8"], d["_alpha"] = m.h7, m.h8, m.alpha
    if sift:
        d["_phi"] = m.phi
    return model


def _validate_scale_only(features):
    f = _as_features(features)
    if f.ndim != 2:
        raise ValueError("Number of dimensions must be 2.")
    n, cols = f.shape
    if n < 3 or cols != 3:
        raise ValueError(f"Features should be an array with 3 columns and at least 3 rows. "
                         f"It has {cols} columns and {n} rows.")
    return np.ascontiguousarray(f)


def _scale_only(original, features, scale_residual_thresh, spatial_coherence_weight, min_iteration_number,
                max_iteration_number, max_local_optimization_number, seed, confidence, device, batch_slots,
                return_stats):
    f = _validate_scale_only(features)
    p = _params(scale_residual_thresh, 2.0, spatial_coherence_weight, min_iteration_number, max_iteration_number,
                max_local_optimization_number, seed, confidence, batch_slots)
    n = f.shape[0]
    mask = np.zeros(n, dtype=np.uint8)
    H = np.zeros(9, dtype=np.float64)
    m = N.RectModel()
    st = N.Stats()
    ctx = N.context(device)
    rc = N.lib.gcr_rect_scale_only(ctx, f.ctypes.data, n, C.byref(p), 1 if original else 0, mask.ctypes.data,
                                   H.ctypes.data, C.byref(m), C.byref(st))
    num_inliers = N.check(rc)
    inliers = mask.view(bool)
    extra = (st.as_dict(),) if return_stats else ()
    if num_inliers == 0:
        return (None, inliers) + extra
    model = _fill(ScaleBasedRectifyingHomography(), m, sift=False)
    return (H.reshape(3, 3), inliers, model) + extra


# -------------------------------------------------------------- entry points
def findRectifyingHomographyScaleOnly(features, scale_residual_thresh, spatial_coherence_weight=0.0,
                                      min_iteration_number=10000, max_iteration_number=10000,
                                      max_local_optimization_number=50, *, seed=0, confidence=0.95, device=None,
                                      batch_slots=0, return_stats=False):
    """3-SIFT scale-only rectification (bindings.cpp:19-98, 366-374).

    Returns ``(H, inliers, ScaleBasedRectifyingHomography)`` or ``(None, inliers)``
    when no model is found.
    """
    return _scale_only(False, features, scale_residual_thresh, spatial_coherence_weight, min_iteration_number,
                       max_iteration_number, max_local_optimization_number, seed, confidence, device, batch_slots,
                       return_stats)


def findRectifyingHomographyScaleOnlyOriginal(features, scale_residual_thresh, spatial_coherence_weight=0.0,
                                              min_iteration_number=10000, max_iteration_number=10000,
                                              max_local_optimization_number=50, *, seed=0, confidence=0.95,
                                              device=None, batch_slots=0, return_stats=False):
    """Original-parametrisation 3-SIFT solver (bindings.cpp:100-179, 376-384)."""
    return _scale_only(True, features, scale_residual_thresh, spatial_coherence_weight, min_iteration_number,
                       max_iteration_number, max_local_optimization_number, seed, confidence, device, batch_slots,
                       return_stats)


def findRectifyingHomographySIFT(scale_features, orientation_features, scale_residual_thresh,
                                 orientation_residual_thresh, spatial_coherence_weight=0.0,
                                 min_iteration_number=10000, max_iteration_number=10000,
                                 max_local_optimization_number=50, *, seed=0, confidence=0.95, device=None,
                                 batch_slots=0, return_stats=False):
    """Hybrid 2+2 SIFT rectification (bindings.cpp:181-311, 386-396).

    Returns ``(H, scale_inliers, orientation_inliers, SIFTRectifyingHomography)``
    or ``(None, scale_inliers, orientation_inliers, None)``.
    """
    fs = _as_features(scale_features)
    fo = _as_features(orientation_features)
    if fs.ndim != 2 or fo.ndim != 2:
        raise ValueError("Number of dimensions must be 2.")
    ns, cs = fs.shape
    no, co = fo.shape
    if ns < 2 or cs != 3:
        raise ValueError(f"Scale features should be an array with 3 columns and at least 2 rows. "
                         f"It has {cs} columns and {ns} rows.")
    if no < 2 or co != 3:
        raise ValueError(f"Orientation features should be an array with 3 columns and at least 2 rows. "
                         f"It has {co} columns and {no} rows.")
    fs = np.ascontiguousarray(fs)
    fo = np.ascontiguousarray(fo)
    p = _params(scale_residual_thresh, orientation_residual_thresh, spatial_coherence_weight, min_iteration_number,
                max_iteration_number, max_local_optimization_number, seed, confidence, batch_slots)
    ms = np.zeros(ns, dtype=np.uint8)
    mo = np.zeros(no, dtype=np.uint8)
    H = np.zeros(9, dtype=np.float64)
    m = N.RectModel()
    st = N.Stats()
    ctx = N.context(device)
    rc = N.lib.gcr_rect_sift(ctx, fs.ctypes.data, ns, fo.ctypes.data, no, C.byref(p), ms.ctypes.data,
                             mo.ctypes.data, H.ctypes.data, C.byref(m), C.byref(st))
    num_inliers = N.check(rc)
    s_in, o_in = ms.view(bool), mo.view(bool)
    extra = (st.as_dict(),) if return_stats else ()
    if num_inliers == 0:
        return (None, s_in, o_in, None) + extra
    model = _fill(SIFTRectifyingHomography(), m, sift=True)
    return (H.reshape(3, 3), s_in, o_in, model) + extra


def grid_cell_sizes(correspondences, h1, w1, h2, w2, neighborhood_size):
    """Cell sizes of the neighbourhood grid over (x1, y1, x2, y2): each image
    extent divided by `neighborhood_size` cells (upstream GC-RANSAC's
    GridNeighborhoodGraph<4> over {w1, h1, w2, h2} / cells).  An image size
    <= 0 (unknown) is replaced by the correspondences' extent along that axis
    (max coordinate + 1, at least 1 px)."""
    k = float(neighborhood_size)
    sizes = [float(v) for v in (w1, h1, w2, h2)]
    known = [v > 0.0 and math.isfinite(v) for v in sizes]
    if not all(known):
        f = np.asarray(correspondences, dtype=np.float64)
        for col in range(4):
            if known[col]:
                continue
            if not f.size:
                sizes[col] = 1.0
                continue
            c = f[:, col]
            top = float(c.max())                    # NaN / inf present: the finite values only
            if not math.isfinite(top):
                fin = c[np.isfinite(c)]
                top = float(fin.max()) if fin.size else None
            sizes[col] = max(1.0, top + 1.0) if top is not None else 1.0
    return [v / k for v in sizes]


def grid_params(correspondences, h1, w1, h2, w2, neighborhood_size, from_data=True):
    """(cell_number, cell sizes or None) of gcr_params' neighbourhood grid.
    from_data=False leaves an unknown image size's cells at 0 for the engine
    to take from the data (the same values, computed natively)."""
    cells = _as_size_t(neighborhood_size, "neighborhood_size")
    if cells > 0xFFFFFFFF:
        raise ValueError("neighborhood_size does not fit 32 bits")
    if not cells:
        return cells, None
    if from_data:
        return cells, grid_cell_sizes(correspondences, h1, w1, h2, w2, cells)
    k = float(cells)
    return cells, [float(v) / k if float(v) > 0.0 and math.isfinite(float(v)) else 0.0 for v in (w1, h1, w2, h2)]


def _set_grid(p, correspondences, h1, w1, h2, w2, neighborhood_size):
    cells, sizes = grid_params(correspondences, h1, w1, h2, w2, neighborhood_size)
    p.cell_number = cells
    if cells:
        p.cell_size[:] = sizes


def _as_probabilities(probabilities, n, m):
    """The guided sampler's weights as a contiguous float64 vector of length
    n, checked by the engine for a minimal sample of m (before any GPU work:
    a bad vector is a ValueError with the engine's message)."""
    w = np.ascontiguousarray(np.asarray(probabilities, dtype=np.float64))
    if w.ndim != 1 or w.shape[0] != n:
        raise ValueError(f"probabilities must be a vector with one entry per correspondence ({n}); "
                         f"it has shape {tuple(w.shape)}.")
    N.check(N.lib.gcr_host_check_probabilities(w.ctypes.data, n, m))
    return w


PROSAC_MAX_CONVERGENCE = 1 << 40


def _as_scores(scores, n):
    """PROSAC's quality scores as a float64 vector of length n: one per
    correspondence, higher is better, every value finite."""
    q = np.asarray(scores, dtype=np.float64)
    if q.ndim != 1 or q.shape[0] != n:
        raise ValueError(f"probabilities must be a vector with one quality score per correspondence ({n}); "
                         f"it has shape {tuple(q.shape)}.")
    if not np.all(np.isfinite(q)):
        raise ValueError("sampler=1 (PROSAC) orders the correspondences by their scores: every score must be finite.")
    if n > 1 and q.min() == q.max():
        # ties keep the input order, but scores that are ALL equal rank nothing: the run would sample the first
        # rows first for no reason the caller gave (all-ones weights, sampler 3's neutral vector, end up here)
        raise ValueError(f"sampler=1 (PROSAC) needs scores that rank the correspondences: all {n} are equal. "
                         f"Uniform sampling is sampler=0; rows already in quality order take -np.arange(n).")
    return q


def prosac_order(scores):
    """The row order PROSAC samples in: by score descending, ties in input
    order (a stable sort)."""
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")


def _as_convergence(prosac_convergence):
    t = _as_size_t(prosac_convergence, "prosac_convergence")
    if t < 1 or t > PROSAC_MAX_CONVERGENCE:
        raise ValueError(f"prosac_convergence must be in 1 .. 2^40, got {prosac_convergence}.")
    return t


NAPSAC_MAX_ITERATIONS = 1 << 40


def _as_napsac_iterations(napsac_iterations, n):
    """NAPSAC's local length T: None is ceil(n / 2), upstream's sampler_length
    0.5 x N."""
    if napsac_iterations is None:
        return max(1, (n + 1) // 2)
    t = _as_size_t(napsac_iterations, "napsac_iterations")
    if t < 1 or t > NAPSAC_MAX_ITERATIONS:
        raise ValueError(f"napsac_iterations must be in 1 .. 2^40, got {napsac_iterations}.")
    return t


def napsac_extent(correspondences, h1, w1, h2, w2):
    """The extents {w1, h1, w2, h2} NAPSAC's grid layers divide: the image
    sizes, an unknown one (<= 0) taken from the data by grid_cell_sizes' rule."""
    return grid_cell_sizes(correspondences, h1, w1, h2, w2, 1)


def _correspondence_call(entry, guided_entry, correspondences, h1, w1, h2, w2, probabilities, threshold, conf,
                         spatial_coherence_weight, max_iters, min_iters, sampler, lo_number, seed, device,
                         batch_slots, return_stats, min_rows, neighborhood_size, guided_stop=False, min_weights=None,
                         create=None, prosac_convergence=100000, prosac_stop=False, napsac_iterations=None):
    """min_weights: the minimal sample size the probabilities are checked for
    (default: min_rows).  create(ctx, rows, order, out): a resident problem of
    the estimator over `rows`, the caller's rows taken in `order` (sampler=1;
    sampler=2: every row in place)."""
    for name, v in (("h1", h1), ("w1", w1), ("h2", h2), ("w2", w2)):
        _as_double(v, name)
    sampler_id = _as_size_t(sampler, "sampler")
    if sampler_id not in (0, 1, 2, 3):
        raise ValueError(f"Unsupported sampler {sampler}: only 0 (uniform), 1 (PROSAC, ordered by quality scores), "
                         f"2 (NAPSAC, local by position) and 3 (guided by probabilities, importance sampling) are "
                         f"supported.")
    if sampler_id == 2 and probabilities is not None and len(probabilities) != 0:
        raise ValueError("Unsupported sampler 2 with probabilities: NAPSAC samples by position and takes none "
                         "(PROSAC is 1, guided sampling 3).")
    if sampler_id == 0 and probabilities is not None and len(probabilities) != 0:
        raise ValueError("The uniform sampler (0) takes no probabilities; they must be empty (sampler=3 uses them).")
    if sampler_id == 3 and probabilities is None:
        raise ValueError("sampler=3 (guided) needs probabilities, one per correspondence.")
    if sampler_id == 1 and probabilities is None:
        raise ValueError("sampler=1 (PROSAC) needs probabilities: one quality score per correspondence, higher is "
                         "better (rows already in quality order: -np.arange(n)).")
    if guided_stop and sampler_id != 3:
        raise ValueError("guided_stop=True stops on the guided sampler's inlier mass: it needs sampler=3 "
                         "with probabilities.")
    if prosac_stop and sampler_id != 1:
        raise ValueError("prosac_stop=True stops on PROSAC's best-ranked prefix: it needs sampler=1 with quality "
                         "scores.")
    f = _as_features(correspondences)
    if f.ndim != 2:
        raise ValueError("Number of dimensions must be 2.")
    n, cols = f.shape
    if n < min_rows or cols != 4:
        raise ValueError(f"Correspondences should be an array with 4 columns and at least {min_rows} rows. "
                         f"It has {cols} columns and {n} rows.")
    f = np.ascontiguousarray(f)
    p = _params(threshold, 2.0, spatial_coherence_weight, min_iters, max_iters, lo_number, seed, conf, batch_slots)
    _set_grid(p, f, h1, w1, h2, w2, neighborhood_size)
    if guided_stop:
        p.flags |= N.FLAG_GUIDED_STOP
    if prosac_stop:
        p.flags |= N.FLAG_PROSAC_STOP
    mask = np.zeros(n, dtype=np.uint8)
    M = np.zeros(9, dtype=np.float64)
    st = N.Stats()
    w = _as_probabilities(probabilities, n, min_weights or min_rows) if sampler_id == 3 else None
    if sampler_id == 1:
        convergence = _as_convergence(prosac_convergence)
        order = prosac_order(_as_scores(probabilities, n))
    if sampler_id == 2:
        local = _as_napsac_iterations(napsac_iterations, n)
        extent = (C.c_double * 4)(*napsac_extent(f, h1, w1, h2, w2))
    ctx = N.context(device)
    if sampler_id == 1:
        # the resident-problem API on the rows in quality order; the mask goes
        # back to the caller's order
        rows = np.ascontiguousarray(f[order])
        h = C.c_void_p()
        N.check(create(ctx, rows, order, C.byref(h)))
        try:
            N.check(N.lib.gcr_problem_set_prosac(h, convergence))
            ordered = np.zeros(n, dtype=np.uint8)
            rc = N.lib.gcr_problem_run(h, C.byref(p), ordered.ctypes.data_as(C.POINTER(C.c_uint8)), None,
                                       M.ctypes.data_as(C.POINTER(C.c_double)), C.byref(N.RectModel()), C.byref(st))
        finally:
            N.lib.gcr_problem_destroy(h)
        mask[order] = ordered
    elif sampler_id == 2:
        # the resident-problem API on the rows as they are
        h = C.c_void_p()
        N.check(create(ctx, f, np.arange(n), C.byref(h)))
        try:
            N.check(N.lib.gcr_problem_set_napsac(h, extent, local))
            rc = N.lib.gcr_problem_run(h, C.byref(p), mask.ctypes.data_as(C.POINTER(C.c_uint8)), None,
                                       M.ctypes.data_as(C.POINTER(C.c_double)), C.byref(N.RectModel()), C.byref(st))
        finally:
            N.lib.gcr_problem_destroy(h)
    elif sampler_id == 3:
        rc = guided_entry(ctx, f.ctypes.data, n, w.ctypes.data, C.byref(p), mask.ctypes.data, M.ctypes.data,
                          C.byref(st))
    else:
        rc = entry(ctx, f.ctypes.data, n, C.byref(p), mask.ctypes.data, M.ctypes.data, C.byref(st))
    num_inliers = N.check(rc)
    inliers = mask.view(bool)
    extra = (st.as_dict(),) if return_stats else ()
    if num_inliers == 0:
        return (None, inliers) + extra
    return (M.reshape(3, 3), inliers) + extra


def _plain_create(solver):
    def create(ctx, rows, order, out):
        return N.lib.gcr_problem_create(ctx, solver, rows.ctypes.data_as(C.POINTER(C.c_double)), rows.shape[0], None,
                                        0, out)
    return create


def findHomography(correspondences, h1, w1, h2, w2, probabilities=None, threshold=1.0, conf=0.99,
                   spatial_coherence_weight=0.975, max_iters=10000, min_iters=50, sampler=0, lo_number=50, *,
                   neighborhood_size=8, seed=0, device=None, batch_slots=0, return_stats=False, guided_stop=False,
                   prosac_convergence=100000, prosac_stop=False, napsac_iterations=None):
    """4-point homography with graph-cut LO -- an EXTENSION (SURVEY.md §8(f)
    row 3): this fork has no homography estimator (finding 0.1); the argument
    names and order follow upstream pygcransac's findHomography.

    ``correspondences`` is (N, 4) float64: x1, y1, x2, y2.  ``h1, w1, h2, w2``
    are the image sizes: the graph-cut's neighbourhood grid over (x1, y1, x2,
    y2) has ``neighborhood_size`` cells along each axis (cell sizes w1/k, h1/k,
    w2/k, h2/k; a size <= 0 is taken from the data's extent), and
    ``spatial_coherence_weight`` (lambda) weighs its pairwise terms in every
    graph-cut labeling (GCRANSAC.h:759-870); ``neighborhood_size=0`` or
    lambda = 0 gives the empty grid.  ``sampler`` is 0 (uniform, ``probabilities``
    empty) or 3 (guided, upstream's importance sampler): ``probabilities`` then
    holds one weight per correspondence (finite, >= 0, at least 4 of them > 0),
    and every minimal sample of the main loop draws correspondence i with
    probability w[i] / sum(w); a zero weight is never drawn, and local
    optimisation's inner sampler stays uniform.  The adaptive stop is the
    reference's bound on the inlier share I / N, which describes uniform
    sampling; ``guided_stop=True`` (``sampler=3`` only, else ValueError) takes
    the same bound on the best model's inlier MASS, the inliers' share of the
    weights (csrc/guided_stop.h), so a run with informative weights returns as
    soon as its own sampler justifies it.  With all-equal weights both stops
    are identical.  The bound is meaningful when no single weight dominates
    the sum.  ``sampler=1`` is PROSAC (upstream's sampler 1; csrc/prosac.h is
    the definition): ``probabilities`` then holds one quality score per
    correspondence, higher is better, every value finite (a SIFT ratio-test
    value negated -- ``-ratios`` of ``features.match_descriptors`` is one --,
    a descriptor similarity; rows already in quality order:
    ``-np.arange(n)``; scores that are all equal rank nothing and are a
    ValueError).  The rows are sorted by score descending (stable: ties
    keep their order), early iterations sample among the best-ranked rows, the
    pool grows on PROSAC's schedule of ``prosac_convergence`` iterations
    (1 .. 2^40) and past it every iteration is the uniform sampler's; the mask
    comes back in the caller's order.  Only an order is needed.  The stop
    stays the reference's uniform bound unless ``prosac_stop=True``
    (``sampler=1`` only, else ValueError): then it is PROSAC's own
    non-randomness / maximality stop (csrc/prosac_stop.h), the same bound on
    the best model's inlier share over the best-ranked prefix that is
    non-random and that the samples drawn so far cover; it can only end a run
    sooner.  ``guided_stop`` does not apply.  ``sampler=2`` is (progressive)
    NAPSAC (upstream's sampler 2; csrc/napsac.h is the definition): it takes
    no ``probabilities``, only the positions.  During the first
    ``napsac_iterations`` iterations (1 .. 2^40; None: half the number of
    correspondences, upstream's length) a sample's first correspondence is
    drawn uniformly and the others from its cell of a grid over (x1, y1, x2,
    y2) -- 16, 8, 4, then 2 cells per axis over the image sizes, a quarter of
    the length each, the next coarser grid where the cell is too small --
    and from then on every iteration is the uniform sampler's.  It suits
    inliers that are a local structure among outliers spread over the images.
    The stop is the uniform bound, also during the local iterations, where
    it is a heuristic; ``guided_stop`` and ``prosac_stop`` do not apply.  The other four correspondence estimators take it the same way.
    ``threshold`` is the inlier threshold in pixels
    of the second image (MSAC threshold 2.25 * threshold, as the rectification
    solvers).

    Returns ``(H, inliers)`` with H (3, 3) and H[2, 2] = 1, or ``(None, inliers)``.
    """
    return _correspondence_call(N.lib.gcr_find_homography, N.lib.gcr_find_homography_guided, correspondences,
                                h1, w1, h2, w2, probabilities, threshold, conf, spatial_coherence_weight, max_iters,
                                min_iters, sampler, lo_number,
                                seed, device, batch_slots, return_stats, 4, neighborhood_size, guided_stop,
                                create=_plain_create(N.SOLVER_HOMOGRAPHY4), prosac_convergence=prosac_convergence,
                                prosac_stop=prosac_stop, napsac_iterations=napsac_iterations)


def findFundamentalMatrix(correspondences, h1, w1, h2, w2, probabilities=None, threshold=1.0, conf=0.99,
                          spatial_coherence_weight=0.975, max_iters=10000, min_iters=50, sampler=0, lo_number=50,
                          *, neighborhood_size=8, seed=0, device=None, batch_slots=0, return_stats=False,
                          guided_stop=False, prosac_convergence=100000, prosac_stop=False, napsac_iterations=None):
    """7-point fundamental matrix with graph-cut LO -- an EXTENSION like
    findHomography (same arguments, the same neighbourhood grid; upstream
    pygcransac's findFundamentalMatrix order).  The residual is the Sampson distance in pixels; a sample yields up
    to three models, each scored.  ``sampler=3`` with ``probabilities`` (at least
    7 of them > 0) guides the 7-point samples as it does findHomography's, and
    ``guided_stop=True`` stops such a run on the inlier mass, as there;
    ``sampler=1`` with quality scores and ``prosac_convergence`` is PROSAC, as
    there, and ``prosac_stop=True`` its own stop.

    Returns ``(F, inliers)`` with F (3, 3), unit Frobenius norm and
    x2^T F x1 = 0, or ``(None, inliers)``.
    """
    return _correspondence_call(N.lib.gcr_find_fundamental_matrix, N.lib.gcr_find_fundamental_matrix_guided,
                                correspondences, h1, w1, h2, w2, probabilities,
                                threshold, conf, spatial_coherence_weight, max_iters, min_iters, sampler, lo_number,
                                seed, device, batch_slots, return_stats, 7, neighborhood_size, guided_stop,
                                create=_plain_create(N.SOLVER_FUNDAMENTAL7), prosac_convergence=prosac_convergence,
                                prosac_stop=prosac_stop, napsac_iterations=napsac_iterations)


def _as_calibration(K, name):
    k = np.ascontiguousarray(np.asarray(K, dtype=np.float64))
    if k.shape != (3, 3):
        raise ValueError(f"{name} must be a 3 x 3 calibration matrix; it has shape {tuple(k.shape)}.")
    return k


def findEssentialMatrix(correspondences, K1, K2, h1, w1, h2, w2, probabilities=None, threshold=1.0, conf=0.99,
                        spatial_coherence_weight=0.975, max_iters=10000, min_iters=50, sampler=0, lo_number=50, *,
                        neighborhood_size=8, seed=0, device=None, batch_slots=0, return_stats=False,
                        guided_stop=False, prosac_convergence=100000, prosac_stop=False, napsac_iterations=None):
    """5-point essential matrix with graph-cut LO for calibrated cameras -- an
    EXTENSION like findFundamentalMatrix (upstream pygcransac's
    findEssentialMatrix order; csrc/ess.h is the solver's definition).

    ``correspondences`` is (N, 4) float64 in PIXELS, ``K1`` and ``K2`` are the
    3 x 3 calibration matrices (finite, third row exactly (0, 0, 1),
    K[1, 0] == 0, positive focal lengths; skew allowed).  The estimator runs on
    K^-1 x with the Sampson distance; ``threshold`` is in pixels and is divided
    by the mean of the four focal lengths (upstream's rule).  The neighbourhood
    grid lies over the pixel coordinates, as findFundamentalMatrix's.  A sample
    yields up to ten models, each scored.  ``sampler``, ``probabilities`` (at
    least 5 of them > 0) and ``guided_stop`` as in findHomography, and so are
    ``sampler=1`` (PROSAC: quality scores), ``prosac_convergence`` and
    ``prosac_stop``.

    Returns ``(E, inliers)`` with E (3, 3), unit Frobenius norm and
    (K2^-1 x2)^T E (K1^-1 x1) = 0, or ``(None, inliers)``.
    """
    k1 = _as_calibration(K1, "K1")
    k2 = _as_calibration(K2, "K2")
    # the engine's own check of the matrices, before any GPU work
    N.check(N.lib.gcr_host_essential_normalise(None, 0, k1.ctypes.data, k2.ctypes.data, 0.0, None, None))

    def entry(ctx, f, n, p, mask, M, st):
        return N.lib.gcr_find_essential_matrix(ctx, f, n, k1.ctypes.data, k2.ctypes.data, None, p, mask, M, st)

    def guided_entry(ctx, f, n, w, p, mask, M, st):
        return N.lib.gcr_find_essential_matrix(ctx, f, n, k1.ctypes.data, k2.ctypes.data, w, p, mask, M, st)

    def create(ctx, rows, order, out):
        return N.lib.gcr_problem_create_essential(ctx, rows.ctypes.data, rows.shape[0], k1.ctypes.data,
                                                  k2.ctypes.data, out)

    return _correspondence_call(entry, guided_entry, correspondences, h1, w1, h2, w2, probabilities, threshold, conf,
                                spatial_coherence_weight, max_iters, min_iters, sampler, lo_number, seed, device,
                                batch_slots, return_stats, 5, neighborhood_size, guided_stop, create=create,
                                prosac_convergence=prosac_convergence,
                                prosac_stop=prosac_stop, napsac_iterations=napsac_iterations)


def _as_rotation(G, name):
    g = np.ascontiguousarray(np.asarray(G, dtype=np.float64))
    if g.shape != (3, 3):
        raise ValueError(f"{name} must be a 3 x 3 rotation matrix; it has shape {tuple(g.shape)}.")
    return g


def findGravityEssentialMatrix(correspondences, K1, K2, gravity_source, gravity_destination, h1, w1, h2, w2,
                               probabilities=None, threshold=1.0, conf=0.99, spatial_coherence_weight=0.975,
                               max_iters=10000, min_iters=50, sampler=0, lo_number=50, *, neighborhood_size=8, seed=0,
                               device=None, batch_slots=0, return_stats=False, guided_stop=False,
                               prosac_convergence=100000, prosac_stop=False, napsac_iterations=None):
    """3-point essential matrix with graph-cut LO for calibrated cameras whose
    gravity direction is known (a phone, a vehicle, any IMU rig) -- an
    EXTENSION like findEssentialMatrix (upstream pygcransac's
    findGravityEssentialMatrix order).  Upstream's solver is not part of this
    project and parity with it is unpinned: csrc/grav.h is the definition.

    Everything as findEssentialMatrix, plus ``gravity_source`` and
    ``gravity_destination``: 3 x 3 rotations G1, G2, Gi taking a direction in
    camera i to a frame whose y axis is the gravity direction (finite,
    orthonormal to 1e-9, determinant > 0).  In those frames the relative pose
    is a rotation about y and a translation, so a sample is three
    correspondences and yields up to four models; at 80 % outliers the stop
    needs about 570 iterations where the 5-point solver needs about 14 400.
    A half turn about the vertical between the aligned frames is outside the
    solver's parametrisation.  ``probabilities`` need at least 3 weights > 0
    (``sampler=3``; with ``sampler=1``, PROSAC, they are quality scores).

    Returns ``(E, inliers)`` with E (3, 3) in the ordinary K-normalised frames,
    findEssentialMatrix's convention: unit Frobenius norm and
    (K2^-1 x2)^T E (K1^-1 x1) = 0; or ``(None, inliers)``.
    """
    k1 = _as_calibration(K1, "K1")
    k2 = _as_calibration(K2, "K2")
    g1 = _as_rotation(gravity_source, "gravity_source")
    g2 = _as_rotation(gravity_destination, "gravity_destination")
    # the engine's own checks of the matrices, before any GPU work
    N.check(N.lib.gcr_host_essential_normalise(None, 0, k1.ctypes.data, k2.ctypes.data, 0.0, None, None))
    N.check(N.lib.gcr_host_check_gravity(g1.ctypes.data, g2.ctypes.data))

    def entry(ctx, f, n, p, mask, M, st):
        return N.lib.gcr_find_gravity_essential_matrix(ctx, f, n, k1.ctypes.data, k2.ctypes.data, g1.ctypes.data,
                                                       g2.ctypes.data, None, p, mask, M, st)

    def guided_entry(ctx, f, n, w, p, mask, M, st):
        return N.lib.gcr_find_gravity_essential_matrix(ctx, f, n, k1.ctypes.data, k2.ctypes.data, g1.ctypes.data,
                                                       g2.ctypes.data, w, p, mask, M, st)

    def create(ctx, rows, order, out):
        return N.lib.gcr_problem_create_gravity_essential(ctx, rows.ctypes.data, rows.shape[0], k1.ctypes.data,
                                                          k2.ctypes.data, g1.ctypes.data, g2.ctypes.data, out)

    return _correspondence_call(entry, guided_entry, correspondences, h1, w1, h2, w2, probabilities, threshold, conf,
                                spatial_coherence_weight, max_iters, min_iters, sampler, lo_number, seed, device,
                                batch_slots, return_stats, 3, neighborhood_size, guided_stop, create=create,
                                prosac_convergence=prosac_convergence,
                                prosac_stop=prosac_stop, napsac_iterations=napsac_iterations)


def findHomographySIFT(correspondences, h1, w1, h2, w2, probabilities=None, threshold=1.0, conf=0.99,
                       spatial_coherence_weight=0.975, max_iters=10000, min_iters=50, sampler=0, lo_number=50, *,
                       neighborhood_size=8, seed=0, device=None, batch_slots=0, return_stats=False,
                       guided_stop=False, prosac_convergence=100000, prosac_stop=False, napsac_iterations=None):
    """Homography from TWO SIFT correspondences with graph-cut LO -- an
    EXTENSION like findHomography (what upstream pygcransac's findHomography
    runs with its SIFT-based solver).  Upstream's solver is not part of this
    project and parity with it is unpinned: csrc/sifth.h is the definition.

    ``correspondences`` is (N, 8) float64: x1, y1, x2, y2 in pixels, the
    feature sizes q1, q2 as lengths (cv2's ``kp.size`` or any fixed multiple of
    it on both sides; finite, > 0) and the orientations alpha1, alpha2 in
    RADIANS (finite); ``features.py`` hands out both.  A correspondence of two
    oriented, scaled keypoints gives four constraints on H, so a sample is two
    correspondences and yields up to three models: the stop needs about 113
    iterations at 80 % outliers where findHomography needs about 2880.  A model
    from two noisy features covers few inliers (an orientation error grows
    with the distance from the sample), so the estimator rests on local
    optimisation; scoring, the threshold, LO's fits (the 4-point estimator's
    non-minimal fit), the neighbourhood grid and every other argument are
    findHomography's.  ``probabilities`` (``sampler=3``) need at least 2 weights
    > 0.  With ``sampler=1`` (PROSAC, as in findHomography) they are quality
    scores; the SIFT columns are sorted with their rows.

    Returns ``(H, inliers)`` with H (3, 3) and H[2, 2] = 1, or ``(None, inliers)``.
    """
    f8 = _as_features(correspondences)
    if f8.ndim != 2:
        raise ValueError("Number of dimensions must be 2.")
    n, cols = f8.shape
    if n < 4 or cols != 8:
        raise ValueError(f"Correspondences should be an array with 8 columns and at least 4 rows. "
                         f"It has {cols} columns and {n} rows.")
    sift = np.ascontiguousarray(f8[:, 4:8], dtype=np.float64)
    # the engine's own check of the SIFT columns, before any GPU work
    N.check(N.lib.gcr_host_check_sift(sift.ctypes.data, n))

    def entry(ctx, f, n, p, mask, M, st):
        return N.lib.gcr_find_homography_sift(ctx, f, sift.ctypes.data, n, None, p, mask, M, st)

    def guided_entry(ctx, f, n, w, p, mask, M, st):
        return N.lib.gcr_find_homography_sift(ctx, f, sift.ctypes.data, n, w, p, mask, M, st)

    def create(ctx, rows, order, out):
        cols = np.ascontiguousarray(sift[order])
        return N.lib.gcr_problem_create_sift_homography(ctx, rows.ctypes.data, cols.ctypes.data, rows.shape[0], out)

    return _correspondence_call(entry, guided_entry, np.ascontiguousarray(f8[:, :4]), h1, w1, h2, w2, probabilities,
                                threshold, conf, spatial_coherence_weight, max_iters, min_iters, sampler, lo_number,
                                seed, device, batch_slots, return_stats, 4, neighborhood_size, guided_stop,
                                min_weights=2, create=create, prosac_convergence=prosac_convergence,
                                prosac_stop=prosac_stop, napsac_iterations=napsac_iterations)


# ------------------------------------------------------ many small problems --
_MANY_KINDS = {"homography": (N.SOLVER_HOMOGRAPHY4, 4), "fundamental": (N.SOLVER_FUNDAMENTAL7, 7)}


def _per_problem(v, count, dtype, name):
    a = np.asarray(v)
    if a.ndim == 0:
        a = np.full(count, a[()])
    if a.shape != (count,):
        raise ValueError(f"{name} must be a scalar or one value per problem ({count}), got shape {a.shape}")
    if dtype is np.uint64:
        if not np.issubdtype(a.dtype, np.integer) or (a.size and int(a.min()) < 0):
            raise ValueError(f"{name} must be integers >= 0")
    return np.ascontiguousarray(a, dtype=dtype)


def verify_many(problems, kind, threshold, iterations=1024, *, seed=0, backend="gpu", device=None, refine=False):
    """The best RANSAC hypothesis of many small correspondence problems in ONE
    call (gcr_verify_many; csrc/verify_many.h is the definition): a fixed number
    of launches for all problems, one upload, one synchronisation, one download.

    ``problems`` is a sequence of (n_p, 4) float64 arrays of rows x1, y1, x2,
    y2, each with at least 4 (``kind="homography"``) or 7
    (``kind="fundamental"``) finite rows.  ``threshold`` (pixels, finite, > 0)
    and ``seed`` are a scalar or one value per problem.  ``iterations`` is the
    number of slots per problem, 1 .. 65536: every slot draws one uniform
    minimal sample (retried up to 101 times until it yields a model), every
    model is MSAC-scored against all of the problem's rows, and the first
    strict best wins -- exactly what ``gcr_problem_verify_batch`` computes for
    one resident problem.  No stop criterion, local optimisation or graph cut.

    Returns a list with one dict per problem: ``model`` (3 x 3, the winning
    hypothesis' own matrix, or ``None`` when no hypothesis scored above 0),
    ``mask`` (bool, n_p: the model's MSAC inliers), ``inliers`` (= mask.sum()),
    ``score``, ``slot`` (-1 without a model) and ``iterations`` (the sum of the
    slots' iteration increments).  ``refine=True`` adds ``refined``: the
    least-squares fit of the mask's rows (the estimators' non-minimal fit), or
    ``None`` if it rejects them or there are fewer rows than it needs.
    ``backend="host"`` runs the host twin without a GPU and returns the same
    bytes."""
    if kind not in _MANY_KINDS:
        raise ValueError(f"kind must be 'homography' or 'fundamental', got {kind!r}")
    if backend not in ("gpu", "host"):
        raise ValueError(f"backend must be 'gpu' or 'host', got {backend!r}")
    solver, m = _MANY_KINDS[kind]
    probs = []
    for k, q in enumerate(problems):
        a = np.ascontiguousarray(q, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError(f"problems[{k}] must have shape (n, 4): rows x1, y1, x2, y2; got {a.shape}")
        probs.append(a)
    P = len(probs)
    if P == 0:
        return []
    thr = _per_problem(threshold, P, np.float64, "threshold")
    seeds = _per_problem(seed, P, np.uint64, "seed")
    S = _as_size_t(iterations, "iterations")
    if not 1 <= S <= 65536:
        raise ValueError(f"iterations must be in 1 .. 65536, got {S}")
    off = np.zeros(P + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(a) for a in probs])
    rows = np.ascontiguousarray(np.concatenate(probs, axis=0))
    total = int(off[-1])
    out = (N.ManyResult * P)()
    masks = np.zeros(max(total, 1), dtype=np.uint8)
    if backend == "host":
        N.check(N.lib.gcr_host_verify_many(solver, rows.ctypes.data, off.ctypes.data, P, thr.ctypes.data,
                                           seeds.ctypes.data, S, 16, out, masks.ctypes.data))
    else:
        N.check(N.lib.gcr_verify_many(N.context(device), solver, rows.ctypes.data, off.ctypes.data, P,
                                      thr.ctypes.data, seeds.ctypes.data, S, out, masks.ctypes.data, None))
    rec = np.frombuffer(out, dtype=N.MANY_DT)
    fit = N.lib.gcr_host_fit_h if solver == N.SOLVER_HOMOGRAPHY4 else N.lib.gcr_host_fit_f
    res = []
    for p in range(P):
        r = rec[p]
        lo, hi = int(off[p]), int(off[p + 1])
        mask = masks[lo:hi].astype(bool)
        have = int(r["best_slot"]) >= 0
        d = {"model": r["best_model"].reshape(3, 3).copy() if have else None, "mask": mask,
             "inliers": int(r["best_inliers"]), "score": float(r["best_score"]), "slot": int(r["best_slot"]),
             "iterations": int(r["iterations"])}
        if refine:
            d["refined"] = None
            idx = np.ascontiguousarray(np.flatnonzero(mask), dtype=np.uint32)
            if have and len(idx) >= m:
                M = np.zeros(9)
                if N.check(fit(_dp(probs[p]), len(probs[p]), idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(idx),
                               _dp(M))) == 1:
                    d["refined"] = M.reshape(3, 3)
        res.append(d)
    return res


__all__.append("verify_many")
