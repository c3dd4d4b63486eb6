"""Shared cases of the scorer conformance tests at feature-count edges
(test_scorer_edge_cases.py on the CPU, test_gpu_scorer_edges.py on the GPU).
CPU only: data from pygcransac.synthetic, models and references from the oracle.

The batch scorers tile features by fixed constants with a different code path
on each side of each: 64 (a wave, a small-scorer chunk), 120 / 420 / 960 (a
round of k_score_split at H = 64 / 16 / 4), 960 and 896 (a round of k_score_fm
without / with a generating wave), 256 (kMaskBlock) and 8192 (kLoBlock).  Every
class size here sits on one of them, one below or one above, below one wave,
or at the estimator's sample size m.

Kinds: 0 scale-only, 1 scale-only (original), 2 hybrid (two classes), 3
homography, 4 fundamental matrix -- the solver numbers of include/gcr.h.
A shape is (n0, n1), n1 = 0 for the one-class kinds.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_ffi as O
from pygcransac import synthetic as S

SEED = 20261020
OUTLIERS = 0.5
EDGES = (63, 64, 65, 119, 120, 121, 255, 256, 257, 419, 420, 421, 895, 896, 897, 959, 960, 961, 1793, 1921)
REGIMES = ("typical", "full", "empty")
NMODELS = 13                     # a prime: the tiling is coprime with H = 4, 16 and 64
NTRUTH = 4                       # of them the ground truth perturbed by 1e-4 (high counts)
NH = {4: 37, 16: 2061, 64: 16387}    # hypotheses per launch, by hypotheses per workgroup: a ragged last workgroup
RECT_KINDS = (0, 1, 2)
CORR_KINDS = (3, 4)
KIND_NAME = {0: "scale3", 1: "scale3orig", 2: "sift22", 3: "h4", 4: "f7"}
SAMPLE = {0: (3,), 1: (3,), 2: (2, 2), 3: (4,), 4: (7,)}


def shapes(kind):
    """Every (n0, n1) of `kind`."""
    if kind == 2:
        ns = (3,) + EDGES
        out = [(2, 2)]
        for n in ns:
            out += [(n, 2), (2, n), (n, n)]
        return out + [(961, 65), (65, 961)]
    m = SAMPLE[kind][0]
    # the original scale-only solver generates no scoring model from 3 or 4 features
    small = () if kind == 1 else (m, m + 1)
    return [(n, 0) for n in small + EDGES]


def small_limit_shapes(kind):
    """The small scorer's limits (kinds 0 and 2): padded pair totals on both
    sides of the split scorer's 2 x kLoBlock = 16384 pairs, and one kLoBlock
    = 8192 block edge."""
    if kind == 0:
        return [(n, 0) for n in (8191, 8192, 8193, 16384, 16385)]
    return [(8192, 8192), (8192, 8193), (8191, 65), (8193, 65)]


def mask_shapes(kind):
    """kMaskBlock = 256 and its neighbours, the smallest shape with a model, 65."""
    ns = (255, 256, 257, 65)
    return [minimal_shape(kind)] + [(n, n if kind == 2 else 0) for n in ns]


FUSED_N = (63, 64, 65, 895, 896, 897, 1793)       # k_score_fm<K, 16, true>: rounds of 896 features
IMBALANCE = [(64, 2), (2, 64), (896, 2), (2, 896), (897, 2), (2, 897), (961, 65), (65, 961)]


def fused_shapes(kind):
    """Shapes of the per-slot checks of the fused generate + score launch."""
    out = [minimal_shape(kind)] + [(n, n if kind == 2 else 0) for n in FUSED_N]
    out += IMBALANCE if kind == 2 else []
    return list(dict.fromkeys(out))


def chained_shapes(kind):
    """Shapes of the chained and grouped fused launches (records per batch)."""
    if kind == 2:
        return [(64, 64), (896, 896), (897, 897), (896, 2), (2, 896)]
    if kind in (0, 1):
        return [(n, 0) for n in (64, 896, 897)]
    return [(SAMPLE[kind][0] + 1, 0), (64, 0), (960, 0), (961, 0)]


def shape_id(shape):
    return f"{shape[0]}" if shape[1] == 0 else f"{shape[0]}x{shape[1]}"


@functools.lru_cache(maxsize=None)
def problem(kind, shape):
    """(f0, f1 or None, the generator's thresholds (thr0, thr1))."""
    n0, n1 = shape
    if kind == 2:
        fs, fo, _, _, ts, to = S.problem_m2(n0, n1, outlier_ratio=OUTLIERS, seed=SEED)
        out = fs, fo, (ts, to)
    elif kind in (0, 1):
        f, _, t = S.problem_m1(n0, outlier_ratio=OUTLIERS, seed=SEED)
        out = f, None, (t, 0.0)
    elif kind == 3:
        c, _, _, t = S.problem_h(n0, OUTLIERS, seed=SEED)
        out = c, None, (t, 0.0)
    else:
        c, _, _, t = S.problem_f(n0, OUTLIERS, seed=SEED)
        out = c, None, (t, 0.0)
    for a in out[:2]:
        if a is not None:
            a.setflags(write=False)
    return out


def thresholds(kind, shape, regime):
    """typical: the generator's own; full: nearly every pair an inlier;
    empty: at most the sample's own pairs."""
    if regime == "typical":
        return problem(kind, shape)[2]
    if kind in RECT_KINDS:
        t = (8.0, 0.75) if regime == "full" else (1e-7, 1e-9)
        return t if kind == 2 else (t[0], 0.0)
    return (1e4, 0.0) if regime == "full" else (1e-9, 0.0)


def _truth(kind):
    gt = S.GroundTruth()
    if kind in RECT_KINDS:
        # s = (t / alpha)^3: alpha^3 s / t^3 = 1, the original solver's s / (alpha^3 t^3) = 1 at 1 / alpha
        alpha = 1.0 / gt.alpha if kind == 1 else gt.alpha
        return np.array([gt.h7, gt.h8, alpha, gt.phi])
    if kind == 3:
        return (S.H_GT / S.H_GT[2, 2]).ravel()
    return S.two_view_geometry()[3].ravel()


def _slot_models(kind, f0, f1, want):
    out = []
    for s in range(512):
        if len(out) >= want:
            break
        if kind in RECT_KINDS:
            inc, m = O.slot(kind, f0, f1, SEED, s)
            if inc <= 101:
                out.append(m)
        elif kind == 3:
            inc, m = O.h_slot(f0, SEED, s)
            if inc <= 101:
                out.append(m)
        else:
            _, ms = O.f_slot(f0, SEED, s)
            out += list(ms)
    return out[:want]


@functools.lru_cache(maxsize=None)
def models(kind, shape):
    """NMODELS models, (13, 7) or (13, 9): NTRUTH times the ground truth with
    every parameter perturbed by a relative 1e-4 (high counts), the rest from
    the oracle's minimal solver on slots 0, 1, ... (counts near m; where the
    shape yields fewer, more perturbed truths fill up)."""
    f0, f1, _ = problem(kind, shape)
    gen = _slot_models(kind, f0, f1, NMODELS - NTRUTH)
    rng = np.random.default_rng([SEED, kind, shape[0], shape[1]])
    gt = _truth(kind)
    out = []
    for _ in range(NMODELS - len(gen)):
        p = gt * (1.0 + 1e-4 * rng.standard_normal(gt.shape))
        if kind in RECT_KINDS:
            out.append(np.array([0.0, 0.0, 1.0, p[0], p[1], p[2], p[3]]))
        elif kind == 3:
            out.append(p / p[8])
        else:
            out.append(p)
    a = np.array(out + gen, dtype=np.float64)
    a.setflags(write=False)
    return a


def tile(kind, shape, nh):
    return np.resize(models(kind, shape), (nh, models(kind, shape).shape[1]))


def finish(kind, n0, n1, v0, v1, tot, thr):
    """MSACScoringFunction::getScore's finish (MSAC_scoring_function.hpp:
    108-127) of arrays of raw accumulators, one IEEE operation per step as the
    reference takes them: counts (n, 2), per-class values (n, 2), value (n,).
    A score with a class below its sample size is all zeros."""
    T = [msac_T(t) for t in thr]
    n = [np.atleast_1d(np.asarray(a)).astype(np.int64) for a in (n0, n1)]
    v = [np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (v0, v1)]
    s = np.atleast_1d(np.asarray(tot, dtype=np.float64)).copy()
    K = len(SAMPLE[kind])
    ok = np.ones(s.shape, dtype=bool)
    nv = [np.zeros_like(s), np.zeros_like(s)]
    for c in range(K):
        ok &= n[c] >= SAMPLE[kind][c]
        nv[c] = v[c] / T[c] + n[c].astype(np.float64)
        s = s - v[c]
        s = s + nv[c]
    counts = np.stack([np.where(ok, n[0], 0), np.where(ok, n[1], 0) if K == 2 else np.zeros_like(n[0])], axis=1)
    values = np.stack([np.where(ok, nv[0], 0.0), np.where(ok, nv[1], 0.0)], axis=1)
    return counts, values, np.where(ok, s, 0.0)


@functools.lru_cache(maxsize=None)
def reference(kind, shape, regime):
    """The oracle's score of every model of the shape, computed once and
    shared: counts (13, 2), per-class values (13, 2; the correspondence
    kinds have one class: the value), value (13,), masks (a tuple of (m0, m1
    or None) per model: pairs within the threshold, before the finish)."""
    f0, f1, _ = problem(kind, shape)
    thr = thresholds(kind, shape, regime)
    counts, values, value, masks = [], [], [], []
    for m in models(kind, shape):
        if kind in RECT_KINDS:
            r = O.score(kind, f0, f1, m, thr[0], thr[1], want_masks=True)
            counts.append([int(c) for c in r["counts"]])
            values.append([float(x) for x in r["values"]])
            value.append(r["value"])
            masks.append(r["masks"])
        else:
            r = (O.h_score if kind == 3 else O.f_score)(f0, m, thr[0], want_mask=True)
            counts.append([r["count"] if r["count"] >= SAMPLE[kind][0] else 0, 0])
            values.append([r["value"], 0.0])
            value.append(r["value"])
            masks.append((r["mask"], None))
    out = (np.array(counts, dtype=np.int64), np.array(values), np.array(value), tuple(masks))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def raw_counts(kind, shape, regime):
    """(13, 2) pairs within the threshold per model and class, before the
    finish zeroes a score below the sample size: what the kernels' survivor
    queues carry."""
    return np.array([[int(mk[0].sum()), 0 if mk[1] is None else int(mk[1].sum())]
                     for mk in reference(kind, shape, regime)[3]])


def minimal_shape(kind):
    """The smallest shape of `kind` whose slots yield a model."""
    for shape in shapes(kind):
        f0, f1, _ = problem(kind, shape)
        if _slot_models(kind, f0, f1, 1):
            return shape
    raise AssertionError("no shape yields a model")


def msac_T(thr):
    return (2.25 * thr) * thr


def lo_T(thr):
    t = 1.5 * thr
    return t * t
