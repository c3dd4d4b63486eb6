"""The inputs and the reference of the scorer edge tests (scorer_edge_cases.py;
the GPU side is test_gpu_scorer_edges.py), by the oracle alone: conditions, not
measurements, so that no GPU comparison there passes by being vacuous.

Regimes: every shape's 13 models must load the kernels as the regime's name
says (pairs within the threshold per model, before the finish zeroes a score
below the sample size -- what the survivor queues carry).

Reference: homography and fundamental-matrix residuals are rational functions
of the inputs, so the oracle's decisions and MSAC values are compared with
fractions.Fraction arithmetic on the same doubles.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import oracle_ffi as O
import scorer_edge_cases as E


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    O.lib()


def test_shapes_cover_the_tiling_constants():
    for kind in E.RECT_KINDS + E.CORR_KINDS:
        sizes = {n for sh in E.shapes(kind) for n in sh}
        for c in (64, 120, 256, 420, 896, 960):
            assert {c - 1, c, c + 1} <= sizes, (kind, c)
        assert {2 * 896 + 1, 2 * 960 + 1} <= sizes               # a third round's first feature
    assert {(961, 65), (65, 961), (2, 2), (896, 2), (2, 896)} <= set(E.shapes(2))
    assert (3, 0) in E.shapes(0) and (4, 0) in E.shapes(3) and (7, 0) in E.shapes(4) and (8, 0) in E.shapes(4)
    assert min(E.shapes(1)) == (63, 0)
    for h, nh in E.NH.items():
        assert nh % h != 0 and nh % E.NMODELS != 0               # a ragged last workgroup, no tiling period


@pytest.mark.parametrize("kind", E.RECT_KINDS + E.CORR_KINDS, ids=lambda k: E.KIND_NAME[k])
def test_models_are_distinct_and_tile_without_period(kind):
    for shape in E.shapes(kind):
        m = E.models(kind, shape)
        assert m.shape == (E.NMODELS, 7 if kind in E.RECT_KINDS else 9)
        assert np.isfinite(m).all()
        t = E.tile(kind, shape, 37)
        assert np.array_equal(t[13:26], m) and np.array_equal(t[26:], m[:11])
    # the slots of every shape above the sample size give generated models
    big = E.models(kind, E.shapes(kind)[-1])
    assert len({r.tobytes() for r in big}) == E.NMODELS


@pytest.mark.parametrize("kind", E.RECT_KINDS + E.CORR_KINDS, ids=lambda k: E.KIND_NAME[k])
def test_typical_regime_has_high_and_low_counts(kind):
    for shape in E.shapes(kind):
        n = shape[0] + shape[1]
        if n < 63:
            continue
        tot = E.raw_counts(kind, shape, "typical").sum(axis=1)
        assert (tot >= n / 4).sum() >= 3, (shape, tot.tolist())
        assert (tot < n / 8).sum() >= 3, (shape, tot.tolist())


@pytest.mark.parametrize("kind", E.RECT_KINDS + E.CORR_KINDS, ids=lambda k: E.KIND_NAME[k])
def test_full_regime_saturates_every_class(kind):
    for shape in E.shapes(kind):
        rc = E.raw_counts(kind, shape, "full")
        for c in range(len(E.SAMPLE[kind])):
            assert (rc[:, c] >= 0.9 * shape[c]).sum() >= 7, (shape, c, rc[:, c].tolist())


@pytest.mark.parametrize("kind", E.RECT_KINDS + E.CORR_KINDS, ids=lambda k: E.KIND_NAME[k])
def test_empty_regime_keeps_at_most_the_sample(kind):
    for shape in E.shapes(kind):
        rc = E.raw_counts(kind, shape, "empty")
        for c, m in enumerate(E.SAMPLE[kind]):
            # the original scale-only solver's models do not even keep their sample
            assert rc[:, c].max() <= (0 if kind == 1 else m), (shape, c, rc[:, c].tolist())
        if kind == 1:
            counts, _, value, _ = E.reference(kind, shape, "empty")
            assert not counts.any() and not value.any()


def test_finish_restates_the_oracle_score():
    # E.finish over the oracle's own inlier sums gives the oracle's finished score
    for kind, shape in ((0, (257, 0)), (2, (65, 961)), (2, (257, 2)), (3, (65, 0)), (4, (121, 0))):
        f0, f1, _ = E.problem(kind, shape)
        thr = E.thresholds(kind, shape, "typical")
        counts, values, value, allmasks = E.reference(kind, shape, "typical")
        for q, m in enumerate(E.models(kind, shape)):
            masks = allmasks[q]
            acc, tot = [0.0, 0.0], 0.0
            for c, f in enumerate((f0, f1)[:len(E.SAMPLE[kind])]):
                if kind in E.RECT_KINDS:
                    r2 = O.residuals(kind, c, f, m)
                else:
                    r2 = (O.h_residuals if kind == 3 else O.f_residuals)(f, m)
                for v in r2[masks[c]]:
                    acc[c] += -v
                    tot += -v
            got = E.finish(kind, masks[0].sum(), 0 if masks[1] is None else masks[1].sum(), acc[0], acc[1], tot, thr)
            assert got[0][0].tolist() == counts[q].tolist() and got[2][0] == value[q], (kind, shape, q)
            assert got[1][0].tolist() == values[q].tolist(), (kind, shape, q)


# ------------------------------------------------- exact rational reference --
EXACT_MODELS = 6
EXACT_MAX_N = 961


def _exact_r2(kind, row, m):
    x1, y1, x2, y2 = row
    if kind == 3:
        w = m[6] * x1 + m[7] * y1 + m[8]
        if w == 0:
            return None
        du = (m[0] * x1 + m[1] * y1 + m[2]) / w - x2
        dv = (m[3] * x1 + m[4] * y1 + m[5]) / w - y2
        return du * du + dv * dv
    a0 = m[0] * x1 + m[1] * y1 + m[2]
    a1 = m[3] * x1 + m[4] * y1 + m[5]
    a2 = m[6] * x1 + m[7] * y1 + m[8]
    b0 = m[0] * x2 + m[3] * y2 + m[6]
    b1 = m[1] * x2 + m[4] * y2 + m[7]
    num = x2 * a0 + y2 * a1 + a2
    den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1
    return None if den == 0 else num * num / den


@functools.lru_cache(maxsize=None)
def _exact_residuals(kind, shape):
    """Fraction r^2 of every pair under the shape's first EXACT_MODELS models."""
    corr = [[Fraction(float(v)) for v in row] for row in E.problem(kind, shape)[0]]
    out = []
    for m in E.models(kind, shape)[:EXACT_MODELS]:
        mf = [Fraction(float(v)) for v in m]
        out.append([_exact_r2(kind, row, mf) for row in corr])
    return out


def _exact_shapes(kind):
    return [sh for sh in E.shapes(kind) if sh[0] <= EXACT_MAX_N]


@pytest.mark.parametrize("kind", E.CORR_KINDS, ids=lambda k: E.KIND_NAME[k])
def test_oracle_decisions_match_exact_arithmetic(kind):
    """O.h_score / O.f_score inlier masks against exact r^2 <= T (T the
    double the oracle compares with).  A pair whose exact r^2 lies within
    1e-9 T of T is set aside, at most 1 % of the pairs; every other decision
    agrees."""
    pairs = aside = 0
    for shape in _exact_shapes(kind):
        ex = _exact_residuals(kind, shape)
        for regime in ("typical", "full"):
            T = Fraction(E.msac_T(E.thresholds(kind, shape, regime)[0]))
            band = T / 10**9
            ref = E.reference(kind, shape, regime)
            for q in range(EXACT_MODELS):
                mask = ref[3][q][0]
                for i, r2 in enumerate(ex[q]):
                    pairs += 1
                    if r2 is None or abs(r2 - T) <= band:
                        aside += 1
                        continue
                    assert bool(mask[i]) == (r2 <= T), (shape, regime, q, i, float(r2), float(T))
    print(f"{E.KIND_NAME[kind]}: {pairs} decisions, {aside} set aside")
    assert pairs == 2 * EXACT_MODELS * sum(sh[0] for sh in _exact_shapes(kind)) and aside <= pairs // 100


def _value_errors(kind):
    """max over the shapes of |oracle value - (k - sum r^2 / T)| / k, the
    oracle's own inlier set, exact arithmetic on the right."""
    worst = 0.0
    for shape in _exact_shapes(kind):
        ex = _exact_residuals(kind, shape)
        for regime in ("typical", "full"):
            T = Fraction(E.msac_T(E.thresholds(kind, shape, regime)[0]))
            ref = E.reference(kind, shape, regime)
            for q in range(EXACT_MODELS):
                value, masks = float(ref[2][q]), ref[3][q]
                k = int(ref[0][q][0])
                if k == 0:
                    continue
                assert k == int(masks[0].sum())
                # exact integers throughout, no reduction (a Fraction would take
                # a gcd of ever longer integers at every step): sum r^2 =
                # num / den, value = vn / vd, T = tn / td, and
                # value - (k - num td / (den tn)) over one denominator
                num, den = 0, 1
                for i in np.flatnonzero(masks[0]):
                    r2 = ex[q][i]
                    num, den = num * r2.denominator + r2.numerator * den, den * r2.denominator
                vn, vd = Fraction(value).as_integer_ratio()
                tn, td = T.as_integer_ratio()
                diff = vn * den * tn - vd * (k * den * tn - num * td)
                worst = max(worst, abs(diff) / (vd * den * tn * k))
    return worst


# measured over the shapes above (N <= 961, typical and full, 6 models each);
# the oracle's score has no libm call, so these are deterministic: the margin
# of 8 covers another host compiler's code for the same IEEE operations
VALUE_ERR_MEASURED = {3: 6.100e-15, 4: 5.397e-14}


@pytest.mark.parametrize("kind", E.CORR_KINDS, ids=lambda k: E.KIND_NAME[k])
def test_oracle_value_matches_exact_arithmetic(kind):
    """The oracle's MSAC value k - sum r^2 / T against exact arithmetic, as
    absolute error per inlier.  Measured worst case over the shapes (N <= 961,
    typical and full, 6 models a shape): 6.100e-15 for the homography,
    5.397e-14 for the fundamental matrix (VALUE_ERR_MEASURED); the bound is
    8 x that."""
    worst = _value_errors(kind)
    print(f"{E.KIND_NAME[kind]}: worst value error per inlier {worst:.3e}")
    assert worst <= 8.0 * VALUE_ERR_MEASURED[kind]
