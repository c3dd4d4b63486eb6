"""The live list of gcr_problem_verify_batches' bound path (k_bound_live and
k_bound in csrc/kernels.hip; run on an MI355X: pytest -m gpu).

k_bound counts the pre-band survivors only of the slots that can be selected:
those with a model and, for the 2-SIFT solver, a valid one.  k_bound_live
lists them per launch group and zeroes the bounds of every other slot;
GCR_VERIFY_BOUND_LIVE=0 lists every slot with a model (the earlier work).  The
records must not depend on the mode and must be the fused path's
(GCR_VERIFY_BOUND=0) field by field on bits.

Shapes.  A wave of k_bound owns 16 list entries, a workgroup 64, a workgroup
of k_bound_live 1024 slots:
  M2 (64, 64), (63, 65), (129, 128), (300, 200), (24, 24); M1 65 and
  M1-original 300 under GCR_VERIFY_BOUND=1 (no validity rule: every slot with
  a model is listed)
  16 slots x 4 batches (7 - 15 live slots a batch: one partial wave), 272 x 9
  (148 - 197 live; launch groups of 4, 4 and 1 batches, the last a single
  partial tile of k_bound_live), 1024 x 4 (606 - 719 live, four tiles of
  k_bound_live, each counting the tiles below it)
  M2 (2, 2): no slot has a model, the list is empty
  a second call at thresholds 1e-150 on the buffer sets the first call left
  M2 (9000, 9000): more pairs than the split scorer's tile holds
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_ffi as O
from gcr_testutil import Problem, bits
from pygcransac import _native as N
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

SEED = 20251121
SLOT0 = 7

SHAPES = {
    "m2_64_64": (N.SOLVER_SIFT22, 64, 64),
    "m2_63_65": (N.SOLVER_SIFT22, 63, 65),
    "m2_129_128": (N.SOLVER_SIFT22, 129, 128),
    "m2_300_200": (N.SOLVER_SIFT22, 300, 200),
    "m2_24_24": (N.SOLVER_SIFT22, 24, 24),
    "m2_2_2": (N.SOLVER_SIFT22, 2, 2),
    "m2_9000_9000": (N.SOLVER_SIFT22, 9000, 9000),
    "m1_65": (N.SOLVER_SCALE3, 65, 0),
    "m1orig_300": (N.SOLVER_SCALE3_ORIGINAL, 300, 0),
}
SWITCHES = ["GCR_VERIFY_GROUPS", "GCR_VERIFY_GROUPS_STAGE", "GCR_VERIFY_CHAIN", "GCR_VERIFY_OVERLAP",
            "GCR_VERIFY_DEFER", "GCR_VERIFY_PIPE", "GCR_FM_PRECONST", "GCR_SCORER", "GCR_PROBE"]
SIZES = [(16, 4), (272, 9), (1024, 4)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if N.lib.gcr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    N.context(0)
    O.lib()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES + ["GCR_VERIFY_BOUND", "GCR_VERIFY_BOUND_SEEDS", "GCR_VERIFY_BOUND_LIVE"]:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def _problem(shape):
    kind, ns, no = SHAPES[shape]
    if kind == N.SOLVER_SIFT22:
        fs, fo, _, _, ts, to = S.problem_m2(ns, no, seed=SEED)
        return kind, Problem(kind, fs, fo), ts, to
    f, _, thr = S.problem_m1(ns, seed=SEED)
    return kind, Problem(kind, f, None), thr, 0.0


def _params(thr0, thr1):
    p = N.default_params()
    p.scale_residual_thresh, p.orientation_residual_thresh, p.seed = thr0, thr1, SEED
    return p


def _fields(res):
    return [(r.models, r.iterations, r.best_slot, bits(r.best_score).item(), r.best_inliers[0], r.best_inliers[1],
             bits([r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
                   r.best_model.alpha, r.best_model.phi]).tolist()) for r in res]


def _records(prob, thr0, thr1, nslots, nb):
    p = _params(thr0, thr1)
    res = (N.BatchResult * nb)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, nb, res, None))
    return _fields(res)


def _walked(prob, thr0, thr1, nslots, nb):
    """slots a batch on k_bound's list in the default mode; raises unless the call takes the bound path"""
    p = _params(thr0, thr1)
    out = np.full(nb, 0xFFFFFFFF, dtype=np.uint32)
    N.check(N.lib.gcr_debug_verify_bound_live(prob.h, C.byref(p), SLOT0, nslots, nb,
                                              out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def _live(kind, prob, nslots, nb):
    """the slots that can be selected, per batch, from the generator's own output"""
    inc, models = prob.generate(SEED, SLOT0, nslots * nb)
    live = inc <= 101
    if kind == N.SOLVER_SIFT22:
        live &= np.maximum(np.abs(models[:, 3]), np.abs(models[:, 4])) < 1e-3          # valid_model_sift22
    return live.reshape(nb, nslots).sum(1)


def _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch):
    """the records of the default path, of the all-slots mode and of the fused path"""
    if kind != N.SOLVER_SIFT22:
        monkeypatch.setenv("GCR_VERIFY_BOUND", "1")      # the scale-only kinds take the bound path on request
    got = _records(prob, thr0, thr1, nslots, nb)
    walked = _walked(prob, thr0, thr1, nslots, nb)
    monkeypatch.setenv("GCR_VERIFY_BOUND_LIVE", "0")
    every = _records(prob, thr0, thr1, nslots, nb)
    monkeypatch.delenv("GCR_VERIFY_BOUND_LIVE")
    monkeypatch.setenv("GCR_VERIFY_BOUND", "0")
    ref = _records(prob, thr0, thr1, nslots, nb)
    monkeypatch.delenv("GCR_VERIFY_BOUND")
    assert len(ref) == nb
    for b in range(nb):
        assert got[b] == ref[b], ("default", b)
        assert every[b] == ref[b], ("all slots", b)
    return ref, walked


@pytest.mark.parametrize("nslots,nb", SIZES)
@pytest.mark.parametrize("shape", ["m2_64_64", "m2_63_65", "m2_129_128", "m2_300_200", "m2_24_24", "m1_65",
                                   "m1orig_300"])
def test_modes_agree(shape, nslots, nb, monkeypatch):
    kind, prob, thr0, thr1 = _problem(shape)
    ref, walked = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    live = _live(kind, prob, nslots, nb)
    print(shape, nslots, nb, "live", live.tolist(), "walked", walked.tolist())
    assert np.array_equal(walked, live)
    assert sum(o[0] for o in ref) > 0 and any(o[2] >= 0 for o in ref)
    if kind == N.SOLVER_SIFT22:
        assert (live % 16 != 0).any()                   # a partial wave of k_bound in a tested batch
        assert (live < nslots).all()                    # the list is shorter than the batch: dead slots exist


@pytest.mark.parametrize("nslots,nb", SIZES)
def test_empty_list(nslots, nb, monkeypatch):
    # 2 + 2 features: every sample is degenerate, no slot has a model
    kind, prob, thr0, thr1 = _problem("m2_2_2")
    inc, _ = prob.generate(SEED, SLOT0, nslots * nb)
    assert (inc > 101).all()
    ref, walked = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    assert all(o[2] == -1 for o in ref)
    assert (walked == 0).all()


@pytest.mark.parametrize("shape", ["m2_129_128", "m2_300_200"])
def test_nothing_survives_from_an_earlier_group(shape, monkeypatch):
    # 9 batches of 272 slots: three launch groups, the buffer sets are reused by
    # the next call, whose thresholds leave only a few slots candidates (the
    # sample's own features have twin residuals of exactly zero in some
    # slots).  A bound or a state kept from the first call would select or
    # score another slot.
    kind, prob, thr0, thr1 = _problem(shape)
    nslots, nb = 272, 9
    first, _ = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    assert all(o[2] >= 0 for o in first)
    second, walked = _legs(kind, prob, 1e-150, 1e-150, nslots, nb, monkeypatch)
    assert np.array_equal(walked, _live(kind, prob, nslots, nb))
    assert second != first
    # and back: the wide call after the narrow one
    again, _ = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    assert again == first


def test_contender_list_at_capacity(monkeypatch):
    # every feature is an inlier of every model and one seed: every other live
    # slot is a contender, 683 - 691 a batch
    kind, prob, _, _ = _problem("m2_300_200")
    monkeypatch.setenv("GCR_VERIFY_BOUND_SEEDS", "1")
    ref, walked = _legs(kind, prob, 50.0, 3.0, 1024, 4, monkeypatch)
    assert np.array_equal(walked, _live(kind, prob, 1024, 4))
    assert all(o[2] >= 0 for o in ref)


def test_more_pairs_than_the_split_scorer_holds(monkeypatch):
    kind, prob, thr0, thr1 = _problem("m2_9000_9000")
    ref, walked = _legs(kind, prob, thr0, thr1, 16, 4, monkeypatch)
    assert np.array_equal(walked, _live(kind, prob, 16, 4))
    assert any(o[2] >= 0 for o in ref)


def test_default_mode_matches_oracle_replay():
    # every record against the oracle's sampler, solver, twin-math MSAC score
    # and `best < score && isValidModel` in slot order
    kind, prob, thr0, thr1 = _problem("m2_300_200")
    nslots, nb = 1024, 5
    p = _params(thr0, thr1)
    res = (N.BatchResult * nb)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, nb, res, None))
    _walked(prob, thr0, thr1, nslots, nb)               # raises unless this configuration takes the bound path
    inc, models, counts, _, value = O.slots_scored(kind, prob.f0, prob.f1, SEED, SLOT0, nslots * nb, [(thr0, thr1)])
    for b in range(nb):
        best, bslot = 0.0, -1
        for j in range(b * nslots, (b + 1) * nslots):
            if inc[j] > 101:
                continue
            valid = max(abs(models[j][3]), abs(models[j][4])) < 1e-3
            if best < value[0][j] and valid:
                best, bslot = value[0][j], j
        r = res[b]
        sl = slice(b * nslots, (b + 1) * nslots)
        assert (r.models, r.iterations) == (int((inc[sl] <= 101).sum()), int(inc[sl].sum())), b
        assert bslot >= 0 and r.best_slot == SLOT0 + bslot, b
        assert bits(r.best_score) == bits(best), b
        assert [r.best_inliers[0], r.best_inliers[1]] == [int(c) for c in counts[0][bslot]], b
        got = [r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
               r.best_model.alpha, r.best_model.phi]
        assert np.array_equal(bits(got), bits(models[bslot])), b
