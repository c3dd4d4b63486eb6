"""The list scorer of gcr_problem_verify_batches' bound path (k_list_resid and
k_list_fold in csrc/kernels.hip; run on an MI355X: pytest -m gpu).

The seeds and the contenders of a batch are scored by the split scorer: one
thread a (model, feature) pair writes each 64-pair chunk's inlier values
compacted, one workgroup a model folds them in feature order.  It takes the
first GCR_VERIFY_BOUND_LISTCAP entries of a list (default and most 128), the
batch scorer k_score_split the entries after them; with 0, or with more pairs
than the fold holds, the batch scorer takes every entry.  The records must not
depend on which scorer scored an entry and must be the fused path's
(GCR_VERIFY_BOUND=0) field by field on bits.

Shapes.  A chunk is 64 pairs of one class, class 1's chunks start at class 0's
count rounded up to 64:
  M2 (64, 64), (63, 65), (129, 128): class 0 ends at, below and above a chunk
  boundary; (24, 24): one partial chunk a class
  16 slots x 4 batches (a list holds at most 16 entries), 272 x 9 (launch
  groups of 4, 4 and 1 batches), 1024 x 4
  M2 (300, 200), 1024 x 4, with the cap at 4 and 8 entries, also with one seed:
  the cap falls inside the lists, the batch scorer scores the rest
  M2 (300, 200) at thresholds 50.0 / 3.0: every feature an inlier of every
  model, full chunks, the contender list far past the default cap
  M2 (300, 200), 272 x 9: the wide call, the same buffer sets at thresholds
  1e-150 (chunks without an inlier), the wide call again
  M2 (2, 2): empty lists; M2 (9000, 9000): more pairs than the fold holds
  M1 65 and M1-original 300 under GCR_VERIFY_BOUND=1: the one-class kinds
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
LIST_CAP = 128              # kListCap (csrc/kernels.h)
FOLD_PAIRS = 16384          # kSplitMaxPairs

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
LO_KNOBS = ["GCR_LO_SPLIT", "GCR_LO_FOLD", "GCR_LO_FUSED", "GCR_LO_ARGMODELS", "GCR_LO_APPROX_FUSE", "GCR_LO_CPW"]
SIZES = [(16, 4), (272, 9), (1024, 4)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if N.lib.gcr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    N.context(0)
    O.lib()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES + LO_KNOBS + ["GCR_VERIFY_BOUND", "GCR_VERIFY_BOUND_SEEDS", "GCR_VERIFY_BOUND_LIVE",
                                    "GCR_VERIFY_BOUND_LISTCAP"]:
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


def _scored(prob, thr0, thr1, nslots, nb):
    """entries a batch on both lists together; raises unless the call takes the bound path"""
    p = _params(thr0, thr1)
    n = nslots * nb
    ub0, ub1 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    scored = np.full(nb, 0xFFFFFFFF, dtype=np.uint32)
    u32 = C.POINTER(C.c_uint32)
    N.check(N.lib.gcr_debug_verify_bound(prob.h, C.byref(p), SLOT0, nslots, nb, ub0.ctypes.data_as(u32),
                                         ub1.ctypes.data_as(u32), scored.ctypes.data_as(u32)))
    return scored


def _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch, listcap=None):
    """the records of the list scorer's path (the cap at `listcap` entries, None: the default), of the batch
    scorer's (GCR_VERIFY_BOUND_LISTCAP=0) and of the fused path; the entries a batch of the first leg"""
    if kind != N.SOLVER_SIFT22:
        monkeypatch.setenv("GCR_VERIFY_BOUND", "1")      # the scale-only kinds take the bound path on request
    if listcap is not None:
        monkeypatch.setenv("GCR_VERIFY_BOUND_LISTCAP", str(listcap))
    got = _records(prob, thr0, thr1, nslots, nb)
    scored = _scored(prob, thr0, thr1, nslots, nb)
    monkeypatch.setenv("GCR_VERIFY_BOUND_LISTCAP", "0")
    batch = _records(prob, thr0, thr1, nslots, nb)
    monkeypatch.delenv("GCR_VERIFY_BOUND_LISTCAP")
    monkeypatch.setenv("GCR_VERIFY_BOUND", "0")
    ref = _records(prob, thr0, thr1, nslots, nb)
    monkeypatch.delenv("GCR_VERIFY_BOUND")
    assert len(ref) == nb
    for b in range(nb):
        assert got[b] == ref[b], ("list scorer", b)
        assert batch[b] == ref[b], ("batch scorer", b)
    return ref, scored


@pytest.mark.parametrize("nslots,nb", SIZES)
@pytest.mark.parametrize("shape", ["m2_64_64", "m2_63_65", "m2_129_128", "m2_24_24"])
def test_chunk_boundaries(shape, nslots, nb, monkeypatch):
    kind, prob, thr0, thr1 = _problem(shape)
    ref, scored = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    print(shape, nslots, nb, "scored", scored.tolist())
    assert sum(o[0] for o in ref) > 0 and any(o[2] >= 0 for o in ref)
    assert (scored > 0).any()                            # the list scorer had entries to score
    if nslots <= LIST_CAP:
        assert (scored <= LIST_CAP).all()                # ... and every one of them: no list reaches the cap


@pytest.mark.parametrize("seeds", [None, 1])
@pytest.mark.parametrize("listcap", [4, 8])
def test_cap_inside_the_lists(listcap, seeds, monkeypatch):
    kind, prob, thr0, thr1 = _problem("m2_300_200")
    if seeds is not None:
        monkeypatch.setenv("GCR_VERIFY_BOUND_SEEDS", str(seeds))
    ref, scored = _legs(kind, prob, thr0, thr1, 1024, 4, monkeypatch, listcap=listcap)
    print("listcap", listcap, "seeds", seeds, "scored", scored.tolist())
    assert all(o[2] >= 0 for o in ref)
    assert (scored > listcap).all()                      # more entries than the list scorer takes of a list
    if seeds is None:
        # at least 64 seeds a batch (k_bound_seeds keeps the fewest bins that
        # hold them; 606 - 719 live slots): the seed list alone goes past the cap
        assert (scored >= 64).all()


def test_every_feature_an_inlier(monkeypatch):
    # full chunks, and every live slot outside the seeds is a contender: a
    # list far past the default cap
    kind, prob, _, _ = _problem("m2_300_200")
    ref, scored = _legs(kind, prob, 50.0, 3.0, 1024, 4, monkeypatch)
    print("scored", scored.tolist())
    print("best inliers", [(o[4], o[5]) for o in ref])
    assert all(o[2] >= 0 for o in ref)
    assert (scored > 2 * LIST_CAP).all()


def test_scratch_keeps_nothing_from_an_earlier_call(monkeypatch):
    # 9 batches of 272 slots: three launch groups on three buffer sets, which
    # the next call reuses at thresholds that leave chunks without an inlier
    # (only a sample's own features have twin residuals of exactly zero); a
    # chunk count or a value kept from the wide call would change a sum
    kind, prob, thr0, thr1 = _problem("m2_300_200")
    nslots, nb = 272, 9
    first, scored = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    assert all(o[2] >= 0 for o in first) and (scored > 0).all()
    second, scored = _legs(kind, prob, 1e-150, 1e-150, nslots, nb, monkeypatch)
    assert second != first
    again, _ = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    assert again == first


@pytest.mark.parametrize("nslots,nb", [(16, 4)])
def test_empty_lists(nslots, nb, monkeypatch):
    # 2 + 2 features: every sample is degenerate, no slot has a model
    kind, prob, thr0, thr1 = _problem("m2_2_2")
    ref, scored = _legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch)
    assert all(o[2] == -1 for o in ref)
    assert (scored == 0).all()


def test_more_pairs_than_the_fold_holds(monkeypatch):
    kind, prob, thr0, thr1 = _problem("m2_9000_9000")
    _, ns, no = SHAPES["m2_9000_9000"]
    assert (ns + 63) // 64 * 64 + (no + 63) // 64 * 64 > FOLD_PAIRS
    ref, scored = _legs(kind, prob, thr0, thr1, 16, 4, monkeypatch)
    assert any(o[2] >= 0 for o in ref) and (scored > 0).any()


@pytest.mark.parametrize("shape", ["m1_65", "m1orig_300"])
def test_one_class_kinds(shape, monkeypatch):
    kind, prob, thr0, thr1 = _problem(shape)
    ref, scored = _legs(kind, prob, thr0, thr1, 272, 9, monkeypatch)
    print(shape, "scored", scored.tolist())
    assert any(o[2] >= 0 for o in ref) and (scored > 0).all()


def test_default_matches_oracle_replay():
    # every record against the oracle's sampler, solver, twin-math MSAC score
    # and `best < score && isValidModel` in slot order
    kind, prob, thr0, thr1 = _problem("m2_300_200")
    nslots, nb = 1024, 5
    p = _params(thr0, thr1)
    res = (N.BatchResult * nb)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, nb, res, None))
    scored = _scored(prob, thr0, thr1, nslots, nb)      # raises unless this configuration takes the bound path
    assert (scored > 0).all()
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
