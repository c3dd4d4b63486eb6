"""The shortened launch chain of gcr_problem_verify_batches' bound path
(csrc/kernels.hip; run on an MI355X: pytest -m gpu).

k_list_fold scores a list's entries past the list scorer's cap itself: the
workgroup of entry j goes on with the entries j + cap, j + 2 cap, ..., computes
their chunks into its own scratch row and folds that row again.
GCR_VERIFY_BOUND_OVER=split gives those entries to the batch scorer in a launch
of their own, GCR_VERIFY_BOUND_LISTCAP=0 every entry.  k_bound deals the feature
rounds of 16 list entries to several waves and adds their counts;
GCR_VERIFY_BOUND_FSPLIT=0 lets one wave walk every feature.  None of this may
change a bound or a record: the legs are compared with one another and with the
fused path (GCR_VERIFY_BOUND=0) field by field on bits.

Shapes.  A chunk is 64 pairs of one class, a feature round of k_bound 64
features of one class:
  M2 (300, 200), 1024 slots x 4 batches, the cap at 4, 8 and 12 entries, also
  with one seed: the rows loop different numbers of times (with the default 64
  seeds both lists can pass the cap, with one seed the contenders' list does)
  M2 (300, 200), 272 x 9 (launch groups of 4, 4 and 1) at cap 8 on the same
  buffer sets at thresholds 50.0 / 3.0 (every chunk full), 1e-150 (no chunk
  has an inlier), 50.0 / 3.0 again: a reused scratch row keeps nothing
  M2 (63, 65), (24, 24), cap 4: the class boundary inside a chunk, one partial
  chunk a class
  M1 65 and M1-original 300 under GCR_VERIFY_BOUND=1: most slots contenders;
  M1 65 also with the cap at 8, since at the default cap none of its lists is
  shown to pass it (111 - 148 entries on both lists together)
  M2 (64, 64), 16 x 4: no list reaches the cap, the loop body never runs
  k_bound: (2, 2) no slot has a model, the live list is empty; (64, 64) one
  round a class, so all waves of an entry group but the first get no feature;
  (65, 63), (255, 257), (256, 256), (257, 255) round counts around a multiple of
  the waves, (300, 200), (1000, 3) one class far below a round, the one-class
  kinds; 16 x 4 (a partial entry group), 272 x 9, 1024 x 4

The debug hook's `scored` is a batch's entries on both lists together.  More
than 2 cap of them means that one list at least holds more than cap, which is
what the overflow cases assert; at most cap means that neither does.
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

SWITCHES = ["GCR_VERIFY_GROUPS", "GCR_VERIFY_GROUPS_STAGE", "GCR_VERIFY_CHAIN", "GCR_VERIFY_OVERLAP",
            "GCR_VERIFY_DEFER", "GCR_VERIFY_PIPE", "GCR_FM_PRECONST", "GCR_SCORER", "GCR_PROBE"]
LO_KNOBS = ["GCR_LO_SPLIT", "GCR_LO_FOLD", "GCR_LO_FUSED", "GCR_LO_ARGMODELS", "GCR_LO_APPROX_FUSE", "GCR_LO_CPW"]
BOUND = ["GCR_VERIFY_BOUND", "GCR_VERIFY_BOUND_SEEDS", "GCR_VERIFY_BOUND_LIVE", "GCR_VERIFY_BOUND_LISTCAP",
         "GCR_VERIFY_BOUND_OVER", "GCR_VERIFY_BOUND_FSPLIT"]
SIZES = [(16, 4), (272, 9), (1024, 4)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if N.lib.gcr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    N.context(0)
    O.lib()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES + LO_KNOBS + BOUND:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def _problem(kind, ns, no):
    if kind == N.SOLVER_SIFT22:
        fs, fo, _, _, ts, to = S.problem_m2(ns, no, seed=SEED)
        return Problem(kind, fs, fo), ts, to
    f, _, thr = S.problem_m1(ns, seed=SEED)
    return Problem(kind, f, None), thr, 0.0


def _params(thr0, thr1):
    p = N.default_params()
    p.scale_residual_thresh, p.orientation_residual_thresh, p.seed = thr0, thr1, SEED
    return p


def _records(prob, thr0, thr1, nslots, nb):
    p = _params(thr0, thr1)
    res = (N.BatchResult * nb)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, nb, res, None))
    return [(r.models, r.iterations, r.best_slot, bits(r.best_score).item(), r.best_inliers[0], r.best_inliers[1],
             bits([r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
                   r.best_model.alpha, r.best_model.phi]).tolist()) for r in res]


def _bounds(prob, thr0, thr1, nslots, nb):
    """every slot's ub0 / ub1 and the entries a batch on both lists together; raises unless the call takes
    the bound path"""
    p = _params(thr0, thr1)
    n = nslots * nb
    ub0, ub1 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    scored = np.full(nb, 0xFFFFFFFF, dtype=np.uint32)
    u32 = C.POINTER(C.c_uint32)
    N.check(N.lib.gcr_debug_verify_bound(prob.h, C.byref(p), SLOT0, nslots, nb, ub0.ctypes.data_as(u32),
                                         ub1.ctypes.data_as(u32), scored.ctypes.data_as(u32)))
    return ub0, ub1, scored


def _with(monkeypatch, env, fn):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return fn()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _over_legs(kind, prob, thr0, thr1, nslots, nb, monkeypatch, cap=None, seeds=None):
    """the records of the default, of GCR_VERIFY_BOUND_OVER=split, of GCR_VERIFY_BOUND_LISTCAP=0 and of the fused
    path, compared on bits; returns the fused path's and the entries a batch of the default leg"""
    base = {}
    if kind != N.SOLVER_SIFT22:
        base["GCR_VERIFY_BOUND"] = "1"                   # the scale-only kinds take the bound path on request
    if seeds is not None:
        base["GCR_VERIFY_BOUND_SEEDS"] = str(seeds)
    capped = dict(base)
    if cap is not None:
        capped["GCR_VERIFY_BOUND_LISTCAP"] = str(cap)
    rec = lambda: _records(prob, thr0, thr1, nslots, nb)
    got = _with(monkeypatch, capped, rec)
    scored = _with(monkeypatch, capped, lambda: _bounds(prob, thr0, thr1, nslots, nb)[2])
    split = _with(monkeypatch, {**capped, "GCR_VERIFY_BOUND_OVER": "split"}, rec)
    batch = _with(monkeypatch, {**base, "GCR_VERIFY_BOUND_LISTCAP": "0"}, rec)
    ref = _with(monkeypatch, {"GCR_VERIFY_BOUND": "0"}, rec)
    assert len(ref) == nb
    for b in range(nb):
        assert got[b] == ref[b], ("default", b)
        assert split[b] == ref[b], ("OVER=split", b)
        assert batch[b] == ref[b], ("LISTCAP=0", b)
    return ref, scored


@pytest.mark.parametrize("seeds", [None, 1])
@pytest.mark.parametrize("cap", [4, 8, 12])
def test_rows_loop_over_the_entries_past_the_cap(cap, seeds, monkeypatch):
    prob, thr0, thr1 = _problem(N.SOLVER_SIFT22, 300, 200)
    ref, scored = _over_legs(N.SOLVER_SIFT22, prob, thr0, thr1, 1024, 4, monkeypatch, cap=cap, seeds=seeds)
    print("cap", cap, "seeds", seeds, "scored", scored.tolist())
    assert all(o[2] >= 0 for o in ref)
    assert (scored > 2 * cap).any()                      # a batch with a list longer than the cap


def test_reused_scratch_row_keeps_nothing(monkeypatch):
    # a row is rewritten for every entry it scores and by the next call: full
    # chunks, then chunks without an inlier (only a sample's own features have
    # twin residuals of exactly zero), then full chunks again
    prob, _, _ = _problem(N.SOLVER_SIFT22, 300, 200)
    nslots, nb, cap = 272, 9, 8
    first, scored = _over_legs(N.SOLVER_SIFT22, prob, 50.0, 3.0, nslots, nb, monkeypatch, cap=cap)
    print("full chunks: scored", scored.tolist())
    assert all(o[2] >= 0 for o in first) and (scored > 2 * cap).any()
    second, scored = _over_legs(N.SOLVER_SIFT22, prob, 1e-150, 1e-150, nslots, nb, monkeypatch, cap=cap)
    print("no inliers: scored", scored.tolist())
    assert second != first and (scored > 2 * cap).any()
    again, _ = _over_legs(N.SOLVER_SIFT22, prob, 50.0, 3.0, nslots, nb, monkeypatch, cap=cap)
    assert again == first


@pytest.mark.parametrize("ns,no", [(63, 65), (24, 24)])
def test_chunk_boundaries_past_the_cap(ns, no, monkeypatch):
    prob, thr0, thr1 = _problem(N.SOLVER_SIFT22, ns, no)
    ref, scored = _over_legs(N.SOLVER_SIFT22, prob, thr0, thr1, 1024, 4, monkeypatch, cap=4)
    print(ns, no, "scored", scored.tolist())
    assert any(o[2] >= 0 for o in ref)
    assert (scored > 2 * 4).any()


@pytest.mark.parametrize("kind,n,cap", [(N.SOLVER_SCALE3, 65, None), (N.SOLVER_SCALE3, 65, 8),
                                        (N.SOLVER_SCALE3_ORIGINAL, 300, None)])
def test_one_class_kinds_past_the_cap(kind, n, cap, monkeypatch):
    prob, thr0, thr1 = _problem(kind, n, 0)
    ref, scored = _over_legs(kind, prob, thr0, thr1, 1024, 4, monkeypatch, cap=cap)
    print(kind, n, cap, "scored", scored.tolist())
    assert any(o[2] >= 0 for o in ref)
    assert (scored > (LIST_CAP if cap is None else cap)).any()       # more entries than the cap ...
    if (kind, cap) != (N.SOLVER_SCALE3, None):
        # ... and on one list alone; M1 65 at the default cap has too few live slots for that
        assert (scored > 2 * (LIST_CAP if cap is None else cap)).any()


def test_no_entry_past_the_cap(monkeypatch):
    prob, thr0, thr1 = _problem(N.SOLVER_SIFT22, 64, 64)
    ref, scored = _over_legs(N.SOLVER_SIFT22, prob, thr0, thr1, 16, 4, monkeypatch)
    print("scored", scored.tolist())
    assert any(o[2] >= 0 for o in ref)
    assert (scored <= LIST_CAP).all()                    # the loop body never runs


FSPLIT_SHAPES = [(N.SOLVER_SIFT22, 2, 2), (N.SOLVER_SIFT22, 64, 64), (N.SOLVER_SIFT22, 65, 63),
                 (N.SOLVER_SIFT22, 255, 257), (N.SOLVER_SIFT22, 256, 256), (N.SOLVER_SIFT22, 257, 255),
                 (N.SOLVER_SIFT22, 300, 200), (N.SOLVER_SIFT22, 1000, 3), (N.SOLVER_SCALE3, 65, 0),
                 (N.SOLVER_SCALE3_ORIGINAL, 300, 0)]


@pytest.mark.parametrize("nslots,nb", SIZES)
@pytest.mark.parametrize("kind,ns,no", FSPLIT_SHAPES)
def test_feature_split_counts_and_records(kind, ns, no, nslots, nb, monkeypatch):
    prob, thr0, thr1 = _problem(kind, ns, no)
    base = {} if kind == N.SOLVER_SIFT22 else {"GCR_VERIFY_BOUND": "1"}
    one = {**base, "GCR_VERIFY_BOUND_FSPLIT": "0"}
    ub0, ub1, scored = _with(monkeypatch, base, lambda: _bounds(prob, thr0, thr1, nslots, nb))
    vb0, vb1, vscored = _with(monkeypatch, one, lambda: _bounds(prob, thr0, thr1, nslots, nb))
    assert np.array_equal(ub0, vb0) and np.array_equal(ub1, vb1)
    assert np.array_equal(scored, vscored)
    rec = lambda: _records(prob, thr0, thr1, nslots, nb)
    got = _with(monkeypatch, base, rec)
    single = _with(monkeypatch, one, rec)
    ref = _with(monkeypatch, {"GCR_VERIFY_BOUND": "0"}, rec)
    assert got == ref and single == ref
    if (ns, no) == (2, 2):
        assert all(o[2] == -1 for o in ref) and not ub0.any() and not ub1.any()    # no slot has a model
    else:
        assert any(o[2] >= 0 for o in ref)
        assert ub0.any() and (kind != N.SOLVER_SIFT22 or ub1.any())
        assert int(ub0.max()) <= ns and int(ub1.max()) <= no
