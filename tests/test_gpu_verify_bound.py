"""The bound path of gcr_problem_verify_batches (csrc/bound.h, k_bound and the
seed / contender lists in csrc/kernels.hip; run on an MI355X: pytest -m gpu).

Every slot's pre-band survivor counts bound its finished score, so only the
slots whose bound can reach the best exactly scored seed are scored exactly.
The records must be those of the fused path (GCR_VERIFY_BOUND=0) field by
field: models, iterations, best slot, score bits, both inlier counts, model
bits.  2-SIFT calls take the bound path by default; the scale-only kinds do
with GCR_VERIFY_BOUND=1 (their bound does not pay at the bench's shape, so
they default to the fused path) and are compared under that setting.

Shapes.  k_bound's round is 64 features of one class (one a lane):
  M2 (64, 64), (63, 65), (129, 128), (2, 2); M1 / M1-original at 64, 65, 3
  (a problem cannot hold fewer features of a class than its minimal sample,
  2 + 2 and 3: gcr_problem_create refuses n = 1, so these are the smallest)
  slots 16, 272 (a partial last workgroup of k_bound's 64 and the scorer's 4),
  1024; batches 4, 9 (no multiple of the 8-batch launch group) and 70 batches
  of 16 slots (crosses the 64-batch selection ring)
  M2 (24, 24) at 512 slots: many slots share a bound and scores tie
  GCR_VERIFY_BOUND_SEEDS=1: the second list does the work
  thresholds 1e-150: no slot is a candidate, S = 0, every live slot is scored
  thresholds so wide that every feature is an inlier of every model: all
  bounds tie at the top, the contender list holds every slot but the seeds
One case is replayed through the oracle; the hook's bounds are checked against
gcr_debug_verify_slots' counts, and its scored counts against half the slots.
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
    "m2_2_2": (N.SOLVER_SIFT22, 2, 2),
    "m2_24_24": (N.SOLVER_SIFT22, 24, 24),
    "m2_300_200": (N.SOLVER_SIFT22, 300, 200),
    "m2_500_500": (N.SOLVER_SIFT22, 500, 500),
    "m1_64": (N.SOLVER_SCALE3, 64, 0),
    "m1_65": (N.SOLVER_SCALE3, 65, 0),
    "m1_3": (N.SOLVER_SCALE3, 3, 0),
    "m1orig_65": (N.SOLVER_SCALE3_ORIGINAL, 65, 0),
    "m1orig_300": (N.SOLVER_SCALE3_ORIGINAL, 300, 0),
}
# the fused path's A/B switches: one set in the environment pins the fused kernel
SWITCHES = ["GCR_VERIFY_GROUPS", "GCR_VERIFY_GROUPS_STAGE", "GCR_VERIFY_CHAIN", "GCR_VERIFY_OVERLAP",
            "GCR_VERIFY_DEFER", "GCR_VERIFY_PIPE", "GCR_FM_PRECONST", "GCR_SCORER", "GCR_PROBE"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if N.lib.gcr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    N.context(0)
    O.lib()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES + ["GCR_VERIFY_BOUND", "GCR_VERIFY_BOUND_SEEDS"]:
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


def _records(prob, thr0, thr1, nslots, nb):
    p = _params(thr0, thr1)
    res = (N.BatchResult * nb)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, nb, res, None))
    return res


def _fields(res):
    return [(r.models, r.iterations, r.best_slot, bits(r.best_score).item(), r.best_inliers[0], r.best_inliers[1],
             bits([r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
                   r.best_model.alpha, r.best_model.phi]).tolist()) for r in res]


def _bound_hook(prob, thr0, thr1, nslots, nb):
    p = _params(thr0, thr1)
    ub0 = np.zeros(nb * nslots, dtype=np.uint32)
    ub1 = np.zeros(nb * nslots, dtype=np.uint32)
    scored = np.zeros(nb, dtype=np.uint32)
    u32 = C.POINTER(C.c_uint32)
    N.check(N.lib.gcr_debug_verify_bound(prob.h, C.byref(p), SLOT0, nslots, nb, ub0.ctypes.data_as(u32),
                                         ub1.ctypes.data_as(u32), scored.ctypes.data_as(u32)))
    return ub0, ub1, scored


def _take_bound_path(prob, monkeypatch):
    """2-SIFT calls take the bound path by default; the scale-only kinds stay
    on the fused path (their bound is too weak to pay) unless GCR_VERIFY_BOUND=1"""
    if prob.kind != N.SOLVER_SIFT22:
        monkeypatch.setenv("GCR_VERIFY_BOUND", "1")


def _both(prob, thr0, thr1, nslots, nb, monkeypatch, seeds=None):
    """records of the bound path and of the fused path; the hook proves the
    first call's configuration takes the bound path"""
    if seeds is not None:
        monkeypatch.setenv("GCR_VERIFY_BOUND_SEEDS", str(seeds))
    _take_bound_path(prob, monkeypatch)
    got = _fields(_records(prob, thr0, thr1, nslots, nb))
    _, _, scored = _bound_hook(prob, thr0, thr1, nslots, nb)
    monkeypatch.setenv("GCR_VERIFY_BOUND", "0")
    ref = _fields(_records(prob, thr0, thr1, nslots, nb))
    monkeypatch.delenv("GCR_VERIFY_BOUND")
    _take_bound_path(prob, monkeypatch)
    assert len(ref) == nb
    for b in range(nb):
        assert got[b] == ref[b], b
    return ref, scored


@pytest.mark.parametrize("nslots,nb", [(16, 4), (272, 9), (1024, 4), (16, 70)])
@pytest.mark.parametrize("shape", ["m2_64_64", "m2_63_65", "m2_129_128", "m2_2_2", "m1_64", "m1_65", "m1_3",
                                   "m1orig_65"])
def test_bound_path_equals_fused_path(shape, nslots, nb, monkeypatch):
    _, prob, thr0, thr1 = _problem(shape)
    ref, _ = _both(prob, thr0, thr1, nslots, nb, monkeypatch)
    if shape not in ("m2_2_2", "m1_3"):
        assert sum(o[0] for o in ref) > 0 and any(o[2] >= 0 for o in ref)     # models generated, a best found


@pytest.mark.parametrize("shape,nslots,nb", [("m2_300_200", 1024, 9), ("m1orig_300", 1024, 9), ("m2_500_500", 272, 4)])
def test_bound_path_equals_fused_path_several_rounds(shape, nslots, nb, monkeypatch):
    _, prob, thr0, thr1 = _problem(shape)
    ref, _ = _both(prob, thr0, thr1, nslots, nb, monkeypatch)
    assert all(o[2] >= 0 for o in ref)


def test_tied_bounds_and_scores(monkeypatch):
    # 24 + 24 features: bounds from a handful of values, equal scores among
    # the slots; the lowest slot must win as in the fused path
    _, prob, thr0, thr1 = _problem("m2_24_24")
    ref, _ = _both(prob, thr0, thr1, 512, 9, monkeypatch)
    assert all(o[2] >= 0 for o in ref)


@pytest.mark.parametrize("shape", ["m2_300_200", "m2_24_24", "m1orig_300"])
def test_one_seed_leaves_the_work_to_the_contenders(shape, monkeypatch):
    _, prob, thr0, thr1 = _problem(shape)
    _, scored = _both(prob, thr0, thr1, 1024, 4, monkeypatch, seeds=1)
    assert (scored > 16).all()          # more than the seed list holds: the second list was used


@pytest.mark.parametrize("shape", ["m1orig_300"])
def test_no_candidate_scores_every_live_slot(shape, monkeypatch):
    # thresholds so small that no slot reaches its minimal counts: S = 0,
    # every live slot is a contender, no best.  (Scale-only: the 2-SIFT
    # solver's four sample features have twin residuals of exactly zero in
    # some slots, which are candidates at any threshold.)
    kind, prob, _, _ = _problem(shape)
    nslots, nb = 1024, 4
    t1 = 1e-150 if kind == N.SOLVER_SIFT22 else 0.0
    ref, scored = _both(prob, 1e-150, t1, nslots, nb, monkeypatch)
    assert all(o[2] == -1 for o in ref)
    ub0, ub1, _ = _bound_hook(prob, 1e-150, t1, nslots, nb)
    m0 = 2 if kind == N.SOLVER_SIFT22 else 3
    live = (ub0 >= m0) & ((ub1 >= 2) if kind == N.SOLVER_SIFT22 else True)
    if kind == N.SOLVER_SIFT22:
        inc, models = prob.generate(SEED, SLOT0, nslots * nb)
        live &= (inc <= 101) & (np.maximum(np.abs(models[:, 3]), np.abs(models[:, 4])) < 1e-3)
    assert np.array_equal(scored, live.reshape(nb, nslots).sum(1))


def test_contender_list_at_capacity(monkeypatch):
    # thresholds so wide that every feature is an inlier of every model: every
    # bound is n0 + n1, the seeds are the first slots of the top bin and every
    # other live slot is a contender (the list's largest fill)
    _, prob, _, _ = _problem("m2_300_200")
    nslots, nb = 1024, 4
    ref, scored = _both(prob, 50.0, 3.0, nslots, nb, monkeypatch, seeds=1)
    ub0, ub1, _ = _bound_hook(prob, 50.0, 3.0, nslots, nb)
    inc, models = prob.generate(SEED, SLOT0, nslots * nb)
    live = (inc <= 101) & (np.maximum(np.abs(models[:, 3]), np.abs(models[:, 4])) < 1e-3)
    assert np.array_equal(ub0[live], np.full(int(live.sum()), 300)) and np.array_equal(ub1[live], np.full(int(live.sum()), 200))
    assert np.array_equal(scored, live.reshape(nb, nslots).sum(1))
    assert (scored > nslots // 2).all()


@pytest.mark.parametrize("shape,env,taken", [("m2_64_64", None, True), ("m2_64_64", "0", False),
                                             ("m2_64_64", "GROUPS", False), ("m1_64", None, False),
                                             ("m1_64", "1", True), ("m1orig_65", None, False)])
def test_which_calls_take_the_bound_path(shape, env, taken, monkeypatch):
    _, prob, thr0, thr1 = _problem(shape)
    if env == "GROUPS":
        monkeypatch.setenv("GCR_VERIFY_GROUPS", "4")        # a set A/B switch pins the fused kernel
    elif env is not None:
        monkeypatch.setenv("GCR_VERIFY_BOUND", env)
    if taken:
        _bound_hook(prob, thr0, thr1, 16, 4)
        with pytest.raises(ValueError):
            _bound_hook(prob, thr0, thr1, 16, 3)            # fewer than 4 batches
    else:
        with pytest.raises(ValueError):
            _bound_hook(prob, thr0, thr1, 16, 4)


def test_bound_path_matches_oracle_replay():
    # every record against the oracle's sampler, solver, twin-math MSAC score
    # and `best < score && isValidModel` in slot order
    kind, prob, thr0, thr1 = _problem("m2_300_200")
    nslots, nb = 1024, 5
    res = _records(prob, thr0, thr1, nslots, nb)
    _bound_hook(prob, thr0, thr1, nslots, nb)           # raises unless this configuration takes the bound path
    inc, models, counts, _, value = O.slots_scored(kind, prob.f0, prob.f1, SEED, SLOT0, nslots * nb, [(thr0, thr1)])
    for b in range(nb):
        s0 = SLOT0 + b * nslots
        best, bslot = 0.0, -1
        for j in range(b * nslots, (b + 1) * nslots):
            if inc[j] > 101:
                continue
            valid = max(abs(models[j][3]), abs(models[j][4])) < 1e-3            # two_sift.hpp:45-61
            if best < value[0][j] and valid:
                best, bslot = value[0][j], j
        r = res[b]
        sl = slice(b * nslots, (b + 1) * nslots)
        assert (r.models, r.iterations) == (int((inc[sl] <= 101).sum()), int(inc[sl].sum())), b
        assert r.best_slot == (SLOT0 + bslot if bslot >= 0 else -1), b
        assert bslot >= 0
        assert bits(r.best_score) == bits(best), b
        assert [r.best_inliers[0], r.best_inliers[1]] == [int(c) for c in counts[0][bslot]], b
        got = [r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
               r.best_model.alpha, r.best_model.phi]
        assert np.array_equal(bits(got), bits(models[bslot])), b


@pytest.mark.parametrize("shape,nslots", [("m2_129_128", 272), ("m2_500_500", 1024), ("m1_65", 272),
                                          ("m1orig_300", 1024)])
def test_bounds_cover_the_inlier_counts(shape, nslots, monkeypatch):
    kind, prob, thr0, thr1 = _problem(shape)
    _take_bound_path(prob, monkeypatch)
    nb = 4
    ub0, ub1, _ = _bound_hook(prob, thr0, thr1, nslots, nb)
    p = _params(thr0, thr1)
    u32, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    for b in range(nb):
        inc = np.zeros(nslots, dtype=np.uint8)
        n0 = np.zeros(nslots, dtype=np.uint32)
        n1 = np.zeros(nslots, dtype=np.uint32)
        v0, v1, tot = np.zeros(nslots), np.zeros(nslots), np.zeros(nslots)
        N.check(N.lib.gcr_debug_verify_slots(prob.h, C.byref(p), SLOT0 + b * nslots, nslots,
                                             inc.ctypes.data_as(C.POINTER(C.c_uint8)), n0.ctypes.data_as(u32),
                                             n1.ctypes.data_as(u32), v0.ctypes.data_as(dp), v1.ctypes.data_as(dp),
                                             tot.ctypes.data_as(dp)))
        sl = slice(b * nslots, (b + 1) * nslots)
        assert (ub0[sl] >= n0).all() and (ub1[sl] >= n1).all(), b
        assert (ub0[sl][inc > 101] == 0).all() and (ub1[sl][inc > 101] == 0).all(), b
        assert n0.sum() > 0


def test_most_slots_are_not_scored():
    # M2 500 + 500 at 1024 slots: the oracle puts the slots whose inlier total
    # at 1.3 x the thresholds reaches the best of 64 seeds at 2 - 4 % of the
    # batch; scoring half of the live slots or more would mean the path
    # passes by scoring everything
    kind, prob, thr0, thr1 = _problem("m2_500_500")
    nslots, nb = 1024, 4
    _, _, scored = _bound_hook(prob, thr0, thr1, nslots, nb)
    inc, models = prob.generate(SEED, SLOT0, nslots * nb)
    live = ((inc <= 101) & (np.maximum(np.abs(models[:, 3]), np.abs(models[:, 4])) < 1e-3)).reshape(nb, nslots).sum(1)
    print("scored", scored.tolist(), "live", live.tolist())
    assert (scored > 0).all() and (2 * scored < live).all()
