"""Several batches per launch of the fused feature-major scorer
(k_score_fm<K, 16, true>, csrc/fm_groups.h): a workgroup stays resident and
scores its 16 slots of G consecutive batches, the wave hand-over running
across the batch boundaries (run on an MI355X: pytest -m gpu).

gcr_problem_verify_batches with GCR_VERIFY_GROUPS = 1, 2, 4, 8 (and stage (a),
GCR_VERIFY_GROUPS_STAGE=a, at 4) must return records identical batch for
batch to GCR_VERIFY_GROUPS=1 and to unchained launches (GCR_VERIFY_CHAIN=0):
models, iterations, best slot, score bits, both inlier counts, model bits.

Shapes.  A round is 14 waves x 64 = 896 features of one class:
  M2 (300, 200)   one round per class, most waves empty
  M2 (1000, 200)  three rounds per batch: the round parity flips between
                  the batches of a launch
  M2 (1000, 900)  four rounds
  M1, M1-original with 1000 features: two rounds of one class
Slots: 2048 (the smallest launch with 16 slots per workgroup), 3000 (a
partial last workgroup).  Batches: 11 (no multiple of G), 70 at 2048 slots
(crosses the 64-batch selection ring, ends on a partial ring), 4 (the
shortest call that takes the two-stream path).  One case is also replayed
through the oracle, slot by slot.
"""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_ffi as O
from gcr_testutil import Problem, bits
from pygcransac import _native as N
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

SEED = 20251121
SLOT0 = 7
THREADS = 16

SHAPES = {
    "m2_300_200": (N.SOLVER_SIFT22, 300, 200),
    "m2_1000_200": (N.SOLVER_SIFT22, 1000, 200),
    "m2_1000_900": (N.SOLVER_SIFT22, 1000, 900),
    "m1_1000": (N.SOLVER_SCALE3, 1000, 0),
    "m1orig_1000": (N.SOLVER_SCALE3_ORIGINAL, 1000, 0),
}
# (GCR_VERIFY_GROUPS, GCR_VERIFY_GROUPS_STAGE, GCR_VERIFY_CHAIN)
RUNS = [("1", "b", "1"), ("2", "b", "1"), ("4", "b", "1"), ("8", "b", "1"), ("4", "a", "1"), ("1", "b", "0")]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if N.lib.gcr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    N.context(0)
    O.lib()


@functools.lru_cache(maxsize=None)
def _problem(shape):
    kind, ns, no = SHAPES[shape]
    if kind == N.SOLVER_SIFT22:
        fs, fo, _, _, ts, to = S.problem_m2(ns, no, seed=SEED)
        return kind, Problem(kind, fs, fo), ts, to
    f, _, thr = S.problem_m1(ns, seed=SEED)
    return kind, Problem(kind, f, None), thr, 0.0


def _records(prob, thr0, thr1, nslots, nb):
    p = N.default_params()
    p.scale_residual_thresh, p.orientation_residual_thresh, p.seed = thr0, thr1, SEED
    res = (N.BatchResult * nb)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, nb, res, None))
    return res


def _fields(res):
    return [(r.models, r.iterations, r.best_slot, bits(r.best_score).item(), r.best_inliers[0], r.best_inliers[1],
             bits([r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
                   r.best_model.alpha, r.best_model.phi]).tolist()) for r in res]


@pytest.mark.parametrize("nslots,nb", [(2048, 11), (3000, 11), (2048, 70), (2048, 4), (3000, 4)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_grouped_launches_equal_single_batch_launches(shape, nslots, nb, monkeypatch):
    _, prob, thr0, thr1 = _problem(shape)
    outs = {}
    for groups, stage, chain in RUNS:
        monkeypatch.setenv("GCR_VERIFY_GROUPS", groups)
        monkeypatch.setenv("GCR_VERIFY_GROUPS_STAGE", stage)
        monkeypatch.setenv("GCR_VERIFY_CHAIN", chain)
        outs[(groups, stage, chain)] = _fields(_records(prob, thr0, thr1, nslots, nb))
    ref = outs[("1", "b", "1")]
    assert len(ref) == nb and sum(o[0] for o in ref) > 0          # models were generated and scored
    for key, got in outs.items():
        for b in range(nb):
            assert got[b] == ref[b], (key, b)


def _oracle_slot(args):
    kind, f0, f1, thr0, thr1, s = args
    inc, m = O.slot(kind, f0, f1, SEED, s)
    if inc > 101:
        return inc, None, None
    return inc, m, O.score(kind, f0, f1, m, thr0, thr1)


def test_grouped_launch_matches_oracle_replay(monkeypatch):
    # 5 batches at G = 4: one launch of four batches on the first stream, one
    # of a single batch on the second; every record against the oracle's
    # sampler, solver, twin-math MSAC score and `best < score && isValidModel`
    # in slot order (as test_gpu_bench_config.py replays the bench's batches)
    kind, prob, thr0, thr1 = _problem("m2_300_200")
    nslots, nb = 2048, 5
    monkeypatch.setenv("GCR_VERIFY_GROUPS", "4")
    res = _records(prob, thr0, thr1, nslots, nb)
    with ThreadPoolExecutor(THREADS) as ex:
        outs = list(ex.map(_oracle_slot, [(kind, prob.f0, prob.f1, thr0, thr1, s)
                                          for s in range(SLOT0, SLOT0 + nb * nslots)], chunksize=64))
    for b in range(nb):
        s0 = SLOT0 + b * nslots
        models = iters = 0
        best, bslot, bcnt, bmodel = 0.0, -1, [0, 0], None
        for j, (inc, m, sc) in enumerate(outs[b * nslots:(b + 1) * nslots]):
            iters += inc
            if m is None:
                continue
            models += 1
            valid = max(abs(m[3]), abs(m[4])) < 1e-3            # two_sift.hpp:45-61
            if best < sc["value"] and valid:
                best, bslot, bcnt, bmodel = sc["value"], s0 + j, [int(c) for c in sc["counts"]], m
        r = res[b]
        assert (r.models, r.iterations, r.best_slot) == (models, iters, bslot), b
        if bslot < 0:
            continue
        assert bits(r.best_score) == bits(best), b
        assert [r.best_inliers[0], r.best_inliers[1]] == bcnt, b
        got = [r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
               r.best_model.alpha, r.best_model.phi]
        assert np.array_equal(bits(got), bits(bmodel)), b
