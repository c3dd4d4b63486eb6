"""Essential-matrix estimator on the GPU: the generator kernel against the host
solver bit for bit, the scorers against a fundamental-matrix problem on the
normalised rows, the pixel neighbourhood grid, whole runs, the guided stop and
the sharded entry."""
import ctypes as C

import numpy as np
import pytest

import essential_cases as EC
import pygcransac
from gcr_testutil import CorrProblem
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

SEED = 0x5EEDFACE12345678
SIZE = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)
DEFAULT = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])


def small_problem():
    """N = 40: 30 inliers of problem_e, 10 random rows; six rows (inliers) are
    copies of one another, so samples holding two of them are degenerate."""
    corr, truth, K, _, _ = S.problem_e(100, 0.5, seed=31)
    rng = np.random.default_rng(32)
    rows = np.concatenate([corr[truth][:30],
                           np.column_stack([rng.uniform(0, S.IMG_W, 10), rng.uniform(0, S.IMG_H, 10),
                                            rng.uniform(0, S.IMG_W, 10), rng.uniform(0, S.IMG_H, 10)])])
    for i in (7, 11, 17, 22, 28):
        rows[i] = rows[3]
    w = np.concatenate([np.ones(30), np.full(10, 0.05)])
    return np.ascontiguousarray(rows), K, w


@pytest.mark.parametrize("guided", (False, True), ids=("uniform", "guided"))
def test_generator_equals_the_host_solver_bitwise(guided):
    rows, K, w = small_problem()
    nslots, slot0 = 333, 2 ** 32 - 100          # no multiple of a workgroup's slots; crosses the 32-bit counter word
    norm, _ = EC.normalise(rows, K, K, 1.0)
    prob = EC.EssProblem(rows, K, K)
    try:
        if guided:
            prob.set_probabilities(w)
        inc, models = prob.generate(SEED, slot0, nslots)
        want_inc = np.full((nslots, 10), 255, dtype=np.uint8)
        want_inc[:, 0] = 102
        want = np.tile(DEFAULT, (nslots, 10, 1))
        open_slots = np.arange(nslots)
        for a in range(101):
            if not len(open_slots):
                break
            idx = prob.sample(SEED, slot0, nslots, a)
            still = []
            for s in open_slots:
                assert idx[s].max() < 40                     # the draw budget never runs out here
                if guided:
                    assert np.all(w[idx[s]] > 0)
                got = EC.solve_minimal(norm, idx[s])
                if not len(got):
                    still.append(s)
                    continue
                want_inc[s, 0] = a + 1
                want_inc[s, 1:len(got)] = 0
                want[s, :len(got)] = got
            open_slots = np.array(still, dtype=np.int64)
        assert np.array_equal(inc, want_inc)
        assert np.array_equal(models.view(np.uint64), want.view(np.uint64))
        # the case is hard enough: retries and many-model slots both occur
        assert (inc[:, 0] > 1).any() and (inc[:, 0] <= 101).all()
        assert ((inc[:, 1:] == 0).sum(axis=1) >= 3).any()
        if not guided:
            # the threaded host twin (the measurements' CPU baseline) is the same function
            hinc, hmodels = np.zeros_like(inc), np.zeros_like(models)
            N.check(N.lib.gcr_host_generate_e(norm.ctypes.data, 40, SEED, slot0, nslots, 3, hinc.ctypes.data,
                                              hmodels.ctypes.data))
            assert np.array_equal(hinc, inc) and np.array_equal(hmodels.view(np.uint64), models.view(np.uint64))
    finally:
        prob.close()


def test_verify_batches_select_the_best_live_model():
    """gcr_problem_verify_batch(es) on an essential problem: every live model of
    the generator is scored, and the best slot is the first strict maximum of
    the MSAC scores of gcr_debug_score_h."""
    corr, _, K, _, thr = S.problem_e(500, 0.5, seed=38)
    nslots = 300
    prob = EC.EssProblem(corr, K, K)
    try:
        p = prob._params(thr)
        p.seed = SEED
        res = (N.BatchResult * 2)()
        N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), 1000, nslots, 2, res, None))
        for b in range(2):
            inc, models = prob.generate(SEED, 1000 + b * nslots, nslots)
            live = (inc.reshape(-1) <= 101)
            assert res[b].models == live.sum()
            assert res[b].iterations == np.where(inc <= 102, inc, 0).sum()
            n0, v0, tot = prob.score(models.reshape(-1, 9), thr)
            T = (2.25 * thr_n(K, thr)) * thr_n(K, thr)
            msac = np.where(live & (n0 >= 5), v0 / T + n0, 0.0)
            j = int(np.argmax(msac))                         # the first maximum
            assert res[b].best_slot == 1000 + b * nslots + j // 10
            assert res[b].best_score == msac[j] and res[b].best_inliers[0] == n0[j]
        one = N.BatchResult()
        assert N.lib.gcr_problem_verify_batch(prob.h, C.byref(p), 1000, nslots, C.byref(one), None) == res[0].models
        assert one.best_slot == res[0].best_slot and one.best_score == res[0].best_score
    finally:
        prob.close()


def thr_n(K, thr):
    return thr / ((K[0, 0] + K[1, 1] + K[0, 0] + K[1, 1]) / 4.0)


def test_scorers_are_the_fundamental_matrix_scorers_on_normalised_rows():
    corr, _, K, E, thr = S.problem_e(300, 0.5, seed=33)
    norm, thr_n = EC.normalise(corr, K, K, thr)
    pe, pf = EC.EssProblem(corr, K, K), CorrProblem(N.SOLVER_FUNDAMENTAL7, norm)
    try:
        _, gen = pe.generate(SEED, 0, 8)
        models = np.ascontiguousarray(np.concatenate([E.reshape(1, 9), gen.reshape(-1, 9)])[:37])
        assert len(models) == 37
        a, b = pe.score(models, thr), pf.score(models, thr_n)
        assert np.array_equal(a[0], b[0]) and a[0].max() > 100
        for u, v in zip(a[1:], b[1:]):
            assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
        for rule in (0, 1, 2):
            for m in models[:5]:
                assert np.array_equal(pe.mask(m, rule, thr, 0.3), pf.mask(m, rule, thr_n, 0.3))
    finally:
        pe.close()
        pf.close()


def test_grid_lies_over_the_pixels():
    """Pixels and K both scaled by 2: the normalised rows are the same bits and
    the pixel grid (cell sizes from the doubled image size) is scaled with
    them, so the edges, the graph cuts and the result are the same."""
    corr, _, K, _, thr = S.problem_e(600, 0.5, seed=34)
    K2 = K.copy()
    K2[:2] *= 2.0
    kw = dict(conf=0.99, spatial_coherence_weight=0.3, max_iters=2000, min_iters=50, neighborhood_size=4, seed=5,
              device=0, return_stats=True)
    E1, m1, st1 = pygcransac.findEssentialMatrix(corr, K, K, *SIZE, threshold=thr, **kw)
    E2, m2, st2 = pygcransac.findEssentialMatrix(2.0 * corr, K2, K2, *(2 * v for v in SIZE), threshold=2.0 * thr, **kw)
    assert E1 is not None and st1["graph_cut_number"] > 0
    assert st1["graph_cut_number"] == st2["graph_cut_number"]
    assert np.array_equal(m1, m2) and E1.tobytes() == E2.tobytes()
    # ... and the grid matters: without it the labeling has no pairwise terms
    kw0 = dict(kw, neighborhood_size=0)
    _, m0, st0 = pygcransac.findEssentialMatrix(corr, K, K, *SIZE, threshold=thr, **kw0)
    assert m0.sum() > 0


@pytest.fixture(scope="module")
def whole():
    corr, truth, K, E, thr = S.problem_e(2000, 0.6, seed=35, noise=0.5)
    kw = dict(threshold=thr, conf=0.99, spatial_coherence_weight=0.0, max_iters=5000, min_iters=50, seed=6, device=0,
              return_stats=True)
    return corr, truth, K, E, thr, kw, pygcransac.findEssentialMatrix(corr, K, K, *SIZE, **kw)


def test_whole_run_finds_the_truth(whole):
    corr, truth, K, E_gt, thr, kw, (E, mask, st) = whole
    prob = EC.EssProblem(corr, K, K)
    try:
        yard = prob.mask(E_gt, 0, thr)                       # the final mask's rule on the true model
    finally:
        prob.close()
    assert E is not None and abs(np.linalg.norm(E) - 1.0) < 1e-12
    print(f"inliers {int(mask.sum())}, yardstick {int(yard.sum())}, truth {int(truth.sum())}, "
          f"iterations {st['iteration_number']}")
    assert yard.sum() >= 0.9 * truth.sum()
    assert mask.sum() >= 0.9 * yard.sum()
    assert (mask & truth).sum() >= 0.9 * mask.sum()
    # the returned mask is the final rule's mask of the returned model
    prob = EC.EssProblem(corr, K, K)
    try:
        assert np.array_equal(prob.mask(E, 0, thr), mask)
    finally:
        prob.close()


def test_runs_are_deterministic_and_independent_of_the_batch(whole):
    corr, truth, K, E_gt, thr, kw, (E, mask, st) = whole
    for bs in (0, 64, 1000):
        E2, mask2, st2 = pygcransac.findEssentialMatrix(corr, K, K, *SIZE, batch_slots=bs, **kw)
        assert E2.tobytes() == E.tobytes() and np.array_equal(mask2, mask), bs
        assert st2["iteration_number"] == st["iteration_number"] and st2["score"] == st["score"], bs


def test_guided_stop_returns_no_later_than_the_uniform_run(whole):
    corr, truth, K, E_gt, thr, kw, (E, mask, st) = whole
    w = np.where(truth, 1.0, 0.05)
    Eg, mg, sg = pygcransac.findEssentialMatrix(corr, K, K, *SIZE, probabilities=w, sampler=3, guided_stop=True, **kw)
    assert Eg is not None and (mg & truth).sum() >= 0.9 * mg.sum()
    print(f"iterations: guided stop {sg['iteration_number']}, uniform {st['iteration_number']}")
    assert sg["iteration_number"] <= st["iteration_number"]


def test_sharded_world_one_equals_the_plain_run():
    corr, _, K, _, thr = S.problem_e(800, 0.5, seed=36)
    fields = dict(scale_residual_thresh=thr, confidence=0.99, min_iteration_number=50, max_iteration_number=3000,
                  seed=8)
    prob = EC.EssProblem(corr, K, K)
    try:
        E, mask, st = prob.run(**fields)
    finally:
        prob.close()
    Es, masks, sts, _ = D.run_problem_sharded(N.SOLVER_ESSENTIAL5, corr, params=fields, rank=0, world=1, device=0,
                                              K1=K, K2=K)
    assert E is not None and Es.tobytes() == E.tobytes()
    assert np.array_equal(masks[0], mask)
    assert sts["iteration_number"] == st["iteration_number"] and sts["score"] == st["score"]


def test_batch_items_cannot_be_essential():
    corr = np.ascontiguousarray(S.problem_e(50, 0.5, seed=37)[0])
    item = N.BatchItem()
    item.solver = N.SOLVER_ESSENTIAL5
    item.f0 = corr.ctypes.data_as(C.POINTER(C.c_double))
    item.n0 = len(corr)
    item.params = N.default_params()
    mask = np.zeros(len(corr), dtype=np.uint8)
    item.mask0_out = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    assert N.lib.gcr_solve_batch(0, C.byref(item), 1, 1) == N.GCR_EINVAL
    assert item.result == N.GCR_EINVAL
