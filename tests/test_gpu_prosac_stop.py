"""The PROSAC stop (GCR_FLAG_PROSAC_STOP, csrc/prosac_stop.h) on the GPU: the
stop kernel against its host twin on scenes and on crafted inlier patterns at
the wave and tile boundaries; whole runs that end at the iteration floor and
lose nothing; the same run on every replay path; the flag-clear run untouched;
refusals.  The header is the definition; the oracle's restatement of it and of
which model's (I*, n*) is in force at each update of the stop is compared with
whole flagged runs in test_gpu_oracle_samplers.py."""
import ctypes as C

import numpy as np
import pytest

import essential_cases as EC
import prosac_cases as PC
import prosac_stop_cases as Q
import pygcransac
from gcr_testutil import CorrProblem, dp
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S
from test_gpu_guided_stop import residuals, same_run
from test_gpu_prosac import check_model_and_mask, informative_scores

pytestmark = pytest.mark.gpu

H4, F7, E5 = PC.H4, PC.F7, PC.E5
SEED = 0x5EEDFACE12345678
T_MAX = 1 << 40                          # every prefix long covered: non-randomness alone decides
B = Q.B
u8p = C.POINTER(C.c_uint8)


def set_prosac(prob, convergence):
    return N.lib.gcr_problem_set_prosac(prob.h, convergence)


def device_stop(prob, models, thr, conf=0.99):
    """gcr_debug_prosac_stop_h: (count, best_i, best_n) per model."""
    models = np.ascontiguousarray(models, dtype=np.float64).reshape(-1, 9)
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.confidence = conf
    out = [np.zeros(len(models), dtype=np.uint32) for _ in range(3)]
    N.check(N.lib.gcr_debug_prosac_stop_h(prob.h, C.byref(p), dp(models), len(models),
                                          *(o.ctypes.data_as(Q.u32p) for o in out)))
    return out


# ------------------------------------------------------ kernel == host ----
NO_INLIERS = {H4: np.array([1.0, 0.0, 1e6, 0.0, 1.0, 1e6, 0.0, 0.0, 1.0]),
              # every epipolar line is x = 1e7: far from any point, pixel or normalised
              F7: np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1e7])}
NO_INLIERS[E5] = NO_INLIERS[F7]
SIZES = (None, 19, 20, 21, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 10007)      # None: N = m


def scene(solver, n):
    """(problem over the rows in score order, truth model, threshold)"""
    if solver == E5:
        corr, truth, K, model, thr = S.problem_e(n, 0.5, seed=21)
    else:
        corr, truth, model, thr = (S.problem_h if solver == H4 else S.problem_f)(n, 0.5, seed=21)
    rows = np.ascontiguousarray(corr[PC.order_of(informative_scores(truth))])
    prob = EC.EssProblem(rows, K, K) if solver == E5 else CorrProblem(solver, rows)
    return prob, np.asarray(model, dtype=np.float64).reshape(9), thr


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("solver", (H4, F7, E5))
def test_stop_kernel_equals_host_twin(solver, size):
    m = PC.M_OF[solver]
    n = m if size is None else size
    prob, truth_model, thr = scene(solver, n)
    try:
        # the truth model, a wrong one (the first hypothesis the uniform
        # generator leaves), one without inliers
        wrong = np.asarray(prob.generate(SEED, 0, 1)[1], dtype=np.float64).reshape(-1, 9)[0]
        models = np.ascontiguousarray(np.stack([truth_model, wrong, NO_INLIERS[solver]]))
        masks = [prob.mask(mod, 0, thr).astype(np.uint8) for mod in models]
        n0 = prob.score(models, thr)[0]
        assert [int(mk.sum()) for mk in masks] == [int(v) for v in n0]
        assert n0[2] == 0
        if n >= 63:
            assert n0[0] > 0.4 * n                     # the truth model holds its inliers
        for convergence, conf in ((PC.DEFAULT_CONVERGENCE, 0.99), (1000, 0.99), (1000, 0.95), (T_MAX, 0.95)):
            N.check(set_prosac(prob, convergence))
            imin, qmin = Q.host_tables(n, m, convergence, conf)
            want = [Q.host_choose(mk, m, imin, qmin) for mk in masks]
            for nm in (1, 3):
                count, bi, bn = device_stop(prob, models[:nm], thr, conf)
                assert np.array_equal(count, n0[:nm]), (solver, n, convergence, conf, nm)
                assert list(zip(bi.tolist(), bn.tolist())) == want[:nm], (solver, n, convergence, conf, nm)
        if n >= 257:
            assert want[0][1] < n                      # informative order: a proper prefix of the truth model
    finally:
        prob.close()


IDENTITY = np.eye(3).reshape(9)


def crafted_problem(mask):
    """H rows whose inlier pattern under the identity is `mask`: x2 = x1, or
    x2 = x1 + 100 for an outlier (threshold 1)"""
    rng = np.random.default_rng(5)
    x1 = rng.uniform(0.0, 900.0, (len(mask), 2))
    x2 = x1 + np.where(np.asarray(mask, dtype=bool), 0.0, 100.0)[:, None]
    return CorrProblem(H4, np.column_stack([x1, x2]))


def crafted_stop(mask, convergence=T_MAX, conf=0.99):
    """(kernel's (count, I*, n*), host twin's (I*, n*)) of the mask"""
    n, m = len(mask), 4
    prob = crafted_problem(mask)
    try:
        assert np.array_equal(prob.mask(IDENTITY, 0, 1.0), np.asarray(mask, dtype=bool))
        N.check(set_prosac(prob, convergence))
        count, bi, bn = device_stop(prob, IDENTITY, 1.0, conf)
    finally:
        prob.close()
    imin, qmin = Q.host_tables(n, m, convergence, conf)
    return (int(count[0]), int(bi[0]), int(bn[0])), Q.host_choose(mask, m, imin, qmin)


@pytest.mark.parametrize("edge", (64, 128, 192, B, 2 * B))
def test_best_prefix_on_either_side_of_a_wave_or_tile_boundary(edge):
    n = 2 * B + 88
    for k in (edge - 1, edge, edge + 1):
        # share 1 up to row k, a few inliers far behind: n* = k, closed by the
        # last lane of a wave / tile, or the first of the next
        mask = Q.prefix_mask(n, k, tail=(n - 3, n - 1))
        got, want = crafted_stop(mask)
        assert want == (k, k) and got == (k + 2, k, k), (k, got, want)
        # ... and a prefix count carried across the boundary: half the rows
        # before the edge, all rows of the 40 after it
        rows = list(range(0, k, 2)) + list(range(k, k + 40))
        mask = Q.mask_of(n, rows)
        got, want = crafted_stop(mask)
        assert got == (len(rows),) + want and want[1] == k + 40, (k, got, want)


def test_equal_ratios_across_two_tiles_choose_the_larger_length():
    n = 600
    assert 200 < B < 400                   # the two lengths lie in different tiles
    mask = Q.mask_of(n, list(range(1, 200, 2)) + list(range(300, 400)))
    got, want = crafted_stop(mask)
    assert want == (200, 400) and got == (200, 200, 400)
    # the same share at 200 only (rows 300 .. 398): the first tile's candidate wins
    mask = Q.mask_of(n, list(range(1, 200, 2)) + list(range(300, 399)))
    got, want = crafted_stop(mask)
    assert want == (100, 200) and got == (199, 100, 200)


def test_conditions_decide_on_the_device_as_on_the_host():
    n = 2000
    # 12 of the first 20: fails coverage under a short schedule, chosen under a long one
    mask = Q.prefix_mask(n, 12)
    assert crafted_stop(mask, 1000) == ((12, 12, n), (12, n))
    assert crafted_stop(mask, T_MAX) == ((12, 12, 20), (12, 20))
    # 5 of the first 20 is below Imin[20] = 7; 7 is not
    assert crafted_stop(Q.prefix_mask(n, 5)) == ((5, 5, n), (5, n))
    assert crafted_stop(Q.prefix_mask(n, 7)) == ((7, 7, 20), (7, 20))
    # all rows, no rows
    assert crafted_stop(np.ones(n, dtype=np.uint8)) == ((n, n, n), (n, n))
    assert crafted_stop(np.zeros(n, dtype=np.uint8)) == ((0, 0, n), (0, n))


# ----------------------------------------------------------- whole runs ----
def find(solver, corr, thr, scores, seed, prosac_stop, batch_slots=0):
    fn = pygcransac.findHomography if solver == H4 else pygcransac.findFundamentalMatrix
    return fn(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, probabilities=scores, threshold=thr, conf=Q.E2E_CONF,
              spatial_coherence_weight=0.0, max_iters=Q.E2E_MAX_ITERS, min_iters=Q.E2E_MIN_ITERS, sampler=1,
              neighborhood_size=0, seed=seed, batch_slots=batch_slots, return_stats=True, prosac_stop=prosac_stop)


@pytest.fixture(scope="module")
def e2e_runs():
    """Each solver's flag-set runs (the seeds of the PROSAC sampling test), computed once."""
    out = {}
    for solver in (H4, F7):
        corr, truth, thr, scores = Q.e2e_problem(solver)
        out[solver] = (corr, truth, thr, scores, [find(solver, corr, thr, scores, seed, True) for seed in Q.E2E_SEEDS])
    return out


@pytest.mark.parametrize("solver", (H4, F7))
def test_flagged_run_stops_early_and_loses_nothing(solver, e2e_runs):
    corr, truth, thr, scores, runs = e2e_runs[solver]
    m = PC.M_OF[solver]
    for seed, (M, mask, st) in zip(Q.E2E_SEEDS, runs):
        clear = find(solver, corr, thr, scores, seed, False)
        assert M is not None, seed
        uniform = Q.host_uniform_number(int(mask.sum()), len(mask), m, Q.E2E_CONF)
        found = int(mask[truth].sum())
        med = float(np.median(residuals(solver, M, corr[truth])))
        print(f"solver {solver} seed {seed}: stop at {st['iteration_number']} (flag clear "
              f"{clear[2]['iteration_number']}, uniform bound of its {int(mask.sum())} inliers {uniform}), truth "
              f"inliers {found} / {int(truth.sum())}, median truth-inlier residual {med:.4f} px")
        assert st["iteration_number"] <= clear[2]["iteration_number"], seed
        assert st["iteration_number"] < uniform, seed
        # the project's `solves` criterion
        assert found >= 0.9 * truth.sum(), (seed, found, int(truth.sum()))
        assert med < thr, (seed, med)


def problem_runner(solver, rows, thr, seed):
    """run(prob, flags) on resident problems over the ordered rows: every bit the call returns"""
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.confidence = Q.E2E_CONF
    p.spatial_coherence_weight = 0.0
    p.min_iteration_number = Q.E2E_MIN_ITERS
    p.max_iteration_number = Q.E2E_MAX_ITERS
    p.seed = seed

    def run(prob, flags):
        p.flags = flags
        mask = np.zeros(len(rows), dtype=np.uint8)
        M = np.zeros(9)
        st = N.Stats()
        rc = N.check(N.lib.gcr_problem_run(prob.h, C.byref(p), mask.ctypes.data_as(u8p), None, dp(M), None,
                                           C.byref(st)))
        return rc, M.tobytes(), mask.tobytes(), st.iteration_number, st.hypotheses, st.score

    return run


@pytest.mark.parametrize("solver", (H4, F7))
def test_flagged_run_is_the_same_on_every_path(solver, e2e_runs, monkeypatch):
    corr, truth, thr, scores, runs = e2e_runs[solver]
    order = PC.order_of(scores)
    rows = np.ascontiguousarray(corr[order])
    params = dict(scale_residual_thresh=thr, confidence=Q.E2E_CONF, spatial_coherence_weight=0.0,
                  min_iteration_number=Q.E2E_MIN_ITERS, max_iteration_number=Q.E2E_MAX_ITERS,
                  flags=N.FLAG_PROSAC_STOP)
    for seed in (0, 3):
        for bs in (0, 64, 4096):
            assert same_run(runs[seed], find(solver, corr, thr, scores, seed, True, batch_slots=bs)), (seed, bs)
        # the sharded entry takes the rows in quality order, as the C ABI does
        M, masks, st, _ = D.run_problem_sharded(solver, rows, params=dict(params, seed=seed), world=1,
                                                prosac_convergence=PC.DEFAULT_CONVERGENCE)
        mask = np.zeros(len(corr), dtype=bool)
        mask[order] = masks[0]
        assert same_run(runs[seed], (M, mask, st)), seed
        # the per-slot replay, and the stop launches' staged copies instead of pinned reads and writes
        for env in ({"GCR_REPLAY": "slots"}, {"GCR_SPECULATE": "0"}, {"GCR_ZEROCOPY": "0"},
                    {"GCR_REPLAY": "slots", "GCR_ZEROCOPY": "0"}):
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)                   # read per run
                assert same_run(runs[seed], find(solver, corr, thr, scores, seed, True)), (seed, env)
        # a handle that ran flag-clear first gives a fresh handle's flag-set run
        run = problem_runner(solver, rows, thr, seed)
        used, fresh = CorrProblem(solver, rows), CorrProblem(solver, rows)
        try:
            N.check(set_prosac(used, PC.DEFAULT_CONVERGENCE))
            N.check(set_prosac(fresh, PC.DEFAULT_CONVERGENCE))
            run(used, 0)
            got, want = run(used, N.FLAG_PROSAC_STOP), run(fresh, N.FLAG_PROSAC_STOP)
        finally:
            used.close()
            fresh.close()
        assert got == want
        M, mask, st = runs[seed]
        assert got[1] == M.tobytes() and got[3] == st["iteration_number"] and got[4] == st["hypotheses"]


@pytest.mark.parametrize("solver", (H4, F7))
def test_flag_clear_run_is_untouched_by_a_flagged_run(solver, e2e_runs):
    corr, truth, thr, scores, _ = e2e_runs[solver]
    rows = np.ascontiguousarray(corr[PC.order_of(scores)])
    run = problem_runner(solver, rows, thr, 2)
    used, fresh = CorrProblem(solver, rows), CorrProblem(solver, rows)
    try:
        N.check(set_prosac(used, PC.DEFAULT_CONVERGENCE))
        N.check(set_prosac(fresh, PC.DEFAULT_CONVERGENCE))
        before = run(used, 0)
        flagged = run(used, N.FLAG_PROSAC_STOP)
        after = run(used, 0)
        assert before == after == run(fresh, 0)
        assert flagged != before and flagged[3] < before[3]
    finally:
        used.close()
        fresh.close()


def test_essential_gravity_and_sift_homography_calls():
    kw = dict(conf=0.99, spatial_coherence_weight=0.0, max_iters=5000, min_iters=50, sampler=1, neighborhood_size=0,
              prosac_stop=True)
    c, truth, K, _, thr = S.problem_e(2000, 0.5, seed=11)
    E, mask = pygcransac.findEssentialMatrix(c, K, K, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W,
                                             probabilities=informative_scores(truth), threshold=thr, seed=5, **kw)
    check_model_and_mask(E, mask, truth)
    c, truth, K, G1, G2, _ = S.problem_g(2000, 0.5, seed=12)
    E, mask = pygcransac.findGravityEssentialMatrix(c, K, K, G1, G2, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W,
                                                    probabilities=informative_scores(truth), threshold=1.0, seed=6,
                                                    **kw)
    check_model_and_mask(E, mask, truth)
    c, truth, _, thr = S.problem_hs(2000, 0.5, seed=13)
    H, mask = pygcransac.findHomographySIFT(c, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W,
                                            probabilities=informative_scores(truth), threshold=thr, seed=7, **kw)
    check_model_and_mask(H, mask, truth)


# ------------------------------------------------------------- refusals ----
def test_refusals():
    corr, truth, _, thr = S.problem_h(300, 0.5, seed=4)
    run = problem_runner(H4, corr, thr, 1)
    prob = CorrProblem(H4, corr)

    def refused(flags, word):
        mask, M = np.zeros(len(corr), dtype=np.uint8), np.zeros(9)
        p = N.default_params()
        p.scale_residual_thresh = thr
        p.flags = flags
        rc = N.lib.gcr_problem_run(prob.h, C.byref(p), mask.ctypes.data_as(u8p), None, dp(M), None, None)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (rc, N.last_error())

    try:
        refused(N.FLAG_PROSAC_STOP, "PROSAC sampling")                                  # a uniform problem
        one = [np.zeros(1, dtype=np.uint32) for _ in range(3)]
        p = N.default_params()
        p.scale_residual_thresh = thr
        assert N.lib.gcr_debug_prosac_stop_h(prob.h, C.byref(p), dp(IDENTITY), 1,
                                             *(o.ctypes.data_as(Q.u32p) for o in one)) == N.GCR_EINVAL
        w = np.where(truth, 1.0, 0.05)
        N.check(N.lib.gcr_problem_set_probabilities(prob.h, w.ctypes.data, len(w)))
        refused(N.FLAG_PROSAC_STOP, "PROSAC sampling")                                  # a guided problem
        refused(N.FLAG_PROSAC_STOP | N.FLAG_GUIDED_STOP, "exclusive")
        N.check(N.lib.gcr_problem_set_probabilities(prob.h, None, 0))
        N.check(set_prosac(prob, PC.DEFAULT_CONVERGENCE))
        refused(N.FLAG_PROSAC_STOP | N.FLAG_GUIDED_STOP, "exclusive")                   # both flags, a PROSAC problem
        assert run(prob, N.FLAG_PROSAC_STOP)[0] > 0                                     # accepted: an inlier count
        N.check(set_prosac(prob, 0))
        refused(N.FLAG_PROSAC_STOP, "PROSAC sampling")                                  # cleared: refused again
    finally:
        prob.close()
    # the one-shot entries sample uniformly or guided
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.flags = N.FLAG_PROSAC_STOP
    mask, M, st = np.zeros(len(corr), dtype=np.uint8), np.zeros(9), N.Stats()
    c = np.ascontiguousarray(corr)
    assert N.lib.gcr_find_homography(N.context(0), c.ctypes.data, len(c), C.byref(p), mask.ctypes.data,
                                     M.ctypes.data, C.byref(st)) == N.GCR_EINVAL
    assert "PROSAC sampling" in N.last_error()
