"""PROSAC sampling on the GPU (csrc/prosac.h): the generators' sampling
function against the host sampler for all five correspondence solvers, the
PROSAC generators against the host sampler + host minimal solvers, uniform
sampling untouched, and whole runs on a budget uniform sampling cannot meet.
Whole-run parity with the oracle's restatement of PROSAC is
test_gpu_oracle_samplers.py's."""
import ctypes as C

import numpy as np
import pytest

import essential_cases as EC
import gravity_cases as GC
import guided_cases as G
import prosac_cases as PC
import pygcransac
import sift_homography_cases as SC
from gcr_testutil import CorrProblem
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S
from test_gpu_guided import GEN_CASES, residuals, same_run

pytestmark = pytest.mark.gpu

H4, F7, E5, G3, S2 = PC.H4, PC.F7, PC.E5, PC.G3, PC.S2
SOLVERS = (H4, F7, E5, G3, S2)
SEED = 0x5EEDFACE12345678
T_SMALL = 1000                                       # g[N] a few hundred slots: a launch crosses the boundary
K_PLAIN = np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 480.0], [0.0, 0.0, 1.0]])


def set_prosac(prob, convergence):
    return N.lib.gcr_problem_set_prosac(prob.h, convergence)


def device_samples(prob, m, seed, slot0, nslots, attempt):
    out = np.zeros((nslots, m), dtype=np.uint32)
    N.check(N.lib.gcr_debug_sample_h(prob.h, seed, slot0, nslots, attempt, out.ctypes.data_as(PC.u32p)))
    return out


def generate(prob, per, seed, slot0, nslots):
    """inc (nslots, per) bytes, models (nslots, per, 9)"""
    inc = np.zeros(nslots * per, dtype=np.uint8)
    H = np.zeros((nslots * per, 9))
    N.check(N.lib.gcr_debug_generate_h(prob.h, seed, slot0, nslots, inc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       H.ctypes.data_as(C.POINTER(C.c_double))))
    return inc.reshape(nslots, per), H.reshape(nslots, per, 9)


def random_problem(solver, n, seed=3):
    """any rows: the sampling function does not read them"""
    rng = np.random.default_rng(seed)
    corr = rng.uniform(0.0, 900.0, (n, 4))
    if solver in (H4, F7):
        return CorrProblem(solver, corr)
    if solver == E5:
        return EC.EssProblem(corr, K_PLAIN, K_PLAIN)
    if solver == G3:
        return GC.GravProblem(corr, K_PLAIN, K_PLAIN, np.eye(3), np.eye(3))
    sift = np.column_stack([rng.uniform(1.0, 9.0, (n, 2)), rng.uniform(-3.0, 3.0, (n, 2))])
    return SC.HProblem(np.column_stack([corr, sift]))


def scene_problem(solver, n, seed=21):
    """(problem, models of a sample's indices on the host, hypotheses per slot)"""
    if solver in (H4, F7):
        corr = (S.problem_h if solver == H4 else S.problem_f)(n, seed=seed)[0]
        return CorrProblem(solver, corr), (lambda idx: G.solve_minimal(solver, corr, idx)), 1 if solver == H4 else 3
    if solver == E5:
        corr, _, K, _, thr = S.problem_e(n, seed=seed)
        rows, _ = EC.normalise(corr, K, K, thr)
        return EC.EssProblem(corr, K, K), (lambda idx: EC.solve_minimal(rows, idx)), 10
    if solver == G3:
        corr, _, K, G1, G2, _ = S.problem_g(n, seed=seed)
        rows, _ = EC.normalise(corr, K, K, 1.0)
        return GC.GravProblem(corr, K, K, G1, G2), (lambda idx: GC.solve_g3(rows, G1, G2, idx)), 4
    rows8 = S.problem_hs(n, seed=seed)[0]
    return SC.HProblem(rows8), (lambda idx: SC.solve_s2(rows8, idx)), 3


# ------------------------------------------------ device sampler == host ----
@pytest.mark.parametrize("solver", SOLVERS)
def test_device_sampler_equals_host_sampler(solver):
    m = PC.M_OF[solver]
    for n in (m, m + 1, 257, 10007):
        gn = int(PC.host_growth(n, m, T_SMALL)[n])
        prob = random_problem(solver, n)
        try:
            N.check(set_prosac(prob, T_SMALL))
            for slot0 in (0, 255, max(gn - 300, 0), 1 << 40):
                for a in (0, 1, 100):
                    got = device_samples(prob, m, SEED, slot0, 2048, a)
                    want = PC.host_samples_prosac(SEED, slot0, 2048, a, n, m, T_SMALL)
                    assert np.array_equal(got, want), (solver, n, slot0, a)
                    assert np.all(got != PC.ALL_ONES)
            # cleared: the same hook draws philox.h's uniform samples
            N.check(set_prosac(prob, 0))
            for slot0, a in ((0, 0), (1 << 40, 100)):
                got = device_samples(prob, m, SEED, slot0, 2048, a)
                assert np.array_equal(got, G.host_samples_uniform(SEED, slot0, 2048, a, n, m)), (solver, n, slot0, a)
        finally:
            prob.close()


# ------------------------------------------------------------ generators ----
PROSAC_GEN_CASES = GEN_CASES + ((H4, {"GCR_GEN_HWIDEN": "1"}), (E5, {}), (G3, {}), (S2, {}))


@pytest.mark.parametrize("n", (257, 10007))
@pytest.mark.parametrize("solver, env", PROSAC_GEN_CASES)
def test_prosac_generator_equals_host_sampler_and_solver(solver, env, n, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)                  # read per launch
    m = PC.M_OF[solver]
    g = PC.host_growth(n, m, T_SMALL)
    gn = int(g[n])
    assert gn > 256
    nslots = 512
    prob, solve, per = scene_problem(solver, n)
    fresh, _, _ = scene_problem(solver, n)
    try:
        N.check(set_prosac(prob, T_SMALL))
        runs = [(slot0,) + generate(prob, per, SEED, slot0, nslots) for slot0 in (0, gn - 256)]
        uniform = generate(fresh, per, SEED, gn, 256)
    finally:
        prob.close()
        fresh.close()

    def host_models(slot, a):
        rc, idx = PC.composed_sample(g, SEED, slot, a, n, m)
        return solve(idx) if rc == 0 else np.zeros((0, 9))

    for slot0, inc, models in runs:
        for s in range(nslots):
            slot = slot0 + s
            first = int(inc[s, 0])
            if first > 101:                       # a pool whose every attempt fails (the first rows of a tiny pool)
                assert first == 102 and np.all(inc[s, 1:] == 255), (slot,)
                if s < 96:
                    assert all(len(host_models(slot, b)) == 0 for b in range(101)), (slot,)
                continue
            a = first - 1
            want = host_models(slot, a)
            k = len(want)
            assert k >= 1, (slot, a)
            assert np.array_equal(models[s, :k].view(np.uint64), want.view(np.uint64)), (slot, a)
            assert inc[s, 1:].tolist() == [0 if q < k else 255 for q in range(1, per)], (slot, a)
            if s < 96:                            # ... and it is the first attempt that gives one
                for b in range(a):
                    assert len(host_models(slot, b)) == 0, (slot, b)
    # past g[N]: the uniform generator's own bytes
    _, inc, models = runs[1]
    assert inc[256:].tobytes() == uniform[0].tobytes() and models[256:].tobytes() == uniform[1].tobytes()


# ------------------------------------------------------ uniform untouched ----
def test_uniform_untouched_after_set_and_clear():
    for solver in SOLVERS:
        fresh, _, per = scene_problem(solver, 2000)
        used, _, _ = scene_problem(solver, 2000)
        try:
            want = generate(fresh, per, SEED, 5, 700)
            N.check(set_prosac(used, PC.DEFAULT_CONVERGENCE))
            prosac = generate(used, per, SEED, 5, 700)
            N.check(set_prosac(used, 0))
            got = generate(used, per, SEED, 5, 700)
        finally:
            fresh.close()
            used.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert prosac[1].tobytes() != want[1].tobytes()


def test_set_prosac_errors():
    f = np.abs(np.random.default_rng(1).normal(1.0, 0.2, (50, 3))) + 0.1
    for kind in (N.SOLVER_SCALE3, N.SOLVER_SCALE3_ORIGINAL):
        h = C.c_void_p()
        N.check(N.lib.gcr_problem_create(N.context(0), kind, f.ctypes.data_as(C.POINTER(C.c_double)), 50, None, 0,
                                         C.byref(h)))
        try:
            assert N.lib.gcr_problem_set_prosac(h, 1000) == N.GCR_EINVAL
            assert "correspondence problems only" in N.last_error()
        finally:
            N.lib.gcr_problem_destroy(h)
    n, m = 50, 4
    prob = CorrProblem(H4, np.random.default_rng(3).uniform(0.0, 900.0, (n, 4)))
    try:
        N.check(set_prosac(prob, T_SMALL))
        want = PC.host_samples_prosac(SEED, 0, 64, 0, n, m, T_SMALL)
        # each refused call leaves the problem as it was
        assert set_prosac(prob, (1 << 40) + 1) == N.GCR_EINVAL and "2^40" in N.last_error()
        w = np.ones(n)
        assert N.lib.gcr_problem_set_probabilities(prob.h, w.ctypes.data, n) == N.GCR_EINVAL
        assert "PROSAC" in N.last_error()
        assert np.array_equal(device_samples(prob, m, SEED, 0, 64, 0), want)
        # the guided stop needs probabilities, which a PROSAC problem cannot have
        p = N.default_params()
        p.flags = N.FLAG_GUIDED_STOP
        mask, M = np.zeros(n, dtype=np.uint8), np.zeros(9)
        assert N.lib.gcr_problem_run(prob.h, C.byref(p), mask.ctypes.data_as(C.POINTER(C.c_uint8)), None,
                                     M.ctypes.data_as(C.POINTER(C.c_double)), None, None) == N.GCR_EINVAL
        assert "PROSAC" in N.last_error()
        # clearing either sampler on a problem that has the other one is fine
        N.check(N.lib.gcr_problem_set_probabilities(prob.h, None, 0))
        assert np.array_equal(device_samples(prob, m, SEED, 0, 64, 0), want)
        N.check(set_prosac(prob, 0))
        # ... and PROSAC on a guided problem is refused: it stays guided
        N.check(N.lib.gcr_problem_set_probabilities(prob.h, w.ctypes.data, n))
        guided = device_samples(prob, m, SEED, 0, 64, 0)
        assert set_prosac(prob, T_SMALL) == N.GCR_EINVAL and "probabilities" in N.last_error()
        assert np.array_equal(device_samples(prob, m, SEED, 0, 64, 0), guided)
        assert np.array_equal(guided, G.host_samples(SEED, 0, 64, 0, w, m))
    finally:
        prob.close()


# ------------------------------------------------------------ whole runs ----
def find(solver, corr, thr, scores, seed, batch_slots=0):
    fn = pygcransac.findHomography if solver == H4 else pygcransac.findFundamentalMatrix
    return fn(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, probabilities=scores, threshold=thr, conf=0.99,
              spatial_coherence_weight=0.0, max_iters=PC.E2E_BUDGET, min_iters=PC.E2E_BUDGET,
              sampler=1 if scores is not None else 0, neighborhood_size=0, seed=seed, batch_slots=batch_slots,
              return_stats=True)


@pytest.fixture(scope="module")
def e2e_runs():
    """The PROSAC run of each solver and seed, computed once."""
    out = {}
    for solver in (H4, F7):
        corr, truth, thr, scores = PC.e2e_problem(solver)
        out[solver] = (corr, truth, thr, scores, [find(solver, corr, thr, scores, seed) for seed in PC.E2E_SEEDS])
    return out


def solves(solver, run, corr, truth, thr):
    """the guided test's criterion: a model, >= 90 % of the truth inliers,
    median truth-inlier residual below the threshold"""
    M, mask = run[0], run[1]
    if M is None or mask[truth].sum() < 0.9 * truth.sum():
        return False
    return float(np.median(residuals(solver, M, corr[truth]))) < thr


@pytest.mark.parametrize("solver", (H4, F7))
def test_prosac_run_meets_a_budget_uniform_sampling_cannot(solver, e2e_runs):
    corr, truth, thr, scores, runs = e2e_runs[solver]
    for seed, (M, mask, st) in zip(PC.E2E_SEEDS, runs):
        assert M is not None, seed
        med = float(np.median(residuals(solver, M, corr[truth])))
        print(f"solver {solver} seed {seed}: inliers {int(mask.sum())}, truth inliers found "
              f"{int(mask[truth].sum())} of {int(truth.sum())}, median truth-inlier residual {med:.4f} px")
        assert mask[truth].sum() >= 0.9 * truth.sum(), (seed, int(mask[truth].sum()), int(truth.sum()))
        assert med < thr, (seed, med)
    # the same budget with uniform sampling (an all-inlier sample has chance 0.05^m per slot)
    solved = [solves(solver, find(solver, corr, thr, None, seed), corr, truth, thr) for seed in PC.E2E_SEEDS]
    print(f"solver {solver}: uniform runs that solve it: {solved}")
    assert sum(solved) <= 1, solved


@pytest.mark.parametrize("solver", (H4, F7))
def test_prosac_run_is_deterministic_and_chunk_independent(solver, e2e_runs):
    corr, truth, thr, scores, runs = e2e_runs[solver]
    order = PC.order_of(scores)
    for seed in (0, 3):
        for bs in (0, 64, 4096):
            assert same_run(runs[seed], find(solver, corr, thr, scores, seed, batch_slots=bs)), (seed, bs)
        # the sharded entry takes the rows in quality order, as the C ABI does
        M, masks, st, _ = D.run_problem_sharded(
            solver, corr[order], params=dict(scale_residual_thresh=thr, confidence=0.99, spatial_coherence_weight=0.0,
                                             min_iteration_number=PC.E2E_BUDGET, max_iteration_number=PC.E2E_BUDGET,
                                             seed=seed),
            world=1, prosac_convergence=PC.DEFAULT_CONVERGENCE)
        mask = np.zeros(len(corr), dtype=bool)
        mask[order] = masks[0]
        assert same_run(runs[seed], (M, mask, st)), seed


@pytest.mark.parametrize("solver", (H4, F7))
def test_no_stale_speculation_after_set_prosac(solver, e2e_runs):
    """A uniform run (which may leave a speculative chunk in flight), then
    set_prosac, then a PROSAC run: the bits of a fresh PROSAC problem; and
    back: cleared, the problem repeats its uniform run."""
    corr, truth, thr, scores, _ = e2e_runs[solver]
    rows = np.ascontiguousarray(corr[PC.order_of(scores)])
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.confidence = 0.99
    p.spatial_coherence_weight = 0.0
    p.min_iteration_number = 50
    p.max_iteration_number = 5000
    p.seed = 2

    def run(prob):
        mask = np.zeros(len(rows), dtype=np.uint8)
        M = np.zeros(9)
        st = N.Stats()
        rc = N.check(N.lib.gcr_problem_run(prob.h, C.byref(p), mask.ctypes.data_as(C.POINTER(C.c_uint8)), None,
                                           M.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(st)))
        return rc, M.tobytes(), mask.tobytes(), st.iteration_number, st.hypotheses, st.score

    used, fresh, plain = CorrProblem(solver, rows), CorrProblem(solver, rows), CorrProblem(solver, rows)
    try:
        uniform = run(used)
        N.check(set_prosac(used, PC.DEFAULT_CONVERGENCE))
        got = run(used)
        N.check(set_prosac(fresh, PC.DEFAULT_CONVERGENCE))
        want = run(fresh)
        assert got == want
        assert got != uniform
        N.check(set_prosac(used, 0))
        assert run(used) == uniform == run(plain)
    finally:
        used.close()
        fresh.close()
        plain.close()


def informative_scores(truth, seed=9):
    return np.random.default_rng(seed).normal(0.0, 1.0, len(truth)) + np.where(truth, 2.0, 0.0)


def check_model_and_mask(M, mask, truth):
    """a model, and a mask in the caller's order (the truth is in that order;
    the rows were sorted by score for the run)"""
    assert M is not None and mask.shape == truth.shape and mask.dtype == bool
    hit = int((mask & truth).sum())
    assert hit >= 0.9 * int(truth.sum()) and hit >= 0.9 * int(mask.sum()), (hit, int(truth.sum()), int(mask.sum()))


def test_essential_gravity_and_sift_homography_calls():
    kw = dict(conf=0.99, spatial_coherence_weight=0.0, max_iters=5000, min_iters=50, sampler=1, neighborhood_size=0)
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
