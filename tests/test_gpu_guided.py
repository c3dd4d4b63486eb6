"""Guided (importance) sampling on the GPU: the generators' sampling function
against the host sampler, the guided generators against the host sampler +
host minimal solver, uniform sampling untouched, and end-to-end runs on a
budget uniform sampling cannot meet."""
import ctypes as C

import numpy as np
import pytest

import guided_cases as G
import pygcransac
from gcr_testutil import CorrProblem
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

H4, F7 = N.SOLVER_HOMOGRAPHY4, N.SOLVER_FUNDAMENTAL7
M_OF = {H4: 4, F7: 7}
SEED = 0x5EEDFACE12345678


def set_probabilities(prob, w):
    if w is None:
        return N.lib.gcr_problem_set_probabilities(prob.h, None, 0)
    w = np.ascontiguousarray(w, dtype=np.float64)
    return N.lib.gcr_problem_set_probabilities(prob.h, w.ctypes.data, len(w))


def device_samples(prob, seed, slot0, nslots, attempt):
    m = M_OF[prob.solver]
    out = np.zeros((nslots, m), dtype=np.uint32)
    N.check(N.lib.gcr_debug_sample_h(prob.h, seed, slot0, nslots, attempt, out.ctypes.data_as(G.u32p)))
    return out


def random_corr(n, seed=3):
    return np.random.default_rng(seed).uniform(0.0, 900.0, (n, 4))


# ------------------------------------------------ device sampler == host ----
@pytest.mark.parametrize("solver", (H4, F7))
@pytest.mark.parametrize("n", G.NS)
def test_device_sampler_equals_host_sampler(n, solver):
    m = M_OF[solver]
    prob = CorrProblem(solver, random_corr(n))
    try:
        for pattern in G.PATTERNS:
            w = G.weights(pattern, n, m)
            if int((w > 0).sum()) < m:
                assert set_probabilities(prob, w) == N.GCR_EINVAL, (pattern, n, m)
                continue
            N.check(set_probabilities(prob, w))
            for slot0 in (0, 1 << 40):
                for a in (0, 1, 100):
                    got = device_samples(prob, SEED, slot0, 2048, a)
                    want = G.host_samples(SEED, slot0, 2048, a, w, m)
                    assert np.array_equal(got, want), (pattern, n, m, slot0, a)
                    ok = got[:, 0] != G.ALL_ONES
                    assert np.all(w[got[ok]] > 0)          # a zero weight is never drawn
                    if n == m:                             # every sample is a permutation of all rows
                        assert np.all(np.sort(got[ok], axis=1) == np.arange(n))
                    if pattern == "ones":
                        assert ok.all()
        # cleared: the same hook draws philox.h's uniform samples
        N.check(set_probabilities(prob, None))
        for slot0, a in ((0, 0), (1 << 40, 100)):
            got = device_samples(prob, SEED, slot0, 2048, a)
            assert np.array_equal(got, G.host_samples_uniform(SEED, slot0, 2048, a, n, m)), (n, m, slot0, a)
    finally:
        prob.close()


# ------------------------------------------------------------ generators ----
def guided_problem(solver, n, seed=21):
    if solver == H4:
        corr, truth, _, _ = S.problem_h(n, seed=seed)
    else:
        corr, truth, _, _ = S.problem_f(n, seed=seed)
    return corr, truth, np.where(truth, 1.0, 0.05)


GEN_CASES = (
    (H4, {}),                                     # k_generate<3, G>
    (F7, {}),                                     # k_generate_fw<4, G>
    (F7, {"GCR_GEN_WIDEN": "0"}),                 # k_generate_f<G>
    (F7, {"GCR_GEN_G": "1"}),
    (F7, {"GCR_GEN_G": "16"}),
    (F7, {"GCR_GEN_G": "64"}),
    (H4, {"GCR_GEN_G": "64"}),
    (F7, {"GCR_GUIDED_FLAT": "1"}),               # the A/B knob: one bucket, a flat search
)


@pytest.mark.parametrize("n", (257, 10007))
@pytest.mark.parametrize("solver, env", GEN_CASES)
def test_guided_generator_equals_host_sampler_and_solver(solver, env, n, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)                  # read per launch
    m = M_OF[solver]
    corr, _, w = guided_problem(solver, n)
    nslots = 512
    prob = CorrProblem(solver, corr)
    try:
        N.check(set_probabilities(prob, w))
        inc, models = prob.generate(SEED, 0, nslots)
    finally:
        prob.close()
    inc = inc.reshape(nslots, -1)
    models = models.reshape(nslots, -1, 9)

    def host_models(slot, a):
        rc, idx = G.host_sample_guided(SEED, slot, a, w, m)
        return G.solve_minimal(solver, corr, idx) if rc == 0 else np.zeros((0, 9))

    assert np.all(inc[:, 0] <= 101)               # weights this good: every slot finds a model
    for s in range(nslots):
        a = int(inc[s, 0]) - 1
        want = host_models(s, a)
        k = len(want)
        assert k >= 1, (s, a)
        assert np.array_equal(models[s, :k].view(np.uint64), want.view(np.uint64)), (s, a)
        if solver == F7:                          # inc[3s + q]: 0 the q-th model exists, 255 not
            assert inc[s, 1:].tolist() == [0 if q < k else 255 for q in (1, 2)], (s, a)
        if s < 96:                                # ... and it is the first attempt that gives one
            for b in range(a):
                assert len(host_models(s, b)) == 0, (s, b)


def test_uniform_untouched_after_set_and_clear():
    for solver in (H4, F7):
        corr, _, w = guided_problem(solver, 2000)
        fresh = CorrProblem(solver, corr)
        used = CorrProblem(solver, corr)
        try:
            want = fresh.generate(SEED, 5, 700)
            N.check(set_probabilities(used, w))
            guided = used.generate(SEED, 5, 700)
            N.check(set_probabilities(used, None))
            got = used.generate(SEED, 5, 700)
        finally:
            fresh.close()
            used.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert guided[1].tobytes() != want[1].tobytes()


def test_set_probabilities_errors():
    f = np.abs(np.random.default_rng(1).normal(1.0, 0.2, (50, 3))) + 0.1
    for kind in (N.SOLVER_SCALE3, N.SOLVER_SCALE3_ORIGINAL):
        h = C.c_void_p()
        N.check(N.lib.gcr_problem_create(N.context(0), kind, f.ctypes.data_as(C.POINTER(C.c_double)), 50, None, 0,
                                         C.byref(h)))
        try:
            w = np.ones(50)
            assert N.lib.gcr_problem_set_probabilities(h, w.ctypes.data, 50) == N.GCR_EINVAL
            assert "homography and fundamental" in N.last_error()
            assert N.lib.gcr_problem_set_probabilities(h, None, 0) == N.GCR_EINVAL
        finally:
            N.lib.gcr_problem_destroy(h)
    prob = CorrProblem(H4, random_corr(50))
    try:
        for bad_n in (49, 51):
            assert set_probabilities(prob, np.ones(bad_n)) == N.GCR_EINVAL
            assert "length" in N.last_error()
        one = np.ones(1)
        assert N.lib.gcr_problem_set_probabilities(prob.h, one.ctypes.data, 0) == N.GCR_EINVAL
        w = np.ones(50)
        w[7] = np.nan
        assert set_probabilities(prob, w) == N.GCR_EINVAL
        # a refused vector leaves the problem as it was (uniform)
        got = device_samples(prob, SEED, 0, 64, 0)
        assert np.array_equal(got, G.host_samples_uniform(SEED, 0, 64, 0, 50, 4))
    finally:
        prob.close()
    assert N.lib.gcr_problem_set_probabilities(None, None, 0) == N.GCR_EINVAL


# ------------------------------------------------------------ end to end ----
def e2e_problem(solver):
    if solver == H4:
        corr, truth, _, thr = S.problem_h(n=2000, outlier_ratio=0.95)
    else:
        corr, truth, _, thr = S.problem_f(n=2000, outlier_ratio=0.95)
    return corr, truth, thr, np.where(truth, 1.0, 0.001)


def find(solver, corr, thr, w, seed, batch_slots=0, **kw):
    fn = pygcransac.findHomography if solver == H4 else pygcransac.findFundamentalMatrix
    return fn(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, probabilities=w, threshold=thr, conf=0.99,
              spatial_coherence_weight=0.0, max_iters=32, min_iters=32, sampler=3 if w is not None else 0,
              neighborhood_size=0, seed=seed, batch_slots=batch_slots, return_stats=True, **kw)


def residuals(solver, M, c):
    """per-correspondence residual in pixels: transfer error (H) or Sampson distance (F)"""
    x1 = np.column_stack([c[:, 0], c[:, 1], np.ones(len(c))])
    x2 = np.column_stack([c[:, 2], c[:, 3], np.ones(len(c))])
    if solver == H4:
        p = x1 @ M.T
        return np.hypot(p[:, 0] / p[:, 2] - c[:, 2], p[:, 1] / p[:, 2] - c[:, 3])
    l2 = x1 @ M.T                                 # F x1
    l1 = x2 @ M                                   # F^T x2
    num = np.sum(x2 * l2, axis=1)
    return np.abs(num) / np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)


@pytest.fixture(scope="module")
def e2e_runs():
    """The guided run of each solver and seed, computed once."""
    out = {}
    for solver in (H4, F7):
        corr, truth, thr, w = e2e_problem(solver)
        out[solver] = (corr, truth, thr, w, [find(solver, corr, thr, w, seed) for seed in range(5)])
    return out


def same_run(a, b):
    keys = ("iteration_number", "hypotheses", "score")
    return ((a[0] is None) == (b[0] is None) and (a[0] is None or a[0].tobytes() == b[0].tobytes()) and
            np.array_equal(a[1], b[1]) and all(a[2][k] == b[2][k] for k in keys))


@pytest.mark.parametrize("solver", (H4, F7))
def test_guided_run_meets_a_budget_uniform_sampling_cannot(solver, e2e_runs):
    corr, truth, thr, w, runs = e2e_runs[solver]
    for seed, (M, mask, st) in enumerate(runs):
        assert M is not None, seed
        assert mask[truth].sum() >= 0.9 * truth.sum(), (seed, int(mask[truth].sum()), int(truth.sum()))
        med = float(np.median(residuals(solver, M, corr[truth])))
        print(f"solver {solver} seed {seed}: inliers {int(mask.sum())}, median truth-inlier residual {med:.4f} px")
        assert med < thr, (seed, med)


@pytest.mark.parametrize("solver", (H4, F7))
def test_guided_run_is_deterministic_and_chunk_independent(solver, e2e_runs):
    corr, truth, thr, w, runs = e2e_runs[solver]
    for seed in (0, 3):
        for bs in (0, 64, 4096):
            assert same_run(runs[seed], find(solver, corr, thr, w, seed, batch_slots=bs)), (seed, bs)
        M, masks, st, _ = D.run_problem_sharded(
            solver, corr, params=dict(scale_residual_thresh=thr, confidence=0.99, spatial_coherence_weight=0.0,
                                      min_iteration_number=32, max_iteration_number=32, seed=seed),
            world=1, probabilities=w)
        assert same_run(runs[seed], (M, masks[0], st)), seed


@pytest.mark.parametrize("solver", (H4, F7))
def test_no_stale_speculation_after_set_probabilities(solver, e2e_runs):
    """A uniform run (which may leave a speculative chunk in flight), then
    set_probabilities, then a guided run: the bits of a fresh guided problem."""
    corr, truth, thr, w, _ = e2e_runs[solver]
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.confidence = 0.99
    p.spatial_coherence_weight = 0.0
    p.min_iteration_number = 50
    p.max_iteration_number = 5000
    p.seed = 2

    def run(prob):
        mask = np.zeros(len(corr), dtype=np.uint8)
        M = np.zeros(9)
        st = N.Stats()
        rc = N.check(N.lib.gcr_problem_run(prob.h, C.byref(p), mask.ctypes.data_as(C.POINTER(C.c_uint8)), None,
                                           M.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(st)))
        return rc, M.tobytes(), mask.tobytes(), st.iteration_number, st.hypotheses, st.score

    used, fresh = CorrProblem(solver, corr), CorrProblem(solver, corr)
    try:
        uniform = run(used)
        N.check(set_probabilities(used, w))
        got = run(used)
        N.check(set_probabilities(fresh, w))
        want = run(fresh)
        assert got == want
        assert got != uniform
        # ... and back: cleared, the problem repeats its uniform run
        N.check(set_probabilities(used, None))
        assert run(used) == uniform
    finally:
        used.close()
        fresh.close()
