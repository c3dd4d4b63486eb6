"""The guided stop (GCR_FLAG_GUIDED_STOP, csrc/guided_stop.h) on the GPU: the
mass kernel against the scorer, the mask kernel and the host quanta; the
uniform stop under equal weights; early stops under informative weights; the
same run on every replay path; refusals."""
import ctypes as C

import numpy as np
import pytest

import guided_cases as G
import pygcransac
from gcr_testutil import CorrProblem, dp
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

H4, F7 = N.SOLVER_HOMOGRAPHY4, N.SOLVER_FUNDAMENTAL7
M_OF = {H4: 4, F7: 7}
SEED = 0x5EEDFACE12345678
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def set_probabilities(prob, w):
    if w is None:
        return N.lib.gcr_problem_set_probabilities(prob.h, None, 0)
    w = np.ascontiguousarray(w, dtype=np.float64)
    return N.lib.gcr_problem_set_probabilities(prob.h, w.ctypes.data, len(w))


def residuals(solver, M, c):
    """per-correspondence residual in pixels: transfer error (H) or Sampson
    distance (F), as tests/test_gpu_guided.py measures it"""
    x1 = np.column_stack([c[:, 0], c[:, 1], np.ones(len(c))])
    x2 = np.column_stack([c[:, 2], c[:, 3], np.ones(len(c))])
    if solver == H4:
        p = x1 @ M.T
        return np.hypot(p[:, 0] / p[:, 2] - c[:, 2], p[:, 1] / p[:, 2] - c[:, 3])
    l2 = x1 @ M.T                                 # F x1
    l1 = x2 @ M                                   # F^T x2
    num = np.sum(x2 * l2, axis=1)
    return np.abs(num) / np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)


def same_run(a, b):
    """identical model bytes, masks, iteration_number, hypotheses and score"""
    keys = ("iteration_number", "hypotheses", "score")
    return ((a[0] is None) == (b[0] is None) and (a[0] is None or a[0].tobytes() == b[0].tobytes()) and
            np.array_equal(a[1], b[1]) and all(a[2][k] == b[2][k] for k in keys))


def inlier_mass(prob, models, thr):
    """gcr_debug_inlier_mass_h: (count, mass) per model."""
    models = np.ascontiguousarray(models, dtype=np.float64)
    p = N.default_params()
    p.scale_residual_thresh = thr
    count = np.zeros(len(models), dtype=np.uint32)
    mass = np.zeros(len(models), dtype=np.uint64)
    N.check(N.lib.gcr_debug_inlier_mass_h(prob.h, C.byref(p), dp(models), len(models), count.ctypes.data_as(u32p),
                                          mass.ctypes.data_as(u64p)))
    return count, mass


def host_quanta(w, m):
    w = np.ascontiguousarray(w, dtype=np.float64)
    q = np.zeros(len(w), dtype=np.uint64)
    Q = C.c_uint64()
    N.check(N.lib.gcr_host_guided_quanta(w.ctypes.data, len(w), m, q.ctypes.data_as(u64p), C.byref(Q)))
    return q, Q.value


# ------------------------------------------------------ kernel == host ----
@pytest.mark.parametrize("n", G.NS)
@pytest.mark.parametrize("solver", (H4, F7))
def test_mass_kernel_equals_scorer_and_host_quanta(solver, n):
    m = M_OF[solver]
    corr, truth, _, thr = (S.problem_h if solver == H4 else S.problem_f)(n, 0.5, seed=21)
    prob = CorrProblem(solver, corr)
    try:
        # the first 33 hypotheses the generator leaves (a slot without a model
        # leaves the default one: it has to count like any other)
        _, models = prob.generate(SEED, 0, 33)
        models = np.ascontiguousarray(models.reshape(-1, 9)[:33])
        masks = np.array([prob.mask(mod, 0, thr) for mod in models])
        n0 = prob.score(models, thr)[0]
        assert np.array_equal(n0, masks.sum(axis=1))
        if n >= 255:
            assert n0.max() > m                       # some hypothesis has inliers beyond its sample
        # without probabilities there is no mass
        p = N.default_params()
        p.scale_residual_thresh = thr
        cnt1, mass1 = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
        assert N.lib.gcr_debug_inlier_mass_h(prob.h, C.byref(p), dp(models), 1, cnt1.ctypes.data_as(u32p),
                                             mass1.ctypes.data_as(u64p)) == N.GCR_EINVAL
        for pattern in ("ones", "zero_runs", "heavy90", "loguniform"):
            w = G.weights(pattern, n, m)
            if int((w > 0).sum()) < m:                # zero_runs at n = 7 leaves 4 positive weights
                assert set_probabilities(prob, w) == N.GCR_EINVAL
                continue
            N.check(set_probabilities(prob, w))
            q, Q = host_quanta(w, m)
            want = np.array([int(q[mk].sum(dtype=np.uint64)) for mk in masks], dtype=np.uint64)
            assert int(want.max()) <= Q < 2 ** 52
            for nm in (1, 33):
                count, mass = inlier_mass(prob, models[:nm], thr)
                assert np.array_equal(count, n0[:nm]), (pattern, nm)
                assert np.array_equal(mass, want[:nm]), (pattern, nm)
    finally:
        prob.close()


# ----------------------------------------------------------- end to end ----
def find(solver, corr, thr, w, seed, guided_stop, batch_slots=0):
    fn = pygcransac.findHomography if solver == H4 else pygcransac.findFundamentalMatrix
    return fn(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, probabilities=w, threshold=thr, conf=0.99,
              spatial_coherence_weight=0.0, max_iters=5000, min_iters=50, sampler=3, neighborhood_size=0, seed=seed,
              batch_slots=batch_slots, return_stats=True, guided_stop=guided_stop)


@pytest.mark.parametrize("solver", (H4, F7))
def test_equal_weights_give_the_uniform_stop(solver):
    corr, truth, _, thr = (S.problem_h if solver == H4 else S.problem_f)(2000, 0.5)
    w = np.ones(len(corr))
    for seed in range(5):
        clear = find(solver, corr, thr, w, seed, False)
        flagged = find(solver, corr, thr, w, seed, True)
        assert clear[0] is not None
        assert clear[2]["iteration_number"] < 5000, seed      # the adaptive stop ended the run, not the budget
        assert same_run(clear, flagged), (seed, clear[2]["iteration_number"], flagged[2]["iteration_number"])


# H: at 80 % outliers the uniform bound (2876 at m = 4) is below max_iters, so
# the flag-clear run would stop by itself; at 85 % it is 9.1e3 (6.2e3 with 10 %
# chance inliers on top): tests/test_guided_stop.py restates the arithmetic.
OUTLIERS = {H4: 0.85, F7: 0.8}


def informative_problem(solver):
    corr, truth, _, thr = (S.problem_h if solver == H4 else S.problem_f)(n=2000, outlier_ratio=OUTLIERS[solver])
    return corr, truth, thr, np.where(truth, 1.0, 0.05)


@pytest.fixture(scope="module")
def informative_runs():
    """Each solver's flag-set runs (seeds 0..4), computed once."""
    out = {}
    for solver in (H4, F7):
        corr, truth, thr, w = informative_problem(solver)
        out[solver] = (corr, truth, thr, w, [find(solver, corr, thr, w, seed, True) for seed in range(5)])
    return out


@pytest.mark.parametrize("solver", (H4, F7))
def test_informative_weights_stop_early_and_lose_nothing(solver, informative_runs):
    corr, truth, thr, w, runs = informative_runs[solver]
    for seed, (M, mask, st) in enumerate(runs):
        clear = find(solver, corr, thr, w, seed, False)
        # flag clear: the uniform bound never ends the run, the budget does.  An
        # iteration is one sampling attempt and the loop tests the budget
        # between slots, so the count is the first one >= max_iters (a slot
        # adds its attempts, at most 102), not max_iters itself.
        assert 5000 <= clear[2]["iteration_number"] < 5000 + 102, (seed, clear[2]["iteration_number"])
        found = int(mask[truth].sum())
        med = float(np.median(residuals(solver, M, corr[truth]))) if M is not None else float("nan")
        print(f"solver {solver} seed {seed}: stop at {st['iteration_number']} (flag clear "
              f"{clear[2]['iteration_number']}), truth inliers "
              f"{found} / {int(truth.sum())}, median truth-inlier residual {med:.4f} px")
        assert M is not None, seed
        assert st["iteration_number"] <= 500, (seed, st["iteration_number"])
        assert found >= 0.9 * truth.sum(), (seed, found, int(truth.sum()))
        assert med < thr, (seed, med)


@pytest.mark.parametrize("solver", (H4, F7))
def test_flagged_run_is_the_same_on_every_path(solver, informative_runs, monkeypatch):
    corr, truth, thr, w, runs = informative_runs[solver]
    params = dict(scale_residual_thresh=thr, confidence=0.99, spatial_coherence_weight=0.0, min_iteration_number=50,
                  max_iteration_number=5000, flags=N.FLAG_GUIDED_STOP)
    for seed in (0, 3):
        for bs in (0, 64, 4096):
            assert same_run(runs[seed], find(solver, corr, thr, w, seed, True, batch_slots=bs)), (seed, bs)
        M, masks, st, _ = D.run_problem_sharded(solver, corr, params=dict(params, seed=seed), world=1,
                                                probabilities=w)
        assert same_run(runs[seed], (M, masks[0], st)), seed
        # ... and GCR_ZEROCOPY=0: the mass launches' staged copies instead of pinned reads and writes
        for env in ({"GCR_REPLAY": "slots"}, {"GCR_SPEC_TRIM": "0"}, {"GCR_SPECULATE": "0"}, {"GCR_PREFETCH": "0"},
                    {"GCR_ZEROCOPY": "0"}, {"GCR_REPLAY": "slots", "GCR_ZEROCOPY": "0"}):
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)                   # read per run
                assert same_run(runs[seed], find(solver, corr, thr, w, seed, True)), (seed, env)


# ------------------------------------------------------------- refusals ----
def run_flagged(handle, n, thr, k2=False):
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.spatial_coherence_weight = 0.0
    p.min_iteration_number = 50
    p.max_iteration_number = 200
    p.flags = N.FLAG_GUIDED_STOP
    mask = np.zeros(n, dtype=np.uint8)
    M = np.zeros(9)
    model = N.RectModel()
    st = N.Stats()
    return N.lib.gcr_problem_run(handle, C.byref(p), mask.ctypes.data_as(C.POINTER(C.c_uint8)), None, dp(M),
                                 C.byref(model), C.byref(st))


def test_refusals():
    corr, truth, _, thr = S.problem_h(300, 0.5, seed=4)
    prob = CorrProblem(H4, corr)
    try:
        assert run_flagged(prob.h, len(corr), thr) == N.GCR_EINVAL          # no probabilities
        assert "guided sampling" in N.last_error()
        N.check(set_probabilities(prob, np.where(truth, 1.0, 0.05)))
        assert run_flagged(prob.h, len(corr), thr) > 0                      # accepted: an inlier count
        N.check(set_probabilities(prob, None))
        assert run_flagged(prob.h, len(corr), thr) == N.GCR_EINVAL          # cleared: refused again
        assert "guided sampling" in N.last_error()
    finally:
        prob.close()
    f, _, rthr = S.problem_m1(200, seed=7)
    f = np.ascontiguousarray(f, dtype=np.float64)
    h = C.c_void_p()
    N.check(N.lib.gcr_problem_create(N.context(0), N.SOLVER_SCALE3, dp(f), len(f), None, 0, C.byref(h)))
    try:
        assert run_flagged(h, len(f), rthr) == N.GCR_EINVAL                 # a rectification problem
        assert "guided sampling" in N.last_error()
    finally:
        N.lib.gcr_problem_destroy(h)
    # the one-shot entries without probabilities, gcr_solve_batch's items among them
    p = N.default_params()
    p.scale_residual_thresh = thr
    p.flags = N.FLAG_GUIDED_STOP
    mask = np.zeros(len(corr), dtype=np.uint8)
    M = np.zeros(9)
    st = N.Stats()
    c = np.ascontiguousarray(corr)
    assert N.lib.gcr_find_homography(N.context(0), c.ctypes.data, len(c), C.byref(p), mask.ctypes.data,
                                     M.ctypes.data, C.byref(st)) == N.GCR_EINVAL
    assert "guided sampling" in N.last_error()
    item = (N.BatchItem * 1)()
    item[0].solver = H4
    item[0].f0 = dp(c)
    item[0].n0 = len(c)
    item[0].params = p
    item[0].mask0_out = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    assert N.lib.gcr_solve_batch(0, item, 1, 1) == N.GCR_EINVAL
    assert item[0].result == N.GCR_EINVAL and "guided sampling" in N.last_error()
