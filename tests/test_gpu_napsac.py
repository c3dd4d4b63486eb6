"""NAPSAC sampling on the GPU (csrc/napsac.h): the generators' sampling
function and every generator kernel against their host twins bit for bit,
uniform sampling untouched, the C ABI's refusals, and whole runs: a local
structure found within 64 iterations, runs that end by the uniform bound,
determinism across batch_slots, the sharded entry, verify_batches and the graph
cut beside the layers.  Whole-run parity with the oracle's restatement of
NAPSAC is test_gpu_oracle_samplers.py's."""
import ctypes as C

import numpy as np
import pytest

import essential_cases as EC
import gravity_cases as GC
import napsac_cases as NC
import guided_cases as G
import pygcransac
import sift_homography_cases as SC
from gcr_testutil import CorrProblem
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S
from test_gpu_guided import same_run

pytestmark = pytest.mark.gpu

H4, F7, E5, G3, S2 = NC.H4, NC.F7, NC.E5, NC.G3, NC.S2
SEED = 0x5EEDFACE12345678
T_SMALL = 1000
SIZE = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)
K_PLAIN = np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 480.0], [0.0, 0.0, 1.0]])


def set_napsac(prob, T, extent=NC.EXTENT):
    return N.lib.gcr_problem_set_napsac(prob.h, (C.c_double * 4)(*[float(v) for v in extent]), T)


def device_samples(prob, m, seed, slot0, nslots, attempt):
    out = np.zeros((nslots, m), dtype=np.uint32)
    N.check(N.lib.gcr_debug_sample_h(prob.h, seed, slot0, nslots, attempt, out.ctypes.data_as(NC.u32p)))
    return out


def generate(prob, per, seed, slot0, nslots):
    """inc (nslots, per) bytes, models (nslots, per, 9)"""
    inc = np.zeros(nslots * per, dtype=np.uint8)
    H = np.zeros((nslots * per, 9))
    N.check(N.lib.gcr_debug_generate_h(prob.h, seed, slot0, nslots, inc.ctypes.data_as(NC.u8p),
                                       H.ctypes.data_as(NC.dpt)))
    return inc.reshape(nslots, per), H.reshape(nslots, per, 9)


def random_problem(solver, n, seed=3):
    """(problem, pixel rows): any rows, the sampling function reads their positions alone"""
    rng = np.random.default_rng(seed)
    corr = rng.uniform(0.0, 900.0, (n, 4))
    if solver in (H4, F7):
        return CorrProblem(solver, corr), corr
    if solver == E5:
        return EC.EssProblem(corr, K_PLAIN, K_PLAIN), corr
    if solver == G3:
        return GC.GravProblem(corr, K_PLAIN, K_PLAIN, np.eye(3), np.eye(3)), corr
    sift = np.column_stack([rng.uniform(1.0, 9.0, (n, 2)), rng.uniform(-3.0, 3.0, (n, 2))])
    return SC.HProblem(np.column_stack([corr, sift])), corr


def scene_problem(solver, n, seed=21):
    """(problem, the host twin's keyword arguments): a scene of the solver with
    a few duplicated rows, so that samples fail and slots retry"""
    def dup(rows):
        rows = rows.copy()
        rows[5:9] = rows[4]
        rows[40:42] = rows[39]
        return np.ascontiguousarray(rows)

    if solver in (H4, F7):
        corr = dup((S.problem_h if solver == H4 else S.problem_f)(n, seed=seed)[0])
        return CorrProblem(solver, corr), dict(rows=corr)
    if solver == E5:
        corr, _, K, _, thr = S.problem_e(n, seed=seed)
        corr = dup(corr)
        return EC.EssProblem(corr, K, K), dict(rows=EC.normalise(corr, K, K, thr)[0], pixels=corr)
    if solver == G3:
        corr, _, K, G1, G2, _ = S.problem_g(n, seed=seed)
        corr = dup(corr)
        return GC.GravProblem(corr, K, K, G1, G2), dict(rows=EC.normalise(corr, K, K, 1.0)[0], pixels=corr, G1=G1, G2=G2)
    rows8 = dup(S.problem_hs(n, seed=seed)[0])
    return SC.HProblem(rows8), dict(rows=rows8[:, :4], sift=rows8[:, 4:8])


# ------------------------------------------------ device sampler == host ----
@pytest.mark.parametrize("solver", NC.SOLVERS)
def test_device_sampler_equals_host_sampler(solver):
    m = NC.M_OF[solver]
    for n in (m, 257):
        prob, rows = random_problem(solver, n)
        try:
            cases = [(T_SMALL, s0) for s0 in (0, 200, T_SMALL - 100)] + [(1 << 40, (1 << 32) - 100)]
            for T, slot0 in cases:
                N.check(set_napsac(prob, T))
                for a in (0, 100):
                    got = device_samples(prob, m, SEED, slot0, 2048, a)
                    want = NC.host_samples(SEED, slot0, 2048, a, rows, m, NC.EXTENT, T)
                    assert np.array_equal(got, want), (solver, n, T, slot0, a)
                    assert np.all(got != NC.ALL_ONES)
            # cleared: the same hook draws philox.h's uniform samples
            N.check(set_napsac(prob, 0))
            got = device_samples(prob, m, SEED, 0, 2048, 0)
            assert np.array_equal(got, G.host_samples_uniform(SEED, 0, 2048, 0, n, m)), (solver, n)
        finally:
            prob.close()


# ------------------------------------------------------------ generators ----
# every generator kernel: k_generate<3>, k_generate_fw<4>, k_generate_e / _g / _s at the default lanes per slot, 1
# and 64; the fixed-group k_generate_f and the widening homography generator k_generate_fw<3> behind their knobs
GEN_CASES = tuple((solver, env) for solver in NC.SOLVERS for env in ({}, {"GCR_GEN_G": "1"}, {"GCR_GEN_G": "64"})) + \
    ((F7, {"GCR_GEN_WIDEN": "0"}), (H4, {"GCR_GEN_HWIDEN": "1"}))


@pytest.mark.parametrize("solver, env", GEN_CASES)
def test_generator_equals_its_host_twin(solver, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)                      # read per launch
    n, nslots, per = 257, 512, NC.PER_OF[solver]
    prob, host = scene_problem(solver, n)
    fresh, _ = scene_problem(solver, n)
    try:
        N.check(set_napsac(prob, T_SMALL))
        retries = 0
        for slot0 in (0, T_SMALL - 256):              # the first quarter boundary; the last one and T
            inc, models = generate(prob, per, SEED, slot0, nslots)
            want_inc, want_models = NC.host_generate(solver, extent=NC.EXTENT, T=T_SMALL, seed=SEED, slot0=slot0,
                                                     nslots=nslots, **host)
            assert inc.tobytes() == want_inc.tobytes(), (solver, slot0, np.flatnonzero((inc != want_inc).any(axis=1))[:8])
            assert models.tobytes() == want_models.tobytes(), (solver, slot0)
            retries += int((inc[:, 0] > 1).sum())
        assert retries > 0
        # past T: the uniform generator's own bytes
        uniform = generate(fresh, per, SEED, T_SMALL, 256)
        assert inc[256:].tobytes() == uniform[0].tobytes() and models[256:].tobytes() == uniform[1].tobytes()
        local = generate(fresh, per, SEED, T_SMALL - 256, 256)
        assert models[:256].tobytes() != local[1].tobytes()
    finally:
        prob.close()
        fresh.close()


def test_uniform_again_after_clearing():
    for solver in NC.SOLVERS:
        fresh, _ = scene_problem(solver, 300)
        used, _ = scene_problem(solver, 300)
        per = NC.PER_OF[solver]
        try:
            want = generate(fresh, per, SEED, 5, 300)
            N.check(set_napsac(used, 1 << 20))
            local = generate(used, per, SEED, 5, 300)
            N.check(set_napsac(used, 0))
            got = generate(used, per, SEED, 5, 300)
        finally:
            fresh.close()
            used.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert local[1].tobytes() != want[1].tobytes()


# ------------------------------------------------------------------- errors ----
def test_set_napsac_errors():
    f = np.abs(np.random.default_rng(1).normal(1.0, 0.2, (50, 3))) + 0.1
    ext = (C.c_double * 4)(*NC.EXTENT)
    for kind in (N.SOLVER_SCALE3, N.SOLVER_SCALE3_ORIGINAL):
        h = C.c_void_p()
        N.check(N.lib.gcr_problem_create(N.context(0), kind, f.ctypes.data_as(NC.dpt), 50, None, 0, C.byref(h)))
        try:
            assert N.lib.gcr_problem_set_napsac(h, ext, 1000) == N.GCR_EINVAL
            assert "correspondence problems only" in N.last_error()
        finally:
            N.lib.gcr_problem_destroy(h)
    n, m = 50, 4
    rows = np.random.default_rng(3).uniform(0.0, 900.0, (n, 4))
    prob = CorrProblem(H4, rows)
    try:
        N.check(set_napsac(prob, T_SMALL))
        want = NC.host_samples(SEED, 0, 64, 0, rows, m, NC.EXTENT, T_SMALL)
        assert not np.array_equal(want, G.host_samples_uniform(SEED, 0, 64, 0, n, m))
        # each refused call leaves the problem as it was
        assert set_napsac(prob, (1 << 40) + 1) == N.GCR_EINVAL and "2^40" in N.last_error()
        for bad in ((0.0, 1, 1, 1), (1, -2.0, 1, 1), (1, 1, float("nan"), 1), (1, 1, 1, float("inf"))):
            assert set_napsac(prob, T_SMALL, bad) == N.GCR_EINVAL and "extent" in N.last_error()
        assert N.lib.gcr_problem_set_napsac(prob.h, None, T_SMALL) == N.GCR_EINVAL
        w = np.ones(n)
        assert N.lib.gcr_problem_set_probabilities(prob.h, w.ctypes.data, n) == N.GCR_EINVAL
        assert "NAPSAC" in N.last_error()
        assert N.lib.gcr_problem_set_prosac(prob.h, 1000) == N.GCR_EINVAL and "NAPSAC" in N.last_error()
        assert np.array_equal(device_samples(prob, m, SEED, 0, 64, 0), want)
        # neither sampler's own stop applies
        mask, M = np.zeros(n, dtype=np.uint8), np.zeros(9)
        for flag in (N.FLAG_GUIDED_STOP, N.FLAG_PROSAC_STOP):
            p = N.default_params()
            p.flags = flag
            assert N.lib.gcr_problem_run(prob.h, C.byref(p), mask.ctypes.data_as(NC.u8p), None,
                                         M.ctypes.data_as(NC.dpt), None, None) == N.GCR_EINVAL
            assert "NAPSAC" in N.last_error()
        # clearing another sampler on a NAPSAC problem is fine
        N.check(N.lib.gcr_problem_set_probabilities(prob.h, None, 0))
        N.check(N.lib.gcr_problem_set_prosac(prob.h, 0))
        assert np.array_equal(device_samples(prob, m, SEED, 0, 64, 0), want)
        N.check(set_napsac(prob, 0))
        # ... and NAPSAC on a guided or PROSAC problem is refused: it stays what it was
        N.check(N.lib.gcr_problem_set_probabilities(prob.h, w.ctypes.data, n))
        guided = device_samples(prob, m, SEED, 0, 64, 0)
        assert set_napsac(prob, T_SMALL) == N.GCR_EINVAL and "probabilities" in N.last_error()
        assert np.array_equal(device_samples(prob, m, SEED, 0, 64, 0), guided)
        N.check(N.lib.gcr_problem_set_probabilities(prob.h, None, 0))
        N.check(N.lib.gcr_problem_set_prosac(prob.h, 1000))
        prosac = device_samples(prob, m, SEED, 0, 64, 0)
        assert set_napsac(prob, T_SMALL) == N.GCR_EINVAL and "PROSAC" in N.last_error()
        assert np.array_equal(device_samples(prob, m, SEED, 0, 64, 0), prosac)
    finally:
        prob.close()


# ------------------------------------------------------------ whole runs ----
def find_h(corr, thr, seed, sampler, max_iters, min_iters, batch_slots=0, lam=0.0, cells=0, T=None):
    return pygcransac.findHomography(corr, *SIZE, threshold=thr, conf=0.99, spatial_coherence_weight=lam,
                                     max_iters=max_iters, min_iters=min_iters, sampler=sampler, neighborhood_size=cells,
                                     seed=seed, batch_slots=batch_slots, return_stats=True, napsac_iterations=T)


@pytest.fixture(scope="module")
def local_runs():
    """seed -> (corr, truth, thr, NAPSAC run of 64 iterations, converged uniform run, uniform run of 64 iterations)"""
    out = {}
    for seed in NC.E2E_SEEDS:
        corr, truth, thr = NC.e2e_problem(seed)
        out[seed] = (corr, truth, thr, find_h(corr, thr, seed, 2, NC.E2E_BUDGET, NC.E2E_BUDGET),
                     find_h(corr, thr, seed, 0, 10 ** 6, 50), find_h(corr, thr, seed, 0, NC.E2E_BUDGET, NC.E2E_BUDGET))
    return out


def test_local_structure_found_within_64_iterations(local_runs):
    """problem_h_local(2000, 0.9): 200 inliers in a quarter x quarter window.
    Truth inliers found on an MI355X, seeds 0..4 -- NAPSAC in 64 iterations /
    uniform to 0.99 / uniform in 64 iterations: see MEASUREMENTS.md."""
    for seed, (corr, truth, thr, napsac, converged, short) in local_runs.items():
        k = int(truth.sum())
        found = [int(r[1][truth].sum()) if r[0] is not None else 0 for r in (napsac, converged, short)]
        print(f"seed {seed}: truth inliers found of {k}: NAPSAC in {napsac[2]['iteration_number']} iterations "
              f"{found[0]}, uniform to 0.99 ({converged[2]['iteration_number']} iterations) {found[1]}, uniform in "
              f"{short[2]['iteration_number']} iterations {found[2]}")
        assert napsac[0] is not None, seed
        assert found[0] >= found[1] - 0.05 * k, (seed, found)


CONVERGED = ((F7, S.problem_f), (H4, S.problem_h))


@pytest.fixture(scope="module")
def short_local_runs():
    """solver -> (corr, truth, keywords, NAPSAC run with a local phase of 200 slots, uniform run), both to 0.99"""
    out = {}
    for solver, make in CONVERGED:
        corr, truth, _, thr = make(2000, 0.5, seed=17)
        fn = pygcransac.findHomography if solver == H4 else pygcransac.findFundamentalMatrix
        kw = dict(threshold=thr, conf=0.99, spatial_coherence_weight=0.0, max_iters=10 ** 6, min_iters=50,
                  neighborhood_size=0, seed=4, return_stats=True)
        out[solver] = (corr, truth, fn, kw, fn(corr, *SIZE, sampler=2, napsac_iterations=200, **kw),
                       fn(corr, *SIZE, sampler=0, **kw))
    return out


@pytest.mark.parametrize("solver", (F7, H4))
def test_run_with_a_short_local_phase_ends_by_the_uniform_bound(solver, short_local_runs):
    """problem_f / problem_h (2000, 0.5), napsac_iterations = 200, to 0.99:
    the run ends by the stop, not by max_iters, and finds what the uniform run
    finds.  Only the F run gets past the local phase."""
    corr, truth, fn, kw, napsac, uniform = short_local_runs[solver]
    k = int(truth.sum())
    found = [int(r[1][truth].sum()) if r[0] is not None else 0 for r in (napsac, uniform)]
    print(f"solver {solver}: truth inliers found of {k}: NAPSAC (200 local slots) {found[0]} in "
          f"{napsac[2]['iteration_number']} iterations, uniform {found[1]} in {uniform[2]['iteration_number']}")
    assert napsac[0] is not None
    assert 50 <= napsac[2]["iteration_number"] < 10 ** 6
    if solver == F7:
        # the bound at half inliers is log(0.01) / log(1 - 2^-7) = 587 iterations: the run crosses T = 200 and ends
        # in the uniform phase.  (The homography's is 72: that run ends inside the local phase, by the same bound.)
        assert napsac[2]["iteration_number"] > 200
    assert found[0] >= found[1] - 0.05 * k, found


def test_runs_are_deterministic_and_chunk_independent(local_runs, short_local_runs):
    for seed in NC.E2E_SEEDS:
        corr, truth, thr, napsac = local_runs[seed][:4]
        for bs in (0, 64, 1000):
            assert same_run(napsac, find_h(corr, thr, seed, 2, NC.E2E_BUDGET, NC.E2E_BUDGET, batch_slots=bs)), (seed, bs)
    for solver, _ in CONVERGED:
        corr, truth, fn, kw, napsac, _ = short_local_runs[solver]
        for bs in (0, 64, 1000):
            assert same_run(napsac, fn(corr, *SIZE, sampler=2, napsac_iterations=200, batch_slots=bs, **kw)), (solver, bs)


def test_sharded_run_of_one_rank_equals_the_plain_run(local_runs, short_local_runs):
    seed = NC.E2E_SEEDS[0]
    corr, truth, thr, napsac = local_runs[seed][:4]
    M, masks, st, _ = D.run_problem_sharded(
        H4, corr, params=dict(scale_residual_thresh=thr, confidence=0.99, spatial_coherence_weight=0.0,
                              min_iteration_number=NC.E2E_BUDGET, max_iteration_number=NC.E2E_BUDGET, seed=seed),
        world=1, napsac=(NC.EXTENT, NC.e2e_iterations()))
    assert same_run(napsac, (M, masks[0].astype(bool), st))
    corr, truth, fn, kw, napsac, _ = short_local_runs[F7]
    M, masks, st, _ = D.run_problem_sharded(
        F7, corr, params=dict(scale_residual_thresh=kw["threshold"], confidence=0.99, spatial_coherence_weight=0.0,
                              min_iteration_number=50, max_iteration_number=10 ** 6, seed=kw["seed"]),
        world=1, napsac=(NC.EXTENT, 200))
    assert same_run(napsac, (M, masks[0].astype(bool), st))


def test_verify_batches_score_the_napsac_generators_models():
    """2 batches of 300 slots of a NAPSAC problem: the live count, and the first
    maximum of the MSAC score with its inlier count, from scoring that batch's
    generate output one model at a time."""
    corr, truth, thr = NC.e2e_problem(1)
    rows8 = np.column_stack([corr, np.ones((len(corr), 4))])
    ps, ph = SC.HProblem(rows8, sift=False), SC.HProblem(rows8, sift=False)
    nslots = 300
    try:
        N.check(set_napsac(ps, 500))                     # the second batch crosses into the uniform phase
        res = ps.verify_batches(thr, SEED, 0, nslots, 2)
        T = (2.25 * thr) * thr
        for b in range(2):
            inc, models = ps.generate(SEED, b * nslots, nslots)
            live = inc.reshape(-1) <= 101
            assert res[b].models == live.sum() and 0 < live.sum()
            assert res[b].iterations == np.where(inc <= 102, inc, 0).sum()
            n0, v0, tot = ph.score(models.reshape(-1, 9), thr)
            msac = np.where(live & (n0 >= 2), v0 / T + n0, 0.0)
            j = int(np.argmax(msac))                     # the first maximum
            assert res[b].best_slot == b * nslots + j
            assert res[b].best_score == msac[j] and res[b].best_inliers[0] == n0[j]
    finally:
        ps.close()
        ph.close()


def test_graph_cut_runs_beside_the_layers(local_runs):
    seed = NC.E2E_SEEDS[0]
    corr, truth, thr = local_runs[seed][:3]
    M, mask, st = find_h(corr, thr, seed, 2, 5000, 50, lam=0.3, cells=8)
    assert M is not None and st["graph_cut_number"] > 0
    assert same_run((M, mask, st), find_h(corr, thr, seed, 2, 5000, 50, lam=0.3, cells=8, batch_slots=64))


def test_essential_gravity_and_sift_homography_calls():
    def check(M, mask, truth):
        assert M is not None and mask.shape == truth.shape and mask.dtype == bool
        hit = int((mask & truth).sum())
        assert hit >= 0.9 * int(truth.sum()) and hit >= 0.9 * int(mask.sum()), (hit, int(truth.sum()), int(mask.sum()))

    kw = dict(conf=0.99, spatial_coherence_weight=0.0, max_iters=5000, min_iters=50, sampler=2, neighborhood_size=0)
    c, truth, K, _, thr = S.problem_e(2000, 0.5, seed=11)
    check(*pygcransac.findEssentialMatrix(c, K, K, *SIZE, threshold=thr, seed=5, **kw), truth)
    c, truth, K, G1, G2, _ = S.problem_g(2000, 0.5, seed=12)
    check(*pygcransac.findGravityEssentialMatrix(c, K, K, G1, G2, *SIZE, threshold=1.0, seed=6, **kw), truth)
    c, truth, _, thr = S.problem_hs(2000, 0.5, seed=13)
    check(*pygcransac.findHomographySIFT(c, *SIZE, threshold=thr, seed=7, napsac_iterations=300, **kw), truth)
