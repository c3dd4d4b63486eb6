"""Essential matrix with known gravity on the GPU: the sampler and the generator
kernel against their host twins bit for bit, the scorers against a plain
essential problem over the same rows, the pixel neighbourhood grid, whole
runs beside findEssentialMatrix, the guided stop, the sharded entry."""
import ctypes as C

import numpy as np
import pytest

import essential_cases as EC
import gravity_cases as GC
import guided_cases as G
import pygcransac
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

SEED = 0x5EEDFACE12345678
SIZE = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)
DEFAULT = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])


def small_problem(n):
    """n rows of problem_g: three quarters inliers; at n = 257 five rows are
    copies of another, so samples holding two of them have no model.  At n = 3
    the only sample is the three (noisy) inliers in some order."""
    corr, truth, K, G1, G2, _ = S.problem_g(max(4 * n, 40), 0.25, seed=41)
    rows = np.ascontiguousarray(np.concatenate([corr[truth][:n - n // 4], corr[~truth][:n // 4]]))
    assert len(rows) == n
    if n > 30:
        for i in (7, 11, 17, 22, 28):
            rows[i] = rows[3]
    w = np.concatenate([np.ones(n - n // 4), np.full(n // 4, 0.05)])
    return rows, K, G1, G2, w


@pytest.mark.parametrize("n", (3, 257))
def test_device_sampler_equals_host_sampler(n):
    rows, K, G1, G2, w = small_problem(n)
    prob = GC.GravProblem(rows, K, K, G1, G2)
    try:
        for slot0 in (0, 1 << 40):
            for a in (0, 100):
                got = prob.sample(SEED, slot0, 2048, a)
                assert np.array_equal(got, G.host_samples_uniform(SEED, slot0, 2048, a, n, 3)), (n, slot0, a)
        prob.set_probabilities(w)
        for slot0 in (0, 1 << 40):
            for a in (0, 100):
                got = prob.sample(SEED, slot0, 2048, a)
                assert np.array_equal(got, G.host_samples(SEED, slot0, 2048, a, w, 3)), (n, slot0, a)
                ok = got[:, 0] != G.ALL_ONES
                assert ok.any() and np.all(np.sort(got[ok], axis=1)[:, :-1] != np.sort(got[ok], axis=1)[:, 1:])
    finally:
        prob.close()


@pytest.mark.parametrize("gen_g", (None, "1", "64"), ids=("default", "G1", "G64"))
@pytest.mark.parametrize("guided", (False, True), ids=("uniform", "guided"))
@pytest.mark.parametrize("n", (3, 257))
def test_generator_equals_the_host_twin_bitwise(n, guided, gen_g, monkeypatch):
    if gen_g is None:
        monkeypatch.delenv("GCR_GEN_G", raising=False)
    else:
        monkeypatch.setenv("GCR_GEN_G", gen_g)
    rows, K, G1, G2, w = small_problem(n)
    nslots, slot0 = 512, 2 ** 32 - 100              # crosses the 32-bit counter word
    norm, _ = EC.normalise(rows, K, K, 1.0)
    prob = GC.GravProblem(rows, K, K, G1, G2)
    try:
        if guided:
            prob.set_probabilities(w)
        inc, models = prob.generate(SEED, slot0, nslots)
        hinc, hmodels = GC.host_generate(norm, G1, G2, w if guided else None, SEED, slot0, nslots)
        assert np.array_equal(inc, hinc)
        assert np.array_equal(models.view(np.uint64), hmodels.view(np.uint64))
        # the layout: the first byte counts attempts, the others flag the extra models, the rest is the default
        won = inc[:, 0] <= 101
        assert ((inc[:, 1:] == 0) | (inc[:, 1:] == 255)).all() and (inc[~won] == [102, 255, 255, 255]).all()
        live = np.column_stack([won, inc[:, 1:] == 0])
        assert (np.diff(live.astype(int), axis=1) <= 0).all()            # packed to the front
        assert np.array_equal(models[~live], np.tile(DEFAULT, ((~live).sum(), 1)))
        assert np.all(np.isfinite(models))
        # the first 96 slots, attempt by attempt: the device's samples through the host solver; no earlier
        # attempt yields a model, the winning one yields exactly the slot's models
        last = np.where(won, inc[:, 0], 101)[:96].astype(int)
        for a in range(int(last.max())):
            idx = prob.sample(SEED, slot0, 96, a)
            for s in np.flatnonzero(a < last):
                got = GC.solve_g3(norm, G1, G2, idx[s]) if idx[s, 0] != G.ALL_ONES else np.zeros((0, 9))
                if a < last[s] - 1 or not won[s]:
                    assert len(got) == 0, (s, a)
                else:
                    assert len(got) == live[s].sum()
                    assert np.array_equal(got.view(np.uint64), models[s, :len(got)].view(np.uint64))
        if n == 257:
            # the case is hard enough: retries and many-model slots both occur
            assert (inc[:, 0] > 1).any() and won.all() and (live.sum(axis=1) == 4).any()
    finally:
        prob.close()


def test_scorers_are_the_essential_problems_scorers():
    """The model a run returns, scored through a plain essential problem over
    the same rows: the same counts, values and masks as through the gravity
    problem, and the count the run reported."""
    corr, truth, K, G1, G2, E_gt = S.problem_g(600, 0.5, seed=43)
    thr = 1.0
    pg, pe = GC.GravProblem(corr, K, K, G1, G2), EC.EssProblem(corr, K, K)
    try:
        E, mask, st = pg.run(scale_residual_thresh=thr, confidence=0.99, min_iteration_number=50,
                             max_iteration_number=3000, seed=9)
        assert E is not None
        _, gen = pg.generate(SEED, 0, 8)
        models = np.ascontiguousarray(np.concatenate([E.reshape(1, 9), E_gt.reshape(1, 9), gen.reshape(-1, 9)]))
        a, b = pg.score(models, thr), pe.score(models, thr)
        assert np.array_equal(a[0], b[0]) and a[0][0] > 200
        for u, v in zip(a[1:], b[1:]):
            assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
        assert a[0][0] == mask.sum()                  # the run's own count of its model
        assert np.array_equal(pe.mask(E, 0, thr), mask)
    finally:
        pg.close()
        pe.close()


def test_grid_lies_over_the_pixels():
    """lambda > 0.  Pixels and K both scaled by 2: the normalised rows are the
    same bits and the pixel grid (cell sizes from the doubled image size) is
    scaled with them, so the edges, the graph cuts and the result are the same.
    A grid over the normalised rows would not scale: its cells, hundreds of
    pixels wide, would hold every row at either scale."""
    corr, _, K, G1, G2, _ = S.problem_g(600, 0.5, seed=44)
    K2 = K.copy()
    K2[:2] *= 2.0
    kw = dict(threshold=1.0, conf=0.99, spatial_coherence_weight=0.3, max_iters=2000, min_iters=50, neighborhood_size=4,
              seed=5, device=0, return_stats=True)
    find = pygcransac.findGravityEssentialMatrix
    E1, m1, st1 = find(corr, K, K, G1, G2, *SIZE, **kw)
    kw2 = dict(kw, threshold=2.0)
    E2, m2, st2 = find(2.0 * corr, K2, K2, G1, G2, *(2 * v for v in SIZE), **kw2)
    assert E1 is not None and st1["graph_cut_number"] > 0
    assert st1["graph_cut_number"] == st2["graph_cut_number"]
    assert np.array_equal(m1, m2) and E1.tobytes() == E2.tobytes()
    # the essential run's setup over the same pixels and cells cuts a graph as well
    _, _, ste = pygcransac.findEssentialMatrix(corr, K, K, *SIZE, **kw)
    assert ste["graph_cut_number"] > 0
    _, m0, _ = find(corr, K, K, G1, G2, *SIZE, **dict(kw, neighborhood_size=0))
    assert m0.sum() > 0


@pytest.fixture(scope="module")
def whole():
    """seed -> (corr, truth, K, G1, G2, kw, gravity run, essential run) at N = 2000, 80 % outliers"""
    out = {}
    for seed in range(5):
        corr, truth, K, G1, G2, _ = S.problem_g(2000, 0.8, seed=seed)
        kw = dict(threshold=1.0, conf=0.99, spatial_coherence_weight=0.0, max_iters=10 ** 6, min_iters=50, seed=seed,
                  device=0, return_stats=True)
        out[seed] = (corr, truth, K, G1, G2, kw, pygcransac.findGravityEssentialMatrix(corr, K, K, G1, G2, *SIZE, **kw),
                     pygcransac.findEssentialMatrix(corr, K, K, *SIZE, **kw))
    return out


@pytest.mark.parametrize("seed", range(5))
def test_whole_run_finds_the_truth_in_fewer_iterations(whole, seed):
    corr, truth, K, G1, G2, kw, (E, mask, st), (Ee, me, ste) = whole[seed]
    assert E is not None and abs(np.linalg.norm(E) - 1.0) < 1e-12
    assert GC.constrained_form(E, G1, G2) < 1e-14
    found = int((mask & truth).sum())
    print(f"seed {seed}: truth inliers found {found} of {int(truth.sum())}, mask {int(mask.sum())}, iterations "
          f"{st['iteration_number']} (5-point: {ste['iteration_number']}, found {int((me & truth).sum())})")
    assert found >= 0.95 * truth.sum()
    assert st["iteration_number"] < ste["iteration_number"]


def test_runs_are_deterministic_and_independent_of_the_batch(whole):
    corr, truth, K, G1, G2, kw, (E, mask, st), _ = whole[0]
    for bs in (0, 64, 1000):
        E2, mask2, st2 = pygcransac.findGravityEssentialMatrix(corr, K, K, G1, G2, *SIZE, batch_slots=bs, **kw)
        assert E2.tobytes() == E.tobytes() and np.array_equal(mask2, mask), bs
        assert st2["iteration_number"] == st["iteration_number"] and st2["score"] == st["score"], bs


def test_guided_stop_stops_earlier_and_keeps_the_inliers(whole):
    corr, truth, K, G1, G2, kw, _, _ = whole[1]
    w = np.where(truth, 1.0, 0.05)
    find = pygcransac.findGravityEssentialMatrix
    Eg, mg, sg = find(corr, K, K, G1, G2, *SIZE, probabilities=w, sampler=3, **kw)
    Es, ms, ss = find(corr, K, K, G1, G2, *SIZE, probabilities=w, sampler=3, guided_stop=True, **kw)
    print(f"iterations: guided {sg['iteration_number']}, with guided_stop {ss['iteration_number']}")
    assert Eg is not None and Es is not None
    assert ss["iteration_number"] < sg["iteration_number"]
    assert (ms & truth).sum() >= 0.95 * truth.sum() and (mg & truth).sum() >= 0.95 * truth.sum()


def test_sharded_world_one_equals_the_plain_run():
    corr, _, K, G1, G2, _ = S.problem_g(800, 0.5, seed=46)
    fields = dict(scale_residual_thresh=1.0, confidence=0.99, min_iteration_number=50, max_iteration_number=3000,
                  seed=8)
    prob = GC.GravProblem(corr, K, K, G1, G2)
    try:
        E, mask, st = prob.run(**fields)
    finally:
        prob.close()
    Es, masks, sts, _ = D.run_problem_sharded(N.SOLVER_ESSENTIAL3_GRAVITY, corr, params=fields, rank=0, world=1,
                                              device=0, K1=K, K2=K, G1=G1, G2=G2)
    assert E is not None and Es.tobytes() == E.tobytes()
    assert np.array_equal(masks[0], mask)
    assert sts["iteration_number"] == st["iteration_number"] and sts["score"] == st["score"]


def test_verify_batches_count_the_generators_models():
    corr, _, K, G1, G2, _ = S.problem_g(500, 0.5, seed=47)
    nslots = 300
    prob = GC.GravProblem(corr, K, K, G1, G2)
    try:
        p = prob._params(1.0)
        p.seed = SEED
        res = (N.BatchResult * 2)()
        N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), 1000, nslots, 2, res, None))
        for b in range(2):
            inc, models = prob.generate(SEED, 1000 + b * nslots, nslots)
            live = inc.reshape(-1) <= 101
            assert res[b].models == live.sum()
            assert res[b].iterations == np.where(inc <= 102, inc, 0).sum()
            n0, v0, tot = prob.score(models.reshape(-1, 9), 1.0)
            t = 1.0 / ((K[0, 0] + K[1, 1] + K[0, 0] + K[1, 1]) / 4.0)
            T = (2.25 * t) * t
            msac = np.where(live & (n0 >= 3), v0 / T + n0, 0.0)
            j = int(np.argmax(msac))                         # the first maximum
            assert res[b].best_slot == 1000 + b * nslots + j // 4
            assert res[b].best_score == msac[j] and res[b].best_inliers[0] == n0[j]
    finally:
        prob.close()


def test_batch_items_cannot_be_gravity_essential():
    corr = np.ascontiguousarray(S.problem_g(50, 0.5, seed=48)[0])
    item = N.BatchItem()
    item.solver = N.SOLVER_ESSENTIAL3_GRAVITY
    item.f0 = corr.ctypes.data_as(C.POINTER(C.c_double))
    item.n0 = len(corr)
    item.params = N.default_params()
    mask = np.zeros(len(corr), dtype=np.uint8)
    item.mask0_out = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    assert N.lib.gcr_solve_batch(0, C.byref(item), 1, 1) == N.GCR_EINVAL
    assert item.result == N.GCR_EINVAL
