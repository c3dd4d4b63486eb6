"""Homography from two SIFT correspondences on the GPU: the sampler and the
generator kernel against their host twins bit for bit, the scorers (with the
compaction of many-model slots under the homography kind) against a plain
homography problem over the same rows, whole runs beside findHomography, the
graph cut, the guided stop, the sharded and batch entries."""
import ctypes as C

import numpy as np
import pytest

import guided_cases as G
import sift_homography_cases as SC
import pygcransac
from pygcransac import _native as N
from pygcransac import distributed as D
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

SEED = 0x5EEDFACE12345678
SIZE = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)
DEFAULT = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
PER = SC.PER


def small_problem(n):
    """n = 257: rows of problem_hs, three quarters inliers, five of them copies
    of another, so samples holding two of them (coincident points) have no
    model.  n = 2: TWO_MODEL_PAIR, whose only sample yields two models in
    either order.  Returns the rows and guided weights."""
    if n == 2:
        return np.ascontiguousarray(SC.TWO_MODEL_PAIR), np.array([1.0, 0.05])
    rows, truth, _, _ = S.problem_hs(n, 0.25, seed=41)
    for i in (7, 11, 17, 22, 28):
        rows[i] = rows[3]
    return np.ascontiguousarray(rows), np.where(truth, 1.0, 0.05)


@pytest.mark.parametrize("n", (2, 257))
def test_device_sampler_equals_host_sampler(n):
    rows, w = small_problem(n)
    prob = SC.HProblem(rows)
    try:
        for slot0 in (0, 1 << 40):
            for a in (0, 100):
                got = prob.sample(SEED, slot0, 2048, a)
                assert np.array_equal(got, G.host_samples_uniform(SEED, slot0, 2048, a, n, 2)), (n, slot0, a)
        prob.set_probabilities(w)
        for slot0 in (0, 1 << 40):
            for a in (0, 100):
                got = prob.sample(SEED, slot0, 2048, a)
                assert np.array_equal(got, G.host_samples(SEED, slot0, 2048, a, w, 2)), (n, slot0, a)
                ok = got[:, 0] != G.ALL_ONES
                assert ok.any() and np.all(got[ok, 0] != got[ok, 1])
    finally:
        prob.close()


@pytest.mark.parametrize("gen_g", (None, "1", "64"), ids=("default", "G1", "G64"))
@pytest.mark.parametrize("guided", (False, True), ids=("uniform", "guided"))
@pytest.mark.parametrize("n", (2, 257))
def test_generator_equals_the_host_twin_bitwise(n, guided, gen_g, monkeypatch):
    """At n = 257 retries occur (coincident points, the orientation tests on
    outlier pairs).  A sample with two models is about 1e-5 of all, none is
    expected among 512 slots there: at n = 2 every slot holds two."""
    if gen_g is None:
        monkeypatch.delenv("GCR_GEN_G", raising=False)
    else:
        monkeypatch.setenv("GCR_GEN_G", gen_g)
    rows, w = small_problem(n)
    nslots, slot0 = 512, 2 ** 32 - 100              # crosses the 32-bit counter word
    prob = SC.HProblem(rows)
    try:
        if guided:
            prob.set_probabilities(w)
        inc, models = prob.generate(SEED, slot0, nslots)
        hinc, hmodels = SC.host_generate(rows, w if guided else None, SEED, slot0, nslots)
        assert np.array_equal(inc, hinc)
        assert np.array_equal(models.view(np.uint64), hmodels.view(np.uint64))
        # the layout: the first byte counts attempts, the others flag the extra models, the rest is the default
        won = inc[:, 0] <= 101
        assert ((inc[:, 1:] == 0) | (inc[:, 1:] == 255)).all() and (inc[~won] == [102] + [255] * (PER - 1)).all()
        live = np.column_stack([won, inc[:, 1:] == 0])
        assert (np.diff(live.astype(int), axis=1) <= 0).all()            # packed to the front
        assert np.array_equal(models[~live], np.tile(DEFAULT, ((~live).sum(), 1)))
        assert np.all(np.isfinite(models)) and (models[..., 8] == 1.0).all()
        # the first 96 slots, attempt by attempt: the device's samples through the host solver; no earlier
        # attempt yields a model, the winning one yields exactly the slot's models
        last = np.where(won, inc[:, 0], 101)[:96].astype(int)
        for a in range(int(last.max())):
            idx = prob.sample(SEED, slot0, 96, a)
            for s in np.flatnonzero(a < last):
                got = SC.solve_s2(rows, idx[s]) if idx[s, 0] != G.ALL_ONES else np.zeros((0, 9))
                if a < last[s] - 1 or not won[s]:
                    assert len(got) == 0, (s, a)
                else:
                    assert len(got) == live[s].sum()
                    assert np.array_equal(got.view(np.uint64), models[s, :len(got)].view(np.uint64))
        if n == 257:
            assert (inc[:, 0] > 1).any() and won.all()
        else:
            assert won.all() and (live.sum(axis=1) == 2).all()
    finally:
        prob.close()


@pytest.fixture(scope="module")
def scored():
    """N = 600: the SIFT problem, the plain homography problem over the same rows"""
    rows, truth, H, thr = S.problem_hs(600, 0.5, seed=43)
    ps, ph = SC.HProblem(rows), SC.HProblem(rows, sift=False)
    yield rows, truth, H, thr, ps, ph
    ps.close()
    ph.close()


def test_scorers_are_the_homography_problems_scorers(scored):
    rows, truth, H_gt, thr, ps, ph = scored
    H, mask, st = ps.run(scale_residual_thresh=thr, confidence=0.99, min_iteration_number=50,
                         max_iteration_number=3000, seed=9)
    assert H is not None
    _, gen = ps.generate(SEED, 0, 8)
    models = np.ascontiguousarray(np.concatenate([H.reshape(1, 9), H_gt.reshape(1, 9), gen.reshape(-1, 9)]))
    a, b = ps.score(models, thr), ph.score(models, thr)
    assert np.array_equal(a[0], b[0]) and a[0][0] > 200
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
    assert a[0][0] == mask.sum()                      # the run's own count of its model
    for rule in (0, 1):
        assert np.array_equal(ps.mask(H, rule, thr), ph.mask(H, rule, thr))
    assert np.array_equal(ph.mask(H, 0, thr), mask)


# nh = 3 nslots hypotheses per launch: below 2048 k_score_split (H = 4) behind k_compact, from 2048 k_score_fm
# compacting in its prologue, from 16384 k_score_fm behind k_compact
@pytest.mark.parametrize("nslots", (300, 1000, 5600), ids=("split", "fm_scan", "fm_compact"))
def test_verify_batches_score_the_compacted_models(scored, nslots):
    """The batch's models (dead positions compacted away under KIND 3) scored
    one by one through the plain homography problem: the live count, and the
    first maximum of the MSAC score with its inlier count."""
    rows, truth, H_gt, thr, ps, ph = scored
    res = ps.verify_batches(thr, SEED, 1000, nslots, 2)
    T = (2.25 * thr) * thr
    for b in range(2):
        inc, models = ps.generate(SEED, 1000 + b * nslots, nslots)
        live = inc.reshape(-1) <= 101
        assert res[b].models == live.sum() and 0 < live.sum() < live.size
        assert res[b].iterations == np.where(inc <= 102, inc, 0).sum()
        n0, v0, tot = ph.score(models.reshape(-1, 9), thr)
        msac = np.where(live & (n0 >= 2), v0 / T + n0, 0.0)
        j = int(np.argmax(msac))                         # the first maximum
        assert res[b].best_slot == 1000 + b * nslots + j // PER
        assert res[b].best_score == msac[j] and res[b].best_inliers[0] == n0[j]


@pytest.fixture(scope="module")
def whole():
    """seed -> (rows, truth, kw, SIFT run, 4-point run) at N = 2000, 80 % outliers, lambda = 0"""
    out = {}
    for seed in range(5):
        rows, truth, _, thr = S.problem_hs(2000, 0.8, seed=seed)
        kw = dict(threshold=thr, conf=0.99, spatial_coherence_weight=0.0, max_iters=10 ** 6, min_iters=50, seed=seed,
                  device=0, return_stats=True)
        out[seed] = (rows, truth, kw, pygcransac.findHomographySIFT(rows, *SIZE, **kw),
                     pygcransac.findHomography(np.ascontiguousarray(rows[:, :4]), *SIZE, **kw))
    return out


@pytest.mark.parametrize("seed", range(5))
def test_whole_run_finds_the_truth_in_fewer_iterations(whole, seed):
    rows, truth, kw, (H, mask, st), (H4, m4, st4) = whole[seed]
    assert H is not None and H[2, 2] == 1.0
    found = int((mask & truth).sum())
    print(f"seed {seed}: truth inliers found {found} of {int(truth.sum())}, mask {int(mask.sum())}, iterations "
          f"{st['iteration_number']} (4-point: {st4['iteration_number']}, found {int((m4 & truth).sum())})")
    assert found >= 0.95 * truth.sum()
    assert st["iteration_number"] < st4["iteration_number"]


def test_runs_are_deterministic_and_independent_of_the_batch(whole):
    rows, truth, kw, (H, mask, st), _ = whole[0]
    for bs in (0, 64, 1000):
        H2, mask2, st2 = pygcransac.findHomographySIFT(rows, *SIZE, batch_slots=bs, **kw)
        assert H2.tobytes() == H.tobytes() and np.array_equal(mask2, mask), bs
        assert st2["iteration_number"] == st["iteration_number"] and st2["score"] == st["score"], bs


def test_graph_cut_runs(whole):
    rows, truth, kw, _, _ = whole[2]
    H, mask, st = pygcransac.findHomographySIFT(rows, *SIZE, neighborhood_size=4,
                                                **dict(kw, spatial_coherence_weight=0.3))
    assert H is not None and st["graph_cut_number"] > 0
    assert (mask & truth).sum() >= 0.95 * truth.sum()


def test_guided_stop_stops_earlier_and_keeps_the_inliers(whole):
    rows, truth, kw, _, _ = whole[1]
    w = np.where(truth, 1.0, 0.05)
    find = pygcransac.findHomographySIFT
    Hg, mg, sg = find(rows, *SIZE, probabilities=w, sampler=3, **kw)
    Hs, ms, ss = find(rows, *SIZE, probabilities=w, sampler=3, guided_stop=True, **kw)
    print(f"iterations: guided {sg['iteration_number']}, with guided_stop {ss['iteration_number']}")
    assert Hg is not None and Hs is not None
    assert ss["iteration_number"] < sg["iteration_number"]
    assert (ms & truth).sum() >= 0.95 * truth.sum() and (mg & truth).sum() >= 0.95 * truth.sum()


def test_sharded_world_one_equals_the_plain_run():
    rows, _, _, thr = S.problem_hs(800, 0.5, seed=46)
    fields = dict(scale_residual_thresh=thr, confidence=0.99, min_iteration_number=50, max_iteration_number=3000,
                  seed=8)
    prob = SC.HProblem(rows)
    try:
        H, mask, st = prob.run(**fields)
    finally:
        prob.close()
    Hs, masks, sts, _ = D.run_problem_sharded(N.SOLVER_HOMOGRAPHY2_SIFT, np.ascontiguousarray(rows[:, :4]),
                                              params=fields, rank=0, world=1, device=0, sift=rows[:, 4:])
    assert H is not None and Hs.tobytes() == H.tobytes()
    assert np.array_equal(masks[0], mask)
    assert sts["iteration_number"] == st["iteration_number"] and sts["score"] == st["score"]


def test_a_run_needs_four_rows():
    rows = np.ascontiguousarray(S.problem_hs(8, 0.0, seed=49)[0][:3])
    prob = SC.HProblem(rows)                          # the create entry accepts n >= 2
    try:
        inc, _ = prob.generate(SEED, 0, 16)
        assert (inc[:, 0] <= 102).all()
        with pytest.raises(ValueError, match="at least 4"):
            prob.run(scale_residual_thresh=2.0)
    finally:
        prob.close()


def test_batch_items_cannot_be_sift_homographies():
    corr = np.ascontiguousarray(S.problem_hs(50, 0.5, seed=48)[0][:, :4])
    item = N.BatchItem()
    item.solver = N.SOLVER_HOMOGRAPHY2_SIFT
    item.f0 = corr.ctypes.data_as(C.POINTER(C.c_double))
    item.n0 = len(corr)
    item.params = N.default_params()
    mask = np.zeros(len(corr), dtype=np.uint8)
    item.mask0_out = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    assert N.lib.gcr_solve_batch(0, C.byref(item), 1, 1) == N.GCR_EINVAL
    assert item.result == N.GCR_EINVAL
