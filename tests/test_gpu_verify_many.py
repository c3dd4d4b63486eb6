"""verify_many on the GPU: gcr_verify_many (k_many / k_many_merge / k_many_mask
at the end of csrc/kernels.hip) against the existing path -- a resident problem
per problem, gcr_problem_verify_batch(.., 0, S), gcr_debug_generate_h at the
best slot, gcr_debug_mask_h rule 0 -- and against the host twin, byte for byte:
at the row counts and slot counts that reach every edge of the kernels, for
both kinds, with degenerate problems inside a call, on exact ties, under
permutation and for every slot-block size, and through features.verify_pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import verify_many_cases as VC
from gcr_testutil import CorrProblem
from pygcransac import _native as N
from pygcransac import features as F
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

# m, m + 1, around a wave, past a workgroup, 1000; the score loop takes the rows
# in groups of 4 and then singly: the counts cover every remainder
ROWS = {VC.H4: [4, 5, 63, 64, 65, 257, 1000, 62], VC.F7: [7, 8, 63, 64, 65, 257, 1000, 62]}
SLOTS = [1, 63, 64, 65, 256, 257, 1000]


def gpu(solver, problems, thr, seeds, slots, **kw):
    return VC.run(solver, problems, thr, seeds, slots, ctx=N.context(0), **kw)


def twin(solver, problems, thr, seeds, slots):
    return VC.run(solver, problems, thr, seeds, slots, host=True, threads=16)


def existing(solver, rows, thr, seed, slots):
    """the record, the model and the mask of one problem by the existing path"""
    prob = CorrProblem(solver, rows)
    try:
        p = N.default_params()
        p.scale_residual_thresh = float(thr)
        p.seed = int(seed)
        one = N.BatchResult()
        rc = N.lib.gcr_problem_verify_batch(prob.h, C.byref(p), 0, slots, C.byref(one), None)
        assert rc >= 0, N.last_error()
        rec = dict(models=one.models, iterations=one.iterations, best_slot=one.best_slot, best_score=one.best_score,
                   best_inliers=one.best_inliers[0])
        models = None
        if one.best_slot >= 0:
            _, H = prob.generate(int(seed), one.best_slot, 1)
            models = H.reshape(-1, 9)                   # 1 row, or the slot's 3 hypotheses
        return rec, models, prob
    except Exception:
        prob.close()
        raise


def assert_equals_existing(solver, rows, thr, seed, slots, rec, mask):
    e, models, prob = existing(solver, rows, thr, seed, slots)
    try:
        for k in ("models", "iterations", "best_slot", "best_inliers"):
            assert rec[k] == e[k], (k, rec[k], e[k], len(rows), slots)
        assert np.float64(rec["best_score"]).tobytes() == np.float64(e["best_score"]).tobytes()
        if e["best_slot"] < 0:
            assert not mask.any() and np.array_equal(rec["best_model"], VC.DEFAULT_MODEL)
            return
        assert rec["best_hypothesis"] < len(models)
        model = models[rec["best_hypothesis"]]
        assert rec["best_model"].tobytes() == model.tobytes()
        assert np.array_equal(mask.astype(bool), prob.mask(model, 0, float(thr)))
        assert int(mask.sum()) == rec["best_inliers"]
    finally:
        prob.close()


@functools.lru_cache(maxsize=None)
def mixed(solver):
    """row counts mixed in one call (unaligned offsets), per-problem thresholds and seeds"""
    if solver == VC.H4:
        probs = [VC.rows_h(n, seed=n) for n in ROWS[solver]]
    else:
        probs = [VC.rows_f(n, seed=n) for n in ROWS[solver]]
    thr = [2.0, 1.0, 2.0, 1.5, 2.0, 0.75, 2.0, 3.0]
    seeds = [3, 1 << 40, 5, 6, 7, 8, 9, 10]
    return probs, thr, seeds


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("solver", [VC.H4, VC.F7])
def test_mixed_call_equals_the_existing_path_and_the_twin(solver, slots):
    probs, thr, seeds = mixed(solver)
    got = gpu(solver, probs, thr, seeds, slots)
    assert VC.same(got, twin(solver, probs, thr, seeds, slots))
    for p in range(len(probs)):
        assert_equals_existing(solver, probs[p], thr[p], seeds[p], slots, got[0][p], got[1][p])
    assert (got[0]["best_slot"] >= 0).all()              # every problem of the call has a best, the m-row ones too


def test_one_problem_and_no_mask():
    r = VC.rows_h(100)
    got = gpu(VC.H4, [r], 2.0, 4, 300)
    assert VC.same(got, twin(VC.H4, [r], 2.0, 4, 300))
    assert_equals_existing(VC.H4, r, 2.0, 4, 300, got[0][0], got[1][0])
    rec, untouched = gpu(VC.H4, [r], 2.0, 4, 300, masks=False)
    assert rec.tobytes() == got[0].tobytes() and (untouched[0] == 7).all()


def test_many_problems_smaller_than_a_wave():
    """300 problems of 40 rows: more workgroups than compute units"""
    base = S.problem_h(40 * 300, 0.4, seed=12)[0]
    probs = [base[40 * p:40 * p + 40] for p in range(300)]
    seeds = np.arange(300) * 7 + 1
    got = gpu(VC.H4, probs, 2.0, seeds, 100)
    assert VC.same(got, twin(VC.H4, probs, 2.0, seeds, 100))
    for p in (0, 149, 299):
        assert_equals_existing(VC.H4, probs[p], 2.0, seeds[p], 100, got[0][p], got[1][p])
    assert (got[0]["best_slot"] >= 0).sum() >= 290


def test_a_long_problem():
    """16385 rows: no row count is special to the kernels; the rows of a
    problem are never staged"""
    rows = S.problem_h(16385, 0.5, seed=14)[0]
    probs = [VC.rows_h(9), rows, VC.rows_h(4)]
    got = gpu(VC.H4, probs, 2.0, [1, 2, 3], 65)
    assert VC.same(got, twin(VC.H4, probs, 2.0, [1, 2, 3], 65))
    assert_equals_existing(VC.H4, rows, 2.0, 2, 65, got[0][1], got[1][1])
    assert got[0][1]["best_inliers"] > 7000


@pytest.mark.parametrize("source", ["f_n30", "f_n500", "problem_f"])
def test_fundamental(source):
    """golden rows (slots with two and three models) and a synthetic problem"""
    if source == "problem_f":
        rows, _, _, thr = S.problem_f(500, 0.5, seed=31)
    else:
        rows, thr = VC.golden_f(int(source[3:]))
    probs = [rows, VC.rows_f(7), rows[::-1].copy()]
    got = gpu(VC.F7, probs, thr, [21, 22, 23], 257)
    assert VC.same(got, twin(VC.F7, probs, thr, [21, 22, 23], 257))
    assert got[0][0]["models"] > 257 and got[0][0]["best_slot"] >= 0
    for p in (0, 2):
        assert_equals_existing(VC.F7, probs[p], thr, 21 + p, 257, got[0][p], got[1][p])
    if source == "f_n30":
        # every hypothesis position of a slot wins somewhere across seeds
        seeds = np.arange(40)
        rec, _ = gpu(VC.F7, [rows] * 40, thr, seeds, 64)
        assert rec.tobytes() == twin(VC.F7, [rows] * 40, thr, seeds, 64)[0].tobytes()
        assert set(rec["best_hypothesis"].tolist()) >= {0, 1}


@pytest.mark.parametrize("solver", [VC.H4, VC.F7])
def test_degenerate_problems_inside_a_call(solver):
    m = VC.M_OF[solver]
    rows = VC.rows_h if solver == VC.H4 else VC.rows_f
    probs = [rows(70), VC.one_point(33), rows(m), rows(130, seed=8), VC.one_point(m)]
    thr, seeds = [2.0, 1.0, 1.0, 1.5, 1.0], [1, 2, 3, 4, 5]
    got = gpu(solver, probs, thr, seeds, 130)
    assert VC.same(got, twin(solver, probs, thr, seeds, 130))
    for p in (1, 4):
        r = got[0][p]
        assert r["models"] == 0 and r["iterations"] == 102 * 130 and r["best_slot"] == -1 and not got[1][p].any()
    for p in (0, 2, 3):                                  # the neighbours' results do not move
        alone = gpu(solver, [probs[p]], thr[p], seeds[p], 130)
        assert got[0][p].tobytes() == alone[0][0].tobytes() and np.array_equal(got[1][p], alone[1][0])
        assert_equals_existing(solver, probs[p], thr[p], seeds[p], 130, got[0][p], got[1][p])


def test_ties_go_to_the_lowest_hypothesis():
    """five exact correspondences, ten copies of each: slots that draw the
    same base rows in the same order build the same model bit for bit, so
    distinct slots tie on the best score; the lowest wins, as verify_batch says"""
    base = S.problem_h(5, 0.0, seed=20, noise=0.5)[0]
    rows = np.ascontiguousarray(np.tile(base, (10, 1)))
    slots = 256
    scores = []
    exp, emask = VC.restate(VC.H4, rows, 2.0, 22, slots, scores)
    top = [h for h, sc in scores if sc == exp["best_score"]]
    assert len(top) >= 2 and exp["best_slot"] == min(top) > 0       # the case has the tie it is about
    assert max(top) >= 64                                           # ... across waves of a block or across blocks
    assert len({sc for _, sc in scores}) > 2                        # ... and other slots score lower
    got = gpu(VC.H4, [VC.rows_h(50), rows], 2.0, [1, 22], slots)
    assert VC.record_equals(got[0][1], exp) and np.array_equal(got[1][1], emask)
    assert_equals_existing(VC.H4, rows, 2.0, 22, slots, got[0][1], got[1][1])


def test_independence_of_position_and_block_size(monkeypatch):
    probs, thr, seeds = mixed(VC.H4)
    probs, thr, seeds = list(probs[:6]), thr[:6], seeds[:6]
    slots = 300
    ref = gpu(VC.H4, probs, thr, seeds, slots)
    order = [4, 0, 5, 2, 1, 3]                           # problem 0 first, in the middle; 3 last; ...
    perm = gpu(VC.H4, [probs[k] for k in order], [thr[k] for k in order], [seeds[k] for k in order], slots)
    for pos, k in enumerate(order):
        assert perm[0][pos].tobytes() == ref[0][k].tobytes() and np.array_equal(perm[1][pos], ref[1][k])
    alone = gpu(VC.H4, [probs[3]], thr[3], seeds[3], slots)
    assert alone[0][0].tobytes() == ref[0][3].tobytes() and np.array_equal(alone[1][0], ref[1][3])
    fprobs, fthr, fseeds = mixed(VC.F7)
    fref = gpu(VC.F7, fprobs, fthr, fseeds, slots)
    for block in ("64", "128", "256", "1"):              # an unsupported value is the default
        monkeypatch.setenv("GCR_MANY_BLOCK", block)
        assert VC.same(gpu(VC.H4, probs, thr, seeds, slots), ref), block
        assert VC.same(gpu(VC.F7, fprobs, fthr, fseeds, slots), fref), block


def test_seeds_and_thresholds_are_per_problem():
    r = VC.rows_h(257)
    rec, masks = gpu(VC.H4, [r, r, r, r], [2.0, 2.0, 2.0, 0.5], [7, 8, 7, 7], 256)
    assert rec[0].tobytes() == rec[2].tobytes() and np.array_equal(masks[0], masks[2])
    assert rec[0].tobytes() != rec[1].tobytes() and rec[0].tobytes() != rec[3].tobytes()


def test_kernel_time_is_reported():
    r = VC.rows_h(64)
    rows, off = VC.pack([r])
    thr, seeds = np.array([2.0]), np.array([1], dtype=np.uint64)
    out = (N.ManyResult * 1)()
    ms = C.c_double(-1.0)
    N.check(N.lib.gcr_verify_many(N.context(0), VC.H4, rows.ctypes.data, off.ctypes.data, 1, thr.ctypes.data,
                                  seeds.ctypes.data, 64, out, None, C.byref(ms)))
    assert 0.0 < ms.value < 1000.0


def test_verify_pairs_equals_its_host_backend():
    kp1, d1, kp2, d2, _, _ = S.problem_match(300, 120)
    sets = [(d1, kp1), (d2, kp2), (d2[::-1].copy(), kp2[::-1].copy())]
    pairs = [(0, 1), (0, 2), (1, 0)]
    host = F.verify_pairs(sets, pairs, "homography", [2.0, 3.0, 2.0], iterations=200, seed=[5, 6, 7], refine=True,
                          backend="host")
    with F.DescriptorSet(d1, kp1) as a, F.DescriptorSet(d2, kp2) as b:
        for use in ([a, b, sets[2]], sets):              # resident sets, and arrays uploaded for the call
            got = F.verify_pairs(use, pairs, "homography", [2.0, 3.0, 2.0], iterations=200, seed=[5, 6, 7],
                                 refine=True)
            for (m, ra, rec), (em, er, e) in zip(got, host):
                assert np.array_equal(m, em) and np.array_equal(ra, er) and rec.keys() == e.keys()
                for k in rec:
                    if isinstance(e[k], np.ndarray):
                        assert np.array_equal(rec[k], e[k]), k
                    else:
                        assert rec[k] == e[k], k
                assert rec["model"] is not None
        with pytest.raises(ValueError):
            F.verify_pairs([F.DescriptorSet(d1), b], [(0, 1)], "homography", 2.0)
