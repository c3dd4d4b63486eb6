"""Whole runs under PROSAC sampling (sampler=1, with and without prosac_stop),
under NAPSAC sampling (sampler=2) and of the homography from two SIFT
correspondences, on the GPU against the oracle's independent run loop and its
restatements of csrc/prosac.h, csrc/prosac_stop.h and csrc/napsac.h
(oracle/gcr_oracle.cpp).  Every comparison is bitwise: mask (in the caller's
order), model bytes, bits(score), iteration / LO / graph-cut / slot /
hypothesis counts.  What a run must have done for its comparison to mean
something is asserted on the oracle's result, never on the product's."""
import numpy as np
import pytest

import sampler_run_cases as SR
from pygcransac import _native as N
from pygcransac import distributed as D

pytestmark = pytest.mark.gpu

SOLVER = {"H": N.SOLVER_HOMOGRAPHY4, "F": N.SOLVER_FUNDAMENTAL7, "E": N.SOLVER_ESSENTIAL5,
          "G": N.SOLVER_ESSENTIAL3_GRAVITY, "S": N.SOLVER_HOMOGRAPHY2_SIFT}
MANY = ("F", "E", "G")                      # kinds whose solver gives several models per sample as a rule
BATCHES = (0, 5, 64)
_cache = {}


def case(kind, n, outliers=0.5):
    """The problem of a kind and size, made once."""
    key = (kind, n, outliers)
    if key not in _cache:
        if n == 40:
            _cache[key] = SR.small_problem(kind)
        elif n == SR.N_MAIN:
            _cache[key] = SR.main_problem(kind)
        else:
            _cache[key] = SR.problem(kind, n, outliers, seed=7000 + n)
    return _cache[key]


def frozen(v):
    return v.tobytes() if isinstance(v, np.ndarray) else v


def reference(p, **kw):
    """One oracle run per (problem, parameters) shared by the tests that need it."""
    key = (p["kind"], p["corr"].tobytes(), p["thr"], tuple(sorted((k, frozen(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = SR.run_oracle(p, **kw)
    return _cache[key]


def same(p, batch_slots=0, **kw):
    got = SR.run_gpu(p, batch_slots=batch_slots, **kw)
    what = (p["kind"], len(p["corr"]), batch_slots,
            sorted((k, v) for k, v in kw.items() if k not in ("scores", "weights")))
    SR.assert_same(got, reference(p, **kw), what)
    return got


def found_the_truth(p, ref):
    return ref["num_inliers"] > SR.M_OF[p["kind"]] and (ref["mask"] & p["truth"]).sum() >= 0.9 * p["truth"].sum()


def sharded(p, *, seed, min_it, max_it, confidence, flags=0, **sampling):
    """The run through the sharded entry at world 1 (rows in quality order for
    a PROSAC run, as the C ABI expects them: sorted here by sampler_run_cases'
    own statement of the order), compared with the oracle's run in that order."""
    rows, order, skw = SR.oracle_arguments(p, **sampling)
    fields = dict(scale_residual_thresh=p["thr"], confidence=confidence, min_iteration_number=min_it,
                  max_iteration_number=max_it, seed=seed, flags=flags)
    extra = {}
    if "K" in p:
        extra.update(K1=p["K"], K2=p["K"])
    if "G1" in p:
        extra.update(G1=p["G1"], G2=p["G2"])
    if p["kind"] == "S":
        extra.update(sift=np.ascontiguousarray(rows[:, 4:8]))
    if skw.get("sampler") == 1:
        extra.update(prosac_convergence=skw["prosac_convergence"])
    if skw.get("sampler") == 2:
        extra.update(napsac=(skw["napsac_extent"], skw["napsac_iterations"]))
    M, masks, st, _ = D.run_problem_sharded(SOLVER[p["kind"]], np.ascontiguousarray(rows[:, :4]), params=fields,
                                            rank=0, world=1, device=0, **extra)
    ref = reference(p, seed=seed, min_it=min_it, max_it=max_it, confidence=confidence, lam=0.0, lo=50,
                    neighborhood_size=0, **sampling)
    SR.assert_same((M, masks[0], st), dict(ref, mask=ref.get("sorted_mask", ref["mask"])),
                   (p["kind"], sorted(sampling)))
    return ref


# ------------------------------- the homography from two SIFT correspondences ----
@pytest.mark.parametrize("n,outliers", ((40, 0.25), (600, 0.5), (2000, 0.6)))
def test_s2_plain_run_equals_the_oracle(n, outliers):
    p = case("S", n, outliers)
    same(p, seed=11, max_it=5000)
    ref = reference(p, seed=11, max_it=5000)
    assert ref["num_inliers"] > 2 and ref["stats"]["local_optimization_number"] > 0
    if n == 40:
        assert ref["stats"]["iteration_number"] > ref["stats"]["slots"]     # duplicated rows: slots retried
    else:
        assert found_the_truth(p, ref)


def test_s2_second_problem_equals_the_oracle():
    """synthetic.problem_hs at another size and seed than the shared case"""
    p = SR.problem("S", 800, 0.5, seed=13)
    same(p, seed=7, max_it=5000)
    assert found_the_truth(p, reference(p, seed=7, max_it=5000))


@pytest.mark.parametrize("lo", (0, 1, 50))
def test_s2_lo_budget_equals_the_oracle(lo):
    p = case("S", 600)
    same(p, seed=12, lo=lo)
    ref = reference(p, seed=12, lo=lo)
    assert ref["num_inliers"] > 2 and ref["stats"]["local_optimization_number"] > 0


def test_s2_every_batch_size_equals_the_one_oracle_run():
    p = case("S", 600)
    assert reference(p, seed=18)["stats"]["slots"] > 2 * 37         # chunk boundaries fall inside the run
    for bs in (0, 1, 37, 1000):
        same(p, batch_slots=bs, seed=18)
    st = reference(p, seed=14, min_it=1500, max_it=1500)["stats"]
    assert st["iteration_number"] >= 1500 and st["slots"] > 10 * 37          # many chunks of 37 slots
    for bs in (37, 0):
        same(p, batch_slots=bs, seed=14, min_it=1500, max_it=1500)


@pytest.mark.parametrize("cells", (4, 8))
@pytest.mark.parametrize("lam", (0.3, 0.975))
def test_s2_spatial_coherence_equals_the_oracle(lam, cells):
    p = case("S", 600)
    same(p, seed=15, lam=lam, neighborhood_size=cells)
    ref = reference(p, seed=15, lam=lam, neighborhood_size=cells)
    assert ref["num_inliers"] > 2 and ref["stats"]["graph_cut_number"] > 0


def test_s2_no_model_cases_equal_the_oracle():
    p = case("S", 600)
    rng = np.random.default_rng(21)

    def noise(k):
        return np.column_stack([rng.uniform(0, SR.SIZE[1], k), rng.uniform(0, SR.SIZE[0], k),
                                rng.uniform(0, SR.SIZE[1], k), rng.uniform(0, SR.SIZE[0], k),
                                rng.uniform(2.0, 30.0, k), rng.uniform(2.0, 30.0, k),
                                rng.uniform(-np.pi, np.pi, k), rng.uniform(-np.pi, np.pi, k)])

    cases = {"the fewest rows the entry takes": np.ascontiguousarray(noise(4)),
             "identical rows": np.tile(p["corr"][:1], (50, 1)),
             "pure outliers": np.ascontiguousarray(noise(50))}
    for name, rows in cases.items():
        q = dict(p, corr=rows, thr=p["thr"] if name == "identical rows" else 1e-4)
        kw = dict(seed=16, min_it=200, max_it=200)
        M, mask, st = same(q, **kw)
        ref = reference(q, **kw)
        assert ref["num_inliers"] == 0 and ref["stats"]["iteration_number"] >= 200, name
        assert M is None and not mask.any(), name


def test_s2_sharded_world_one_equals_the_oracle():
    p = case("S", 800)
    ref = sharded(p, seed=8, min_it=50, max_it=3000, confidence=0.99)
    assert found_the_truth(p, ref) and ref["stats"]["local_optimization_number"] > 0


def test_s2_guided_runs_equal_the_oracle_under_both_stops():
    p = case("S", 600)
    w = np.where(p["truth"], 1.0, 0.05)
    w[np.random.default_rng(600).choice(600, 60, replace=False)] = 0.0
    gkw = dict(seed=17, min_it=2, max_it=5000, confidence=1.0 - 1e-12)
    for gs in (False, True):
        for bs in BATCHES:
            same(p, batch_slots=bs, weights=w, guided_stop=gs, **gkw)
    off, on = (reference(p, weights=w, guided_stop=gs, **gkw) for gs in (False, True))
    assert gkw["min_it"] < on["stats"]["iteration_number"] < off["stats"]["iteration_number"] < gkw["max_it"]
    assert found_the_truth(p, off) and found_the_truth(p, on)


# ------------------------------------------------------------------- PROSAC ----
@pytest.mark.parametrize("convergence", SR.CONVERGENCES)
@pytest.mark.parametrize("kind", SR.KINDS)
def test_prosac_runs_equal_the_oracle(kind, convergence):
    p, q, seed = case(kind, SR.N_MAIN), SR.main_scores(kind), SR.PROSAC_SEEDS[kind][1]
    n, m = len(q), SR.M_OF[kind]
    top = int(SR.O.prosac_growth(n, m, convergence)[-1])
    kw = dict(seed=seed, sampler=1, scores=q, prosac_convergence=convergence)
    # the uniform stop at the usual confidence
    same(p, **kw, **SR.PROSAC_KW)
    plain = reference(p, **kw, **SR.PROSAC_KW)
    assert found_the_truth(p, plain) and plain["stats"]["local_optimization_number"] > 0
    # flag clear and flag set, each ended by its own stop, in one launch per chunk of 0 (default), 5 and 64 slots
    for flag in (False, True):
        for bs in BATCHES:
            same(p, batch_slots=bs, prosac_stop=flag, **kw, **SR.PSTOP_KW)
    off = reference(p, prosac_stop=False, **kw, **SR.PSTOP_KW)
    on = reference(p, prosac_stop=True, **kw, **SR.PSTOP_KW)
    assert SR.PSTOP_KW["min_it"] < on["stats"]["iteration_number"] < off["stats"]["iteration_number"] \
        < SR.PSTOP_KW["max_it"]
    assert on["stats"]["slots"] > 2 * 5 and off["stats"]["slots"] > 2 * 64
    assert 0 < on["prosac_star"][0] <= on["prosac_star"][1] < n          # the stop chose a proper prefix
    for r in (off, on):
        assert found_the_truth(p, r) and r["stats"]["local_optimization_number"] > 0
    if kind in MANY:
        assert off["stats"]["hypotheses"] > off["stats"]["slots"]
    # a fixed count: past g[N] under convergence 1000, inside the growth phase under 100000
    for flag in (False, True):
        same(p, prosac_stop=flag, **kw, **SR.CROSS_KW)
    cross = reference(p, prosac_stop=False, **kw, **SR.CROSS_KW)
    if convergence == 1000:
        assert cross["stats"]["slots"] > top
    else:
        assert cross["stats"]["slots"] < top and off["stats"]["slots"] < top


@pytest.mark.parametrize("kind", SR.KINDS)
def test_prosac_small_problems_equal_the_oracle(kind):
    p = case(kind, 40)
    q = SR.quality_scores(p["truth"], 9)
    for flag in (False, True):
        kw = dict(seed=11, max_it=2000, sampler=1, scores=q, prosac_convergence=1000, prosac_stop=flag)
        same(p, **kw)
        ref = reference(p, **kw)
        assert ref["num_inliers"] > SR.M_OF[kind]
        assert ref["stats"]["iteration_number"] > ref["stats"]["slots"]     # slots were retried


def test_prosac_f_2000_equals_the_oracle():
    p = case("F", 2000)
    q = SR.quality_scores(p["truth"], 3)
    for flag in (False, True):
        kw = dict(seed=2, sampler=1, scores=q, prosac_stop=flag, **SR.PSTOP_KW)
        for bs in (0, 64):
            same(p, batch_slots=bs, **kw)
        assert found_the_truth(p, reference(p, **kw))
    assert reference(p, seed=2, sampler=1, scores=q, prosac_stop=False, **SR.PSTOP_KW)["stats"]["slots"] > 2 * 64


@pytest.mark.parametrize("kind", SR.KINDS)
def test_prosac_with_graph_cut_equals_the_oracle(kind):
    p, q, seed = case(kind, SR.N_MAIN), SR.main_scores(kind), SR.PROSAC_SEEDS[kind][1]
    for flag in (False, True):
        kw = dict(seed=seed, sampler=1, scores=q, prosac_convergence=1000, prosac_stop=flag, lam=0.3, **SR.PSTOP_KW)
        same(p, **kw)
        ref = reference(p, **kw)
        assert found_the_truth(p, ref) and ref["stats"]["graph_cut_number"] > 0


@pytest.mark.parametrize("kind", SR.KINDS)
def test_prosac_sharded_world_one_equals_the_oracle(kind):
    p, q, seed = case(kind, SR.N_MAIN), SR.main_scores(kind), SR.PROSAC_SEEDS[kind][1]
    for flag in (False, True):
        ref = sharded(p, seed=seed, flags=N.FLAG_PROSAC_STOP if flag else 0, sampler=1, scores=q,
                      prosac_convergence=1000, prosac_stop=flag, **SR.PSTOP_KW)
        assert found_the_truth(p, ref) and ref["stats"]["slots"] > 2


def test_unordered_scores_and_the_whole_set_make_the_flag_a_no_op():
    for kind in SR.KINDS:
        p, q, seed = SR.flat_case(kind)
        kw = dict(seed=seed, sampler=1, scores=q, min_it=50, max_it=5000, confidence=0.99)
        got = SR.run_gpu(p, prosac_stop=True, **kw)
        SR.assert_same(got, reference(p, prosac_stop=False, **kw), kind)
        assert reference(p, prosac_stop=True, **kw)["prosac_star"][1] == len(q)


# ------------------------------------------------------------------- NAPSAC ----
@pytest.mark.parametrize("T", (SR.NAPSAC_T, None))
@pytest.mark.parametrize("kind", SR.KINDS)
def test_napsac_runs_equal_the_oracle(kind, T):
    p, seed = case(kind, SR.N_MAIN), SR.PROSAC_SEEDS[kind][1]
    kw = dict(seed=seed, sampler=2, napsac_iterations=T)
    for bs in BATCHES:
        same(p, batch_slots=bs, **kw)
    ref = reference(p, **kw)
    assert found_the_truth(p, ref) and ref["stats"]["local_optimization_number"] > 0
    assert ref["stats"]["slots"] > 2 * 5
    if kind in MANY:
        assert ref["stats"]["hypotheses"] > ref["stats"]["slots"]
    if T is not None and kind == "F":
        assert ref["stats"]["slots"] > T and ref["stats"]["slots"] > 2 * 64      # ends past T
    if T is not None and kind == "H":
        assert ref["stats"]["slots"] < T                                        # ends inside the local phase
    if kind in ("E", "G"):
        assert not np.array_equal(p["K"], np.eye(3))       # the layers' pixel rows are not the solver's rows
    # a fixed count that crosses every quarter of T = 200 and T itself in chunks of 64
    fixed = dict(seed=seed, sampler=2, napsac_iterations=SR.NAPSAC_T, min_it=1500, max_it=1500)
    if T is not None:
        for bs in (0, 64):
            same(p, batch_slots=bs, **fixed)
        assert reference(p, **fixed)["stats"]["slots"] > SR.NAPSAC_T + 64


def test_napsac_local_structure_equals_the_oracle():
    p = SR.local_problem()
    for T in (SR.NAPSAC_T, None):
        for bs in BATCHES:
            same(p, batch_slots=bs, seed=3, sampler=2, napsac_iterations=T)
        ref = reference(p, seed=3, sampler=2, napsac_iterations=T)
        assert found_the_truth(p, ref) and ref["stats"]["local_optimization_number"] > 0


@pytest.mark.parametrize("kind", SR.KINDS)
def test_napsac_small_problems_equal_the_oracle(kind):
    p = case(kind, 40)
    kw = dict(seed=11, max_it=2000, sampler=2)
    same(p, **kw)
    ref = reference(p, **kw)
    assert ref["num_inliers"] > SR.M_OF[kind] and ref["stats"]["iteration_number"] > ref["stats"]["slots"]


def test_napsac_f_2000_equals_the_oracle():
    p = case("F", 2000)
    for bs in (0, 64):
        same(p, batch_slots=bs, seed=2, sampler=2)
    ref = reference(p, seed=2, sampler=2)
    assert found_the_truth(p, ref) and ref["stats"]["slots"] > 2 * 64


@pytest.mark.parametrize("kind", SR.KINDS)
def test_napsac_with_graph_cut_equals_the_oracle(kind):
    """neighborhood_size = 8: the graph cut's grid is layer 1's grid"""
    p, seed = case(kind, SR.N_MAIN), SR.PROSAC_SEEDS[kind][1]
    kw = dict(seed=seed, sampler=2, napsac_iterations=SR.NAPSAC_T, lam=0.3, neighborhood_size=8)
    same(p, **kw)
    ref = reference(p, **kw)
    assert found_the_truth(p, ref) and ref["stats"]["graph_cut_number"] > 0


@pytest.mark.parametrize("kind", SR.KINDS)
def test_napsac_sharded_world_one_equals_the_oracle(kind):
    p, seed = case(kind, SR.N_MAIN), SR.PROSAC_SEEDS[kind][1]
    ref = sharded(p, seed=seed, min_it=50, max_it=5000, confidence=0.99, sampler=2, napsac_iterations=SR.NAPSAC_T)
    assert found_the_truth(p, ref)


# ---------------------------------------------------------------- fixtures ----
@pytest.mark.parametrize("name", SR.GOLDEN_NAMES)
def test_sampler_fixture_is_reproduced_bitwise(name):
    p, kw, want = SR.load_golden(name)
    got = SR.run_gpu(p, **kw)
    SR.assert_same(got, want, name)
    assert want["num_inliers"] > SR.M_OF[p["kind"]] and want["stats"]["local_optimization_number"] > 0
