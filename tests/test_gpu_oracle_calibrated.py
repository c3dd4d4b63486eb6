"""Whole runs of the essential-matrix kinds, and guided runs of all four
correspondence kinds, on the GPU against the oracle's independent run loop
(oracle/gcr_oracle.cpp GCRANSAC<> around the host solvers; its restatements of
csrc/guided.h and csrc/guided_stop.h).  Every comparison is bitwise: mask, model
bytes, bits(score), iteration / LO / graph-cut / slot / hypothesis counts."""
import numpy as np
import pytest

import calibrated_cases as CC
from pygcransac import _native as N
from pygcransac import distributed as D

pytestmark = pytest.mark.gpu

KINDS = ("E", "G")
SOLVER = {"E": N.SOLVER_ESSENTIAL5, "G": N.SOLVER_ESSENTIAL3_GRAVITY}
_cache = {}


def case(kind, n, outliers=0.5):
    """The problem of a kind and size, made once."""
    key = (kind, n, outliers)
    if key not in _cache:
        _cache[key] = CC.small_problem(kind) if n == 40 else CC.problem(kind, n, outliers, seed=7000 + n)
    return _cache[key]


def reference(p, **kw):
    """One oracle run per (problem, parameters) shared by the tests that need it."""
    key = (p["kind"], p["corr"].tobytes(), p["K"].tobytes() if "K" in p else None, p["thr"],
           tuple(sorted((k, v) for k, v in kw.items() if k != "weights")),
           None if kw.get("weights") is None else kw["weights"].tobytes())
    if key not in _cache:
        _cache[key] = CC.run_oracle(p, **kw)
    return _cache[key]


def same(p, batch_slots=0, **kw):
    got = CC.run_gpu(p, batch_slots=batch_slots, **kw)
    CC.assert_same(got, reference(p, **kw), (p["kind"], len(p["corr"]), batch_slots, sorted(kw)))
    return got


# ---------------------------------------- plain, LO-budget, batch-size runs ----
@pytest.mark.parametrize("n,outliers", ((40, 0.25), (600, 0.5), (2000, 0.6)))
@pytest.mark.parametrize("kind", KINDS)
def test_plain_run_equals_the_oracle(kind, n, outliers):
    p = case(kind, n, outliers)
    M, mask, st = same(p, seed=11, max_it=5000)
    assert M is not None and mask.sum() > CC.M_OF[kind]
    assert st["local_optimization_number"] > 0                 # LO ran
    assert st["hypotheses"] > st["slots"]                      # some slot gave several models, each scored
    if n == 40:
        assert st["iteration_number"] > st["slots"]            # duplicated rows: samples without a model, retried
    else:
        assert (mask & p["truth"]).sum() >= 0.9 * p["truth"].sum()


@pytest.mark.parametrize("lo", (0, 1, 50))
@pytest.mark.parametrize("kind", KINDS)
def test_lo_budget_equals_the_oracle(kind, lo):
    M, mask, st = same(case(kind, 600), seed=12, lo=lo)
    assert M is not None and st["local_optimization_number"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_every_batch_size_equals_the_one_oracle_run(kind):
    p = case(kind, 600)
    st = reference(p, seed=13)["stats"]
    assert st["hypotheses"] > st["slots"] > 37                 # chunk boundaries fall inside the run
    for bs in (0, 1, 37, 1000):
        same(p, batch_slots=bs, seed=13)
    # a fixed count of iterations: the replay crosses many chunks of 37 slots
    st = reference(p, seed=14, min_it=1500, max_it=1500)["stats"]
    assert st["iteration_number"] >= 1500 and st["slots"] > 20 * 37
    for bs in (37, 0):
        same(p, batch_slots=bs, seed=14, min_it=1500, max_it=1500)


# ------------------ spatial coherence, no-model cases and the sharded entry ----
@pytest.mark.parametrize("cells", (4, 8))
@pytest.mark.parametrize("lam", (0.3, 0.975))
@pytest.mark.parametrize("kind", KINDS)
def test_spatial_coherence_equals_the_oracle(kind, lam, cells):
    M, mask, st = same(case(kind, 600), seed=15, lam=lam, neighborhood_size=cells)
    assert M is not None and st["graph_cut_number"] > 0       # a graph was cut


@pytest.mark.parametrize("kind", KINDS)
def test_grid_lies_over_the_pixels_in_the_oracle_too(kind):
    """Pixels, K, the image size and the threshold doubled: the normalised rows
    keep their bits and the pixel grid is scaled with the pixels, so the run is
    the same -- in the product and in the oracle, whose grid is built over the
    pixel rows it is handed."""
    p = case(kind, 600)
    K2 = p["K"].copy()
    K2[:2] *= 2.0
    p2 = dict(p, corr=2.0 * p["corr"], K=K2, thr=2.0 * p["thr"])
    size2 = tuple(2.0 * v for v in CC.SIZE)
    kw = dict(seed=5, lam=0.3, max_it=2000, neighborhood_size=4)
    a = same(p, **kw)
    b = same(p2, image_size=size2, **kw)
    assert a[2]["graph_cut_number"] > 0
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    # ... and the grid matters to the oracle: without it the labeling has no pairwise terms
    r_pix, r_none = reference(p, **kw), reference(p, **dict(kw, neighborhood_size=0))
    assert not np.array_equal(r_pix["mask"], r_none["mask"]) or r_pix["stats"] != r_none["stats"]


@pytest.mark.parametrize("kind", KINDS)
def test_no_model_cases_equal_the_oracle(kind):
    m = CC.M_OF[kind]
    p = case(kind, 600)
    rng = np.random.default_rng(21)
    noise = np.column_stack([rng.uniform(0, CC.SIZE[1], 50), rng.uniform(0, CC.SIZE[0], 50),
                             rng.uniform(0, CC.SIZE[1], 50), rng.uniform(0, CC.SIZE[0], 50)])
    cases = {"minimal size": np.ascontiguousarray(p["corr"][p["truth"]][:m]),
             "identical rows": np.tile(p["corr"][:1], (50, 1)),
             "pure outliers": np.ascontiguousarray(noise)}
    for name, rows in cases.items():
        # (random rows at a pixel's threshold would gather a sixth inlier by chance somewhere in 200 slots)
        q = dict(p, corr=rows, thr=1e-4 if name == "pure outliers" else p["thr"])
        kw = dict(seed=16, min_it=200, max_it=200)
        M, mask, st = same(q, **kw)
        assert reference(q, **kw)["num_inliers"] == 0, name
        assert M is None and not mask.any(), name
        assert st["iteration_number"] >= 200, name


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_world_one_equals_the_oracle(kind):
    p = case(kind, 800)
    fields = dict(scale_residual_thresh=p["thr"], confidence=0.99, min_iteration_number=50,
                  max_iteration_number=3000, seed=8)
    extra = dict(G1=p["G1"], G2=p["G2"]) if kind == "G" else {}
    M, masks, st, _ = D.run_problem_sharded(SOLVER[kind], p["corr"], params=fields, rank=0, world=1, device=0,
                                            K1=p["K"], K2=p["K"], **extra)
    ref = reference(p, seed=8, min_it=50, max_it=3000, confidence=0.99, lam=0.0, lo=50, neighborhood_size=0)
    CC.assert_same((M, masks[0], st), ref, kind)
    assert M is not None and st["local_optimization_number"] > 0 and st["hypotheses"] > st["slots"]


# ------------------------------------------------------------- guided runs ----
GUIDED = (("H", 600), ("F", 600), ("F", 2000), ("E", 600), ("G", 600))
# The floor of 2 iterations lies under every bound, so each run is ended by its own stop: with these weights
# the inliers hold ~0.95 of the mass, and at confidence 1 - 1e-12 the mass-based bound ends the runs after
# 13 .. 32 slots (the count-based one after 200 .. 3000).  A run ended by the floor would pin no bound at all.
GKW = dict(seed=17, min_it=2, max_it=5000, confidence=1.0 - 1e-12)
SMALL_BATCH = 5


@pytest.mark.parametrize("kind,n", GUIDED)
def test_guided_runs_equal_the_oracle_under_both_stops(kind, n):
    p = case(kind, n)
    w = CC.guided_weights(p["truth"], seed=n)
    assert (w == 0).sum() == n // 10
    off = same(p, weights=w, guided_stop=False, **GKW)
    on = same(p, weights=w, guided_stop=True, **GKW)
    # the flag was exercised, and each bound itself ended its run: not the floor, not the cap
    assert GKW["min_it"] < on[2]["iteration_number"] < off[2]["iteration_number"] < GKW["max_it"]
    for M, mask, st in (off, on):
        assert M is not None and st["local_optimization_number"] > 0
        assert (mask & p["truth"]).sum() >= 0.9 * p["truth"].sum()
    if n == 600:
        # the stops evaluated at chunk boundaries of the replay.  64-slot chunks fall inside the count-stopped
        # run only: with these weights no mass-stopped run reaches a second chunk of 64 (13 .. 24 slots), so
        # that run is also replayed in chunks of 5.
        r_off = reference(p, weights=w, guided_stop=False, **GKW)
        r_on = reference(p, weights=w, guided_stop=True, **GKW)
        assert r_off["stats"]["slots"] > 64 and r_on["stats"]["slots"] > 2 * SMALL_BATCH
        for gs in (False, True):
            same(p, batch_slots=64, weights=w, guided_stop=gs, **GKW)
        same(p, batch_slots=SMALL_BATCH, weights=w, guided_stop=True, **GKW)


@pytest.mark.parametrize("kind", ("H", "F", "E", "G"))
def test_equal_weights_make_the_mass_stop_the_count_stop(kind):
    p = case(kind, 600)
    ones = np.ones(600)
    got = CC.run_gpu(p, weights=ones, guided_stop=True, **GKW)
    CC.assert_same(got, reference(p, weights=ones, guided_stop=False, **GKW), kind)
    assert got[0] is not None and got[2]["iteration_number"] > GKW["min_it"]


# ---------------------------------------------------------------- fixtures ----
@pytest.mark.parametrize("name", CC.CALIB_NAMES)
def test_calib_fixture_is_reproduced_bitwise(name):
    p, kw, want = CC.load_calib(name)
    got = CC.run_gpu(p, **kw)
    CC.assert_same(got, want, name)
    assert got[0] is not None and got[2]["local_optimization_number"] > 0
