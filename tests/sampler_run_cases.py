"""Shared by the whole-run oracle tests of PROSAC runs (sampler=1, with and
without prosac_stop), NAPSAC runs (sampler=2) and the homography from two SIFT
correspondences (kind "S"): the cases, the quality scores, one call signature
for the product and the oracle, the seeds chosen on the CPU and the recorded
fixtures of tests/golden/samplers.  The bitwise comparison is
calibrated_cases.assert_same.

What the oracle side is given it works out by itself: the PROSAC row order
(not pygcransac.prosac_order), NAPSAC's extents and local length (not
pygcransac.napsac_extent), and it scatters the sorted run's mask back, so the
wrapper's sort, unsort and defaults are under test with everything else."""
from __future__ import annotations

import math
import os

import numpy as np

import calibrated_cases as CC
import oracle_ffi as O
from pygcransac import synthetic as S

SIZE = CC.SIZE                                       # h1, w1, h2, w2
KINDS = ("H", "F", "E", "G", "S")
M_OF = dict(CC.M_OF, S=2)
COUNTS = CC.COUNTS
assert_same = CC.assert_same
DEFAULT_CONVERGENCE = 100000
DUPLICATES = (7, 11, 17, 22, 28)                     # rows of a 40-row case that are copies of row 3


def problem(kind, n, outliers, seed):
    """calibrated_cases.problem plus kind "S": corr is (n, 8), the rows of
    problem_h with their SIFT columns."""
    if kind != "S":
        return CC.problem(kind, n, outliers, seed)
    corr, truth, _, thr = S.problem_hs(n, outliers, seed=seed)
    return dict(kind="S", corr=np.ascontiguousarray(corr), truth=truth, thr=thr)


def small_problem(kind):
    """The 40-row cases: duplicated rows make samples without a model, so
    slots take several attempts.  E and G are calibrated_cases'; H, F and S
    are 30 inliers and 10 outliers of their synthetic problem with five rows
    overwritten by a copy of row 3 (for S the SIFT columns with them)."""
    if kind in ("E", "G"):
        return CC.small_problem(kind)
    p = problem(kind, 40, 0.25, seed=41)
    rows = p["corr"].copy()
    for i in DUPLICATES:
        rows[i] = rows[3]
        p["truth"][i] = p["truth"][3]
    return dict(p, corr=np.ascontiguousarray(rows))


def quality_scores(truth, seed):
    """Informative scores with ties: N(2, 1) for the truth rows, N(0, 1) for
    the others, quantised to 0.25."""
    rng = np.random.default_rng(seed)
    q = rng.normal(0.0, 1.0, len(truth)) + np.where(truth, 2.0, 0.0)
    q = np.round(q * 4.0) / 4.0
    assert len(np.unique(q)) < len(q)                # ties exist: the sort's stability matters
    return q


def flat_scores(n):
    """Scores that carry no order beyond the rows' own: -arange(n)."""
    return -np.arange(n, dtype=np.float64)


def quality_order(scores):
    """PROSAC's row order stated on its own: score descending, ties by row."""
    return sorted(range(len(scores)), key=lambda i: (-scores[i], i))


def extent_of(rows4, image_size):
    """NAPSAC's extents (w1, h1, w2, h2) from the image size h1, w1, h2, w2; a
    size that is not a positive finite number is the largest finite
    coordinate of that column + 1, at least 1."""
    h1, w1, h2, w2 = (float(v) for v in image_size)
    out = []
    for col, v in enumerate((w1, h1, w2, h2)):
        if not (v > 0.0 and math.isfinite(v)):
            c = np.asarray(rows4, dtype=np.float64)[:, col]
            c = c[np.isfinite(c)]
            v = max(1.0, float(c.max()) + 1.0) if c.size else 1.0
        out.append(v)
    return tuple(out)


def local_length(napsac_iterations, n):
    """NAPSAC's T: the argument, or half the rows rounded up."""
    return max(1, (n + 1) // 2) if napsac_iterations is None else int(napsac_iterations)


def run_gpu(p, *, seed, min_it=50, max_it=5000, confidence=0.99, lam=0.0, lo=50, neighborhood_size=8, batch_slots=0,
            weights=None, guided_stop=False, image_size=SIZE, sampler=0, scores=None,
            prosac_convergence=DEFAULT_CONVERGENCE, prosac_stop=False, napsac_iterations=None):
    """(M or None, mask, stats) of the product's entry point of p's kind."""
    import pygcransac

    kw = dict(threshold=p["thr"], conf=confidence, spatial_coherence_weight=lam, max_iters=max_it, min_iters=min_it,
              lo_number=lo, neighborhood_size=neighborhood_size, seed=seed, device=0, batch_slots=batch_slots,
              return_stats=True)
    if weights is not None:
        kw.update(probabilities=weights, sampler=3, guided_stop=guided_stop)
    elif sampler == 1:
        kw.update(probabilities=scores, sampler=1, prosac_convergence=prosac_convergence, prosac_stop=prosac_stop)
    elif sampler == 2:
        kw.update(sampler=2, napsac_iterations=napsac_iterations)
    k = p["kind"]
    if k == "H":
        return pygcransac.findHomography(p["corr"], *image_size, **kw)
    if k == "F":
        return pygcransac.findFundamentalMatrix(p["corr"], *image_size, **kw)
    if k == "S":
        return pygcransac.findHomographySIFT(p["corr"], *image_size, **kw)
    if k == "E":
        return pygcransac.findEssentialMatrix(p["corr"], p["K"], p["K"], *image_size, **kw)
    return pygcransac.findGravityEssentialMatrix(p["corr"], p["K"], p["K"], p["G1"], p["G2"], *image_size, **kw)


def oracle_arguments(p, *, sampler=0, scores=None, prosac_convergence=DEFAULT_CONVERGENCE, prosac_stop=False,
                     napsac_iterations=None, image_size=SIZE):
    """(rows the oracle runs on, the order they were taken in or None, its
    sampler keywords)."""
    rows, order, kw = p["corr"], None, {}
    if sampler == 1:
        order = np.array(quality_order(scores), dtype=np.int64)
        rows = np.ascontiguousarray(rows[order])
        kw = dict(sampler=1, prosac_convergence=prosac_convergence, prosac_stop=prosac_stop)
    elif sampler == 2:
        kw = dict(sampler=2, napsac_extent=extent_of(rows[:, :4], image_size),
                  napsac_iterations=local_length(napsac_iterations, len(rows)))
    return rows, order, kw


def run_oracle(p, *, seed, min_it=50, max_it=5000, confidence=0.99, lam=0.0, lo=50, neighborhood_size=8,
               weights=None, guided_stop=False, image_size=SIZE, sampler=0, scores=None,
               prosac_convergence=DEFAULT_CONVERGENCE, prosac_stop=False, napsac_iterations=None):
    """The oracle's run of the same call (batch_slots has no meaning there).
    A PROSAC run is made on the rows in quality order and its mask scattered
    back to the caller's order; "prosac_star" is (I*, n*) of the last stop
    update of a prosac_stop run."""
    from pygcransac import pygcransac as P

    rows, order, skw = oracle_arguments(p, sampler=sampler, scores=scores, prosac_convergence=prosac_convergence,
                                        prosac_stop=prosac_stop, napsac_iterations=napsac_iterations,
                                        image_size=image_size)
    kw = dict(min_it=min_it, max_it=max_it, confidence=confidence, lam=lam, lo=lo, seed=seed, **skw)
    k = p["kind"]
    if k in ("H", "F", "S"):
        if neighborhood_size:
            kw.update(cell_size=P.grid_cell_sizes(rows[:, :4], *image_size, neighborhood_size),
                      cell_number=neighborhood_size)
        fn = {"H": O.find_homography_guided, "F": O.find_fundamental_guided, "S": O.find_homography_sift}[k]
        ref = fn(rows, p["thr"], weights, guided_stop, **kw)
    else:
        kw.update(weights=weights, guided_stop=guided_stop, image_size=image_size,
                  neighborhood_size=neighborhood_size)
        if k == "E":
            ref = O.find_essential(rows, p["K"], p["K"], p["thr"], **kw)
        else:
            ref = O.find_gravity_essential(rows, p["K"], p["K"], p["G1"], p["G2"], p["thr"], **kw)
    if order is not None:
        mask = np.zeros(len(rows), dtype=bool)
        mask[order] = ref["mask"]
        ref = dict(ref, mask=mask, sorted_mask=ref["mask"])
    return ref


# ---- the runs of the GPU tests, their seeds chosen on the CPU ---------------------
# test_oracle_samplers.py asserts on the oracle alone that each of these runs
# does what its test is about (LO ran, the phase it ends in, which stop ended
# it, more slots than two chunks), so the GPU comparison is never vacuous.
N_MAIN = 600
DATA_SEED = 7600                                     # problem(kind, 600, 0.5, DATA_SEED)
# kind -> (seed of quality_scores, seed of the run): with these the flagged run
# ends after more than 10 slots and strictly between the floor and the clear
# run's count, under both convergence lengths, and its last (I*, n*) has n* < N.
# (With most seeds the best-ranked rows are all inliers and the first slots
# already end an H or F run.)
PROSAC_SEEDS = {"H": (1, 3), "F": (0, 0), "E": (0, 0), "G": (1, 2), "S": (11, 4)}
CONVERGENCES = (1000, 100000)
# a fixed count long enough for the convergence-1000 run to pass g[N] (about 1400)
# (a homography run spends 4 .. 5 iterations per slot on samples that fail the orientation test)
CROSS_KW = dict(min_it=12000, max_it=12000, confidence=0.99)
# kind -> (seed of the random order, seed of the run) under which the PROSAC stop chooses n* = N at every update of
# a run whose scores carry no order.  With a minimal sample of 2 every order tried on the 600 rows has a prefix that
# wins, so the S case has 200 rows (the fewer prefixes, the smaller the bias).
FLAT_CASES = {"H": (9, 0), "F": (2, 0), "E": (2, 0), "G": (133, 0), "S": (9, 0)}
# PROSAC, flag clear: the uniform stop at confidence 0.99
PROSAC_KW = dict(min_it=50, max_it=5000, confidence=0.99)
# PROSAC, flag clear against flag set: a floor of 2 iterations and a confidence
# so high that the floor ends no run, as GKW does for guided runs
PSTOP_KW = dict(min_it=2, max_it=5000, confidence=1.0 - 1e-12)
NAPSAC_T = 200


def main_problem(kind):
    return problem(kind, N_MAIN, 0.5, seed=DATA_SEED)


def main_scores(kind):
    return quality_scores(main_problem(kind)["truth"], PROSAC_SEEDS[kind][0])


def flat_case(kind):
    """(problem, scores without order, run seed) of FLAT_CASES"""
    p = problem("S", 200, 0.5, seed=DATA_SEED) if kind == "S" else main_problem(kind)
    order_seed, seed = FLAT_CASES[kind]
    n = len(p["corr"])
    return p, np.random.default_rng(order_seed).permutation(n).astype(np.float64), seed


def local_problem():
    """NAPSAC's own case, a homography whose inliers are a local structure:
    120 inliers in a quarter x quarter window among 480 outliers."""
    corr, truth, _, thr = S.problem_h_local(N_MAIN, 0.8, seed=DATA_SEED)
    return dict(kind="H", corr=corr, truth=truth, thr=thr)


# ---- tests/golden/samplers: recorded oracle runs ----------------------------------
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samplers")
GOLDEN_NAMES = ("h_prosac_stop_n500", "f_napsac_n500", "s_uniform_n40", "e_prosac_n40")
GOLDEN_PARAMS = {
    "h_prosac_stop_n500": dict(seed=0, sampler=1, prosac_convergence=1000, prosac_stop=True, **PSTOP_KW,
                               lam=0.3, lo=50, neighborhood_size=8),
    "f_napsac_n500": dict(seed=20251121, sampler=2, napsac_iterations=NAPSAC_T, min_it=50, max_it=5000,
                          confidence=0.99, lam=0.3, lo=50, neighborhood_size=8),
    "s_uniform_n40": dict(seed=20251121, min_it=50, max_it=2000, confidence=0.99, lam=0.0, lo=50,
                          neighborhood_size=8),
    "e_prosac_n40": dict(seed=20251121, sampler=1, prosac_convergence=1000, min_it=300, max_it=2000,
                         confidence=0.99, lam=0.0, lo=50, neighborhood_size=8),
}
# seeds of the fixtures' quality scores: the flagged H run ends by its own stop after 13 slots (254 with the flag
# clear), the E run's best-ranked rows are not the duplicated ones (138 slots in 300 iterations)
GOLDEN_SCORE_SEED = {"h_prosac_stop_n500": 12, "e_prosac_n40": 9}
INT_KEYS = ("seed", "min_it", "max_it", "lo", "neighborhood_size", "sampler", "prosac_convergence",
            "napsac_iterations")


def golden_problem(name):
    """(problem, scores or None) a fixture of that name is generated from."""
    kind = name[0].upper()
    p = small_problem(kind) if name.endswith("n40") else problem(kind, 500, 0.5, seed=3500)
    scores = quality_scores(p["truth"], GOLDEN_SCORE_SEED[name]) if name in GOLDEN_SCORE_SEED else None
    return p, scores


def save_golden(name, p, scores, kw, ref):
    d = dict(correspondences=p["corr"], thr=np.float64(p["thr"]),
             params=np.array([-1 if kw.get(k) is None else int(kw[k]) for k in INT_KEYS], dtype=np.int64),
             prosac_stop=np.uint8(bool(kw.get("prosac_stop", False))), confidence=np.float64(kw["confidence"]),
             lam=np.float64(kw["lam"]), num_inliers=np.int64(ref["num_inliers"]),
             mask=np.packbits(ref["mask"].astype(np.uint8)), M=ref["H"],
             stats=np.array([ref["stats"][k] for k in COUNTS], dtype=np.int64), score=np.float64(ref["stats"]["score"]))
    if scores is not None:
        d["scores"] = scores
    for k in ("K", "G1", "G2"):
        if k in p:
            d[k] = p[k]
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN_DIR, name + ".npz"), **d)


def load_golden(name):
    """(problem, run keywords of run_gpu / run_oracle, expected result in
    run_oracle's layout) of a fixture."""
    d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    p = dict(kind=name[0].upper(), corr=d["correspondences"], thr=float(d["thr"]))
    for k in ("K", "G1", "G2"):
        if k in d.files:
            p[k] = d[k]
    kw = {k: int(v) for k, v in zip(INT_KEYS, d["params"]) if int(v) >= 0}
    kw.update(confidence=float(d["confidence"]), lam=float(d["lam"]))
    if bool(d["prosac_stop"]):
        kw["prosac_stop"] = True
    if "scores" in d.files:
        kw["scores"] = d["scores"]
    n = len(p["corr"])
    want = dict(num_inliers=int(d["num_inliers"]), mask=np.unpackbits(d["mask"])[:n].astype(bool), H=d["M"],
                stats=dict(zip(COUNTS, (int(v) for v in d["stats"])), score=float(d["score"])))
    return p, kw, want
