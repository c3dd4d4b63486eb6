"""Shared by the whole-run oracle tests of the calibrated kinds (essential
matrix, essential matrix with known gravity) and of guided runs: the cases,
the guided weight vectors, one call signature for the product and the oracle,
and the bitwise comparison of the two results."""
from __future__ import annotations

import os

import numpy as np

import oracle_ffi as O
from gcr_testutil import bits
from pygcransac import synthetic as S

SIZE = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)          # h1, w1, h2, w2
M_OF = {"H": 4, "F": 7, "E": 5, "G": 3}
COUNTS = ("iteration_number", "local_optimization_number", "graph_cut_number", "slots", "hypotheses")
CALIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calib")
CALIB_NAMES = ("e_n40", "e_n500", "g_n40", "g_n500")


def problem(kind, n, outliers, seed):
    """dict(kind, corr, truth, thr[, K][, G1, G2]) of pygcransac.synthetic's problem of that kind."""
    if kind == "H":
        corr, truth, _, thr = S.problem_h(n, outliers, seed=seed)
        return dict(kind=kind, corr=corr, truth=truth, thr=thr)
    if kind == "F":
        corr, truth, _, thr = S.problem_f(n, outliers, seed=seed)
        return dict(kind=kind, corr=corr, truth=truth, thr=thr)
    if kind == "E":
        corr, truth, K, _, thr = S.problem_e(n, outliers, seed=seed)
        return dict(kind=kind, corr=corr, truth=truth, thr=thr, K=K)
    corr, truth, K, G1, G2, _ = S.problem_g(n, outliers, seed=seed)
    return dict(kind=kind, corr=corr, truth=truth, thr=1.0, K=K, G1=np.ascontiguousarray(G1),
                G2=np.ascontiguousarray(G2))


def small_problem(kind):
    """The 40-row cases of the GPU tests: duplicated rows make samples without
    a model, so slots take several attempts."""
    if kind == "E":
        from test_gpu_essential import small_problem as sp

        rows, K, w = sp()
        return dict(kind="E", corr=rows, truth=w == 1.0, thr=1.0, K=K)
    from test_gpu_gravity_essential import small_problem as sp

    rows, K, G1, G2, w = sp(40)
    return dict(kind="G", corr=rows, truth=w == 1.0, thr=1.0, K=K, G1=np.ascontiguousarray(G1),
                G2=np.ascontiguousarray(G2))


def guided_weights(truth, seed):
    """1 for inliers, 0.05 for outliers, then 10 % of the rows (inliers and
    outliers alike) set to 0; far more than 7 rows keep a positive weight."""
    w = np.where(truth, 1.0, 0.05)
    rng = np.random.default_rng(seed)
    w[rng.choice(len(w), len(w) // 10, replace=False)] = 0.0
    assert int((w > 0).sum()) >= 7
    return w


def run_gpu(p, *, seed, min_it=50, max_it=5000, confidence=0.99, lam=0.0, lo=50, neighborhood_size=8, batch_slots=0,
            weights=None, guided_stop=False, image_size=SIZE):
    """(M or None, mask, stats) of the product's entry point of p's kind."""
    import pygcransac

    kw = dict(threshold=p["thr"], conf=confidence, spatial_coherence_weight=lam, max_iters=max_it, min_iters=min_it,
              lo_number=lo, neighborhood_size=neighborhood_size, seed=seed, device=0, batch_slots=batch_slots,
              return_stats=True)
    if weights is not None:
        kw.update(probabilities=weights, sampler=3, guided_stop=guided_stop)
    k = p["kind"]
    if k == "H":
        return pygcransac.findHomography(p["corr"], *image_size, **kw)
    if k == "F":
        return pygcransac.findFundamentalMatrix(p["corr"], *image_size, **kw)
    if k == "E":
        return pygcransac.findEssentialMatrix(p["corr"], p["K"], p["K"], *image_size, **kw)
    return pygcransac.findGravityEssentialMatrix(p["corr"], p["K"], p["K"], p["G1"], p["G2"], *image_size, **kw)


def run_oracle(p, *, seed, min_it=50, max_it=5000, confidence=0.99, lam=0.0, lo=50, neighborhood_size=8,
               weights=None, guided_stop=False, image_size=SIZE):
    """The oracle's run of the same call (batch_slots has no meaning there)."""
    from pygcransac import pygcransac as P

    kw = dict(min_it=min_it, max_it=max_it, confidence=confidence, lam=lam, lo=lo, seed=seed)
    k = p["kind"]
    if k in ("H", "F"):
        if neighborhood_size:
            kw.update(cell_size=P.grid_cell_sizes(p["corr"], *image_size, neighborhood_size),
                      cell_number=neighborhood_size)
        fn = O.find_homography_guided if k == "H" else O.find_fundamental_guided
        return fn(p["corr"], p["thr"], weights, guided_stop, **kw)
    kw.update(weights=weights, guided_stop=guided_stop, image_size=image_size, neighborhood_size=neighborhood_size)
    if k == "E":
        return O.find_essential(p["corr"], p["K"], p["K"], p["thr"], **kw)
    return O.find_gravity_essential(p["corr"], p["K"], p["K"], p["G1"], p["G2"], p["thr"], **kw)


def assert_same(got, ref, what=""):
    """test_fundamental._assert_same for any kind: mask, model bytes,
    bits(score) and the five counts, no tolerance anywhere."""
    M, mask, st = got
    rs = ref["stats"]
    assert np.array_equal(mask, ref["mask"]), what
    for k in COUNTS:
        assert st[k] == rs[k], (what, k, st[k], rs[k])
    assert bits(st["score"]) == bits(rs["score"]), what
    if ref["num_inliers"] == 0:
        assert M is None, what
    else:
        assert M is not None and np.array_equal(bits(M), bits(ref["H"])), what


def sampson(rows, E):
    """Squared Sampson distance of (n, 4) rows to E (3, 3), in numpy."""
    E = np.reshape(E, (3, 3))
    h1 = np.column_stack([rows[:, :2], np.ones(len(rows))])
    h2 = np.column_stack([rows[:, 2:], np.ones(len(rows))])
    a, b = h1 @ E.T, h2 @ E
    num = np.einsum("ij,ij->i", h2, a)
    return num * num / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


# ---- tests/golden/calib: recorded oracle runs ---------------------------------
CALIB_PARAMS = {
    "e_n40": dict(seed=20251121, min_it=50, max_it=2000, confidence=0.99, lam=0.0, lo=50, neighborhood_size=8),
    "g_n40": dict(seed=20251121, min_it=50, max_it=2000, confidence=0.99, lam=0.0, lo=50, neighborhood_size=8),
    "e_n500": dict(seed=20251121, min_it=50, max_it=5000, confidence=0.99, lam=0.3, lo=50, neighborhood_size=8),
    "g_n500": dict(seed=20251121, min_it=50, max_it=5000, confidence=0.99, lam=0.3, lo=50, neighborhood_size=8),
}
PARAM_KEYS = ("seed", "min_it", "max_it", "lo", "neighborhood_size")


def calib_problem(name):
    """The problem a fixture of that name is generated from."""
    kind = name[0].upper()
    return small_problem(kind) if name.endswith("n40") else problem(kind, 500, 0.5, seed=3500)


def load_calib(name):
    """(problem, run parameters, expected result in run_oracle's layout) of a fixture."""
    d = np.load(os.path.join(CALIB_DIR, name + ".npz"))
    kind = name[0].upper()
    p = dict(kind=kind, corr=d["correspondences"], thr=float(d["thr"]), K=d["K1"])
    assert np.array_equal(d["K1"], d["K2"])
    if kind == "G":
        p.update(G1=d["G1"], G2=d["G2"])
    kw = {k: int(v) for k, v in zip(PARAM_KEYS, d["params"])}
    kw.update(confidence=float(d["confidence"]), lam=float(d["lam"]))
    n = len(p["corr"])
    want = dict(num_inliers=int(d["num_inliers"]), mask=np.unpackbits(d["mask"])[:n].astype(bool), H=d["M"],
                stats=dict(zip(COUNTS, (int(v) for v in d["stats"])), score=float(d["score"])))
    return p, kw, want
