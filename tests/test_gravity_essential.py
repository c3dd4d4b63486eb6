"""Essential matrix with known gravity, host side: csrc/grav.h's 3-point solver
and the constrained non-minimal fit against an independent numpy restatement
(tests/gravity_cases.py), the constrained form of every model, degenerate
samples, the Python and C entry points' errors.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import gravity_cases as GC
import pygcransac
from pygcransac import _native as N
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
N_CASES = 320
# Measured over the kept cases (317 of 320): the worst distance of a model of
# gcr_host_solve_g3 from the restatement's is 5.4e-9 (the worst cases are the
# ones whose quartic has two roots 1e-3 apart: the roots' own conditioning).
# The bound is 10 x that, for libm and ordering differences between numpy and
# the header.  The structure figures (constrained_form) are 1.0e-15 at worst;
# their bound is the same factor over that.
WORST_MEASURED = 5.4e-9
TOL = 10 * WORST_MEASURED
STRUCT_MEASURED = 1.0e-15
STRUCT_TOL = 10 * STRUCT_MEASURED
# Noisy fit (0.5 px, k = 50 of 80 inliers): over 300 scenes the worst Sampson
# cost over E_gt's on the fitted rows is 6.0 (median 1.17, 99th percentile
# 3.8: an algebraic fit, then the projection), and 6.0 over the 40 scenes used
# here; the stated factor is 10.
NOISY_MEASURED = 6.0
NOISY_FACTOR = 10.0


@pytest.fixture(scope="module")
def minimal_cases():
    """(rows (3, 4), G1, G2, E_gt, restatement's models, well posed) of N_CASES
    seeded samples: ten samples of three inliers from each of 32 noise-free
    problem_g scenes, computed once."""
    rng = np.random.default_rng(20261020)
    out = []
    for case in range(N_CASES):
        rows, G1, G2, E = GC.scene(1000 + case // 10)
        r3 = np.ascontiguousarray(rows[rng.choice(len(rows), 3, replace=False)])
        ref, well, rem = GC.ref_solve(r3, G1, G2)
        out.append((r3, G1, G2, E, ref, well, rem))
    return out


def test_host_solver_against_the_restatement(minimal_cases):
    kept = [c for c in minimal_cases if c[5]]
    assert len(kept) >= 0.95 * N_CASES, f"the restatement left out {N_CASES - len(kept)} of {N_CASES} cases"
    worst = worst_truth = 0.0
    for r3, G1, G2, E, ref, _, _ in kept:
        got = GC.solve_g3(r3, G1, G2)
        assert len(got) == len(ref), (len(got), len(ref), r3.tolist())
        for a, b in zip(got, ref):                              # both in ascending root order
            d = GC.dist_pm(a.reshape(3, 3), b)
            worst = max(worst, d)
            assert d < TOL, (d, r3.tolist())
        # one model is the truth, as closely as the restatement's own
        d_ref = min(GC.dist_pm(b, E) for b in ref)
        d_got = min(GC.dist_pm(a.reshape(3, 3), E) for a in got)
        worst_truth = max(worst_truth, d_got)
        assert d_ref < TOL and d_got < d_ref + TOL, (d_ref, d_got)
    print(f"kept {len(kept)} of {N_CASES}, worst distance to the restatement {worst:.3e}, to E_gt {worst_truth:.3e}")


def test_the_sextic_is_divisible_by_one_plus_s_squared(minimal_cases):
    assert max(c[6] for c in minimal_cases) < 1e-12          # the remainder grav.h drops, relative


def test_models_have_the_constrained_form(minimal_cases):
    many = 0
    for r3, G1, G2, _, _, _, _ in minimal_cases:
        got = GC.solve_g3(r3, G1, G2)
        assert len(got) <= 4 and np.all(np.isfinite(got))
        many += len(got) == 4
        for m in got:
            assert abs(np.linalg.norm(m) - 1.0) < 1e-12
            assert GC.constrained_form(m, G1, G2) < STRUCT_TOL
            h1 = np.column_stack([r3[:, :2], np.ones(3)])
            h2 = np.column_stack([r3[:, 2:], np.ones(3)])
            assert np.abs(np.einsum("ij,jk,ik->i", h2, m.reshape(3, 3), h1)).max() < 1e-9     # the three equations
    assert many > N_CASES // 4


@pytest.mark.parametrize("k", (5, 8, 50))
def test_fit_of_exact_inliers_recovers_the_truth(k):
    rng = np.random.default_rng(7 + k)
    for seed in range(2000, 2020):
        rows, G1, G2, E = GC.scene(seed)
        idx = rng.permutation(len(rows))[:k]
        got = GC.host_fit(rows, idx, G1, G2)
        assert got is not None
        assert abs(np.linalg.norm(got) - 1.0) < 1e-12
        assert GC.constrained_form(got, G1, G2) < STRUCT_TOL
        assert GC.dist_pm(got.reshape(3, 3), E) < TOL, (seed, k)


def test_fit_of_noisy_inliers_keeps_the_form_and_the_cost():
    rng = np.random.default_rng(5)
    worst = 0.0
    for seed in range(2000, 2040):
        rows, G1, G2, E = GC.scene(seed, n=80, noise=0.5)
        idx = rng.permutation(len(rows))[:50]
        got = GC.host_fit(rows, idx, G1, G2)
        assert got is not None
        assert GC.constrained_form(got, G1, G2) < STRUCT_TOL
        ratio = GC.sampson(rows[idx], got).sum() / GC.sampson(rows[idx], E).sum()
        worst = max(worst, ratio)
        assert ratio < NOISY_FACTOR, (seed, ratio)
    print(f"worst Sampson cost over E_gt's: {worst:.2f}")


def test_fit_of_three_and_four_is_the_minimal_solvers_first_model(minimal_cases):
    checked = 0
    for r3, G1, G2, _, _, _, _ in minimal_cases[:100]:
        rows = np.ascontiguousarray(np.concatenate([r3, r3[:1] + 0.01]))
        models = GC.solve_g3(rows, G1, G2)
        for idx in (np.arange(3), np.arange(4)):
            got = GC.host_fit(rows, idx, G1, G2)
            if not len(models):
                assert got is None
                continue
            assert got.view(np.uint64).tolist() == models[0].view(np.uint64).tolist()
            checked += 1
    assert checked >= 180
    r3, G1, G2 = minimal_cases[0][:3]
    assert GC.host_fit(r3, np.arange(2), G1, G2) is None       # fewer than 3: no model


def _pure_rotation(rows, G1, G2, angle):
    p = np.column_stack([rows[:3, 0], rows[:3, 1], np.ones(3)])
    R = G2.T @ GC.ry(np.cos(angle), np.sin(angle)) @ G1
    q = p @ R.T
    return np.ascontiguousarray(np.column_stack([p[:, 0], p[:, 1], q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]]))


def test_degenerate_samples_give_no_model_or_finite_ones(minimal_cases):
    rows, G1, G2, _ = GC.scene(2000)
    eye = np.eye(3)
    t = np.arange(3) * 0.1
    cases = {
        "three identical rows": (np.tile([0.25, -0.5, 0.125, 0.75], (3, 1)), eye, eye, True),
        "all-zero rows": (np.zeros((3, 4)), G1, G2, True),
        "collinear rays": (np.column_stack([0.3 + t, -0.1 + 2.0 * t, 0.05 + 1.5 * t, 0.2 - 0.5 * t]), eye, eye, False),
        "pure rotation": (_pure_rotation(rows, G1, G2, 0.2), G1, G2, False),
        "no motion": (np.column_stack([rows[:3, :2], rows[:3, :2]]), eye, eye, True),
    }
    old = np.seterr(all="raise")                   # numpy's own traps stay quiet too
    try:
        for name, (r3, g1, g2, none) in cases.items():
            r3 = np.ascontiguousarray(r3)
            got = GC.solve_g3(r3, g1, g2)
            assert np.all(np.isfinite(got)), name
            if none:
                assert len(got) == 0, name
            for k in (3, 4, 6):                    # n = 3 exactly, and the constrained fit on repeated rows
                fit = GC.host_fit(np.ascontiguousarray(np.tile(r3, (2, 1))), np.arange(k), g1, g2)
                assert fit is None or np.all(np.isfinite(fit)), name
        for bad in (np.nan, np.inf, -np.inf):
            for at in range(12):
                r3, g1, g2 = (np.array(v, copy=True) for v in minimal_cases[at][:3])
                r3[at // 4, at % 4] = bad
                assert len(GC.solve_g3(r3, g1, g2)) == 0
                assert GC.host_fit(r3, np.arange(3), g1, g2) is None
    finally:
        np.seterr(**old)


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/grav_host.cpp: the minimal solver and the fit over seeded
    scenes and the degenerate samples, a stand-alone host program built with
    ASan + UBSan."""
    exe = str(tmp_path / "grav_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                           "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "grav_host.cpp"),
                           os.path.join(CSRC, "host_fit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout


def test_problem_g_is_consistent():
    corr, truth, K, G1, G2, E = S.problem_g(400, 0.5, seed=3, noise=0.0)
    assert corr.shape == (400, 4) and truth.sum() == 200
    for G in (G1, G2):
        assert np.abs(G @ G.T - np.eye(3)).max() < 1e-12 and np.linalg.det(G) > 0
    rows, _ = GC.normalise(corr, K, K, 1.0)
    assert GC.constrained_form(E, G1, G2) < 1e-12 and abs(np.linalg.norm(E) - 1.0) < 1e-15
    res = np.sqrt(GC.sampson(rows, E))
    assert res[truth].max() < 1e-12 and np.median(res[~truth]) > 1e-3
    assert (corr >= 0).all() and (corr[:, 0::2] < S.IMG_W).all() and (corr[:, 1::2] < S.IMG_H).all()


# --------------------------------------------------------------------- API --
def test_signature():
    find = pygcransac.findGravityEssentialMatrix
    names = list(inspect.signature(find).parameters)
    assert names[:17] == ["correspondences", "K1", "K2", "gravity_source", "gravity_destination", "h1", "w1", "h2", "w2",
                          "probabilities", "threshold", "conf", "spatial_coherence_weight", "max_iters", "min_iters",
                          "sampler", "lo_number"]
    sig = inspect.signature(find).parameters
    assert (sig["threshold"].default, sig["conf"].default, sig["spatial_coherence_weight"].default,
            sig["max_iters"].default, sig["min_iters"].default, sig["sampler"].default,
            sig["lo_number"].default) == (1.0, 0.99, 0.975, 10000, 50, 0, 50)
    for kw in ("neighborhood_size", "seed", "device", "batch_slots", "return_stats", "guided_stop"):
        assert sig[kw].kind is inspect.Parameter.KEYWORD_ONLY
    assert "findGravityEssentialMatrix" in pygcransac.__all__
    assert N.SOLVER_ESSENTIAL3_GRAVITY == 6


K_OK = np.array([[1000.0, 0.5, 640.0], [0.0, 990.0, 480.0], [0.0, 0.0, 1.0]])
G_OK = S._rot(0.1, -0.05, 0.07)


def _bad_G():
    scaled = G_OK * (1.0 + 1e-6)
    sheared = G_OK.copy()
    sheared[0, 1] += 1e-6
    nan = G_OK.copy()
    nan[1, 2] = np.nan
    inf = G_OK.copy()
    inf[0, 0] = np.inf
    return {"scaled": scaled, "sheared": sheared, "reflection": np.diag([1.0, -1.0, 1.0]) @ G_OK, "zero": np.zeros((3, 3)),
            "nan": nan, "inf": inf, "shape": np.eye(4), "vector": np.ones(9)}


def test_python_value_errors():
    find = pygcransac.findGravityEssentialMatrix
    corr = np.random.default_rng(0).uniform(0, 900, (50, 4))
    size = (960, 1280, 960, 1280)
    ones = np.ones(50)
    with pytest.raises(ValueError, match="at least 3 rows"):
        find(corr[:2], K_OK, K_OK, G_OK, G_OK, *size)
    with pytest.raises(ValueError, match="4 columns"):
        find(corr[:, :3], K_OK, K_OK, G_OK, G_OK, *size)
    for name, G in _bad_G().items():
        with pytest.raises(ValueError, match="gravity_source"):
            find(corr, K_OK, K_OK, G, G_OK, *size)
        with pytest.raises(ValueError, match="gravity_destination"):
            find(corr, K_OK, K_OK, G_OK, G, *size)
    with pytest.raises(ValueError, match="K1"):
        find(corr, np.eye(4), K_OK, G_OK, G_OK, *size)
    with pytest.raises(ValueError, match="K2"):
        find(corr, K_OK, -K_OK, G_OK, G_OK, *size)
    for bad in (1, 2, 4):
        with pytest.raises(ValueError, match="sampler"):
            find(corr, K_OK, K_OK, G_OK, G_OK, *size, probabilities=ones, sampler=bad)
    with pytest.raises(ValueError, match="sampler"):
        find(corr, K_OK, K_OK, G_OK, G_OK, *size, probabilities=ones, sampler=0)
    with pytest.raises(ValueError, match="probabilities"):
        find(corr, K_OK, K_OK, G_OK, G_OK, *size, sampler=3)
    for wrong in (np.ones(49), np.ones(51), np.ones((50, 1))):
        with pytest.raises(ValueError, match="one entry per correspondence"):
            find(corr, K_OK, K_OK, G_OK, G_OK, *size, probabilities=wrong, sampler=3)
    few = np.zeros(50)
    few[:2] = 1.0
    with pytest.raises(ValueError, match="at least 3 probabilities > 0, got 2"):
        find(corr, K_OK, K_OK, G_OK, G_OK, *size, probabilities=few, sampler=3)
    with pytest.raises(ValueError, match="guided_stop"):
        find(corr, K_OK, K_OK, G_OK, G_OK, *size, guided_stop=True)
    with pytest.raises(ValueError, match="guided_stop"):
        find(corr, K_OK, K_OK, G_OK, G_OK, *size, sampler=0, guided_stop=True)


def test_c_entry_errors():
    corr = np.zeros((8, 4))
    h = C.c_void_p()
    k, g = np.ascontiguousarray(K_OK), np.ascontiguousarray(G_OK)
    # no calibration, no rotations: EINVAL whatever else is passed, the message names the new entry
    rc = N.lib.gcr_problem_create(None, N.SOLVER_ESSENTIAL3_GRAVITY, corr.ctypes.data_as(GC.dpt), 8, None, 0, C.byref(h))
    assert rc == N.GCR_EINVAL and "gcr_problem_create_gravity_essential" in N.last_error()
    create = N.lib.gcr_problem_create_gravity_essential
    assert create(None, corr.ctypes.data, 8, None, k.ctypes.data, g.ctypes.data, g.ctypes.data, C.byref(h)) == N.GCR_EINVAL
    rc = create(None, corr.ctypes.data, 8, k.ctypes.data, k.ctypes.data, None, g.ctypes.data, C.byref(h))
    assert rc == N.GCR_EINVAL and "gravity_source" in N.last_error()
    rc = create(None, corr.ctypes.data, 8, k.ctypes.data, k.ctypes.data, g.ctypes.data, None, C.byref(h))
    assert rc == N.GCR_EINVAL and "gravity_destination" in N.last_error()
    p = N.default_params()
    find = N.lib.gcr_find_gravity_essential_matrix
    for name, G in _bad_G().items():
        if np.shape(G) != (3, 3):
            continue
        gb = np.ascontiguousarray(G, dtype=np.float64)
        # a null context: the rotations are checked before anything touches a device
        rc = find(None, corr.ctypes.data, 8, k.ctypes.data, k.ctypes.data, gb.ctypes.data, g.ctypes.data, None,
                  C.byref(p), None, None, None)
        assert rc == N.GCR_EINVAL and "gravity_source" in N.last_error(), name
        rc = find(None, corr.ctypes.data, 8, k.ctypes.data, k.ctypes.data, g.ctypes.data, gb.ctypes.data, None,
                  C.byref(p), None, None, None)
        assert rc == N.GCR_EINVAL and "gravity_destination" in N.last_error(), name
        assert N.lib.gcr_host_check_gravity(gb.ctypes.data, g.ctypes.data) == N.GCR_EINVAL
        assert N.lib.gcr_host_check_gravity(g.ctypes.data, gb.ctypes.data) == N.GCR_EINVAL
    assert N.lib.gcr_host_check_gravity(g.ctypes.data, g.ctypes.data) == N.GCR_OK
    # an orthonormality error of 1e-10 passes (the bound is 1e-9)
    near = np.ascontiguousarray(G_OK * (1.0 + 4e-11))
    assert N.lib.gcr_host_check_gravity(near.ctypes.data, g.ctypes.data) == N.GCR_OK
    # gcr_host_solve_minimal cannot carry the rotations; the new entry checks its indices
    models, cnt = np.zeros(36), C.c_uint32()
    idx = np.array([0, 1, 2], dtype=np.uint32)
    rc = N.lib.gcr_host_solve_minimal(N.SOLVER_ESSENTIAL3_GRAVITY, corr.ctypes.data_as(GC.dpt), 8,
                                      idx.ctypes.data_as(GC.u32p), models.ctypes.data_as(GC.dpt), C.byref(cnt))
    assert rc == N.GCR_EINVAL and "gcr_host_solve_g3" in N.last_error()
    idx = np.array([0, 1, 8], dtype=np.uint32)
    assert N.lib.gcr_host_solve_g3(corr.ctypes.data, 8, idx.ctypes.data, g.ctypes.data, g.ctypes.data,
                                   models.ctypes.data, C.byref(cnt)) == N.GCR_EINVAL
    inc, out = np.zeros(4, dtype=np.uint8), np.zeros(36)
    assert N.lib.gcr_host_generate_g(corr.ctypes.data, 2, g.ctypes.data, g.ctypes.data, None, 1, 0, 1, 1,
                                     inc.ctypes.data, out.ctypes.data) == N.GCR_EINVAL      # fewer than 3 rows
