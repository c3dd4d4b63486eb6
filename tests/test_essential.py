"""Essential-matrix estimator, host side: csrc/ess.h's 5-point solver and the
non-minimal fit against an independent numpy restatement
(tests/essential_cases.py), degenerate samples, the Python and C entry
points' errors, the threshold normalisation.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import essential_cases as EC
import pygcransac
from pygcransac import _native as N
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
N_CASES = 320
FILTER = 1e-9           # the restatement's closest model to +-E_gt (kept cases)
CONTRACT = 1e-6         # the project's contract for the host solver on kept cases


@pytest.fixture(scope="module")
def minimal_cases():
    """(rows, E_gt, restatement's distance) of N_CASES seeded 5-point scenes,
    computed once."""
    rng = np.random.default_rng(20261019)
    out = []
    for _ in range(N_CASES):
        rows, E = EC.scene(rng, 5)
        out.append((rows, E, EC.closest(EC.ref_solve(rows), E)))
    return out


def host_basis(rows):
    """ess.h's step 2 restated: the elimination basis ((e5..e8) = unit vectors)
    of the null space, then Gram-Schmidt: X, Y, Z, W up to rounding."""
    _, _, vt = np.linalg.svd(EC.epipolar_rows(rows))
    Nn = vt[5:9].T                                  # 9 x 4
    V = Nn @ np.linalg.inv(Nn[5:9, :])              # columns with (e5..e8) = unit vectors
    Q = []
    for k in range(4):
        v = V[:, k].copy()
        for _ in range(2):
            for q in Q:
                v -= (q @ v) * q
        Q.append(v / np.linalg.norm(v))
    return Q


def test_host_solver_against_the_restatement(minimal_cases):
    kept = [(r, E) for r, E, d in minimal_cases if d < FILTER]
    assert len(kept) >= 0.9 * N_CASES, f"the restatement lost {N_CASES - len(kept)} of {N_CASES} cases"
    worst = 0.0
    for rows, E in kept:
        models = EC.solve_minimal(rows)
        d = EC.closest(models, E)
        worst = max(worst, d)
        assert d < CONTRACT, (d, rows.tolist())
    print(f"kept {len(kept)} of {N_CASES}, worst distance {worst:.3e}")


def test_models_are_valid_and_in_root_order(minimal_cases):
    A_of = EC.epipolar_rows
    many = 0
    for rows, _, _ in minimal_cases:
        models = EC.solve_minimal(rows)
        assert len(models) <= 10
        assert np.all(np.isfinite(models))
        many += len(models) >= 4
        if not len(models):
            continue
        assert np.allclose(np.linalg.norm(models, axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.abs(A_of(rows) @ models.T).max() < 1e-6           # the five epipolar equations
        for m in models:
            Em = m.reshape(3, 3)
            assert abs(np.linalg.det(Em)) < 1e-6
            assert np.abs(2.0 * Em @ Em.T @ Em - np.trace(Em @ Em.T) * Em).max() < 1e-6
        # ascending root order: z = (E . Z) / (E . W) on the orthonormal basis
        _, _, Z, W = host_basis(rows)
        z = (models @ Z) / (models @ W)
        assert np.all(np.diff(z) > 0), z
    assert many > N_CASES // 4


def test_nonminimal_fit_against_the_restatement():
    rng = np.random.default_rng(7)
    cases, kept = 60, 0
    for _ in range(cases):
        rows, E = EC.scene(rng, 35)
        if EC.closest(EC.ref_solve(rows), E) >= FILTER:
            continue
        kept += 1
        idx = rng.permutation(35)
        got = EC.host_fit(rows, idx)
        assert got is not None
        assert abs(np.linalg.norm(got) - 1.0) < 1e-12
        assert EC.dist_pm(got.reshape(3, 3), E) < CONTRACT
    assert kept >= 0.9 * cases


def test_fit_of_five_is_the_minimal_solvers_first_model(minimal_cases):
    checked = 0
    for rows, _, _ in minimal_cases[:100]:
        models = EC.solve_minimal(rows)
        got = EC.host_fit(rows, np.arange(5))
        if not len(models):
            assert got is None
            continue
        assert got.view(np.uint64).tolist() == models[0].view(np.uint64).tolist()
        checked += 1
    assert checked >= 90
    rows = minimal_cases[0][0]
    assert N.lib.gcr_host_fit_e(rows.ctypes.data_as(EC.dpt), 5, np.arange(4, dtype=np.uint32).ctypes.data_as(EC.u32p),
                                4, np.zeros(9).ctypes.data_as(EC.dpt)) == 0          # fewer than 5: rejected


def test_degenerate_samples_give_no_model(minimal_cases):
    same = np.tile([0.25, -0.5, 0.125, 0.75], (5, 1))
    assert len(EC.solve_minimal(same)) == 0
    t = np.arange(5) * 0.1 - 0.2
    line = np.column_stack([0.3 + t, -0.1 + 2.0 * t, 0.05 + 1.5 * t, 0.2 - 0.5 * t])
    assert len(EC.solve_minimal(line)) == 0
    old = np.seterr(all="raise")                   # numpy's own traps stay quiet too
    try:
        for bad in (np.nan, np.inf, -np.inf):
            for at in range(20):
                rows = minimal_cases[at][0].copy()
                rows[at // 4, at % 4] = bad
                assert len(EC.solve_minimal(rows)) == 0
                assert EC.host_fit(rows, np.arange(5)) is None
    finally:
        np.seterr(**old)


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/ess_host.cpp: the minimal solver and the fit over seeded
    scenes and the degenerate samples, a stand-alone host program built with
    ASan + UBSan."""
    exe = str(tmp_path / "ess_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                           "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "ess_host.cpp"),
                           os.path.join(CSRC, "host_fit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout


# --------------------------------------------------------------------- API --
def test_signature():
    names = list(inspect.signature(pygcransac.findEssentialMatrix).parameters)
    assert names[:15] == ["correspondences", "K1", "K2", "h1", "w1", "h2", "w2", "probabilities", "threshold", "conf",
                          "spatial_coherence_weight", "max_iters", "min_iters", "sampler", "lo_number"]
    sig = inspect.signature(pygcransac.findEssentialMatrix).parameters
    assert (sig["threshold"].default, sig["conf"].default, sig["spatial_coherence_weight"].default,
            sig["max_iters"].default, sig["min_iters"].default, sig["sampler"].default,
            sig["lo_number"].default) == (1.0, 0.99, 0.975, 10000, 50, 0, 50)
    for kw in ("neighborhood_size", "seed", "device", "batch_slots", "return_stats", "guided_stop"):
        assert sig[kw].kind is inspect.Parameter.KEYWORD_ONLY
    assert "findEssentialMatrix" in pygcransac.__all__
    assert N.SOLVER_ESSENTIAL5 == 5


K_OK = np.array([[1000.0, 0.5, 640.0], [0.0, 990.0, 480.0], [0.0, 0.0, 1.0]])     # skew allowed


def _bad_K():
    def with_(i, j, v):
        K = K_OK.copy()
        K[i, j] = v
        return K
    return {"third row x": with_(2, 0, 1e-9), "third row y": with_(2, 1, -1.0), "third row w": with_(2, 2, 2.0),
            "K10": with_(1, 0, 0.1), "fx zero": with_(0, 0, 0.0), "fx negative": with_(0, 0, -1000.0),
            "fy zero": with_(1, 1, 0.0), "nan": with_(0, 2, np.nan), "inf focal": with_(1, 1, np.inf),
            "inf skew": with_(0, 1, -np.inf), "shape": np.eye(4), "vector": np.ones(9)}


def test_python_value_errors():
    find = pygcransac.findEssentialMatrix
    corr = np.random.default_rng(0).uniform(0, 900, (50, 4))
    size = (960, 1280, 960, 1280)
    ones = np.ones(50)
    with pytest.raises(ValueError, match="at least 5 rows"):
        find(corr[:4], K_OK, K_OK, *size)
    with pytest.raises(ValueError, match="4 columns"):
        find(corr[:, :3], K_OK, K_OK, *size)
    for name, K in _bad_K().items():
        with pytest.raises(ValueError, match="K1"):
            find(corr, K, K_OK, *size)
        with pytest.raises(ValueError, match="K2"):
            find(corr, K_OK, K, *size)
    for bad in (1, 2, 4):
        with pytest.raises(ValueError, match="sampler"):
            find(corr, K_OK, K_OK, *size, probabilities=ones, sampler=bad)
    with pytest.raises(ValueError, match="sampler"):
        find(corr, K_OK, K_OK, *size, probabilities=ones, sampler=0)
    with pytest.raises(ValueError, match="probabilities"):
        find(corr, K_OK, K_OK, *size, sampler=3)
    for wrong in (np.ones(49), np.ones(51), np.ones((50, 1))):
        with pytest.raises(ValueError, match="one entry per correspondence"):
            find(corr, K_OK, K_OK, *size, probabilities=wrong, sampler=3)
    few = np.zeros(50)
    few[:4] = 1.0
    with pytest.raises(ValueError, match="at least 5 probabilities > 0, got 4"):
        find(corr, K_OK, K_OK, *size, probabilities=few, sampler=3)
    with pytest.raises(ValueError, match="guided_stop"):
        find(corr, K_OK, K_OK, *size, guided_stop=True)
    with pytest.raises(ValueError, match="guided_stop"):
        find(corr, K_OK, K_OK, *size, sampler=0, guided_stop=True)


def test_c_entry_errors():
    corr = np.zeros((8, 4))
    h = C.c_void_p()
    # no calibration: EINVAL whatever else is passed, the message names the new entry
    rc = N.lib.gcr_problem_create(None, N.SOLVER_ESSENTIAL5, corr.ctypes.data_as(EC.dpt), 8, None, 0, C.byref(h))
    assert rc == N.GCR_EINVAL and "gcr_problem_create_essential" in N.last_error()
    k = np.ascontiguousarray(K_OK)
    assert N.lib.gcr_problem_create_essential(None, corr.ctypes.data, 8, None, k.ctypes.data, C.byref(h)) == N.GCR_EINVAL
    assert N.lib.gcr_problem_create_essential(None, corr.ctypes.data, 8, k.ctypes.data, None, C.byref(h)) == N.GCR_EINVAL
    p = N.default_params()
    assert N.lib.gcr_find_essential_matrix(None, corr.ctypes.data, 8, k.ctypes.data, None, None, C.byref(p), None,
                                           None, None) == N.GCR_EINVAL
    for name, K in _bad_K().items():
        if np.shape(K) != (3, 3):
            continue
        kb = np.ascontiguousarray(K, dtype=np.float64)
        rc = N.lib.gcr_host_essential_normalise(None, 0, kb.ctypes.data, k.ctypes.data, 1.0, None, None)
        assert rc == N.GCR_EINVAL and "K1" in N.last_error(), name
        rc = N.lib.gcr_host_essential_normalise(None, 0, k.ctypes.data, kb.ctypes.data, 1.0, None, None)
        assert rc == N.GCR_EINVAL and "K2" in N.last_error(), name
    # the minimal solver's index check
    models, cnt = np.zeros(90), C.c_uint32()
    idx = np.array([0, 1, 2, 3, 8], dtype=np.uint32)
    assert N.lib.gcr_host_solve_minimal(N.SOLVER_ESSENTIAL5, corr.ctypes.data_as(EC.dpt), 8, idx.ctypes.data_as(EC.u32p),
                                        models.ctypes.data_as(EC.dpt), C.byref(cnt)) == N.GCR_EINVAL


def test_normalisation_and_threshold_follow_the_formula():
    corr, _, K, E, thr = S.problem_e(200, 0.5, seed=3, noise=0.0)
    K2 = K_OK
    got, t = EC.normalise(corr, K, K2, thr)
    assert t == thr / ((K[0, 0] + K[1, 1] + K2[0, 0] + K2[1, 1]) / 4.0)
    # x^ = K^-1 x, against numpy's inverse
    h1 = np.column_stack([corr[:, :2], np.ones(len(corr))]) @ np.linalg.inv(K).T
    h2 = np.column_stack([corr[:, 2:], np.ones(len(corr))]) @ np.linalg.inv(K2).T
    assert np.allclose(got[:, :2], h1[:, :2], rtol=1e-13, atol=1e-15)
    assert np.allclose(got[:, 2:], h2[:, :2], rtol=1e-13, atol=1e-15)
    # problem_e's truth: noise-free inliers satisfy x^2^T E x^1 = 0 in normalised coordinates
    both, _ = EC.normalise(corr, K, K, thr)
    truth = S.problem_e(200, 0.5, seed=3, noise=0.0)[1]
    res = np.abs(EC.epipolar_rows(both) @ E.reshape(9))
    assert res[truth].max() < 1e-12 and np.median(res[~truth]) > 1e-3
    assert abs(np.linalg.norm(E) - 1.0) < 1e-15
