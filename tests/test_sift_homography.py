"""Homography from two SIFT correspondences, host side: csrc/sifth.h's 2-point
solver on exact data against the ground truth and against its eight
constraints restated in numpy, the rejected samples, the host twin of the
generator, the Python and C entry points' errors.  No GPU."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

import sift_homography_cases as SC
import pygcransac
from pygcransac import _native as N
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
N_SAMPLES = 300
# The distance of the best model from H_GT (h_distance): a restatement with an
# SVD null space and numpy.roots reached 8.1e-10 on such samples; the bound is
# three orders above that.
TRUTH_TOL = 1e-6
# Relative residual of the eight constraints of every returned model
# (constraint_residuals): measured 1.9e-15 at worst over the 300 samples; the
# bound is 100 x that and must stay below 1e-6.  The worst distance from H_GT
# measured beside it is 6.3e-10.
RESIDUAL_MEASURED = 1.9e-15
RESIDUAL_TOL = 100 * RESIDUAL_MEASURED
SEED = 0x5EEDFACE12345678


@pytest.fixture(scope="module")
def exact():
    """problem_hs without outliers and without noise, and 300 seeded samples of two rows"""
    rows, truth, H, _ = S.problem_hs(400, 0.0, seed=3, noise=0.0, scale_noise=0.0, angle_noise=0.0)
    assert truth.all()
    rng = np.random.default_rng(20261020)
    pairs = [rng.choice(len(rows), 2, replace=False) for _ in range(N_SAMPLES)]
    return rows, H, pairs


def test_exact_samples_return_the_truth_and_satisfy_the_constraints(exact):
    rows, H, pairs = exact
    assert RESIDUAL_TOL < 1e-6
    worst = worst_res = 0.0
    counts = np.zeros(SC.PER + 1, dtype=int)
    for idx in pairs:
        models = SC.solve_s2(rows, idx)
        counts[len(models)] += 1
        assert 1 <= len(models) <= 4, idx             # (the solver's own limit is 3: a cubic)
        worst = max(worst, min(SC.h_distance(m, H) for m in models))
        for m in models:
            assert m[8] == 1.0 and np.all(np.isfinite(m))
            worst_res = max(worst_res, SC.constraint_residuals(m, rows[idx]).max())
            assert SC.orientation_maps_forward(m, rows[idx]), idx
    print(f"models per sample {counts.tolist()}, worst distance of the best model from H_GT {worst:.3g} "
          f"(bound {TRUTH_TOL:g}), worst relative constraint residual {worst_res:.3g} (bound {RESIDUAL_TOL:g})")
    assert worst < TRUTH_TOL
    assert worst_res < RESIDUAL_TOL


def test_the_sample_order_gives_the_same_models_up_to_rounding(exact):
    rows, H, pairs = exact
    for idx in pairs[:40]:
        a, b = SC.solve_s2(rows, idx), SC.solve_s2(rows, idx[::-1])
        assert len(a) == len(b)
        assert min(SC.h_distance(m, H) for m in b) < TRUTH_TOL


def test_coincident_points_return_no_model(exact):
    rows, _, pairs = exact
    r = rows[pairs[0]].copy()
    both = r.copy()
    both[1, :4] = both[0, :4]
    assert len(SC.solve_s2(both)) == 0
    first = r.copy()
    first[1, :2] = first[0, :2]                     # coincide in the first image only
    assert len(SC.solve_s2(first)) == 0
    second = r.copy()
    second[1, 2:4] = second[0, 2:4]                 # ... in the second image only
    assert len(SC.solve_s2(second)) == 0
    assert len(SC.solve_s2(r)) >= 1


def test_an_opposite_orientation_returns_no_model_near_the_truth(exact):
    rows, H, pairs = exact
    for idx in pairs[:60]:
        for which in (0, 1):
            r = rows[idx].copy()
            r[which, 7] += math.pi
            for m in SC.solve_s2(r):
                assert SC.h_distance(m, H) > 1e-3, (idx, which)


def test_parallel_orientations_are_outside_the_chart(exact):
    """Both orientations of the second image equal: the first six columns of the
    linear system are dependent, the sample is rejected (csrc/sifth.h (b))."""
    rows, _, pairs = exact
    r = rows[pairs[1]].copy()
    r[1, 7] = r[0, 7]
    models = SC.solve_s2(r)
    assert len(models) == 0


def test_bad_sift_columns_are_value_errors_naming_the_column(exact):
    rows, _, _ = exact
    size = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)
    for col, name in ((4, "q1"), (5, "q2")):
        for bad in (0.0, -1.0, np.nan, np.inf):
            r = rows[:50].copy()
            r[7, col] = bad
            with pytest.raises(ValueError, match=name):
                pygcransac.findHomographySIFT(r, *size)
            assert N.lib.gcr_host_check_sift(np.ascontiguousarray(r[:, 4:]).ctypes.data, 50) == N.GCR_EINVAL
            assert name in N.last_error() and "row 7" in N.last_error()
    for col, name in ((6, "alpha1"), (7, "alpha2")):
        for bad in (np.nan, -np.inf):
            r = rows[:50].copy()
            r[49, col] = bad
            with pytest.raises(ValueError, match=name):
                pygcransac.findHomographySIFT(r, *size)
    assert SC.check_sift(rows[:, 4:]) == N.GCR_OK


@pytest.mark.parametrize("guided", (False, True), ids=("uniform", "guided"))
def test_host_twin_is_thread_independent_and_equals_the_solver(guided):
    rows, truth, _, _ = S.problem_hs(257, 0.25, seed=41)
    for i in (7, 11, 17, 22, 28):
        rows[i] = rows[3]
    w = np.where(truth, 1.0, 0.05) if guided else None
    nslots, slot0 = 256, 2 ** 32 - 100
    inc1, m1 = SC.host_generate(rows, w, SEED, slot0, nslots, threads=1)
    inc16, m16 = SC.host_generate(rows, w, SEED, slot0, nslots, threads=16)
    assert np.array_equal(inc1, inc16) and np.array_equal(m1.view(np.uint64), m16.view(np.uint64))
    won = inc1[:, 0] <= 101
    assert won.all() and (inc1[:, 0] > 1).any()
    live = np.column_stack([won, inc1[:, 1:] == 0])
    # the winning attempt's sample through the solver: the slot's models
    import guided_cases as G
    for s in range(64):
        a = int(inc1[s, 0]) - 1
        idx = (G.host_samples(SEED, slot0 + s, 1, a, w, 2) if guided
               else G.host_samples_uniform(SEED, slot0 + s, 1, a, len(rows), 2))[0]
        got = SC.solve_s2(rows, idx)
        assert len(got) == live[s].sum()
        assert np.array_equal(got.view(np.uint64), m1[s, :len(got)].view(np.uint64))


def test_host_twin_packs_a_many_model_sample():
    """Samples with two models are about 1e-5 of all; TWO_MODEL_PAIR is one, in either order of its rows."""
    rows = SC.TWO_MODEL_PAIR
    assert len(SC.solve_s2(rows)) == 2 and len(SC.solve_s2(rows[::-1])) == 2
    inc, m = SC.host_generate(rows, None, SEED, 0, 64, threads=2)
    assert (inc == [1, 0, 255]).all()
    both = {SC.solve_s2(rows).tobytes(), SC.solve_s2(rows[::-1]).tobytes()}
    assert {m[s, :2].tobytes() for s in range(64)} <= both
    assert (m[:, 2] == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]).all()


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/sifth_host.cpp: the solver over seeded homographies and over
    degenerate and non-finite samples, a stand-alone host program built with
    ASan + UBSan."""
    exe = str(tmp_path / "sifth_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "sifth_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout


def test_problem_hs_is_problem_h_plus_consistent_columns():
    rows, truth, H, thr = S.problem_hs(400, 0.5, seed=5)
    corr, truth_h, _, _ = S.problem_h(400, 0.5, seed=5)
    assert rows.shape == (400, 8) and np.array_equal(rows[:, :4], corr) and np.array_equal(truth, truth_h)
    assert (rows[:, 4] >= 2.0).all() and (rows[:, 4] <= 30.0).all() and (rows[:, 5] > 0).all()
    exact, _, _, _ = S.problem_hs(400, 0.5, seed=5, noise=0.0, scale_noise=0.0, angle_noise=0.0)
    res = SC.constraint_residuals(H, exact)
    assert res[truth].max() < 1e-12 and np.median(res[~truth].max(axis=1)) > 1e-3
    # the noise levels: 5 % on the size ratio, 2 degrees on alpha2
    dq = np.log(rows[truth, 5] / exact[truth, 5])
    da = rows[truth, 7] - exact[truth, 7]
    assert 0.04 < dq.std() < 0.06 and math.radians(1.6) < da.std() < math.radians(2.4)


# --------------------------------------------------------------------- API --
def test_signature():
    find = pygcransac.findHomographySIFT
    ref = inspect.signature(pygcransac.findHomography).parameters
    sig = inspect.signature(find).parameters
    assert list(sig) == list(ref)
    for name in sig:
        assert sig[name].default == ref[name].default and sig[name].kind == ref[name].kind, name
    assert "findHomographySIFT" in pygcransac.__all__
    assert N.SOLVER_HOMOGRAPHY2_SIFT == 7


def _message(fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    return str(e.value)


def test_python_value_errors_are_find_homographys():
    rows = S.problem_hs(50, 0.5, seed=2)[0]
    size = (960, 1280, 960, 1280)
    ones = np.ones(50)
    fs, fh = pygcransac.findHomographySIFT, pygcransac.findHomography
    # the column and row counts: findHomography's sentence, with this entry's 8 columns
    assert _message(fs, rows[:, :7], *size) == _message(fh, rows[:, :3], *size).replace(
        "4 columns", "8 columns").replace("has 3 columns", "has 7 columns")
    assert _message(fs, rows[:3], *size) == _message(fh, rows[:3, :4], *size).replace(
        "4 columns", "8 columns").replace("has 4 columns", "has 8 columns")
    assert "at least 4 rows" in _message(fs, rows[:3], *size)
    for bad in (1, 2, 4):
        assert _message(fs, rows, *size, probabilities=ones, sampler=bad) == \
            _message(fh, rows[:, :4], *size, probabilities=ones, sampler=bad)
    assert _message(fs, rows, *size, probabilities=ones, sampler=0) == \
        _message(fh, rows[:, :4], *size, probabilities=ones, sampler=0)
    assert _message(fs, rows, *size, sampler=3) == _message(fh, rows[:, :4], *size, sampler=3)
    assert _message(fs, rows, *size, guided_stop=True) == _message(fh, rows[:, :4], *size, guided_stop=True)
    assert "guided_stop" in _message(fs, rows, *size, sampler=0, guided_stop=True)
    few = np.zeros(50)
    few[:1] = 1.0
    assert "at least 2 probabilities > 0, got 1" in _message(fs, rows, *size, probabilities=few, sampler=3)


def test_c_entry_errors():
    rows = np.ascontiguousarray(S.problem_hs(8, 0.5, seed=2)[0])
    corr, sift = np.ascontiguousarray(rows[:, :4]), np.ascontiguousarray(rows[:, 4:])
    h = C.c_void_p()
    rc = N.lib.gcr_problem_create(None, N.SOLVER_HOMOGRAPHY2_SIFT, corr.ctypes.data_as(SC.dpt), 8, None, 0, C.byref(h))
    assert rc == N.GCR_EINVAL and "gcr_problem_create_sift_homography" in N.last_error()
    create = N.lib.gcr_problem_create_sift_homography
    assert create(None, corr.ctypes.data, None, 8, C.byref(h)) == N.GCR_EINVAL
    p = N.default_params()
    find = N.lib.gcr_find_homography_sift
    # a null context: the columns are checked before anything touches a device
    bad = sift.copy()
    bad[5, 1] = 0.0
    rc = find(None, corr.ctypes.data, bad.ctypes.data, 8, None, C.byref(p), None, None, None)
    assert rc == N.GCR_EINVAL
    rc = create(None, corr.ctypes.data, bad.ctypes.data, 8, C.byref(h))
    assert rc == N.GCR_EINVAL
    assert find(None, corr.ctypes.data, sift.ctypes.data, 3, None, C.byref(p), None, None, None) == N.GCR_EINVAL
    assert "at least 4" in N.last_error()
    # gcr_host_solve_minimal cannot carry the columns; the new entries check their arguments
    models, cnt = np.zeros(27), C.c_uint32()
    idx = np.array([0, 1], dtype=np.uint32)
    rc = N.lib.gcr_host_solve_minimal(N.SOLVER_HOMOGRAPHY2_SIFT, corr.ctypes.data_as(SC.dpt), 8,
                                      idx.ctypes.data_as(SC.u32p), models.ctypes.data_as(SC.dpt), C.byref(cnt))
    assert rc == N.GCR_EINVAL and "gcr_host_solve_s2" in N.last_error()
    idx = np.array([0, 8], dtype=np.uint32)
    assert N.lib.gcr_host_solve_s2(corr.ctypes.data, sift.ctypes.data, 8, idx.ctypes.data, models.ctypes.data,
                                   C.byref(cnt)) == N.GCR_EINVAL
    inc, out = np.zeros(3, dtype=np.uint8), np.zeros(27)
    assert N.lib.gcr_host_generate_s(corr.ctypes.data, sift.ctypes.data, 1, None, 1, 0, 1, 1, inc.ctypes.data,
                                     out.ctypes.data) == N.GCR_EINVAL      # fewer than 2 rows
    assert N.lib.gcr_host_generate_s(corr.ctypes.data, sift.ctypes.data, 2, None, 1, 0, 1, 1, inc.ctypes.data,
                                     out.ctypes.data) == N.GCR_OK
