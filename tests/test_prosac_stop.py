"""The PROSAC stop (GCR_FLAG_PROSAC_STOP, csrc/prosac_stop.h) on the host: the
tables, the choice and the stop number against Python restatements of the
header, the wrapper's keyword, and the data the GPU whole-run test relies on."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import prosac_cases as PC
import prosac_stop_cases as Q
import pygcransac
from pygcransac import _native as N
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
MS = (2, 3, 4, 5, 7)
T_MAX = 1 << 40                          # coverage holds for every share worth naming: qmin ~ 1e-9 and below


# ---------------------------------------------------------------- tables ----
@pytest.mark.parametrize("n", (7, 20, 21, 257, 2000, 10007))
def test_tables_equal_the_restatement(n):
    for m in MS:
        for convergence in (1000, 100000):
            for conf in (0.95, 0.99):
                imin, qmin = Q.host_tables(n, m, convergence, conf)
                want_i, want_q = Q.tables_ref(n, m, convergence, conf)
                assert np.array_equal(imin, want_i), (n, m, convergence, conf)
                assert qmin.tobytes() == want_q.tobytes(), (n, m, convergence, conf)
                assert not imin[:m].any() and not qmin[:m].any()
                assert np.all(imin[m:] > m) and np.all((qmin[m:] > 0.0) & (qmin[m:] < 1.0))
                # a longer prefix needs more inliers and is covered by more slots
                assert np.all(np.diff(imin[m:].astype(np.int64)) >= 0) and np.all(np.diff(qmin[m:]) <= 0)


def test_imin_is_the_issue_formula():
    # n = 20, m = 4: 4 + ceil(1 + 1.6449 sqrt(0.95)) = 4 + ceil(2.603) = 7
    assert Q.imin_ref(20, 4) == 7
    # n = 10000, m = 7: 7 + ceil(500 + 1.6449 sqrt(475)) = 7 + ceil(535.85) = 543
    assert Q.imin_ref(10000, 7) == 543
    assert Q.MIN_LENGTH == 20 and N.FLAG_PROSAC_STOP == 4


# ---------------------------------------------------------------- choice ----
def check_choice(mask, m, imin, qmin):
    got = Q.host_choose(mask, m, imin, qmin)
    want = Q.choose_ref(mask, m, imin, qmin)
    assert got == want, (len(mask), m, got, want)
    # always at least as good as (I_N, N), a prefix, and consistent with the mask
    I_N, n = int(np.count_nonzero(mask)), len(mask)
    assert got[0] * n >= I_N * got[1] and 1 <= got[1] <= n
    assert got[0] == int(np.count_nonzero(mask[:got[1]]))
    return got


@pytest.mark.parametrize("m", MS)
def test_choice_on_random_masks(m):
    rng = np.random.default_rng(100 + m)
    for n in (m, 7, 19, 20, 21, 257, 2000):
        if n < m:
            continue
        for convergence in (1000, 100000, T_MAX):
            imin, qmin = Q.host_tables(n, m, convergence, 0.99)
            for share in (0.0, 0.05, 0.3, 0.9, 1.0):
                # inliers crowd the top of the order, as informative scores make them
                p = np.clip(share * 3.0 * np.exp(-3.0 * np.arange(n) / n), 0.0, 1.0)
                mask = (rng.random(n) < p).astype(np.uint8)
                got = check_choice(mask, m, imin, qmin)
                if n < Q.MIN_LENGTH:
                    assert got == (int(mask.sum()), n)       # only n = N qualifies
            assert check_choice(np.ones(n, dtype=np.uint8), m, imin, qmin) == (n, n)
            assert check_choice(np.zeros(n, dtype=np.uint8), m, imin, qmin) == (0, n)


def test_short_problems_choose_n_itself():
    for n in range(7, 20):
        imin, qmin = Q.host_tables(n, 4, T_MAX, 0.99)
        mask = Q.prefix_mask(n, n - 2)                           # the best prefix has share 1
        assert check_choice(mask, 4, imin, qmin) == (n - 2, n)
    # at N = 20 the only other length would be 20 itself, which is N: still n = N
    imin, qmin = Q.host_tables(20, 4, T_MAX, 0.99)
    assert check_choice(Q.prefix_mask(20, 18), 4, imin, qmin) == (18, 20)
    # at N = 21 length 20 is a candidate
    imin, qmin = Q.host_tables(21, 4, T_MAX, 0.99)
    assert check_choice(Q.prefix_mask(21, 20), 4, imin, qmin) == (20, 20)
    assert check_choice(Q.prefix_mask(21, 19), 4, imin, qmin) == (19, 20)


def test_equal_ratios_choose_the_larger_length():
    n, m = 600, 4
    imin, qmin = Q.host_tables(n, m, T_MAX, 0.99)
    # share 1 at every length up to 40
    assert check_choice(Q.prefix_mask(n, 40), m, imin, qmin) == (40, 40)
    # share 1/2 at 200 and at 400 and nowhere above it: rows 0..199 alternate
    # (outlier first), 200..299 outliers, 300..399 inliers
    mask = Q.mask_of(n, list(range(1, 200, 2)) + list(range(300, 400)))
    cum = np.cumsum(mask)
    assert cum[199] * 400 == cum[399] * 200 == 100 * 400
    assert all(2 * int(cum[k - 1]) <= k for k in range(20, n + 1))
    for k in (200, 400):
        assert Q.feasible_ref(int(cum[k - 1]), k, m, imin, qmin) == (True, True)
    assert check_choice(mask, m, imin, qmin) == (200, 400)


def test_a_prefix_that_fails_only_coverage_is_not_chosen():
    n, m = 2000, 4
    imin, qmin = Q.host_tables(n, m, 1000, 0.99)
    mask = Q.prefix_mask(n, 12)                                   # 12 of the first 20: the best share of all
    assert Q.feasible_ref(12, 20, m, imin, qmin) == (True, False)
    assert check_choice(mask, m, imin, qmin) == (12, n)
    # the same mask under a schedule that has long covered the first 20 rows
    imin2, qmin2 = Q.host_tables(n, m, T_MAX, 0.99)
    assert np.array_equal(imin, imin2)
    assert Q.feasible_ref(12, 20, m, imin2, qmin2) == (True, True)
    assert check_choice(mask, m, imin2, qmin2) == (12, 20)


def test_a_prefix_that_fails_only_non_randomness_is_not_chosen():
    n, m = 2000, 4
    imin, qmin = Q.host_tables(n, m, T_MAX, 0.99)
    mask = Q.prefix_mask(n, 5)                                    # 5 of the first 20 (Imin[20] = 7)
    assert Q.feasible_ref(5, 20, m, imin, qmin) == (False, True)
    assert all(Q.feasible_ref(5, k, m, imin, qmin)[0] is False for k in range(20, n))
    assert check_choice(mask, m, imin, qmin) == (5, n)
    assert check_choice(Q.prefix_mask(n, 7), m, imin, qmin) == (7, 20)       # at Imin it is


# ----------------------------------------------------------- stop number ----
@pytest.mark.parametrize("n", (7, 256, 10007))
def test_n_star_equal_n_is_the_uniform_stop(n):
    for m in (2, 4, 7):
        for conf in (0.95, 0.99):
            for inl in range(n + 1):
                got = Q.host_stop_number(inl, n, m, conf)
                assert got == Q.host_uniform_number(inl, n, m, conf) == Q.iteration_number_ref(inl, n, m, conf)


def test_equal_scores_reduce_to_the_uniform_stop():
    """Scores that rank nothing leave the inliers anywhere: when the choice is
    n* = N the stop is the uniform one, and whatever it is, never above it."""
    rng = np.random.default_rng(7)
    chose_n = 0
    for n, m in ((300, 4), (2000, 4), (2000, 7)):
        imin, qmin = Q.host_tables(n, m, 100000, 0.99)
        for share in (0.05, 0.2, 0.5):
            for _ in range(20):
                mask = (rng.random(n) < share).astype(np.uint8)
                bi, bn = Q.host_choose(mask, m, imin, qmin)
                uniform = Q.host_uniform_number(int(mask.sum()), n, m, 0.99)
                got = Q.host_stop_number(bi, bn, m, 0.99)
                assert got <= uniform, (n, m, share, bi, bn)
                if bn == n:
                    chose_n += 1
                    assert got == uniform
    assert chose_n > 0


def test_stop_number_branches():
    for m in (4, 7):
        assert Q.host_stop_number(0, 100, m, 0.99) == Q.U64_MAX              # the epsilon guard
        assert Q.host_stop_number(100, 100, m, 0.99) == 0                    # log(0): ceil(-0 ...) = 0
    out = C.c_uint64()
    assert N.lib.gcr_host_prosac_stop_number(1, 2, 4, 0.99, None) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop_number(1, 2, 4, 1.0, C.byref(out)) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop_number(1, 0, 4, 0.99, C.byref(out)) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop_number(3, 2, 4, 0.99, C.byref(out)) == N.GCR_EINVAL
    assert "PROSAC stop" in N.last_error()


def test_host_entry_errors():
    imin = np.zeros(11, dtype=np.uint32)
    qmin = np.zeros(11)
    ip, qp = imin.ctypes.data_as(Q.u32p), qmin.ctypes.data_as(Q.f64p)
    assert N.lib.gcr_host_prosac_stop_tables(10, 4, 1000, 0.99, None, qp) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop_tables(10, 4, 1000, 0.99, ip, None) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop_tables(3, 4, 1000, 0.99, ip, qp) == N.GCR_EINVAL           # fewer than m
    assert N.lib.gcr_host_prosac_stop_tables(10, 4, 0, 0.99, ip, qp) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop_tables(10, 4, 1000, 0.0, ip, qp) == N.GCR_EINVAL
    mask = np.zeros(10, dtype=np.uint8)
    bi, bn = C.c_uint32(), C.c_uint32()
    mp = mask.ctypes.data_as(Q.u8p)
    assert N.lib.gcr_host_prosac_stop(None, 10, 4, ip, qp, C.byref(bi), C.byref(bn)) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop(mp, 3, 4, ip, qp, C.byref(bi), C.byref(bn)) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_stop(mp, 10, 4, ip, qp, None, C.byref(bn)) == N.GCR_EINVAL


def test_header_under_sanitizers(tmp_path):
    """tests/cpp/prosac_stop_host.cpp: prosac_stop.h's tables, choice and stop
    number in a stand-alone host program built with ASan + UBSan
    (float-cast-overflow included): N = m, N = 20, n = N - 1, the largest
    products of the choice's order and the largest growth entries."""
    exe = str(tmp_path / "prosac_stop_host")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "cpp", "prosac_stop_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout


# --------------------------------------------------------------- wrapper ----
FIVE = (pygcransac.findHomography, pygcransac.findFundamentalMatrix, pygcransac.findEssentialMatrix,
        pygcransac.findGravityEssentialMatrix, pygcransac.findHomographySIFT)


def test_keyword_on_all_five_signatures():
    for fn in FIVE:
        par = inspect.signature(fn).parameters["prosac_stop"]
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    assert N.FLAG_PROSAC_STOP == 4 and N.FLAG_GUIDED_STOP == 2 and N.FLAG_NO_LO == 1


def test_python_keyword_errors():
    corr, truth, _, thr = S.problem_h(200, 0.5, seed=5)
    img = (S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W)
    for fn in (pygcransac.findHomography, pygcransac.findFundamentalMatrix):
        with pytest.raises(ValueError, match="prosac_stop"):
            fn(corr, *img, threshold=thr, sampler=0, prosac_stop=True)
        with pytest.raises(ValueError, match="prosac_stop"):
            fn(corr, *img, probabilities=np.ones(len(corr)), threshold=thr, sampler=3, prosac_stop=True)
    K = np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 480.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="prosac_stop"):
        pygcransac.findEssentialMatrix(corr, K, K, *img, threshold=thr, sampler=0, prosac_stop=True)
    with pytest.raises(ValueError, match="prosac_stop"):
        pygcransac.findGravityEssentialMatrix(corr, K, K, np.eye(3), np.eye(3), *img, threshold=thr, sampler=0,
                                              prosac_stop=True)
    rows8 = S.problem_hs(200, 0.5, seed=5)[0]
    with pytest.raises(ValueError, match="prosac_stop"):
        pygcransac.findHomographySIFT(rows8, *img, threshold=thr, sampler=0, prosac_stop=True)


# -------------------------------------------- the GPU whole-run test's data ----
@pytest.mark.parametrize("solver", (PC.H4, PC.F7))
def test_whole_run_data_stops_at_the_iteration_floor(solver):
    """tests/test_gpu_prosac_stop.py holds its runs to min_iters = 50 and asserts
    that the flag ends them below the uniform bound: on this data the stop of
    the truth-inlier set in score order picks a short prefix and needs no more
    than the floor, while the uniform bound is beyond any budget."""
    corr, truth, thr, scores = Q.e2e_problem(solver)
    m = PC.M_OF[solver]
    mask = truth[PC.order_of(scores)].astype(np.uint8)
    n = len(mask)
    imin, qmin = Q.host_tables(n, m, PC.DEFAULT_CONVERGENCE, Q.E2E_CONF)
    bi, bn = Q.host_choose(mask, m, imin, qmin)
    assert (bi, bn) == Q.choose_ref(mask, m, imin, qmin)
    stop = Q.host_stop_number(bi, bn, m, Q.E2E_CONF)
    uniform = Q.host_uniform_number(int(mask.sum()), n, m, Q.E2E_CONF)
    print(f"solver {solver}: I* {bi}, n* {bn}, stop {stop}, uniform {uniform}")
    assert bn < n
    assert stop <= Q.E2E_MIN_ITERS
    assert uniform > Q.E2E_MAX_ITERS
