"""Guided (importance) sampling, host side: csrc/guided.h's definition against
an independent numpy restatement, the draw frequencies, the host minimal
solver against the oracle's slot models, and the API's errors.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guided_cases as G
import oracle_ffi as O
import pygcransac
from pygcransac import _native as N
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
GCR_EINTERNAL = -1                     # include/gcr.h: the draw budget ran out
# (seed, slot, attempt); the third has a 64-bit seed and a slot past 2^40
ADDRESSES = ((0, 0, 0), (7, 12345, 1), (0xDEADBEEFCAFEF00D, (1 << 40) + 3, 100), ((1 << 63) + 5, (1 << 32) - 1, 17))


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.mark.parametrize("n", G.NS)
@pytest.mark.parametrize("pattern", G.PATTERNS)
def test_host_sampler_equals_the_restated_definition(pattern, n):
    for m in (4, 7):
        w = G.weights(pattern, n, m)
        if int((w > 0).sum()) < m:
            rc, _ = G.host_sample_guided(0, 0, 0, w, m)
            assert rc == N.GCR_EINVAL and "probabilities > 0" in N.last_error()
            continue
        c = G.cdf_of(w)
        # a budget that runs out costs 4096 restated draws: two addresses are enough there
        for seed, slot, a in (ADDRESSES[:2] if pattern == "heavy" else ADDRESSES):
            want = G.ref_sample(c, seed, slot, a, m)
            rc, got = G.host_sample_guided(seed, slot, a, w, m)
            if want is None:
                assert rc == GCR_EINTERNAL, (pattern, n, m, seed, slot, a)
                continue
            assert rc == 0, N.last_error()
            assert got.tolist() == want, (pattern, n, m, seed, slot, a)
            assert np.all(w[got] > 0)                      # a zero weight is never drawn
            if pattern == "exactly_m":                     # a permutation of the positive entries
                assert sorted(got.tolist()) == np.nonzero(w)[0].tolist()


def test_heavy_entry_forces_repeats():
    """With 90 % of the mass on one entry a sample of 7 needs repeats: the
    restated stream consumes more than 7 words, and the engine agrees with it."""
    n, m = 1000, 7
    w = G.weights("heavy90", n, m)
    c = G.cdf_of(w)
    total = float(c[-1])
    repeats = 0
    for slot in range(32):
        want = G.ref_sample(c, 3, slot, 0, m)
        rc, got = G.host_sample_guided(3, slot, 0, w, m)
        assert rc == 0 and got.tolist() == want
        seen = set()
        for W in G.words(3, slot, 0):
            i = int(np.searchsorted(c, float(W >> 11) * 2.0 ** -53 * total, side="right"))
            repeats += i in seen
            seen.add(i)
            if len(seen) == m:
                break
    assert repeats > 32


def test_draw_frequencies_follow_the_weights():
    w = np.array([0, 1, 2, 3, 0, 4, 0, 6], dtype=np.float64)
    draws = 16000
    counts = np.zeros(8, dtype=np.int64)
    out = np.zeros(1, dtype=np.uint32)
    for slot in range(draws):
        rc = N.lib.gcr_host_sample_guided(20251121, slot, 0, 0, 0, w.ctypes.data, 8, 1, out.ctypes.data_as(G.u32p))
        assert rc == 0
        counts[out[0]] += 1
    assert np.all(counts[w == 0] == 0)
    # 5 sigma of a binomial at 16 000 draws (sigma <= 0.004)
    assert np.all(np.abs(counts / draws - w / 16.0) < 0.02), counts / draws


@pytest.mark.parametrize("solver", (N.SOLVER_HOMOGRAPHY4, N.SOLVER_FUNDAMENTAL7))
def test_host_minimal_solver_equals_the_oracle_slot_models(solver):
    """Uniform slots: the indices the oracle samples at the attempt its slot
    reports, solved by gcr_host_solve_minimal, give the oracle's slot models
    bit for bit (H, and every one of F's up to three models)."""
    if solver == N.SOLVER_HOMOGRAPHY4:
        corr, m, slot_of = S.problem_h(500, 0.5, seed=5)[0], 4, O.h_slot
    else:
        corr, m, slot_of = S.problem_f(800, 0.5, seed=6)[0], 7, O.f_slot
    n = corr.shape[0]
    seed = 0x123456789ABCDEF
    checked = 0
    for slot in range(64):
        inc, models = slot_of(corr, seed, slot)
        if inc > 101:
            continue
        models = np.asarray(models).reshape(-1, 9)
        idx = O.sample(seed, slot, inc - 1, 0, 0, n, m)
        got = G.solve_minimal(solver, corr, idx)
        assert got.shape == models.shape, (slot, inc)
        assert np.array_equal(got.view(np.uint64), models.view(np.uint64)), (slot, inc)
        for a in range(inc - 1):                           # the earlier attempts gave no model
            assert len(G.solve_minimal(solver, corr, O.sample(seed, slot, a, 0, 0, n, m))) == 0
        checked += 1
    assert checked >= 60


def test_two_level_search_equals_flat_search_at_every_edge(tmp_path):
    """tests/cpp/guided_search.cpp: the two-level index, the flat index and (up
    to N = 1000) a linear scan of the definition agree at every CDF entry and its neighbours,
    at 0 and at the total (the u-rounded-up rule, which draws almost never
    hit), for N < 256, partial last buckets and zero runs across bucket
    boundaries.  A stand-alone host program, built with ASan + UBSan: a read
    past the CDF or the coarse table fails it."""
    exe = str(tmp_path / "guided_search")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "cpp", "guided_search.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout


# ------------------------------------------------------------------ errors --
BAD = {
    "nan": lambda w: w.__setitem__(3, np.nan),
    "inf": lambda w: w.__setitem__(3, np.inf),
    "negative": lambda w: w.__setitem__(3, -1e-300),
}


@pytest.mark.parametrize("find, m", ((pygcransac.findHomography, 4), (pygcransac.findFundamentalMatrix, 7)))
def test_python_value_errors(find, m):
    corr = np.random.default_rng(0).uniform(0, 900, (50, 4))
    args = (corr, 960, 1280, 960, 1280)
    ones = np.ones(50)
    with pytest.raises(ValueError, match="sampler"):       # today's error stays
        find(*args, probabilities=ones, sampler=0)
    for bad in (1, 2, 4, 5, 17):
        with pytest.raises(ValueError, match="sampler"):
            find(*args, probabilities=ones, sampler=bad)
    with pytest.raises(ValueError, match="probabilities"):
        find(*args, sampler=3)
    for wrong in (np.ones(49), np.ones(51), np.ones((50, 1)), np.ones(0)):
        with pytest.raises(ValueError, match="one entry per correspondence"):
            find(*args, probabilities=wrong, sampler=3)
    for name, spoil in BAD.items():
        w = ones.copy()
        spoil(w)
        with pytest.raises(ValueError, match="finite and >= 0"):
            find(*args, probabilities=w, sampler=3)
    few = np.zeros(50)
    few[:m - 1] = 1.0
    with pytest.raises(ValueError, match=f"at least {m} probabilities > 0, got {m - 1}"):
        find(*args, probabilities=few, sampler=3)
    big = np.full(50, 1e308)
    with pytest.raises(ValueError, match="not finite"):
        find(*args, probabilities=big, sampler=3)


def test_host_entry_errors():
    w = np.ones(8)
    out = np.zeros(4, dtype=np.uint32)
    p = out.ctypes.data_as(G.u32p)
    assert N.lib.gcr_host_sample_guided(0, 0, 0, 0, 0, None, 8, 4, p) == N.GCR_EINVAL
    assert N.lib.gcr_host_sample_guided(0, 0, 0, 0, 0, w.ctypes.data, 0, 4, p) == N.GCR_EINVAL
    assert N.lib.gcr_host_sample_guided(0, 0, 0, 0, 0, w.ctypes.data, 8, 33, p) == N.GCR_EINVAL
    assert N.lib.gcr_host_check_probabilities(w.ctypes.data, 8, 7) == 0
    assert N.lib.gcr_host_check_probabilities(w.ctypes.data, 6, 7) == N.GCR_EINVAL
    corr = np.zeros((8, 4))
    models = np.zeros(27)
    cnt = C.c_uint32()
    dp = C.POINTER(C.c_double)
    idx = np.array([0, 1, 2, 8], dtype=np.uint32)          # row 8 of 8
    assert N.lib.gcr_host_solve_minimal(N.SOLVER_HOMOGRAPHY4, corr.ctypes.data_as(dp), 8, idx.ctypes.data_as(G.u32p),
                                        models.ctypes.data_as(dp), C.byref(cnt)) == N.GCR_EINVAL
    assert N.lib.gcr_host_solve_minimal(N.SOLVER_SCALE3, corr.ctypes.data_as(dp), 8, idx.ctypes.data_as(G.u32p),
                                        models.ctypes.data_as(dp), C.byref(cnt)) == N.GCR_EINVAL
