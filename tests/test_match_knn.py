"""k-nearest-neighbour search, host side: csrc/match_knn.h's plain-loop
definition (gcr_host_knn_descriptors) against an independent numpy restatement
(tests/knn_cases.py) bit for bit, k = 2 against the 2-NN matcher, the crafted
inputs, every argument error, the merge under sanitizers, the one-to-many rule
(matches_from_knn) and the repeated-structure generator.  No GPU."""
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

import knn_cases as KC
import match_cases as MC
from pygcransac import _native as N
from pygcransac import features as F
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
NONE = KC.NONE


@pytest.mark.parametrize("dim", MC.DIMS)
@pytest.mark.parametrize("n1,n2", MC.SHAPES)
def test_host_twin_equals_restatement(n1, n2, dim):
    d1, d2 = MC.random_pair(n1, n2, dim)
    for k in KC.KS:
        got, exp = KC.host(d1, d2, k), KC.restate(d1, d2, k)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), k
        if n2 < k:
            assert (got[0][:, n2:] == NONE).all() and (got[1][:, n2:] == NONE).all()
            assert (got[0][:, :n2] != NONE).all()


@pytest.mark.parametrize("n2", [1, 2, 3, 4, 5, 7, 8, 9])
def test_fewer_columns_than_k(n2):
    """n2 < k (the tail is NONE), n2 == k and n2 == k + 1 for every k"""
    d1, d2 = MC.random_pair(40, n2, 64)
    for k in range(1, 9):
        got = KC.host(d1, d2, k)
        assert KC.same(got, KC.restate(d1, d2, k)), k
        m = min(k, n2)
        assert (got[0][:, :m] < n2).all()
        assert (got[0][:, m:] == NONE).all() and (got[1][:, m:] == NONE).all()


@pytest.mark.parametrize("dim", MC.DIMS)
@pytest.mark.parametrize("n1,n2", MC.SHAPES)
def test_k2_is_the_two_nn_matcher(n1, n2, dim):
    d1, d2 = MC.random_pair(n1, n2, dim)
    idx, dist = KC.host(d1, d2, 2)
    e = MC.host(d1, d2)
    assert np.array_equal(idx[:, 0], e[0]) and np.array_equal(dist[:, 0], e[1])
    assert np.array_equal(idx[:, 1], e[2]) and np.array_equal(dist[:, 1], e[3])


def test_threads_do_not_change_the_bytes():
    d1, d2 = MC.random_pair(1000, 257, 128)
    for k in (3, 8):
        one = KC.host(d1, d2, k, 1)
        for threads in (16, 3, 0, -5, 1000):
            assert KC.same(KC.host(d1, d2, k, threads), one), (k, threads)
        assert KC.same(KC.host(d1[:2], d2, k, 16), [o[:2] for o in one])          # more threads than rows


def test_crafted_rows():
    cases = KC.all_crafted()
    assert set(cases) == {"alphabet", "all_equal", "descending", "ascending", "sign_shift", "padding", "duplicates",
                          "permutation"}
    for name, (d1, d2) in cases.items():
        for k in KC.KS:
            assert KC.same(KC.host(d1, d2, k), KC.restate(d1, d2, k)), (name, k)
    d1, d2 = cases["alphabet"]
    assert d1.shape == (130, 32) and d2.shape == (515, 32) and len(np.unique(np.concatenate([d1, d2]))) == 2
    idx, dist = KC.host(d1, d2, 8)
    assert (dist[:, :-1] == dist[:, 1:]).any(axis=1).all()                        # every row has a tie in its list
    tie = dist[:, :-1] == dist[:, 1:]
    assert (idx[:, :-1][tie] < idx[:, 1:][tie]).all()
    idx, dist = KC.host(*cases["all_equal"], 8)
    assert (idx == np.arange(8)).all() and (dist == dist[:, :1]).all()
    d1, d2 = cases["descending"]
    assert d2.shape == (256, 32) and not d1.any() and np.array_equal(d2[:, 0], 255 - np.arange(256))
    idx, dist = KC.host(d1, d2, 8)
    assert (idx == 255 - np.arange(8)).all() and (dist == 32 * np.arange(8) ** 2).all()
    idx, dist = KC.host(*cases["ascending"], 8)
    assert (idx == np.arange(8)).all() and (dist == 32 * np.arange(8) ** 2).all()
    idx, dist = KC.host(*cases["padding"], 5)
    assert (idx == np.arange(5)).all() and (dist == 128 * 255 * 255).all()


def test_largest_distance_fits():
    idx, dist = KC.host(np.zeros((2, 512), np.uint8), np.full((9, 512), 255, np.uint8), 8)
    assert (dist == 33292800).all() and (idx == np.arange(8)).all()


# ------------------------------------------------------------------ errors --
def test_c_entries_reject_bad_arguments():
    d = np.zeros((4, 64), np.uint8)
    out = [np.zeros((4, 8), np.uint32) for _ in range(2)]
    p = [o.ctypes.data for o in out]
    big = (1 << 24) + 1

    def both(d1, n1, d2, n2, dim, k, ptrs, word):
        # the device entry with a NULL context: the check runs before any GPU work
        rc = N.lib.gcr_knn_descriptors(None, d1, n1, d2, n2, dim, k, *ptrs, None)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (word, N.last_error())
        rc = N.lib.gcr_host_knn_descriptors(d1, n1, d2, n2, dim, k, 1, *ptrs)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (word, N.last_error())

    a = d.ctypes.data
    both(None, 4, a, 4, 64, 3, p, "d1")
    both(a, 4, None, 4, 64, 3, p, "d2")
    both(a, 4, a, 4, 64, 3, [None, p[1]], "idx_out")
    both(a, 4, a, 4, 64, 3, [p[0], None], "dist_out")
    both(a, 0, a, 4, 64, 3, p, "n1")
    both(a, big, a, 4, 64, 3, p, "n1")
    both(a, 4, a, 0, 64, 3, p, "n2")
    both(a, 4, a, big, 64, 3, p, "n2")
    for dim in (0, 16, 48, 100, 544, 1024):
        both(a, 4, a, 4, dim, 3, p, "dim")
    for k in (0, 9, 1000):
        both(a, 4, a, 4, 64, k, p, "k must be")
    # good arguments and no context: still an error, of the context
    assert N.lib.gcr_knn_descriptors(None, a, 4, a, 4, 64, 8, *p, None) == N.GCR_EINVAL
    assert "context" in N.last_error()
    assert N.lib.gcr_host_knn_descriptors(a, 4, a, 4, 64, 8, 1, *p) == 0
    # the set entry's checks that need no context
    for args, word in (((None, None, None, 3, *p, None), "a is NULL"), ((None, 1, None, 3, *p, None), "b is NULL")):
        assert N.lib.gcr_knn_sets(*args) == N.GCR_EINVAL and word in N.last_error(), N.last_error()
    for k in (0, 9):
        assert N.lib.gcr_knn_sets(None, 1, 1, k, *p, None) == N.GCR_EINVAL and "k must be" in N.last_error()
    assert N.lib.gcr_knn_sets(None, 1, 1, 3, None, p[1], None) == N.GCR_EINVAL and "idx_out" in N.last_error()
    assert N.lib.gcr_knn_sets(None, 1, 1, 3, p[0], None, None) == N.GCR_EINVAL and "dist_out" in N.last_error()
    assert N.lib.gcr_knn_sets(None, 1, 1, 3, *p, None) == N.GCR_EINVAL and "context" in N.last_error()
    assert N.lib.gcr_abi_version() == 5


def test_python_errors():
    d = np.zeros((4, 128), np.uint8)
    for bad in (d.astype(np.float32), d.astype(np.int8)):
        with pytest.raises(ValueError, match="quantize_descriptors"):
            F.knn_descriptors(bad, d, 3, backend="host")
        with pytest.raises(ValueError, match="quantize_descriptors"):
            F.knn_descriptors(d, bad, 3, backend="host")
    with pytest.raises(ValueError, match="dimension"):
        F.knn_descriptors(d, np.zeros((4, 64), np.uint8), 3, backend="host")
    with pytest.raises(ValueError, match="multiple of 32"):
        F.knn_descriptors(np.zeros((4, 48), np.uint8), np.zeros((4, 48), np.uint8), 3, backend="host")
    with pytest.raises(ValueError, match="shape"):
        F.knn_descriptors(np.zeros(128, np.uint8), d, 3, backend="host")
    with pytest.raises(ValueError, match="at least one row"):
        F.knn_descriptors(np.zeros((0, 128), np.uint8), d, 3, backend="host")
    with pytest.raises(ValueError, match="backend"):
        F.knn_descriptors(d, d, 3, backend="cpu")
    for k in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            F.knn_descriptors(d, d, k, backend="host")
        with pytest.raises(ValueError, match="k must be"):                        # never reaches a device
            F.knn_descriptors(d, d, k)
    idx, dist = F.knn_descriptors(d, d, np.int64(3), backend="host")
    assert idx.shape == dist.shape == (4, 3) and idx.dtype == dist.dtype == np.uint32
    u = np.zeros((3, 2), np.uint32)
    for bad_idx, bad_dist in ((u.astype(np.int64), u), (u, u.astype(np.float64)), (u, u[:, :1]), (u[0], u[0]),
                              (np.zeros((3, 9), np.uint32), np.zeros((3, 9), np.uint32)),
                              (np.zeros((3, 0), np.uint32), np.zeros((3, 0), np.uint32))):
        with pytest.raises(ValueError):
            F.matches_from_knn(bad_idx, bad_dist)
    for ratio in (None, 0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="ratio"):
            F.matches_from_knn(u, u, ratio=ratio)
    for mg in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_group"):
            F.matches_from_knn(u, u, max_group=mg)


def test_signatures_and_exports():
    sig = inspect.signature(F.knn_descriptors).parameters
    assert list(sig) == ["desc1", "desc2", "k", "backend", "device"]
    assert sig["backend"].default == "gpu" and sig["backend"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["device"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(F.matches_from_knn).parameters
    assert list(sig) == ["idx", "dist", "ratio", "max_group"]
    assert sig["ratio"].default == 0.8 and sig["max_group"].default is None
    assert list(inspect.signature(F.DescriptorSet.knn).parameters) == ["self", "other", "k"]
    sig = inspect.signature(S.problem_match_repeated).parameters
    assert list(sig) == ["n", "groups", "repeats", "seed", "desc_noise", "dim"]
    assert (sig["n"].default, sig["groups"].default, sig["repeats"].default, sig["desc_noise"].default) == \
        (1000, 100, 3, 20.0)
    assert "knn_descriptors" in F.__all__ and "matches_from_knn" in F.__all__
    assert "sampler=3" in F.matches_from_knn.__doc__ and "1.0 / group" in F.matches_from_knn.__doc__


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/match_knn_host.cpp: the definition against a sort, k = 2
    against match.h, the merge at every split point and in every merge order;
    a stand-alone host program built with ASan + UBSan."""
    exe = str(tmp_path / "match_knn_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "cpp", "match_knn_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout


# ------------------------------------------------------- matches_from_knn --
def test_matches_from_knn_table():
    # dist rows against ratio 0.8 (rr = 0.64), k = 4
    idx = np.array([[10, 11, 12, 13],          # 0: gap after the first (10 < 0.64 * 100)
                    [20, 21, 22, 23],          # 1: gap after the second
                    [30, 31, 32, 33],          # 2: gap after the third
                    [40, 41, 42, 43],          # 3: no gap
                    [50, 51, NONE, NONE],      # 4: two columns only, gap after the first
                    [60, 61, NONE, NONE],      # 5: two columns only, no gap: the tail never makes one
                    [70, NONE, NONE, NONE],    # 6: a single column
                    [80, 81, 82, 83],          # 7: distance 0 at the head, then a gap after the second
                    [90, 91, 92, 93],          # 8: all zero: 0 < 0.64 * 0 fails
                    [95, 96, 97, 98]],         # 9: just past the bound: 65 < 0.64 * 100 fails
                   dtype=np.uint32)
    dist = np.array([[10, 100, 100, 100],
                     [90, 100, 1000, 1000],
                     [90, 95, 100, 1000],
                     [90, 95, 100, 105],
                     [10, 100, NONE, NONE],
                     [90, 100, NONE, NONE],
                     [5, NONE, NONE, NONE],
                     [0, 0, 7, 8],
                     [0, 0, 0, 0],
                     [65, 100, 101, 102]], dtype=np.uint32)
    m, g, r = F.matches_from_knn(idx, dist, ratio=0.8)
    assert m.dtype == np.int64 and g.dtype == np.int64 and r.dtype == np.float64
    assert m.tolist() == [[0, 10], [1, 20], [1, 21], [2, 30], [2, 31], [2, 32], [4, 50], [7, 80], [7, 81]]
    assert g.tolist() == [1, 2, 2, 3, 3, 3, 1, 2, 2]
    exp = [np.sqrt(10 / 100), np.sqrt(100 / 1000), np.sqrt(100 / 1000), np.sqrt(100 / 1000), np.sqrt(100 / 1000),
           np.sqrt(100 / 1000), np.sqrt(10 / 100), 0.0, 0.0]
    assert np.array_equal(r, np.array(exp))
    # max_group: a larger group is no match
    m, g, r = F.matches_from_knn(idx, dist, ratio=0.8, max_group=2)
    assert m.tolist() == [[0, 10], [1, 20], [1, 21], [4, 50], [7, 80], [7, 81]] and g.tolist() == [1, 2, 2, 1, 2, 2]
    m, g, r = F.matches_from_knn(idx, dist, ratio=0.8, max_group=1)
    assert m.tolist() == [[0, 10], [4, 50]] and g.tolist() == [1, 1]
    assert np.array_equal(F.matches_from_knn(idx, dist, max_group=7)[0], F.matches_from_knn(idx, dist)[0])
    # a wider ratio: the SMALLEST group with a gap
    m, g, _ = F.matches_from_knn(idx, dist, ratio=0.99)
    assert g[m[:, 0] == 1].tolist() == [1] and g[m[:, 0] == 3].tolist() == [1] and g[m[:, 0] == 9].tolist() == [1]
    # the first two columns alone: the plain ratio test; one column: nothing to compare
    m, g, _ = F.matches_from_knn(idx[:, :2], dist[:, :2])
    assert m.tolist() == [[0, 10], [4, 50]] and g.tolist() == [1, 1]
    m, g, r = F.matches_from_knn(idx[:, :1], dist[:, :1])
    assert m.shape == (0, 2) and g.shape == (0,) and r.shape == (0,)


@pytest.fixture(scope="module")
def problem():
    return S.problem_match()


def test_matches_from_knn_k2_is_match_descriptors(problem):
    _, d1, _, d2, _, _ = problem
    idx, dist = F.knn_descriptors(d1, d2, 2, backend="host")
    for ratio in (0.8, 0.6, 0.95):
        m, g, r = F.matches_from_knn(idx, dist, ratio=ratio)
        em, er = F.match_descriptors(d1, d2, ratio=ratio, mutual=False, backend="host")
        assert len(em) > 0 and np.array_equal(m, em) and np.array_equal(r, er) and (g == 1).all()


# ------------------------------------------------------------ the generator --
@functools.lru_cache(maxsize=None)
def _repeated():
    return S.problem_match_repeated()


def test_problem_match_repeated_shapes():
    kp1, d1, kp2, d2, pairs, H = _repeated()
    dim = inspect.signature(S.problem_match_repeated).parameters["dim"].default
    assert kp1.shape == kp2.shape == (1000, 4) and d1.shape == d2.shape == (1000, dim)
    assert d1.dtype == d2.dtype == np.uint8 and pairs.shape == (300, 2) and pairs.dtype == np.int64
    assert len(set(pairs[:, 0])) == 300 and len(set(pairs[:, 1])) == 300 and (np.diff(pairs[:, 0]) > 0).all()
    # the shared keypoints follow H_gt within problem_hs's pixel noise, each at its own position
    c = F.correspondences_from_matches(kp1, kp2, pairs)
    p = (H @ np.column_stack([c[:, 0], c[:, 1], np.ones(len(c))]).T).T
    assert np.abs(p[:, :2] / p[:, 2:] - c[:, 2:4]).max() < 3.0
    assert len(np.unique(c[:, :2], axis=0)) == 300
    again = S.problem_match_repeated()
    assert all(np.array_equal(x, y) for x, y in zip(_repeated(), again))
    assert not np.array_equal(S.problem_match_repeated(seed=5)[1], d1)
    small = S.problem_match_repeated(n=50, groups=4, repeats=5, dim=32)
    assert small[1].shape == (50, 32) and small[4].shape == (20, 2)
    assert S.problem_match_repeated(n=20, groups=0, dim=32)[4].shape == (0, 2)
    with pytest.raises(ValueError):
        S.problem_match_repeated(n=10, groups=4, repeats=3)


def test_repeated_structure_defeats_the_ratio_test_and_knn_recovers_it():
    kp1, d1, kp2, d2, pairs, _ = _repeated()
    truth = set(map(tuple, pairs.tolist()))
    m, _ = F.match_descriptors(d1, d2, ratio=0.8, mutual=False, backend="host")
    kept = len(truth & set(map(tuple, m.tolist())))
    print(f"ratio test keeps {kept} of {len(truth)} truth pairs")
    assert kept <= 0.05 * len(truth)
    idx, dist = F.knn_descriptors(d1, d2, 4, backend="host")
    mk, group, ratios = F.matches_from_knn(idx, dist, ratio=0.8)
    got = set(map(tuple, mk.tolist()))
    print(f"matches_from_knn holds {len(truth & got)} of {len(truth)} truth pairs in {len(mk)} matches; "
          f"largest gap ratio of a shared row {ratios[np.isin(mk[:, 0], pairs[:, 0])].max():.3f}")
    assert truth <= got
    # every shared row's group is `repeats`
    shared = np.isin(mk[:, 0], pairs[:, 0])
    assert set(mk[shared, 0].tolist()) == set(pairs[:, 0].tolist())
    assert (group[shared] == 3).all()
    assert (np.bincount(mk[shared, 0])[pairs[:, 0]] == 3).all()
