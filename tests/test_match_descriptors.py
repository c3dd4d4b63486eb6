"""Descriptor matching, host side: csrc/match.h's plain-loop definition
(gcr_host_match_descriptors) against an independent numpy restatement
(tests/match_cases.py) bit for bit, the crafted inputs, the Python front end
(match_descriptors, quantize_descriptors, correspondences_from_matches), the
synthetic generator and every error.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import match_cases as MC
import pygcransac
from pygcransac import _native as N
from pygcransac import features as F
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")


@pytest.mark.parametrize("dim", MC.DIMS)
@pytest.mark.parametrize("n1,n2", MC.SHAPES)
def test_host_twin_equals_restatement(n1, n2, dim):
    d1, d2 = MC.random_pair(n1, n2, dim)
    got, exp = MC.host(d1, d2), MC.restate(d1, d2)
    for g, e, name in zip(got, exp, ("idx", "dist", "idx2", "dist2")):
        assert np.array_equal(g, e), name
    if n2 == 1:
        assert (got[2] == MC.NONE).all() and (got[3] == MC.NONE).all()


@pytest.mark.parametrize("dim", MC.DIMS)
def test_crafted_rows(dim):
    cases = MC.crafted(dim)
    for name, (d1, d2) in cases.items():
        assert MC.same(MC.host(d1, d2), MC.restate(d1, d2)), name
    idx, dist, idx2, dist2 = MC.host(*cases["padding"])
    assert (dist == dim * 255 * 255).all() and (dist2 == dim * 255 * 255).all()
    assert (idx == 0).all() and (idx2 == 1).all()
    idx, dist, idx2, dist2 = MC.host(*cases["duplicates"])
    assert (dist == dist2).all() and (idx < idx2).all()
    d1, d2 = cases["permutation"]
    idx, dist, _, _ = MC.host(d1, d2)
    assert (dist == 0).all() and np.array_equal(d2[idx], d1) and len(set(idx)) == len(d1)
    d1, d2 = cases["sign_shift"]
    assert set(np.unique(d1)) <= {0, 127, 128, 255} and len(np.unique(d2)) == 4


def test_threads_do_not_change_the_bytes():
    d1, d2 = MC.random_pair(1000, 257, 128)
    one = MC.host(d1, d2, 1)
    for threads in (3, 16, 0, -5, 1000):
        assert MC.same(MC.host(d1, d2, threads), one), threads
    assert MC.same(MC.host(d1[:2], d2, 16), [o[:2] for o in one])        # more threads than rows


def test_largest_distance_fits():
    d1 = np.zeros((2, 512), np.uint8)
    d2 = np.full((3, 512), 255, np.uint8)
    idx, dist, idx2, dist2 = MC.host(d1, d2)
    assert (dist == 33292800).all() and (dist2 == 33292800).all() and (idx == 0).all() and (idx2 == 1).all()


# ------------------------------------------------------------ the generator --
@pytest.fixture(scope="module")
def problem():
    return S.problem_match()


def test_problem_match_shapes(problem):
    kp1, d1, kp2, d2, pairs, H = problem
    assert kp1.shape == kp2.shape == (1000, 4) and d1.shape == d2.shape == (1000, 128)
    assert d1.dtype == d2.dtype == np.uint8 and pairs.shape == (400, 2) and pairs.dtype == np.int64
    assert len(set(pairs[:, 0])) == 400 and len(set(pairs[:, 1])) == 400 and (np.diff(pairs[:, 0]) > 0).all()
    assert not np.array_equal(pairs[:, 0], pairs[:, 1])                 # image 2 is permuted
    # the shared keypoints follow H_gt within problem_hs's pixel noise (0.5 px sigma)
    c = F.correspondences_from_matches(kp1, kp2, pairs)
    p = (H @ np.column_stack([c[:, 0], c[:, 1], np.ones(len(c))]).T).T
    assert np.abs(p[:, :2] / p[:, 2:] - c[:, 2:4]).max() < 3.0
    again = S.problem_match()
    assert all(np.array_equal(x, y) for x, y in zip(problem, again))
    other = S.problem_match(seed=5)
    assert not np.array_equal(other[1], d1)
    small = S.problem_match(n=50, shared=0, dim=32)
    assert small[1].shape == (50, 32) and small[4].shape == (0, 2)
    with pytest.raises(ValueError):
        S.problem_match(n=10, shared=11)


def test_match_descriptors_on_problem_match(problem):
    kp1, d1, kp2, d2, pairs, _ = problem
    truth = set(map(tuple, pairs.tolist()))
    m, r = F.match_descriptors(d1, d2, ratio=0.8, mutual=True, backend="host")
    got = set(map(tuple, m.tolist()))
    assert m.dtype == np.int64 and r.dtype == np.float64 and m.shape == (len(r), 2)
    assert not (got - truth) and len(got & truth) >= 0.99 * len(truth)
    assert (np.diff(m[:, 0]) > 0).all()
    m, r = F.match_descriptors(d1, d2, ratio=None, mutual=False, backend="host")
    assert len(m) == 1000 and np.array_equal(m[:, 0], np.arange(1000))
    got = set(map(tuple, m.tolist()))
    assert truth <= got
    true = np.array([tuple(x) in truth for x in m.tolist()])
    assert r[true].max() < r[~true].min()
    # the ratios are sqrt(dist / dist2), the ratio test float(dist) < ratio^2 float(dist2)
    idx, dist, idx2, dist2 = MC.host(d1, d2)
    assert np.array_equal(m[:, 1], idx.astype(np.int64))
    assert np.array_equal(r, np.sqrt(dist.astype(np.float64) / dist2.astype(np.float64)))
    for ratio in (0.5, 0.7, 0.95):
        mr, rr = F.match_descriptors(d1, d2, ratio=ratio, mutual=False, backend="host")
        keep = dist.astype(np.float64) < (ratio * ratio) * dist2.astype(np.float64)
        assert np.array_equal(mr[:, 0], np.nonzero(keep)[0]) and np.array_equal(rr, r[keep])
    # mutual: i is the nearest of its nearest
    mm, _ = F.match_descriptors(d1, d2, ratio=None, mutual=True, backend="host")
    back = MC.host(d2, d1)[0]
    assert np.array_equal(mm[:, 0], np.nonzero(back[idx] == np.arange(1000))[0])


def test_ratio_edge_cases():
    d1 = np.zeros((3, 32), np.uint8)
    d1[1] = 7
    # one column: no second neighbour -> ratio 1.0, the ratio test fails, ratio=None keeps the row
    m, r = F.match_descriptors(d1, d1[:1], ratio=0.8, mutual=False, backend="host")
    assert m.shape == (0, 2) and m.dtype == np.int64 and r.shape == (0,)
    m, r = F.match_descriptors(d1, d1[:1], ratio=None, mutual=False, backend="host")
    assert np.array_equal(m, [[0, 0], [1, 0], [2, 0]]) and np.array_equal(r, [1.0, 1.0, 1.0])
    # 0 / 0 (two equal nearest rows): ratio 1.0; the test 0 < r^2 * 0 fails
    m, r = F.match_descriptors(d1, d1, ratio=None, mutual=False, backend="host")
    assert np.array_equal(m, [[0, 0], [1, 1], [2, 0]]) and np.array_equal(r, [1.0, 0.0, 1.0])
    m, r = F.match_descriptors(d1, d1, ratio=0.8, mutual=True, backend="host")
    assert np.array_equal(m, [[1, 1]]) and np.array_equal(r, [0.0])


# ----------------------------------------------------------------- helpers --
def test_quantize_descriptors():
    x = np.array([[-0.1, 0.0, 0.001, 0.25, 0.4990234375, 0.5, 1.0, 0.0009765625 * 3]])
    q = F.quantize_descriptors(x)
    assert q.dtype == np.uint8 and np.array_equal(q, [[0, 0, 1, 128, 255, 255, 255, 2]])   # rint: 1.5 -> 2 (half to even)
    assert np.array_equal(F.quantize_descriptors(x, scale=100.0), [[0, 0, 0, 25, 50, 50, 100, 0]])
    rng = np.random.default_rng(3)
    d = np.abs(rng.normal(size=(20, 128)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.array_equal(F.quantize_descriptors(d), np.clip(np.rint(512.0 * d), 0, 255).astype(np.uint8))
    with pytest.raises(ValueError):
        F.quantize_descriptors(np.zeros(5))
    with pytest.raises(ValueError):
        F.quantize_descriptors(np.array([[np.nan]]))


def test_correspondences_from_matches():
    kp1 = np.array([[1.0, 2.0, 3.0, 90.0], [4.0, 5.0, 6.0, -1.0], [7.0, 8.0, 9.0, 180.0]])
    kp2 = np.array([[10.0, 20.0, 30.0, 45.0], [40.0, 50.0, 60.0, 0.0]])
    m = np.array([[2, 0], [0, 1]])
    c = F.correspondences_from_matches(kp1, kp2, m)
    assert c.dtype == np.float64 and np.array_equal(c, [[7, 8, 10, 20], [1, 2, 40, 50]])
    c8 = F.correspondences_from_matches(kp1, kp2, m, sift=True)
    assert np.array_equal(c8, [[7, 8, 10, 20, 9, 30, np.deg2rad(180.0), np.deg2rad(45.0)],
                               [1, 2, 40, 50, 3, 60, np.deg2rad(90.0), 0.0]])
    # the (M, 8) rows are what findHomographySIFT's own check accepts
    assert N.lib.gcr_host_check_sift(np.ascontiguousarray(c8[:, 4:8]).ctypes.data, 2) == 0
    with pytest.raises(ValueError, match="2 matched keypoints"):
        F.correspondences_from_matches(kp1, kp2, np.array([[1, 0], [1, 1], [0, 0]]), sift=True)
    assert F.correspondences_from_matches(kp1, kp2, np.array([[1, 0]])).shape == (1, 4)      # angle unused
    assert F.correspondences_from_matches(kp1, kp2, np.zeros((0, 2), np.int64), sift=True).shape == (0, 8)

    class KP:
        def __init__(self, row):
            self.pt, self.size, self.angle = (row[0], row[1]), row[2], row[3]

    assert np.array_equal(F.correspondences_from_matches([KP(r) for r in kp1], [KP(r) for r in kp2], m, sift=True), c8)
    for bad in (np.array([[0, 2]]), np.array([[3, 0]]), np.array([[-1, 0]]), np.array([0, 1]), np.array([[0.5, 1.0]])):
        with pytest.raises(ValueError):
            F.correspondences_from_matches(kp1, kp2, bad)


# ------------------------------------------------------------------ errors --
def test_python_errors():
    d = np.zeros((4, 128), np.uint8)
    for bad in (d.astype(np.float32), d.astype(np.int8), d.astype(np.int64)):
        with pytest.raises(ValueError, match="quantize_descriptors"):
            F.match_descriptors(bad, d, backend="host")
        with pytest.raises(ValueError, match="quantize_descriptors"):
            F.match_descriptors(d, bad, backend="host")
    with pytest.raises(ValueError, match="dimension"):
        F.match_descriptors(d, np.zeros((4, 64), np.uint8), backend="host")
    for shape in ((4, 48), (4, 16), (4, 544), (4, 0)):
        with pytest.raises(ValueError, match="multiple of 32"):
            F.match_descriptors(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), backend="host")
    with pytest.raises(ValueError, match="shape"):
        F.match_descriptors(np.zeros(128, np.uint8), d, backend="host")
    with pytest.raises(ValueError, match="at least one row"):
        F.match_descriptors(np.zeros((0, 128), np.uint8), d, backend="host")
    with pytest.raises(ValueError, match="backend"):
        F.match_descriptors(d, d, backend="cpu")
    with pytest.raises(ValueError, match="ratio"):
        F.match_descriptors(d, d, ratio=-1.0, backend="host")
    # the bad calls above never reach a device: backend="gpu" fails the same way
    with pytest.raises(ValueError, match="quantize_descriptors"):
        F.match_descriptors(d.astype(np.float32), d)
    with pytest.raises(ValueError, match="multiple of 32"):
        F.match_descriptors(np.zeros((4, 48), np.uint8), np.zeros((4, 48), np.uint8))


def test_c_entries_reject_bad_arguments():
    d = np.zeros((4, 64), np.uint8)
    out = [np.zeros(4, np.uint32) for _ in range(4)]
    p = [o.ctypes.data for o in out]
    big = (1 << 24) + 1

    def both(d1, n1, d2, n2, dim, ptrs, word):
        # the device entry with a NULL context: the check runs before any GPU work
        rc = N.lib.gcr_match_descriptors(None, d1, n1, d2, n2, dim, *ptrs, None)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (word, N.last_error())
        rc = N.lib.gcr_host_match_descriptors(d1, n1, d2, n2, dim, 1, *ptrs)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (word, N.last_error())

    a = d.ctypes.data
    both(None, 4, a, 4, 64, p, "d1")
    both(a, 4, None, 4, 64, p, "d2")
    for k, name in enumerate(("idx_out", "dist_out", "idx2_out", "dist2_out")):
        both(a, 4, a, 4, 64, p[:k] + [None] + p[k + 1:], name)
    both(a, 0, a, 4, 64, p, "n1")
    both(a, big, a, 4, 64, p, "n1")
    both(a, 4, a, 0, 64, p, "n2")
    both(a, 4, a, big, 64, p, "n2")
    for dim in (0, 16, 48, 100, 544, 1024):
        both(a, 4, a, 4, dim, p, "dim")
    # good arguments and no context: still an error, of the context
    assert N.lib.gcr_match_descriptors(None, a, 4, a, 4, 64, *p, None) == N.GCR_EINVAL
    assert "context" in N.last_error()
    assert N.lib.gcr_host_match_descriptors(a, 4, a, 4, 64, 1, *p) == 0
    assert N.lib.gcr_abi_version() == 5
    assert MC.tiling() == (128, 64, 256)


def test_signatures_and_exports():
    names = list(inspect.signature(F.match_descriptors).parameters)
    assert names == ["desc1", "desc2", "ratio", "mutual", "backend", "device"]
    sig = inspect.signature(F.match_descriptors).parameters
    assert sig["ratio"].default == 0.8 and sig["mutual"].default is True and sig["backend"].default == "gpu"
    assert sig["backend"].kind is inspect.Parameter.KEYWORD_ONLY and sig["device"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(F.quantize_descriptors).parameters) == ["desc", "scale"]
    assert inspect.signature(F.quantize_descriptors).parameters["scale"].default == 512.0
    assert list(inspect.signature(F.correspondences_from_matches).parameters) == ["kp1", "kp2", "matches", "sift"]
    assert list(inspect.signature(S.problem_match).parameters) == ["n", "shared", "seed", "desc_noise", "dim"]
    for n in ("match_descriptors", "quantize_descriptors", "correspondences_from_matches"):
        assert n in F.__all__
    assert "sampler=1" in F.match_descriptors.__doc__ and "match_descriptors" in pygcransac.findHomography.__doc__


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/match_host.cpp: the definition, the merge and the planner on
    the crafted inputs, a stand-alone host program built with ASan + UBSan."""
    exe = str(tmp_path / "match_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "cpp", "match_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout
