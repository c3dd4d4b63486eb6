"""k-nearest-neighbour search on the GPU: gcr_knn_descriptors
(csrc/match_knn.hip, int8 matrix cores) against the host twin bit for bit -- at
the shared shapes, at the 2-NN kernel's tiling edges, at every dim class and
both list capacities, with the column split free and pinned, on the crafted
inputs --, k = 2 against gcr_match_descriptors, DescriptorSet.knn against the
array entry, and the pipeline knn_descriptors -> matches_from_knn -> guided
sampling on the repeated-structure image pair."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_cases as KC
import match_cases as MC
import pygcransac
from pygcransac import _native as N
from pygcransac import features as F
from pygcransac import synthetic as S
from test_gpu_match_descriptors import EDGES

pytestmark = pytest.mark.gpu

KS_GPU = [1, 3, 4, 5, 8]


@functools.lru_cache(maxsize=None)
def _pair(n1, n2, dim):
    return MC.random_pair(n1, n2, dim)


@functools.lru_cache(maxsize=None)
def _expected(n1, n2, dim, k):
    return KC.host(*_pair(n1, n2, dim), k, 16)


def _check(d1, d2, k, exp, what=""):
    got = KC.gpu(d1, d2, k)
    for g, e, name in zip(got, exp, ("idx", "dist")):
        bad = np.argwhere(g != e)
        assert bad.size == 0, (f"{what} k={k} {name}: {len(bad)} entries differ, first (row, rank) {bad[:5].tolist()}: "
                               f"{g[tuple(bad[:5].T)]} != {e[tuple(bad[:5].T)]}")


def _set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("GCR_MATCH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("GCR_MATCH_SPLIT", str(split))


@pytest.mark.parametrize("dim", MC.DIMS)
@pytest.mark.parametrize("n1,n2", MC.SHAPES)
def test_gpu_equals_host_twin(n1, n2, dim):
    for k in KS_GPU:
        _check(*_pair(n1, n2, dim), k, _expected(n1, n2, dim, k))


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("n1,n2", EDGES)
def test_tiling_edges(n1, n2, split, monkeypatch):
    _set_split(monkeypatch, split)
    for k in (3, 8):
        _check(*_pair(n1, n2, 128), k, _expected(n1, n2, 128, k))


# test_gpu_match_descriptors.py's pinned-split shapes: splits of 128, 128 and 1 to 192 columns
@pytest.mark.parametrize("dim", MC.DIMS)
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("n1,n2", [(129, 383), (129, 384), (129, 385), (1000, 257)])
def test_pinned_splits(n1, n2, split, dim, monkeypatch):
    monkeypatch.setenv("GCR_MATCH_SPLIT", str(split))
    _check(*_pair(n1, n2, dim), 8, _expected(n1, n2, dim, 8))


@pytest.mark.parametrize("dim", [32, 64, 96, 160, 256, 480])
def test_other_dims(dim):
    for k in (3, 8):                                      # both capacities
        _check(*_pair(70, 200, dim), k, _expected(70, 200, dim, k))


@pytest.mark.parametrize("n2", [1, 3, 7, 8])
def test_fewer_columns_than_k(n2):
    exp = _expected(40, n2, 128, 8)
    assert (exp[0][:, n2:] == KC.NONE).all() and (exp[1][:, n2:] == KC.NONE).all() and (exp[0][:, :n2] < n2).all()
    _check(*_pair(40, n2, 128), 8, exp)


@pytest.mark.parametrize("split", [None, 1, 3])
def test_crafted_rows(split, monkeypatch):
    _set_split(monkeypatch, split)
    for name, (d1, d2) in KC.all_crafted().items():
        for k in KC.KS:
            _check(d1, d2, k, KC.host(d1, d2, k, 16), name)


@pytest.mark.parametrize("split", [None, 3])
def test_k2_is_the_two_nn_kernel(split, monkeypatch):
    _set_split(monkeypatch, split)
    for n1, n2, dim in ((129, 257, 128), (1000, 257, 32), (40, 1, 128), (70, 200, 512)):
        d1, d2 = _pair(n1, n2, dim)
        idx, dist = KC.gpu(d1, d2, 2)
        e = MC.gpu(d1, d2)
        assert np.array_equal(idx[:, 0], e[0]) and np.array_equal(dist[:, 0], e[1]), (n1, n2, dim)
        assert np.array_equal(idx[:, 1], e[2]) and np.array_equal(dist[:, 1], e[3]), (n1, n2, dim)


def test_two_calls_give_the_same_bytes():
    d1, d2 = _pair(1000, 257, 128)
    for k in (4, 8):
        assert KC.same(KC.gpu(d1, d2, k), KC.gpu(d1, d2, k))


def test_kernel_time_is_reported():
    d1, d2 = _pair(129, 257, 128)
    for k in (3, 8):
        ms = C.c_double(-1.0)
        got = KC.gpu(d1, d2, k, ms=C.byref(ms))
        assert KC.same(got, _expected(129, 257, 128, k)) and 0.0 < ms.value < 1000.0


# ---------------------------------------------------------- resident sets --
def _workspace():
    out = (C.c_uint64 * 2)()
    N.check(N.lib.gcr_debug_match_workspace(N.context(None), out))
    return int(out[0]), int(out[1])


def test_descriptor_set_knn_equals_the_array_entry():
    d1, d2 = _pair(129, 257, 128)
    with F.DescriptorSet(d1) as a, F.DescriptorSet(d2) as b:
        for k in KS_GPU:
            assert KC.same(a.knn(b, k), _expected(129, 257, 128, k)), k
            assert KC.same(b.knn(a, k), KC.host(d2, d1, k, 16)), k          # a set on either side
            assert KC.same(a.knn(a, k), KC.host(d1, d1, k, 16)), k          # and against itself
        idx, dist = a.knn(b, 8)
        assert idx.shape == dist.shape == (129, 8) and idx.dtype == dist.dtype == np.uint32
        assert KC.same(F.knn_descriptors(d1, d2, 8), (idx, dist))
        assert (a.knn(a, 1)[0][:, 0] == np.arange(129)).all()
        for k in (0, 9, 2.0):
            with pytest.raises(ValueError, match="k must be"):
                a.knn(b, k)
        with pytest.raises(ValueError, match="DescriptorSet"):
            a.knn(d2, 3)
    with pytest.raises(ValueError, match="closed"):
        a.knn(b, 3)
    with F.DescriptorSet(d1) as a, F.DescriptorSet(np.zeros((4, 64), np.uint8)) as c:
        with pytest.raises(ValueError, match="dimension"):
            a.knn(c, 3)


# pinned to 3 splits the large pair needs less than under the planner's own 5: each case grows the workspace
@pytest.mark.parametrize("split", [3, None])
def test_descriptor_set_knn_interleaved_while_the_workspace_grows(split, monkeypatch):
    _set_split(monkeypatch, split)
    d1, d2 = _pair(129, 257, 128)
    rng = np.random.default_rng(77)
    big1 = rng.integers(0, 256, (5000, 128), dtype=np.uint8)
    big2 = rng.integers(0, 256, (1100, 128), dtype=np.uint8)
    splits = 3 if split else 5                            # the planner: at most one split per 256 columns
    need = 2 * (splits + 1) * 5000 * 8 * 4                # idx and dist: the partials and the results
    exp_match = F.match_descriptors(d1, d2, backend="host")
    with F.DescriptorSet(d1) as a, F.DescriptorSet(d2) as b, F.DescriptorSet(big1) as p, F.DescriptorSet(big2) as q:
        first = a.knn(b, 8)
        m = a.match(b)
        assert np.array_equal(m[0], exp_match[0]) and np.array_equal(m[1], exp_match[1])
        before = _workspace()
        big = p.knn(q, 8)
        after = _workspace()
        assert after[1] >= need
        if before[1] < need:                              # unless an earlier test left a larger workspace behind
            assert after[0] == before[0] + 1 and after[1] > before[1]
        assert KC.same(big, KC.host(big1, big2, 8, 16))
        again = a.knn(b, 8)
        m = a.match(b)
        assert np.array_equal(m[0], exp_match[0]) and np.array_equal(m[1], exp_match[1])
        assert KC.same(first, again) and KC.same(first, _expected(129, 257, 128, 8))
        assert KC.same(a.knn(b, 3), _expected(129, 257, 128, 3))
        assert _workspace() == after                      # smaller shapes allocate nothing


# ------------------------------------------------------------- end to end --
def test_guided_homography_from_one_to_many_matches():
    """Every shared keypoint has three equally good candidates, one of them
    true: a third of the correspondences are inliers.  Each gets the weight
    1 / group."""
    kp1, d1, kp2, d2, pairs, _ = S.problem_match_repeated()
    idx, dist = F.knn_descriptors(d1, d2, 4)
    assert KC.same((idx, dist), F.knn_descriptors(d1, d2, 4, backend="host"))
    m, group, _ = F.matches_from_knn(idx, dist, ratio=0.8)
    truth = set(map(tuple, pairs.tolist()))
    true = np.array([tuple(x) in truth for x in m.tolist()])
    assert true.sum() == len(pairs)
    corr = F.correspondences_from_matches(kp1, kp2, m)
    H, mask = pygcransac.findHomography(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, probabilities=1.0 / group,
                                        threshold=2.0, max_iters=5000, sampler=3, guided_stop=True, seed=1)
    mask = np.asarray(mask).astype(bool)
    found = int((mask & true).sum()) if H is not None else 0
    print(f"{len(m)} correspondences, {int(true.sum())} true; inliers {int(mask.sum()) if H is not None else 0}, "
          f"true inliers {found}")
    assert H is not None and found >= 0.95 * len(pairs)
