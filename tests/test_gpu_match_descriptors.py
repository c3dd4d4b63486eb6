"""Descriptor matching on the GPU: gcr_match_descriptors (csrc/match.hip, int8
matrix cores) against the host twin bit for bit -- at the shared shapes, at the
kernel's tiling constants minus one, exact and plus one, at every dim class,
with the column split free and pinned, on the crafted inputs -- and the
pipeline match_descriptors -> estimator on the synthetic image pair."""
import functools

import numpy as np
import pytest

import match_cases as MC
import pygcransac
from pygcransac import features as F
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

# the kernel's tiling (csrc/match.h; asserted against gcr_match_tiling below)
ROWS_PER_WG, STEP_COLS, SPLIT_MIN_COLS = 128, 64, 256
NAMES = ("idx", "dist", "idx2", "dist2")


@functools.lru_cache(maxsize=None)
def _case(n1, n2, dim):
    d1, d2 = MC.random_pair(n1, n2, dim)
    return d1, d2, MC.host(d1, d2, 16)


def _check(d1, d2, exp):
    got = MC.gpu(d1, d2)
    for g, e, name in zip(got, exp, NAMES):
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, f"{name}: {bad.size} rows differ, first {bad[:5]}: {g[bad[:5]]} != {e[bad[:5]]}"


def test_tiling_constants():
    assert MC.tiling() == (ROWS_PER_WG, STEP_COLS, SPLIT_MIN_COLS)


@pytest.mark.parametrize("dim", MC.DIMS)
@pytest.mark.parametrize("n1,n2", MC.SHAPES)
def test_gpu_equals_host_twin(n1, n2, dim):
    _check(*_case(n1, n2, dim))


# rows per workgroup (n1), columns per step and the least columns per split
# (n2), each minus one, exact and plus one; two workgroups and several steps
EDGES = ([(ROWS_PER_WG + k, 70) for k in (-1, 0, 1)] + [(2 * ROWS_PER_WG + k, 70) for k in (-1, 0, 1)] +
         [(40, STEP_COLS + k) for k in (-1, 0, 1)] + [(40, 32 + k) for k in (-1, 0, 1)] +
         [(40, SPLIT_MIN_COLS + k) for k in (-1, 0, 1)] + [(40, 2 * SPLIT_MIN_COLS + k) for k in (-1, 0, 1)])


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("n1,n2", EDGES)
def test_tiling_edges(n1, n2, split, monkeypatch):
    if split is None:
        monkeypatch.delenv("GCR_MATCH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("GCR_MATCH_SPLIT", str(split))
    _check(*_case(n1, n2, 128))


# pinned to 3 splits the columns per split are ceil(n2 / 3) rounded up to whole
# steps: 128 at n2 = 383 and 384, 192 at 385; 1000 x 257 gives splits of 128, 128, 1
@pytest.mark.parametrize("dim", MC.DIMS)
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("n1,n2", [(129, 383), (129, 384), (129, 385), (1000, 257)])
def test_pinned_splits(n1, n2, split, dim, monkeypatch):
    monkeypatch.setenv("GCR_MATCH_SPLIT", str(split))
    _check(*_case(n1, n2, dim))


@pytest.mark.parametrize("dim", [32, 64, 96, 160, 256, 480])
def test_other_dims(dim):
    _check(*_case(70, 200, dim))


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("dim", MC.DIMS)
def test_crafted_rows(dim, split, monkeypatch):
    if split is None:
        monkeypatch.delenv("GCR_MATCH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("GCR_MATCH_SPLIT", str(split))
    for name, (d1, d2) in MC.crafted(dim).items():
        exp = MC.host(d1, d2, 16)
        got = MC.gpu(d1, d2)
        assert MC.same(got, exp), name
    idx, dist, idx2, dist2 = MC.gpu(*MC.crafted(dim)["padding"])
    assert (dist == dim * 255 * 255).all() and (idx == 0).all() and (idx2 == 1).all()


def test_two_calls_give_the_same_bytes():
    d1, d2, _ = _case(1000, 257, 128)
    assert MC.same(MC.gpu(d1, d2), MC.gpu(d1, d2))


def test_kernel_time_is_reported():
    import ctypes as C

    from pygcransac import _native as N
    d1, d2, exp = _case(129, 257, 128)
    out = [np.empty(len(d1), dtype=np.uint32) for _ in range(4)]
    ms = C.c_double(-1.0)
    N.check(N.lib.gcr_match_descriptors(N.context(None), d1.ctypes.data, len(d1), d2.ctypes.data, len(d2), 128,
                                        *[o.ctypes.data for o in out], C.byref(ms)))
    assert MC.same(out, exp) and 0.0 < ms.value < 1000.0


# ------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def problem():
    return S.problem_match()


def test_front_end_backends_agree(problem):
    _, d1, _, d2, _, _ = problem
    for kw in (dict(ratio=0.8, mutual=True), dict(ratio=None, mutual=False)):
        mg, rg = F.match_descriptors(d1, d2, **kw)
        mh, rh = F.match_descriptors(d1, d2, backend="host", **kw)
        assert np.array_equal(mg, mh) and np.array_equal(rg, rh)


def test_prosac_homography_from_all_matches(problem):
    """Every nearest neighbour kept (60 % of the matches are false), the
    ratios as PROSAC's quality scores."""
    kp1, d1, kp2, d2, pairs, _ = problem
    m, r = F.match_descriptors(d1, d2, ratio=None, mutual=False)
    assert len(m) == 1000
    truth = set(map(tuple, pairs.tolist()))
    true = np.array([tuple(x) in truth for x in m.tolist()])
    assert true.sum() == len(pairs)
    corr = F.correspondences_from_matches(kp1, kp2, m)
    H, mask = pygcransac.findHomography(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, probabilities=-r, threshold=2.0,
                                        conf=0.99, max_iters=5000, min_iters=50, sampler=1, seed=1)
    mask = np.asarray(mask).astype(bool)
    assert H is not None and int((mask & true).sum()) >= 0.95 * len(pairs)


def test_sift_homography_from_filtered_matches(problem):
    kp1, d1, kp2, d2, pairs, _ = problem
    m, r = F.match_descriptors(d1, d2, ratio=0.8, mutual=True)
    truth = set(map(tuple, pairs.tolist()))
    true = np.array([tuple(x) in truth for x in m.tolist()])
    c8 = F.correspondences_from_matches(kp1, kp2, m, sift=True)
    assert c8.shape == (len(m), 8)
    H, mask = pygcransac.findHomographySIFT(c8, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, threshold=2.0, conf=0.99,
                                            max_iters=5000, min_iters=50, seed=1)
    mask = np.asarray(mask).astype(bool)
    assert H is not None and int((mask & true).sum()) >= 0.95 * len(pairs)
