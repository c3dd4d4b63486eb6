"""Guided descriptor matching on the GPU: gcr_match_descriptors_guided
(csrc/match.hip, k_match_geo) against the host twin bit for bit -- at the
shared shapes, at the kernel's tiling constants minus one, exact and plus one,
at every dim class, with the column split free and pinned, both kinds, both
directions, on the lattice and the generic family and on every crafted input
-- and the pipeline match_descriptors -> findHomography ->
match_descriptors_guided on the synthetic image pair."""
import ctypes as C
import functools

import numpy as np
import pytest

import match_cases as MC
import match_geo_cases as G
import pygcransac
from pygcransac import features as F
from pygcransac import synthetic as S
from test_gpu_match_descriptors import EDGES

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _family(n1, n2, dim):
    """name -> (case, host result forward, host result reverse)"""
    return {name: (case, G.host(case, 0, 16), G.host(case, 1, 16)) for name, case in G.family_cases(n1, n2, dim).items()}


def _check_family(n1, n2, dim):
    for name, (case, fwd, rev) in _family(n1, n2, dim).items():
        for reverse, exp in ((0, fwd), (1, rev)):
            diff = G.differences(G.gpu(case, reverse), exp)
            assert not diff, f"{name} reverse={reverse}: {diff}"


def _pin(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("GCR_MATCH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("GCR_MATCH_SPLIT", str(split))


@pytest.mark.parametrize("n1,n2", MC.SHAPES)
def test_gpu_equals_host_twin(n1, n2):
    _check_family(n1, n2, 128)


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("n1,n2", EDGES)
def test_tiling_edges(n1, n2, split, monkeypatch):
    """Rows per workgroup, columns per step, per tile and the least columns per
    split, each minus one, exact and plus one.  The kernel's rows are image 2
    in reverse, so the swapped pair runs too: either image meets the row and
    the column edges in either direction."""
    _pin(monkeypatch, split)
    _check_family(n1, n2, 128)
    _check_family(n2, n1, 128)


@pytest.mark.parametrize("dim", [32, 512, 96, 160])
@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("n1,n2", [(129, 385), (70, 200)])
def test_dims_and_pinned_splits(n1, n2, split, dim, monkeypatch):
    _pin(monkeypatch, split)
    _check_family(n1, n2, dim)


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("dim", MC.DIMS)
def test_crafted_rows(dim, split, monkeypatch):
    _pin(monkeypatch, split)
    cases = G.crafted(dim)
    for name, case in cases.items():
        for reverse in (0, 1):
            diff = G.differences(G.gpu(case, reverse), G.host(case, reverse, 16))
            assert not diff, f"{name} reverse={reverse}: {diff}"
    for reverse in (0, 1):
        assert all((o == G.NONE).all() for o in G.gpu(cases["nothing"], reverse))
    idx, dist, idx2, dist2 = G.gpu(cases["single"])
    assert np.array_equal(cases["single"][3][idx], cases["single"][2]) and (idx2 == G.NONE).all() and \
        (dist2 == G.NONE).all() and (dist != G.NONE).all()
    idx, dist, idx2, dist2 = G.gpu(cases["padding"])
    assert (dist == dim * 255 * 255).all() and (idx == 0).all() and (idx2 == 1).all()


@pytest.mark.parametrize("name", ["inf_identity", "inf_identity_F"])
def test_infinite_bound_gives_the_unguided_bytes(name):
    case = G.crafted(128)[name]
    d1, d2 = case[:2]
    assert MC.same(G.gpu(case, 0), MC.gpu(d1, d2))
    assert MC.same(G.gpu(case, 1), MC.gpu(d2, d1))


def test_two_calls_give_the_same_bytes():
    for kind in G.KINDS:
        case = G.lattice_case(1000, 257, 128, kind, 1)
        for reverse in (0, 1):
            assert MC.same(G.gpu(case, reverse), G.gpu(case, reverse))


def test_kernel_time_is_reported():
    case, fwd, _ = _family(129, 257, 128)["generic-F"]
    ms = C.c_double(-1.0)
    assert MC.same(G.gpu(case, 0, ms=ms), fwd) and 0.0 < ms.value < 1000.0


# ------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def noisy():
    return S.problem_match(1000, 400, desc_noise=70.0)


def test_front_end_backends_agree(noisy):
    kp1, d1, kp2, d2, _, H_gt = noisy
    Fm = G.skew(G.E_GENERIC) @ H_gt
    for model, kind in ((H_gt, "homography"), (Fm, "fundamental")):
        for kw in (dict(), dict(ratio=0.8), dict(mutual=False, max_distance=1000000)):
            mg, rg = F.match_descriptors_guided(d1, d2, kp1, kp2, model, kind, 3.0, **kw)
            mh, rh = F.match_descriptors_guided(d1, d2, kp1, kp2, model, kind, 3.0, backend="host", **kw)
            assert len(mg) > 0 and np.array_equal(mg, mh) and np.array_equal(rg, rh)


def test_guided_matching_with_the_estimated_homography(noisy):
    """match_descriptors -> findHomography -> match_descriptors_guided: the
    truth pairs found with the estimated H against those found with H_gt (the
    reference).  Measured: 63 plain matches (all true); with the estimated H
    400 of 400 truth pairs (401 returned), with H_gt 400 (401 returned):
    ratio 1.000."""
    kp1, d1, kp2, d2, pairs, H_gt = noisy
    truth = set(map(tuple, pairs.tolist()))
    m, _ = F.match_descriptors(d1, d2, ratio=0.8, mutual=True)
    corr = F.correspondences_from_matches(kp1, kp2, m)
    H, mask = pygcransac.findHomography(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, threshold=2.0, conf=0.99,
                                        max_iters=5000, min_iters=50, seed=1)
    assert H is not None
    mg, _ = F.match_descriptors_guided(d1, d2, kp1, kp2, H, "homography", 3.0)
    mr, _ = F.match_descriptors_guided(d1, d2, kp1, kp2, H_gt, "homography", 3.0)
    found = len(set(map(tuple, mg.tolist())) & truth)
    ref = len(set(map(tuple, mr.tolist())) & truth)
    print(f"plain matches {len(m)}, inliers {int(np.asarray(mask).sum())}; truth pairs found with the estimated H "
          f"{found} of {len(mg)} returned, with H_gt {ref} of {len(mr)}: ratio {found / ref:.3f}")
    assert ref >= 380 and found >= 0.9 * ref
