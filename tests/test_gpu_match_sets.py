"""Descriptor sets on the GPU: DescriptorSet.match / match_guided / match_pairs
(csrc/match_sets.hip: the searches on resident sets, k_match_select_*) against
the array functions byte for byte -- at the select kernels' rows per workgroup
minus one, exact and plus one, with the column split free and pinned, on the
crafted inputs, with sets reused on either side -- the workspace's allocation
count, the errors, and the pipeline match -> findHomography -> match_guided
on two sets."""
import ctypes as C

import numpy as np
import pytest

import match_cases as MC
import match_geo_cases as MGC
import match_sets_cases as MSC
import pygcransac
from pygcransac import _native as N
from pygcransac import features as F
from pygcransac import synthetic as S

pytestmark = pytest.mark.gpu

R = MSC.select_rows()
SHAPES = [(1, 1), (1, 2), (2, 1), (129, 257), (R - 1, 70), (R, 70), (R + 1, 70), (3 * R + 1, 300)]
GRID = [(ratio, mutual) for ratio in MSC.RATIOS for mutual in (False, True)]


def _pin(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("GCR_MATCH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("GCR_MATCH_SPLIT", str(split))


def _check_plain(d1, d2, name=""):
    """a.match(b) against the array function on the GPU and on the host, over the option grid"""
    with F.DescriptorSet(d1) as a, F.DescriptorSet(d2) as b:
        assert len(a) == len(d1) and a.dim == d1.shape[1] and not a.has_keypoints
        for ratio, mutual in GRID:
            got = a.match(b, ratio=ratio, mutual=mutual)
            assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[0].shape == (len(got[1]), 2)
            for backend in ("gpu", "host"):
                exp = F.match_descriptors(d1, d2, ratio=ratio, mutual=mutual, backend=backend)
                assert MSC.same_result(got, exp), (name, ratio, mutual, backend, len(got[0]), len(exp[0]))
            if ratio == 1e-9:
                assert len(got[0]) == 0, name                  # random rows: no distance 0


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_match_equals_the_array_function(n1, n2):
    _check_plain(*MC.random_pair(n1, n2, 128), name=f"{n1}x{n2}")


def test_crafted_rows():
    for name, (d1, d2) in MC.crafted(128).items():
        with F.DescriptorSet(d1) as a, F.DescriptorSet(d2) as b:
            for ratio, mutual in GRID:
                got = a.match(b, ratio=ratio, mutual=mutual)
                for backend in ("gpu", "host"):
                    exp = F.match_descriptors(d1, d2, ratio=ratio, mutual=mutual, backend=backend)
                    assert MSC.same_result(got, exp), (name, ratio, mutual, backend)


@pytest.mark.parametrize("dim", [32, 128, 512])
def test_dims(dim):
    _check_plain(*MC.random_pair(129, 257, dim), name=f"dim {dim}")


@pytest.mark.parametrize("split", [None, 1, 3])
def test_pinned_splits(split, monkeypatch):
    _pin(monkeypatch, split)
    _check_plain(*MC.random_pair(3 * R + 1, 300, 128), name=f"split {split}")


# ------------------------------------------------------------------- reuse --
def test_one_set_on_either_side_and_against_itself():
    d1, d2 = MC.random_pair(R + 1, 300, 128)
    with F.DescriptorSet(d1) as a, F.DescriptorSet(d2) as b:
        first = a.match(b)
        assert MSC.same_result(first, F.match_descriptors(d1, d2))
        assert MSC.same_result(b.match(a), F.match_descriptors(d2, d1))
        own = a.match(a, ratio=None)
        assert MSC.same_result(own, F.match_descriptors(d1, d1, ratio=None))
        assert np.array_equal(own[0][:, 0], own[0][:, 1]) and len(own[0]) == len(d1)
        assert MSC.same_result(a.match(b), first)


def test_three_sets_in_all_ordered_pairs():
    rng = np.random.default_rng(11)
    ds = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in (70, R + 1, 300)]
    sets = [F.DescriptorSet(d) for d in ds]
    try:
        for i in range(3):
            for j in range(3):
                if i != j:
                    assert MSC.same_result(sets[i].match(sets[j], ratio=None),
                                           F.match_descriptors(ds[i], ds[j], ratio=None)), (i, j)
    finally:
        for s in sets:
            s.close()


# ------------------------------------------------------------------ guided --
def _sets_guided(a, b, kind, h, T, ratio, mutual, md):
    """gcr_match_sets_guided with the squared bound as given (the Python front end takes pixels)"""
    matches = np.empty((len(a), 2), dtype=np.uint32)
    ratios = np.empty(len(a))
    m = C.c_size_t()
    h = np.ascontiguousarray(h, dtype=np.float64)
    N.check(N.lib.gcr_match_sets_guided(a._ctx, a._handle, b._handle, int(kind), h.ctypes.data, float(T),
                                        MSC.options(ratio, mutual, md), matches.ctypes.data, ratios.ctypes.data,
                                        len(a), C.byref(m), None))
    return matches[:m.value].astype(np.int64), ratios[:m.value].copy()


def _check_guided(name, case):
    d1, d2, p1, p2, kind, h, T = case
    fwd, back = MGC.host(case, 0, 16), MGC.host(case, 1, 16)[0]
    found = fwd[0] != MGC.NONE
    mid = float(np.median(fwd[1][found])) if found.any() else 1000.0
    t = float(np.sqrt(T))
    in_pixels = np.isfinite(t) and t > 0 and t * t == T
    with F.DescriptorSet(d1, p1) as a, F.DescriptorSet(d2, p2) as b:
        assert a.has_keypoints and b.has_keypoints
        for mutual in (False, True):
            for ratio, md in ((None, None), (0.8, None), (None, 0), (0.8, mid), (1e9, mid)):
                got = _sets_guided(a, b, kind, h, T, ratio, mutual, md)
                exp = MSC.numpy_rule(fwd, back if mutual else None, True, ratio, md)
                assert MSC.same_result(got, exp), (name, mutual, ratio, md, len(got[0]), len(exp[0]))
                if in_pixels:
                    model, kname = np.reshape(h, (3, 3)), MSC.KIND_NAMES[kind]
                    got = a.match_guided(b, model, kname, t, ratio=ratio, mutual=mutual, max_distance=md)
                    exp = F.match_descriptors_guided(d1, d2, p1, p2, model, kname, t, ratio=ratio, mutual=mutual,
                                                     max_distance=md)
                    assert MSC.same_result(got, exp), (name, mutual, ratio, md, "front end")
    return fwd


@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 1), (33, 31), (129, 257), (R + 1, 70)])
def test_guided_equals_the_array_function(n1, n2):
    for name, case in MGC.family_cases(n1, n2, 128).items():
        _check_guided(f"{name} {n1}x{n2}", case)


def test_guided_crafted_rows():
    cases = MGC.crafted(128)
    for name, case in cases.items():
        fwd = _check_guided(name, case)
        if name == "nothing":
            assert (fwd[0] == MGC.NONE).all()                 # rows without a candidate, mutual included above
        if name == "single":
            assert (fwd[2] == MGC.NONE).all() and (fwd[0] != MGC.NONE).all()


@pytest.mark.parametrize("name", ["inf_identity", "inf_identity_F"])
def test_infinite_bound_gives_the_unguided_bytes(name):
    d1, d2, p1, p2, kind, h, T = MGC.crafted(128)[name]
    assert T == MGC.INF
    with F.DescriptorSet(d1, p1) as a, F.DescriptorSet(d2, p2) as b:
        for ratio, mutual in GRID:
            if ratio == 1e-9:
                continue
            # the two rules differ only where there is no second neighbour: not here (257 columns)
            got = _sets_guided(a, b, kind, h, T, ratio, mutual, None)
            assert MSC.same_result(got, a.match(b, ratio=ratio, mutual=mutual)), (ratio, mutual)
            assert MSC.same_result(got, F.match_descriptors(d1, d2, ratio=ratio, mutual=mutual)), (ratio, mutual)


# ------------------------------------------------------------- match_pairs --
def test_match_pairs_equals_the_single_calls():
    rng = np.random.default_rng(12)
    ds = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in (1, 70, 129, R + 1, 300)]
    sets = [F.DescriptorSet(d) for d in ds]
    pairs = [(0, 1), (1, 0), (4, 3), (3, 4), (2, 2), (4, 3), (0, 0), (1, 4), (4, 1), (3, 3), (2, 0), (3, 1)]
    try:
        assert F.match_pairs(sets, []) == []
        for ratio, mutual in ((0.8, True), (None, False), (1e9, True)):
            got = F.match_pairs(sets, pairs, ratio=ratio, mutual=mutual)
            assert len(got) == len(pairs)
            for (ia, ib), g in zip(pairs, got):
                assert MSC.same_result(g, sets[ia].match(sets[ib], ratio=ratio, mutual=mutual)), (ia, ib, ratio)
        one = F.match_pairs(sets, [(4, 3)], ratio=None, mutual=True)[0]
        assert MSC.same_result(one, F.match_descriptors(ds[4], ds[3], ratio=None, mutual=True))
        with pytest.raises(ValueError, match="index past"):
            F.match_pairs(sets, [(0, 5)])
    finally:
        for s in sets:
            s.close()


# --------------------------------------------------------------- workspace --
def test_fitting_calls_allocate_nothing():
    d1, d2 = MC.random_pair(3 * R + 1, 300, 128)
    with F.DescriptorSet(d1) as a, F.DescriptorSet(d2) as b, F.DescriptorSet(d1[:70]) as small:
        first = a.match(b)                                     # the warm-up: may grow the workspace
        allocs, held = MSC.workspace()
        assert allocs >= 1 and held > 0
        for _ in range(5):
            assert MSC.same_result(a.match(b), first)
        small.match(b)
        assert MSC.workspace() == (allocs, held)
    big1, big2 = MC.random_pair(40 * R, 2000, 128)
    with F.DescriptorSet(big1) as a, F.DescriptorSet(big2) as b:
        a.match(b)
        grown = MSC.workspace()
        assert grown[0] >= allocs and grown[1] >= held
        a.match(b)
        assert MSC.workspace() == grown


def test_kernel_times_are_reported():
    d1, d2 = MC.random_pair(R + 1, 300, 128)
    with F.DescriptorSet(d1) as a, F.DescriptorSet(d2) as b:
        matches = np.empty((len(a), 2), dtype=np.uint32)
        ratios = np.empty(len(a))
        m = C.c_size_t()
        ms = np.full(4, -1.0)
        N.check(N.lib.gcr_match_sets(a._ctx, a._handle, b._handle, MSC.options(0.8, True), matches.ctypes.data,
                                     ratios.ctypes.data, len(a), C.byref(m), ms.ctypes.data))
        assert (ms > 0.0).all() and ms[0] < 1000.0 and ms[1:].sum() <= ms[0] * 1.5 + 0.1


# ------------------------------------------------------------------ errors --
def test_errors():
    d = np.zeros((4, 128), np.uint8)
    a, b = F.DescriptorSet(d), F.DescriptorSet(np.zeros((4, 64), np.uint8))
    kp = F.DescriptorSet(d, np.zeros((4, 2)))
    with pytest.raises(ValueError, match="differ in dimension"):
        a.match(b)
    with pytest.raises(ValueError, match="keypoints"):
        kp.match_guided(a, np.eye(3), "homography", 1.0)
    with pytest.raises(ValueError, match="kind"):
        kp.match_guided(kp, np.eye(3), "affine", 1.0)
    with pytest.raises(ValueError, match="threshold"):
        kp.match_guided(kp, np.eye(3), "homography", 0.0)
    with pytest.raises(ValueError, match="ratio"):
        a.match(a, ratio=-1.0)
    with pytest.raises(ValueError, match="DescriptorSet"):
        a.match(d)
    # the C entry: cap below the rows, sets without positions, different dim; nothing is written
    matches = np.full((4, 2), 7, dtype=np.uint32)
    ratios = np.zeros(4)
    m = C.c_size_t(99)
    opt = MSC.options(0.8, True)
    args = (matches.ctypes.data, ratios.ctypes.data)
    ctx = a._ctx
    rc = N.lib.gcr_match_sets(ctx, a._handle, a._handle, opt, *args, 3, C.byref(m), None)
    assert rc == N.GCR_EINVAL and "cap" in N.last_error() and m.value == 99 and (matches == 7).all()
    rc = N.lib.gcr_match_sets(ctx, a._handle, b._handle, opt, *args, 4, C.byref(m), None)
    assert rc == N.GCR_EINVAL and "dim" in N.last_error()
    rc = N.lib.gcr_match_sets(ctx, a._handle, None, opt, *args, 4, C.byref(m), None)
    assert rc == N.GCR_EINVAL and "b is NULL" in N.last_error()
    ident = np.eye(3)
    rc = N.lib.gcr_match_sets_guided(ctx, kp._handle, a._handle, 3, ident.ctypes.data, 1.0, opt, *args, 4, C.byref(m),
                                     None)
    assert rc == N.GCR_EINVAL and "b has no positions" in N.last_error()
    for kind, T, word in ((5, 1.0, "kind"), (3, -1.0, "sq_threshold"), (3, float("nan"), "sq_threshold")):
        rc = N.lib.gcr_match_sets_guided(ctx, kp._handle, kp._handle, kind, ident.ctypes.data, T, opt, *args, 4,
                                         C.byref(m), None)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (word, N.last_error())
    hs = (C.c_void_p * 2)(a._handle, kp._handle)
    pr = np.array([[0, 2]], dtype=np.uint32)
    offs = np.array([0, 4], dtype=np.uintp)
    cnt = np.zeros(1, dtype=np.uintp)
    rc = N.lib.gcr_match_set_pairs(ctx, C.addressof(hs), 2, pr.ctypes.data, 1, opt, *args, offs.ctypes.data,
                                   cnt.ctypes.data, None)
    assert rc == N.GCR_EINVAL and "nsets" in N.last_error()
    pr[0, 1] = 1
    offs[1] = 3
    rc = N.lib.gcr_match_set_pairs(ctx, C.addressof(hs), 2, pr.ctypes.data, 1, opt, *args, offs.ctypes.data,
                                   cnt.ctypes.data, None)
    assert rc == N.GCR_EINVAL and "offsets" in N.last_error()
    n, dim, has = C.c_size_t(), C.c_uint32(), C.c_int()
    assert N.lib.gcr_descriptors_info(kp._handle, C.byref(n), C.byref(dim), C.byref(has)) == 0
    assert (n.value, dim.value, has.value) == (4, 128, 1)
    # a closed set
    a.close()
    a.close()                                                  # twice is fine
    assert a.closed
    for call in (lambda: a.match(kp), lambda: kp.match(a), lambda: F.match_pairs([kp, a], [(0, 0)]),
                 lambda: a.__enter__()):
        with pytest.raises(ValueError, match="closed"):
            call()
    b.close()
    kp.close()


# ------------------------------------------------------------- end to end --
def test_matching_estimating_and_guided_matching_on_two_sets():
    """test_gpu_match_guided.py's flow on two resident sets: match -> findHomography
    -> match_guided, against the array functions at every step."""
    kp1, d1, kp2, d2, pairs, H_gt = S.problem_match(1000, 400, desc_noise=70.0)
    truth = set(map(tuple, pairs.tolist()))
    with F.DescriptorSet(d1, kp1) as a, F.DescriptorSet(d2, kp2) as b:
        m, r = a.match(b, ratio=0.8, mutual=True)
        assert MSC.same_result((m, r), F.match_descriptors(d1, d2, ratio=0.8, mutual=True))
        corr = F.correspondences_from_matches(kp1, kp2, m)
        H, mask = pygcransac.findHomography(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, threshold=2.0, conf=0.99,
                                            max_iters=5000, min_iters=50, seed=1)
        assert H is not None
        mg = a.match_guided(b, H, "homography", 3.0)
        eg = F.match_descriptors_guided(d1, d2, kp1, kp2, H, "homography", 3.0)
        assert MSC.same_result(mg, eg)
        mr = a.match_guided(b, H_gt, "homography", 3.0)
        er = F.match_descriptors_guided(d1, d2, kp1, kp2, H_gt, "homography", 3.0)
        assert MSC.same_result(mr, er)
        found = len(set(map(tuple, mg[0].tolist())) & truth)
        ref = len(set(map(tuple, er[0].tolist())) & truth)
        assert len(mg[0]) == len(eg[0]) and len(mr[0]) == len(er[0]) and found >= 0.9 * ref > 0
