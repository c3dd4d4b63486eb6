"""Descriptor sets, host side: csrc/match_select.h's rule (gcr_host_match_select)
on the host twins' search results against the Python front end
(match_descriptors / match_descriptors_guided with backend="host") byte for
byte and against an independent numpy statement of the rule; the stand-alone
program under the sanitizers; exports, signatures and every error that is
reached before GPU work.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import match_cases as MC
import match_geo_cases as MGC
import match_sets_cases as MSC
from pygcransac import _native as N
from pygcransac import features as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")


def _plain_inputs():
    out = {f"{n1}x{n2}": MC.random_pair(n1, n2, 32) for n1, n2 in MC.SHAPES + [(3, 1)]}
    out.update(MC.crafted(32))
    return out


@pytest.fixture(scope="module")
def plain_searches():
    """name -> (d1, d2, forward search, reverse search's idx) by the host twin, computed once"""
    return {name: (d1, d2, MC.host(d1, d2, 4), MC.host(d2, d1, 4)[0]) for name, (d1, d2) in _plain_inputs().items()}


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("ratio", MSC.RATIOS)
def test_select_equals_the_front_end(plain_searches, ratio, mutual):
    for name, (d1, d2, fwd, back) in plain_searches.items():
        got = MSC.as_front_end(MSC.host_select(fwd, back if mutual else None, 0, ratio))
        exp = F.match_descriptors(d1, d2, ratio=ratio, mutual=mutual, backend="host")
        assert MSC.same_result(got, exp), (name, len(got[0]), len(exp[0]))
        assert MSC.same_result(got, MSC.numpy_rule(fwd, back if mutual else None, False, ratio)), name
        if ratio == 1e-9:
            assert len(got[0]) == 0 or (fwd[1][got[0][:, 0]] == 0).all(), name       # only dist 0 < r^2 dist2
        if ratio is None and not mutual:
            assert len(got[0]) == len(d1), name                                       # every row kept


def _guided_inputs():
    cases = dict(MGC.crafted(32))
    cases.update(MGC.family_cases(129, 257, 32))
    cases.update({f"small-{k}": v for k, v in MGC.family_cases(33, 31, 32).items()})
    return cases


@pytest.fixture(scope="module")
def guided_searches():
    """name -> (case, forward search, reverse search's idx) by the host twin"""
    return {name: (case, MGC.host(case, 0, 4), MGC.host(case, 1, 4)[0]) for name, case in _guided_inputs().items()}


def _mid_distance(fwd):
    found = fwd[0] != MGC.NONE
    return float(np.median(fwd[1][found])) if found.any() else 1000.0


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("ratio", MSC.RATIOS)
def test_guided_select_equals_the_front_end(guided_searches, ratio, mutual):
    compared = 0
    for name, (case, fwd, back) in guided_searches.items():
        d1, d2, p1, p2, kind, h, T = case
        for md in (None, 0, _mid_distance(fwd)):
            got = MSC.as_front_end(MSC.host_select(fwd, back if mutual else None, 1, ratio, md))
            assert MSC.same_result(got, MSC.numpy_rule(fwd, back if mutual else None, True, ratio, md)), (name, md)
            t = float(np.sqrt(T))
            if np.isfinite(t) and t > 0 and t * t == T:      # the front end takes the bound in pixels
                exp = F.match_descriptors_guided(d1, d2, p1, p2, np.reshape(h, (3, 3)), MSC.KIND_NAMES[kind], t,
                                                 ratio=ratio, mutual=mutual, max_distance=md, backend="host")
                assert MSC.same_result(got, exp), (name, md, len(got[0]), len(exp[0]))
                compared += 1
    assert compared >= 3 * 10


def test_guided_rows_without_and_with_one_candidate(guided_searches):
    # nothing admissible: no match, mutual or not (back[NONE] is never read: the program under ASan holds that)
    case, fwd, back = guided_searches["nothing"]
    assert (fwd[0] == MGC.NONE).all()
    for b in (None, back):
        m, r = MSC.host_select(fwd, b, 1)
        assert m.shape == (0, 2) and r.shape == (0,)
    # exactly one candidate per row: it passes any ratio test (nothing competes), with ratio 1.0
    case, fwd, back = guided_searches["single"]
    one = (fwd[0] != MGC.NONE) & (fwd[2] == MGC.NONE)
    assert one.sum() >= 60
    m, r = MSC.host_select(fwd, None, 1, ratio=1e-9)
    assert np.array_equal(m[:, 0], np.nonzero(one)[0]) and (r == 1.0).all()
    # in reverse some rows have no candidate: the mutual check still finds the pairs
    assert (back == MGC.NONE).any()
    mm, _ = MSC.host_select(fwd, back, 1, ratio=0.8)
    assert 0 < len(mm) <= len(m) and (back[mm[:, 1]] == mm[:, 0]).all()
    # the plain rule on the same rows drops them: no second neighbour fails the ratio test
    assert len(MSC.host_select(fwd, None, 0, ratio=0.8)[0]) == 0


def test_ratio_edge_cases_through_select():
    """test_ratio_edge_cases of test_match_descriptors.py, through the select entry"""
    d1 = np.zeros((3, 32), np.uint8)
    d1[1] = 7
    one = MC.host(d1, d1[:1])
    m, r = MSC.host_select(one, None, 0, ratio=0.8)
    assert m.shape == (0, 2) and m.dtype == np.uint32 and r.shape == (0,)
    m, r = MSC.host_select(one, None, 0)
    assert np.array_equal(m, [[0, 0], [1, 0], [2, 0]]) and np.array_equal(r, [1.0, 1.0, 1.0])
    # 0 / 0 (two equal nearest rows): ratio 1.0; the test 0 < r^2 * 0 fails
    own = MC.host(d1, d1)
    m, r = MSC.host_select(own, None, 0)
    assert np.array_equal(m, [[0, 0], [1, 1], [2, 0]]) and np.array_equal(r, [1.0, 0.0, 1.0])
    m, r = MSC.host_select(own, own[0], 0, ratio=0.8)
    assert np.array_equal(m, [[1, 1]]) and np.array_equal(r, [0.0])
    # a larger cap changes nothing and nothing is written past M
    m2, r2 = MSC.host_select(own, own[0], 0, ratio=0.8, cap=10)
    assert np.array_equal(m2, m) and np.array_equal(r2, r)


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/match_select_host.cpp: the rule on searched and crafted rows
    (every row kept, none kept, idx == kMatchNone under mutual) and the
    argument check, a stand-alone host program built with ASan + UBSan."""
    exe = str(tmp_path / "match_select_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "cpp", "match_select_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout


def test_exports_and_signatures():
    for name in ("DescriptorSet", "match_pairs", "match_descriptors", "match_descriptors_guided"):
        assert name in F.__all__
    sig = inspect.signature(F.DescriptorSet.__init__).parameters
    assert list(sig) == ["self", "desc", "keypoints", "device"]
    assert sig["keypoints"].default is None and sig["device"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(F.DescriptorSet.match).parameters
    assert list(sig) == ["self", "other", "ratio", "mutual"] and sig["ratio"].default == 0.8
    assert sig["mutual"].default is True
    sig = inspect.signature(F.DescriptorSet.match_guided).parameters
    assert list(sig) == ["self", "other", "model", "kind", "threshold", "ratio", "mutual", "max_distance"]
    assert sig["ratio"].default is None and sig["mutual"].default is True and sig["max_distance"].default is None
    sig = inspect.signature(F.match_pairs).parameters
    assert list(sig) == ["sets", "pairs", "ratio", "mutual"] and sig["ratio"].default == 0.8
    for attr in ("dim", "has_keypoints", "close", "__len__", "__enter__", "__exit__"):
        assert hasattr(F.DescriptorSet, attr), attr
    # the array functions keep their signatures; binary descriptors are a documented recipe
    assert list(inspect.signature(F.match_descriptors).parameters) == ["desc1", "desc2", "ratio", "mutual", "backend",
                                                                       "device"]
    assert "unpackbits" in F.match_descriptors.__doc__
    for fn in ("gcr_descriptors_create", "gcr_descriptors_destroy", "gcr_descriptors_info", "gcr_match_sets",
               "gcr_match_sets_guided", "gcr_match_set_pairs", "gcr_host_match_select", "gcr_match_select_tiling",
               "gcr_debug_match_workspace"):
        assert hasattr(N.lib, fn), fn
    assert N.lib.gcr_abi_version() == 5
    R = MSC.select_rows()
    assert R >= 64 and R % 64 == 0
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "match_sets.hip" in text and "match_select.h" in text


def test_unpackbits_gives_the_hamming_order():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (20, 32), dtype=np.uint8), rng.integers(0, 256, (30, 32), dtype=np.uint8)
    idx, dist, _, _ = MC.host(np.unpackbits(a, axis=1), np.unpackbits(b, axis=1))
    ham = np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2)
    assert np.array_equal(dist, ham.min(1)) and np.array_equal(idx, ham.argmin(1))


def test_python_errors_before_gpu_work():
    d = np.zeros((4, 128), np.uint8)
    with pytest.raises(ValueError, match="quantize_descriptors"):
        F.DescriptorSet(d.astype(np.float32))
    with pytest.raises(ValueError, match="shape"):
        F.DescriptorSet(np.zeros(128, np.uint8))
    for shape in ((4, 48), (4, 16), (4, 544), (4, 0)):
        with pytest.raises(ValueError, match="multiple of 32"):
            F.DescriptorSet(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match="at least one row"):
        F.DescriptorSet(np.zeros((0, 128), np.uint8))
    with pytest.raises(ValueError, match="one keypoint per descriptor"):
        F.DescriptorSet(d, np.zeros((3, 2)))
    with pytest.raises(ValueError, match="non-finite"):
        F.DescriptorSet(d, np.full((4, 2), np.nan))
    with pytest.raises(ValueError, match="DescriptorSets"):
        F.match_pairs([d], [(0, 0)])
    with pytest.raises(ValueError, match="integer pairs"):
        F.match_pairs([], [(0, 1, 2)])
    with pytest.raises(ValueError, match="index past"):
        F.match_pairs([], [(0, 0)])
    assert F.match_pairs([], []) == []


def test_c_entries_reject_bad_arguments():
    """every check that precedes GPU work, with a NULL context"""
    out = C.c_void_p()
    d = np.zeros((4, 64), np.uint8)
    a = d.ctypes.data
    big = (1 << 24) + 1

    def create(ptr, n, dim, pos, outp, word):
        rc = N.lib.gcr_descriptors_create(None, ptr, n, dim, pos, outp)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (word, N.last_error())

    create(a, 4, 64, None, None, "out")
    create(None, 4, 64, None, C.byref(out), "d is NULL")
    create(a, 0, 64, None, C.byref(out), " n ")
    create(a, big, 64, None, C.byref(out), " n ")
    for dim in (0, 16, 48, 100, 544, 1024):
        create(a, 4, dim, None, C.byref(out), "dim")
    for bad in (np.nan, np.inf, -np.inf):
        pos = np.zeros((4, 2))
        pos[3, 1] = bad
        create(a, 4, 64, pos.ctypes.data, C.byref(out), "positions")
    create(a, 4, 64, None, C.byref(out), "context")          # good arguments and no context
    assert out.value is None
    N.lib.gcr_descriptors_destroy(None)                       # safe on NULL
    assert N.lib.gcr_descriptors_info(None, None, None, None) == N.GCR_EINVAL and "set" in N.last_error()

    opt = MSC.options(0.8, True)
    m = C.c_size_t()
    buf = np.zeros(8, np.uint32)
    rat = np.zeros(4)
    assert N.lib.gcr_match_sets(None, None, None, opt, buf.ctypes.data, rat.ctypes.data, 4, C.byref(m), None) \
        == N.GCR_EINVAL and "a is NULL" in N.last_error()
    ident = np.eye(3)
    assert N.lib.gcr_match_sets_guided(None, None, None, 3, ident.ctypes.data, 1.0, opt, buf.ctypes.data,
                                       rat.ctypes.data, 4, C.byref(m), None) == N.GCR_EINVAL
    assert "a is NULL" in N.last_error()
    offs = np.zeros(2, np.uintp)
    cnt = np.zeros(1, np.uintp)
    pr = np.zeros(2, np.uint32)
    args = (pr.ctypes.data, 1, opt, buf.ctypes.data, rat.ctypes.data, offs.ctypes.data, cnt.ctypes.data, None)
    assert N.lib.gcr_match_set_pairs(None, None, 0, *args) == N.GCR_EINVAL and "sets is NULL" in N.last_error()
    hs = (C.c_void_p * 1)()
    assert N.lib.gcr_match_set_pairs(None, C.addressof(hs), 1, pr.ctypes.data, 1, None, *args[3:]) == N.GCR_EINVAL
    assert "opt is NULL" in N.last_error()
    assert N.lib.gcr_match_set_pairs(None, C.addressof(hs), 1, *args) == N.GCR_EINVAL and "context" in N.last_error()
    assert N.lib.gcr_debug_match_workspace(None, (C.c_uint64 * 2)()) == N.GCR_EINVAL and "context" in N.last_error()
    N.lib.gcr_match_select_tiling(None)                       # safe on NULL

    # the host select entry: every argument
    s = [np.zeros(4, np.uint32) for _ in range(4)]
    p = [x.ctypes.data for x in s]

    def select(ptrs, n, back, nb, guided, o, mo, ro, cap, mp, word):
        rc = N.lib.gcr_host_match_select(*ptrs, n, back, nb, guided, o, mo, ro, cap, mp)
        assert rc == N.GCR_EINVAL and word in N.last_error(), (word, N.last_error())

    good = (p, 4, None, 0, 0, opt, buf.ctypes.data, rat.ctypes.data, 4, C.byref(m))
    assert N.lib.gcr_host_match_select(*good[0], *good[1:]) == 0
    for k, name in enumerate(("idx", "dist", "idx2", "dist2")):
        select(p[:k] + [None] + p[k + 1:], *good[1:], name + " is NULL")
    select(p, 0, *good[2:], " n ")
    select(p, big, *good[2:], " n ")
    select(p, 4, p[0], 0, *good[4:], "nb")
    select(p, 4, None, 0, 2, *good[5:], "guided")
    select(p, 4, None, 0, 0, None, *good[6:], "opt")
    select(*good[:6], None, *good[7:], "matches_out")
    select(*good[:7], None, *good[8:], "ratios_out")
    select(*good[:8], 3, good[9], "cap")
    select(*good[:9], None, "m_out")
    for rr in (0.0, -1.0, np.inf, np.nan):
        bad = MSC.options(0.8, False)
        bad.rr = rr
        select(*good[:5], bad, *good[6:], "rr")
    bad = MSC.options(None, False, 5.0)
    select(*good[:5], bad, *good[6:], "guided entries only")
    bad.max_distance = -1.0
    select(p, 4, None, 0, 1, bad, *good[6:], "max_distance")
