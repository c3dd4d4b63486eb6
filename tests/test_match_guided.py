"""Guided descriptor matching, host side: csrc/match_geo.h's plain-loop
definition (gcr_host_match_descriptors_guided) against an independent numpy
restatement (tests/match_geo_cases.py) bit for bit, the crafted inputs, the
Python front end (match_descriptors_guided, fundamental_from_essential), every
error, and what guided matching recovers on the synthetic image pair.  No GPU."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import match_cases as MC
import match_geo_cases as G
from pygcransac import _native as N
from pygcransac import features as F
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
INF = float("inf")


def _check(case, reverse, name=""):
    diff = G.differences(G.host(case, reverse), G.restate(*case, reverse))
    assert not diff, f"{name} reverse={reverse}: {diff}"


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("n1,n2", MC.SHAPES)
def test_host_twin_equals_restatement(n1, n2, reverse):
    for name, case in G.family_cases(n1, n2, 128).items():
        _check(case, reverse, name)


@pytest.mark.parametrize("dim", [32, 512])
@pytest.mark.parametrize("n1,n2", [(33, 31), (129, 257)])
def test_host_twin_other_dims(n1, n2, dim):
    for name, case in G.family_cases(n1, n2, dim).items():
        for reverse in (0, 1):
            _check(case, reverse, name)


def test_lattice_shares_and_exact_bounds():
    """The lattice bounds give a low and a middle admissible share, and under
    H residuals equal to T exist (r^2 == T is admissible)."""
    for kind in G.KINDS:
        for share, (lo, hi) in enumerate(((0.05, 0.20), (0.40, 0.60))):
            _, _, p1, p2, _, h, T = G.lattice_case(129, 257, 128, kind, share)
            assert T == int(T)
            r = G.residuals(kind, p1, p2, h)
            assert lo <= (r <= T).mean() <= hi, (kind, share, (r <= T).mean())
            if kind == G.H:
                assert np.array_equal(r, np.rint(r)) and (r == T).sum() > 100
    # the generic family: the truth pairs of problem_match are admissible at 3 px
    _, _, p1, p2, _, h, T = G.generic_case(1000, 1000, 128, G.H)
    assert 300 <= G.admissible(G.H, p1, p2, h, T).sum() <= 500
    _, _, p1, p2, _, h, T = G.generic_case(1000, 1000, 128, G.F)
    assert 0.003 <= G.admissible(G.F, p1, p2, h, T).mean() <= 0.03


@pytest.mark.parametrize("dim", MC.DIMS)
def test_crafted_rows(dim):
    cases = G.crafted(dim)
    for name, case in cases.items():
        for reverse in (0, 1):
            _check(case, reverse, name)
    # nothing admissible: four sentinels
    for reverse in (0, 1):
        assert all((o == G.NONE).all() for o in G.host(cases["nothing"], reverse))
    # one admissible column: the keypoint at the same place, no second
    d1, d2, p1, p2, *_ = cases["single"]
    idx, dist, idx2, dist2 = G.host(cases["single"])
    assert np.array_equal(p2[idx], p1) and (dist != G.NONE).all() and (idx2 == G.NONE).all() and (dist2 == G.NONE).all()
    back = G.host(cases["single"], 1)
    assert (back[0] != G.NONE).sum() == len(d1) and np.array_equal(back[0][idx], np.arange(len(d1)))
    assert (back[2] == G.NONE).all()
    # T = +inf: the unguided matcher's bytes, in both directions
    for name in ("inf_identity", "inf_identity_F"):
        d1, d2 = cases[name][:2]
        assert MC.same(G.host(cases[name]), MC.host(d1, d2)), name
        assert MC.same(G.host(cases[name], 1), MC.host(d2, d1)), name
    # w = 0: the rows with x1 = 5 have infinite (y1 != 0) or NaN (y1 == 0) residuals
    d1, d2, p1, p2, kind, h, T = cases["w_zero"]
    r = G.residuals(kind, p1, p2, h)
    inf_rows = np.isinf(r).all(1)
    nan_rows = np.isnan(r).all(1)
    assert inf_rows.sum() >= 3 and nan_rows.sum() >= 3 and (inf_rows | nan_rows).sum() == (p1[:, 0] == 5.0).sum()
    idx = G.host(cases["w_zero"])[0]
    assert (idx[inf_rows | nan_rows] == G.NONE).all() and (idx != G.NONE).any()
    full = G.host(cases["w_zero_inf"])
    assert (full[0][nan_rows] == G.NONE).all() and (full[0][~nan_rows] != G.NONE).all()
    assert MC.same([o[inf_rows] for o in full], [o[inf_rows] for o in MC.host(d1, d2)])
    # the descriptor sets that catch padding and tie mistakes, every column admissible at r == T == 0
    idx, dist, idx2, dist2 = G.host(cases["padding"])
    assert (dist == dim * 255 * 255).all() and (dist2 == dim * 255 * 255).all() and (idx == 0).all() and (idx2 == 1).all()
    idx, dist, idx2, dist2 = G.host(cases["duplicates"])
    assert (dist == dist2).all() and (idx < idx2).all()
    assert MC.same(G.host(cases["duplicates"]), MC.host(*cases["duplicates"][:2]))


def test_skip_case_has_empty_and_full_tiles():
    """The layout the kernel's skip path needs: 32 x 32 tiles, whole 64-column
    steps and a whole workgroup's 128 rows without an admissible pair, beside
    tiles with some."""
    d1, d2, p1, p2, kind, h, T = G.crafted()["skip"]
    adm = G.admissible(kind, p1, p2, h, T)
    assert len(d1) == 300 and len(d2) == 200
    for lo, hi in G.SKIP_FAR_ROWS:
        assert not adm[lo:hi].any()
    for lo, hi in G.SKIP_FAR_COLS:
        assert not adm[:, lo:hi].any()
    assert not adm[128:256].any() and not adm[:, 0:64].any()             # a workgroup's rows, a step's columns
    tiles = [adm[r:r + 32, c:c + 32].any() for r in range(0, 300, 32) for c in range(0, 200, 32)]
    assert 10 <= sum(tiles) <= len(tiles) - 10
    assert adm[0:32, 64:96].any() and adm[0:32, 128:160].any() and adm[256:300, 192:200].any()


def test_threads_do_not_change_the_bytes():
    for kind in G.KINDS:
        case = G.lattice_case(1000, 257, 128, kind, 0)
        for reverse in (0, 1):
            one = G.host(case, reverse, 1)
            for threads in (3, 16, 0, -5, 1000):
                assert MC.same(G.host(case, reverse, threads), one), (kind, reverse, threads)
    small = G.lattice_case(2, 257, 128, G.H, 1)
    assert MC.same(G.host(small, 0, 16), G.host(small, 0, 1))            # more threads than rows


@pytest.mark.parametrize("kind", G.KINDS)
def test_reverse_is_forward_on_the_transposed_problem(kind):
    for share in (0, 1):
        case = G.lattice_case(129, 257, 128, kind, share)
        assert MC.same(G.host(case, 1), G.host(G.transposed(case), 0))
        assert MC.same(G.host(case, 0), G.host(G.transposed(case), 1))


# ------------------------------------------------------------- the front end --
def _tiny():
    """Three keypoints on a line in image 1, five in image 2; identity model.
    Admissible at 1.5 px: (0, 0), (0, 1), (1, 2), (2, 3); image-2 keypoint 4 is far."""
    p1 = np.array([[0.0, 0.0], [10.0, 0.0], [20.0, 0.0]])
    p2 = np.array([[0.0, 1.0], [1.0, 0.0], [10.0, 0.0], [20.0, 1.0], [500.0, 500.0]])
    d1 = np.zeros((3, 32), np.uint8)
    d2 = np.zeros((5, 32), np.uint8)
    d2[0, 0], d2[1, 0], d2[2, 0], d2[3, 0], d2[4, 0] = 3, 4, 9, 2, 0     # squared distances 9, 16, 81, 4, 0
    return d1, d2, p1, p2


def test_front_end_rules():
    d1, d2, p1, p2 = _tiny()
    kw = dict(model=np.eye(3), kind="homography", threshold=1.5, backend="host")
    m, r = F.match_descriptors_guided(d1, d2, p1, p2, mutual=False, **kw)
    assert m.dtype == np.int64 and r.dtype == np.float64
    assert np.array_equal(m, [[0, 0], [1, 2], [2, 3]])
    # sqrt(dist / dist2) among the ADMISSIBLE candidates; 1.0 where there is a single one
    assert np.array_equal(r, [np.sqrt(9.0 / 16.0), 1.0, 1.0])
    # the unguided nearest of every row is image-2 keypoint 4 (distance 0), which no row admits
    assert (F.match_descriptors(d1, d2, ratio=None, mutual=False, backend="host")[0][:, 1] == 4).all()
    # ratio: float(dist) < ratio^2 float(dist2) on the two admissible candidates; a single candidate passes
    m, r = F.match_descriptors_guided(d1, d2, p1, p2, ratio=0.8, mutual=False, **kw)
    assert np.array_equal(m, [[0, 0], [1, 2], [2, 3]])                   # 9 < 0.64 * 16 = 10.24
    m, r = F.match_descriptors_guided(d1, d2, p1, p2, ratio=0.75, mutual=False, **kw)
    assert np.array_equal(m, [[1, 2], [2, 3]]) and np.array_equal(r, [1.0, 1.0])     # 9 < 0.5625 * 16 = 9 fails
    # max_distance: dist <= max_distance
    m, _ = F.match_descriptors_guided(d1, d2, p1, p2, mutual=False, max_distance=9, **kw)
    assert np.array_equal(m, [[0, 0], [2, 3]])
    m, _ = F.match_descriptors_guided(d1, d2, p1, p2, mutual=False, max_distance=8.5, **kw)
    assert np.array_equal(m, [[2, 3]])
    m, r = F.match_descriptors_guided(d1, d2, p1, p2, mutual=False, max_distance=0, **kw)
    assert m.shape == (0, 2) and m.dtype == np.int64 and r.shape == (0,)
    # mutual: image-2 keypoint 1 also has image-1 keypoint 0 first, but 0's first is 0
    m, _ = F.match_descriptors_guided(d1, d2, p1, p2, mutual=True, **kw)
    assert np.array_equal(m, [[0, 0], [1, 2], [2, 3]])
    d1b = d1.copy()
    d1b[1, 0] = 3                                                         # keypoint 1 of image 1 now nearer to column 0 ...
    p1b = p1.copy()
    p1b[1] = [0.5, 0.5]                                                   # ... and admissible for columns 0 and 1 only
    m, _ = F.match_descriptors_guided(d1b, d2, p1b, p2, mutual=False, **kw)
    assert np.array_equal(m, [[0, 0], [1, 0], [2, 3]])
    m, _ = F.match_descriptors_guided(d1b, d2, p1b, p2, mutual=True, **kw)
    assert np.array_equal(m, [[1, 0], [2, 3]])                            # column 0's first is row 1 (distance 0)
    # keypoint rows (x, y, size, angle) and objects with .pt are read like (N, 2) positions
    k1 = np.column_stack([p1, np.full(3, 4.0), np.full(3, -1.0)])
    k2 = np.column_stack([p2, np.full(5, 4.0), np.full(5, 30.0)])

    class KP:
        def __init__(self, row):
            self.pt, self.size, self.angle = (row[0], row[1]), row[2], row[3]

    ref = F.match_descriptors_guided(d1, d2, p1, p2, **kw)
    for a, b in ((k1, k2), ([KP(x) for x in k1], [KP(x) for x in k2])):
        got = F.match_descriptors_guided(d1, d2, a, b, **kw)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # threshold is in pixels: the bound handed down is threshold^2 (r^2 == T admissible)
    m, _ = F.match_descriptors_guided(d1, d2, p1, p2, np.eye(3), "homography", 1.0, mutual=False, backend="host")
    assert np.array_equal(m, [[0, 0], [1, 2], [2, 3]])
    m, _ = F.match_descriptors_guided(d1, d2, p1, p2, np.eye(3), "homography", 0.999, mutual=False, backend="host")
    assert np.array_equal(m, [[1, 2]])


def test_front_end_equals_the_c_entry():
    case = G.generic_case(129, 257, 128, G.F)
    d1, d2, p1, p2, kind, h, T = case
    idx, dist, idx2, dist2 = G.host(case)
    back = G.host(case, 1)[0]
    m, r = F.match_descriptors_guided(d1, d2, p1, p2, h.reshape(3, 3), "fundamental", 3.0, mutual=False, backend="host")
    rows = np.nonzero(idx != G.NONE)[0]
    assert 0 < len(rows) < len(d1) and np.array_equal(m[:, 0], rows) and np.array_equal(m[:, 1], idx[rows])
    m, r = F.match_descriptors_guided(d1, d2, p1, p2, h.reshape(3, 3), "fundamental", 3.0, backend="host")
    keep = rows[back[idx[rows]] == rows]
    assert np.array_equal(m[:, 0], keep) and (np.diff(m[:, 0]) > 0).all()
    two = idx2[keep] != G.NONE
    assert two.any() and (~two).any()
    exp = np.ones(len(keep))
    exp[two] = np.sqrt(dist[keep][two].astype(np.float64) / dist2[keep][two].astype(np.float64))
    assert np.array_equal(r, exp)


def test_fundamental_from_essential():
    K1 = np.array([[800.0, 0.0, 640.0], [0.0, 810.0, 480.0], [0.0, 0.0, 1.0]])
    K2 = np.array([[700.0, 2.0, 600.0], [0.0, 705.0, 470.0], [0.0, 0.0, 1.0]])
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    E = G.skew((0.3, -0.2, 1.0)) @ R
    Fm = F.fundamental_from_essential(E, K1, K2)
    assert Fm.shape == (3, 3) and np.allclose(K2.T @ Fm @ K1, E, rtol=0, atol=1e-12)
    # a scene point seen by both cameras satisfies x2^T F x1 = 0 in pixels
    X = np.array([0.4, -0.3, 5.0])
    x1 = K1 @ X
    x2 = K2 @ (R @ X + np.array([0.3, -0.2, 1.0]))
    assert abs((x2 / x2[2]) @ Fm @ (x1 / x1[2])) < 1e-9
    with pytest.raises(ValueError):
        F.fundamental_from_essential(np.eye(4), K1, K2)


def test_python_errors():
    d1, d2, p1, p2 = _tiny()
    ok = dict(desc1=d1, desc2=d2, kp1=p1, kp2=p2, model=np.eye(3), kind="homography", threshold=1.5, backend="host")

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            F.match_descriptors_guided(**{**ok, **kw})

    bad("quantize_descriptors", desc1=d1.astype(np.float32))
    bad("dimension", desc2=np.zeros((5, 64), np.uint8))
    bad("multiple of 32", desc1=np.zeros((3, 48), np.uint8), desc2=np.zeros((5, 48), np.uint8))
    bad("at least one row", desc1=np.zeros((0, 32), np.uint8), kp1=np.zeros((0, 2)))
    bad("backend", backend="cpu")
    bad("kind", kind="essential")
    bad("kind", kind=3)
    bad("one keypoint per descriptor", kp1=p1[:2])
    bad("one keypoint per descriptor", kp2=np.zeros((4, 4)))
    bad("keypoint array", kp1=np.zeros((3, 3)))
    bad("non-finite", kp2=np.where(np.arange(10).reshape(5, 2) == 3, np.nan, p2))
    bad("3 x 3", model=np.eye(4))
    bad("3 x 3", model=np.full((3, 3), np.inf))
    for t in (0.0, -1.0, INF, float("nan")):
        bad("threshold", threshold=t)
    bad("ratio", ratio=-1.0)
    bad("max_distance", max_distance=-1)
    # the bad calls never reach a device: backend="gpu" fails the same way
    bad("kind", kind="essential", backend="gpu")
    bad("threshold", threshold=0.0, backend="gpu")


def test_c_entries_reject_bad_arguments():
    d = np.zeros((4, 64), np.uint8)
    pos = np.zeros((4, 2))
    model = np.eye(3).reshape(9).copy()
    out = [np.zeros(4, np.uint32) for _ in range(4)]
    ptrs = [o.ctypes.data for o in out]
    a, p, m = d.ctypes.data, pos.ctypes.data, model.ctypes.data
    good = dict(d1=a, n1=4, p1=p, d2=a, n2=4, p2=p, dim=64, kind=G.H, model=m, T=1.0, reverse=0)

    def call(ptrs=ptrs, **kw):
        g = {**good, **kw}
        args = (g["d1"], g["n1"], g["p1"], g["d2"], g["n2"], g["p2"], g["dim"], g["kind"], g["model"], g["T"],
                g["reverse"])
        # the device entry with a NULL context: the check runs before any GPU work
        return (N.lib.gcr_match_descriptors_guided(None, *args, *ptrs, None), N.last_error(),
                N.lib.gcr_host_match_descriptors_guided(*args, 1, *ptrs), N.last_error())

    def both(word, **kw):
        rc_d, err_d, rc_h, err_h = call(**kw)
        assert rc_d == N.GCR_EINVAL and word in err_d, (word, err_d)
        assert rc_h == N.GCR_EINVAL and word in err_h, (word, err_h)

    both("d1", d1=None)
    both("d2", d2=None)
    both("p1", p1=None)
    both("p2", p2=None)
    both("model", model=None)
    for k, name in enumerate(("idx_out", "dist_out", "idx2_out", "dist2_out")):
        both(name, ptrs=ptrs[:k] + [None] + ptrs[k + 1:])
    both("n1", n1=0)
    both("n2", n2=(1 << 24) + 1)
    for dim in (0, 16, 48, 544):
        both("dim", dim=dim)
    for kind in (-1, 0, 1, 2, 5, 6, 7, 8):
        both("kind", kind=kind)
    for T in (-1.0, -0.0 - 1e-300, float("nan"), -INF):
        both("sq_threshold", T=T)
    both("reverse", reverse=2)
    for v in (INF, -INF, float("nan")):
        for k in (0, 8):
            bad_model = model.copy()
            bad_model[k] = v
            both("model", model=bad_model.ctypes.data)
    # good arguments: T = 0 and T = +inf are allowed; without a context the device entry names the context
    for T in (0.0, 1.0, INF):
        rc_d, err_d, rc_h, _ = call(T=T)
        assert rc_d == N.GCR_EINVAL and "context" in err_d and rc_h == 0
    assert N.lib.gcr_abi_version() == 5


def test_signatures_and_exports():
    sig = inspect.signature(F.match_descriptors_guided).parameters
    assert list(sig) == ["desc1", "desc2", "kp1", "kp2", "model", "kind", "threshold", "ratio", "mutual", "max_distance",
                         "backend", "device"]
    assert sig["ratio"].default is None and sig["mutual"].default is True and sig["max_distance"].default is None
    assert sig["backend"].default == "gpu" and sig["backend"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["device"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(F.fundamental_from_essential).parameters) == ["E", "K1", "K2"]
    for n in ("match_descriptors_guided", "fundamental_from_essential"):
        assert n in F.__all__
    assert "2.25" in F.match_descriptors_guided.__doc__


# ------------------------------------------------- what guided matching finds --
@pytest.fixture(scope="module")
def noisy():
    """Descriptor noise at which the plain matcher loses most true pairs."""
    return S.problem_match(1000, 400, desc_noise=70.0)


def _truth_found(matches, pairs):
    truth = set(map(tuple, pairs.tolist()))
    got = set(map(tuple, matches.tolist()))
    return len(got & truth), len(got)


def test_guided_matching_recovers_the_truth_pairs(noisy):
    """Measured with this code (host twin), default seed: plain 63 of 400 truth
    pairs; H-guided 400 (401 returned); F-guided mutual 400 (654 returned);
    F-guided with ratio 0.8: 285 of 291 returned, precision 0.979."""
    kp1, d1, kp2, d2, pairs, H_gt = noisy
    plain, _ = F.match_descriptors(d1, d2, ratio=0.8, mutual=True, backend="host")
    plain_true, _ = _truth_found(plain, pairs)
    m, _ = F.match_descriptors_guided(d1, d2, kp1, kp2, H_gt, "homography", 3.0, backend="host")
    true, total = _truth_found(m, pairs)
    print(f"plain {plain_true}; H-guided {true} of {total}")
    assert true >= 380
    Fm = G.skew(G.E_GENERIC) @ H_gt
    m, _ = F.match_descriptors_guided(d1, d2, kp1, kp2, Fm, "fundamental", 3.0, backend="host")
    true, total = _truth_found(m, pairs)
    print(f"F-guided {true} of {total}")
    assert true >= 380
    m, _ = F.match_descriptors_guided(d1, d2, kp1, kp2, Fm, "fundamental", 3.0, ratio=0.8, backend="host")
    true, total = _truth_found(m, pairs)
    print(f"F-guided, ratio 0.8: {true} of {total}")
    assert true >= 3 * plain_true and true >= 0.9 * total


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/match_geo_host.cpp: the factorised evaluation against
    geo_sq_residual bit for bit, the definition in both directions and the
    crafted cases, a stand-alone host program built with ASan + UBSan."""
    exe = str(tmp_path / "match_geo_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "cpp", "match_geo_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout
