"""verify_many, host side: csrc/verify_many.h's twin (gcr_host_verify_many)
against an independent numpy restatement field for field, the degenerate
problem, every argument error through both C entries, the masks, the Python
entry points (pygcransac.verify_many, features.verify_pairs) and the twin as a
stand-alone program under ASan + UBSan.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pygcransac
import verify_many_cases as VC
from pygcransac import _native as N
from pygcransac import features as F
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
SLOTS = 70


@pytest.mark.parametrize("solver,n", [(VC.H4, 4), (VC.H4, 5), (VC.H4, 64), (VC.F7, 7), (VC.F7, 8), (VC.F7, 30)])
def test_twin_equals_restatement(solver, n):
    rows, thr = (VC.rows_h(n), 2.0) if solver == VC.H4 else (VC.golden_f(30)[0][:n], VC.golden_f(30)[1])
    seed = 11 + n
    rec, masks = VC.run(solver, [rows], thr, seed, SLOTS, host=True)
    exp, emask = VC.restate(solver, rows, thr, seed, SLOTS)
    assert VC.record_equals(rec[0], exp), (rec[0], exp)
    assert np.array_equal(masks[0], emask)
    assert int(masks[0].sum()) == int(rec[0]["best_inliers"])
    if n >= 30:
        assert rec[0]["best_slot"] >= 0 and rec[0]["models"] > 0        # the case is not a vacuous one


def test_fundamental_slots_with_two_and_three_models():
    rows, thr = VC.golden_f(30)
    rec, _ = VC.run(VC.F7, [rows], thr, 5, SLOTS, host=True)
    exp, _ = VC.restate(VC.F7, rows, thr, 5, SLOTS)
    assert VC.record_equals(rec[0], exp)
    assert rec[0]["models"] > SLOTS                                      # some slot gave more than one model


@pytest.mark.parametrize("solver", [VC.H4, VC.F7])
def test_all_one_point(solver):
    """no sample of identical rows yields a model: every slot spends its 101
    attempts (inc 102), nothing is scored, the mask is zero"""
    rows = VC.one_point(12)
    rec, masks = VC.run(solver, [rows], 1.0, 3, SLOTS, host=True)
    r = rec[0]
    assert r["models"] == 0 and r["iterations"] == 102 * SLOTS and r["best_slot"] == -1
    assert r["best_inliers"] == 0 and r["best_score"] == 0.0 and r["best_hypothesis"] == 0
    assert np.array_equal(r["best_model"], VC.DEFAULT_MODEL)
    assert not masks[0].any()
    exp, _ = VC.restate(solver, rows, 1.0, 3, 3)
    assert exp["iterations"] == 102 * 3 and exp["best_slot"] == -1


def test_degenerate_neighbours_do_not_move_the_others():
    probs = [VC.rows_h(40), VC.one_point(9), VC.rows_h(4), VC.rows_h(33, seed=4)]
    whole = VC.run(VC.H4, probs, [2.0, 1.0, 2.0, 1.5], [1, 2, 3, 4], SLOTS, host=True)
    for p, (thr, seed) in enumerate(zip([2.0, 1.0, 2.0, 1.5], [1, 2, 3, 4])):
        alone = VC.run(VC.H4, [probs[p]], thr, seed, SLOTS, host=True)
        assert whole[0][p].tobytes() == alone[0][0].tobytes() and np.array_equal(whole[1][p], alone[1][0])


def test_threads_do_not_change_the_bytes():
    probs = [VC.rows_h(20 + 3 * k, seed=k) for k in range(9)]
    a = VC.run(VC.H4, probs, 2.0, np.arange(9), 40, host=True, threads=1)
    for t in (2, 16, 99):
        assert VC.same(a, VC.run(VC.H4, probs, 2.0, np.arange(9), 40, host=True, threads=t))


def test_seeds_and_thresholds_are_per_problem():
    r = VC.rows_h(64)
    rec, _ = VC.run(VC.H4, [r, r, r, r], [2.0, 2.0, 2.0, 0.5], [7, 8, 7, 7], SLOTS, host=True)
    assert rec[0].tobytes() == rec[2].tobytes()
    assert rec[0].tobytes() != rec[1].tobytes() and rec[0].tobytes() != rec[3].tobytes()


# ---------------------------------------------------------------- errors --
def _both(solver, rows, off, P, thr, seeds, slots, out="ok"):
    """the return codes of the device entry (NULL context: the checks come
    before the GPU) and the host entry, and the device entry's message"""
    res = (N.ManyResult * max(P, 1))()
    outp = res if out == "ok" else None
    ptr = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    rd = N.lib.gcr_verify_many(None, solver, ptr(rows), ptr(off), P, ptr(thr), ptr(seeds), slots, outp, None, None)
    msg = N.last_error()
    rh = N.lib.gcr_host_verify_many(solver, ptr(rows), ptr(off), P, ptr(thr), ptr(seeds), slots, 2, outp, None)
    return rd, rh, msg


def test_c_entries_reject_bad_arguments():
    rows, off = VC.pack([VC.rows_h(6), VC.rows_h(5)])
    thr, seeds = np.array([1.0, 2.0]), np.array([1, 2], dtype=np.uint64)

    def bad(word, **kw):
        a = dict(solver=VC.H4, rows=rows, off=off, P=2, thr=thr, seeds=seeds, slots=8)
        a.update(kw)
        rd, rh, msg = _both(**a)
        assert rd == N.GCR_EINVAL and rh == N.GCR_EINVAL, (word, rd, rh)
        assert word in msg, (word, msg)

    for solver in (0, 1, 2, 5, 6, 7, 8, -1):
        bad("solver", solver=solver)
    bad("nproblems", P=0)
    bad("row_offset", off=np.array([0, 6, 5], dtype=np.uint64))               # descending
    bad("row_offset", off=np.array([1, 6, 11], dtype=np.uint64))              # does not start at 0
    bad("fewer than", off=np.array([0, 3, 11], dtype=np.uint64))              # 3 rows < 4
    bad("fewer than", solver=VC.F7, off=np.array([0, 6, 11], dtype=np.uint64))    # 6 rows < 7
    for v in (np.nan, np.inf, -np.inf):
        r = rows.copy()
        r[7, 2] = v
        bad("row 1 of problem 1", rows=r)
    for v in (0.0, -1.0, np.nan, np.inf):
        bad("thresholds[1]", thr=np.array([1.0, v]))
    bad("nslots", slots=0)
    bad("nslots", slots=65537)
    for name in ("rows", "off", "thr", "seeds"):
        bad("NULL", **{name: None})
    bad("NULL", out=None)
    # good arguments reach the context check through the device entry, and run through the host entry
    rd, rh, msg = _both(VC.H4, rows, off, 2, thr, seeds, 8)
    assert rd == N.GCR_EINVAL and "context" in msg and rh == 0


def test_python_errors():
    r = VC.rows_h(10)
    with pytest.raises(ValueError):
        pygcransac.verify_many([r], "essential", 1.0, backend="host")
    with pytest.raises(ValueError):
        pygcransac.verify_many([r], "homography", 1.0, backend="cpu")
    with pytest.raises(ValueError):
        pygcransac.verify_many([r[:, :3]], "homography", 1.0, backend="host")
    with pytest.raises(ValueError):
        pygcransac.verify_many([r[:3]], "homography", 1.0, backend="host")
    with pytest.raises(ValueError):
        pygcransac.verify_many([r], "fundamental", 1.0, backend="host", iterations=0)
    with pytest.raises(ValueError):
        pygcransac.verify_many([r, r], "homography", [1.0, 2.0, 3.0], backend="host")
    with pytest.raises(ValueError):
        pygcransac.verify_many([r], "homography", -1.0, backend="host")
    assert pygcransac.verify_many([], "homography", 1.0, backend="host") == []
    assert "verify_many" in pygcransac.__all__ and "verify_pairs" in F.__all__


# ---------------------------------------------------------------- Python --
@pytest.mark.parametrize("kind,solver", [("homography", VC.H4), ("fundamental", VC.F7)])
def test_masks_are_the_models_inliers(kind, solver):
    if solver == VC.H4:
        probs, thr = [VC.rows_h(n, seed=n) for n in (4, 17, 64, 200)] + [VC.one_point(8)], [2.0, 2.0, 1.0, 2.0, 1.0]
    else:
        probs, thr = [VC.golden_f(30)[0], VC.rows_f(120), VC.rows_f(7), VC.one_point(9)], [0.75, 1.0, 1.0, 1.0]
    recs = pygcransac.verify_many(probs, kind, thr, 50, seed=9, backend="host", refine=True)
    assert len(recs) == len(probs)
    seen = 0
    for rows, t, r in zip(probs, thr, recs):
        assert r["mask"].dtype == bool and r["mask"].shape == (len(rows),)
        assert int(r["mask"].sum()) == r["inliers"]
        if r["model"] is None:
            assert r["slot"] == -1 and not r["mask"].any() and r["refined"] is None and r["score"] == 0.0
            continue
        seen += 1
        with np.errstate(all="ignore"):
            r2 = VC.sq_residual(solver, rows, r["model"].reshape(9))
        assert np.array_equal(r["mask"], r2 <= (2.25 * t) * t)
        assert r["inliers"] >= VC.M_OF[solver] and r["score"] > 0 and 0 <= r["slot"] < 50
        assert r["iterations"] >= 50
        if r["refined"] is not None:
            assert r["refined"].shape == (3, 3) and np.isfinite(r["refined"]).all()
    assert seen >= 2


def test_refine_fits_the_masks_rows():
    rows, truth, Hgt, thr = S.problem_h(150, 0.3, seed=21)
    (r,) = pygcransac.verify_many([rows], "homography", thr, 200, seed=1, backend="host", refine=True)
    assert r["inliers"] >= 0.8 * truth.sum() and r["refined"] is not None
    idx = np.ascontiguousarray(np.flatnonzero(r["mask"]), dtype=np.uint32)
    M = np.zeros(9)
    assert N.lib.gcr_host_fit_h(rows.ctypes.data_as(C.POINTER(C.c_double)), len(rows),
                                idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(idx),
                                M.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert np.array_equal(r["refined"], M.reshape(3, 3))
    assert np.abs(r["refined"] / r["refined"][2, 2] - Hgt / Hgt[2, 2]).max() < 0.05 * np.abs(Hgt).max()


def test_verify_pairs_is_the_three_steps():
    kp1, d1, kp2, d2, _, _ = S.problem_match(300, 120)
    sets = [(d1, kp1), (d2, kp2), (d2[::-1].copy(), kp2[::-1].copy())]
    pairs = [(0, 1), (0, 2), (1, 0)]
    thr, seeds = [2.0, 3.0, 2.0], [5, 6, 7]
    got = F.verify_pairs(sets, pairs, "homography", thr, ratio=0.8, mutual=True, iterations=64, seed=seeds,
                         refine=True, backend="host")
    assert len(got) == 3
    rows = []
    for (ia, ib), (m, ra, _) in zip(pairs, got):
        em, er = F.match_descriptors(sets[ia][0], sets[ib][0], 0.8, True, backend="host")
        assert np.array_equal(m, em) and np.array_equal(ra, er) and len(m) >= 50
        rows.append(F.correspondences_from_matches(sets[ia][1], sets[ib][1], em))
    exp = pygcransac.verify_many(rows, "homography", thr, 64, seed=seeds, backend="host", refine=True)
    for (_, _, rec), e in zip(got, exp):
        assert rec.keys() == e.keys()
        for k in rec:
            if isinstance(e[k], np.ndarray):
                assert np.array_equal(rec[k], e[k]) and rec[k].dtype == e[k].dtype, k
            else:
                assert rec[k] == e[k], k
        assert rec["model"] is not None and rec["inliers"] >= 40


def test_verify_pairs_skips_pairs_with_too_few_matches():
    rng = np.random.default_rng(2)
    kp = np.column_stack([rng.uniform(0, 900, (40, 2)), np.full(40, 3.0), np.zeros(40)])
    da, db = (rng.integers(0, 256, (40, 128), dtype=np.uint8) for _ in range(2))
    kp1, d1, kp2, d2, _, _ = S.problem_match(200, 100)
    got = F.verify_pairs([(da, kp), (db, kp), (d1, kp1), (d2, kp2)], [(0, 1), (2, 3)], "fundamental", 1.0, ratio=0.5,
                         iterations=32, seed=1, refine=True, backend="host")
    m, _, rec = got[0]
    assert len(m) < 7 and rec["model"] is None and rec["slot"] == -1 and rec["mask"].shape == (len(m),)
    assert rec["refined"] is None and rec["iterations"] == 0
    assert got[1][2]["model"] is not None
    with pytest.raises(ValueError):
        F.verify_pairs([(da, None), (db, kp)], [(0, 1)], "homography", 1.0, backend="host")
    with pytest.raises(ValueError):
        F.verify_pairs([(da, kp), (db, kp)], [(0, 2)], "homography", 1.0, backend="host")


# ------------------------------------------------------------- sanitizers --
def _sanitizer_toolchain(tmp_path):
    if shutil.which("g++") is None:
        return False
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")],
                       capture_output=True)
    return r.returncode == 0


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/verify_many_host.cpp: the twin on a few hundred random
    problems, the degenerate ones included, each problem of a packed call
    against the same problem alone, problems of minimal length at both ends of
    the buffer, and the merge rule in every order; a stand-alone host program
    built with ASan + UBSan"""
    if not _sanitizer_toolchain(tmp_path):
        pytest.skip("the toolchain lacks the sanitizer runtime")
    exe = str(tmp_path / "verify_many_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "verify_many_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout
