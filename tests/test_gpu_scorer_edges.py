"""Scorer conformance at feature-count edges, every path and kind (run on an
MI355X: pytest -m gpu).  The shapes, data, regimes and models are those of
scorer_edge_cases.py (test_scorer_edge_cases.py pins them on the CPU): class
sizes on, one below and one above every tiling constant of the scorers, 13
models tiled over ragged hypothesis counts, three threshold regimes (typical,
every pair an inlier, no pair an inlier).

Every comparison is bitwise against the oracle: inlier counts and the MSAC
sums v0, v1 and tot after getScore's finish.  There is no tolerance.  A test
loops over all shapes and regimes of its kind and reports every mismatch as
shape/regime/model, so a failure names the tiling that broke; its id names
the kernel variant.

The scorer behind GCR_SCORER is chosen once per process: the k_score_split<K,
16, 420> checks run in one child process (this file as a script).
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_ffi as O
import scorer_edge_cases as E
from gcr_testutil import CorrProblem, Problem, bits, dp, u8p, u32p
from pygcransac import _native as N

pytestmark = pytest.mark.gpu

THREADS = 16
SLOT0 = 7
NB = 11
ALL_KINDS = E.RECT_KINDS + E.CORR_KINDS
assert (N.SOLVER_SCALE3, N.SOLVER_SCALE3_ORIGINAL, N.SOLVER_SIFT22, N.SOLVER_HOMOGRAPHY4,
        N.SOLVER_FUNDAMENTAL7) == ALL_KINDS


def _kid(k):
    return E.KIND_NAME[k]


def _pid(path):
    # "k_score_split<K,4,960>" -> "k_score_split-K-4-960"
    return path[0].replace("<", "-").replace(">", "").replace(",", "-").replace("+", "-and-").replace("|", "-or-")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if N.lib.gcr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    N.context(0)
    O.lib()


def _open(kind, shape):
    f0, f1, _ = E.problem(kind, shape)
    return Problem(kind, f0, f1) if kind in E.RECT_KINDS else CorrProblem(kind, f0)


def _score(prob, kind, tiled, thr):
    """Raw accumulators (n0, n1, v0, v1, tot) of gcr_debug_score[_h]."""
    n = len(tiled)
    if kind in E.CORR_KINDS:
        n0, v0, tot = prob.score(tiled, thr[0])
        return n0, np.zeros(n, np.uint32), v0, np.zeros(n), tot
    a = np.ascontiguousarray(tiled, dtype=np.float64)
    ms = (N.RectModel * n).from_buffer_copy(a)
    p = N.default_params()
    p.scale_residual_thresh, p.orientation_residual_thresh = thr
    n0, n1 = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    v0, v1, tot = np.zeros(n), np.zeros(n), np.zeros(n)
    N.check(N.lib.gcr_debug_score(prob.h, C.byref(p), ms, n, n0.ctypes.data_as(u32p), n1.ctypes.data_as(u32p),
                                  dp(v0), dp(v1), dp(tot)))
    return n0, n1, v0, v1, tot


def _mismatches(kind, shape, regime, nh, raw):
    """Every hypothesis of a tiled launch against the oracle: hypothesis i
    carries model i mod 13, so its raw accumulators equal those of hypothesis
    i mod 13 bit for bit, and the first 13, finished, equal the oracle's."""
    tag = f"{E.shape_id(shape)}/{regime}"
    bad = []
    for name, a in zip(("n0", "n1", "v0", "v1", "tot"), raw):
        a = a if a.dtype == np.uint32 else bits(a)
        diff = np.flatnonzero(a != np.resize(a[:E.NMODELS], nh))
        if len(diff):
            bad.append(f"{tag}: {name} of hypothesis {int(diff[0])} (model {int(diff[0]) % E.NMODELS}) differs from "
                       f"hypothesis {int(diff[0]) % E.NMODELS}, {len(diff)} of {nh}")
    k = min(nh, E.NMODELS)
    counts, values, value = E.finish(kind, *[a[:k] for a in raw], E.thresholds(kind, shape, regime))
    rc, rv, rt, _ = E.reference(kind, shape, regime)
    for j in range(k):
        if counts[j].tolist() != rc[j].tolist():
            bad.append(f"{tag}: model {j} counts {counts[j].tolist()} != {rc[j].tolist()}")
        elif bits(value[j]) != bits(rt[j]) or (kind in E.RECT_KINDS and not np.array_equal(bits(values[j]),
                                                                                          bits(rv[j]))):
            bad.append(f"{tag}: model {j} value {float(value[j])!r} != {float(rt[j])!r} (counts {rc[j].tolist()})")
    return bad


def _sweep(kind, nh, shapes=None):
    """gcr_debug_score[_h] of every shape x regime at nh hypotheses: (cases, mismatches)."""
    bad, cases = [], 0
    for shape in shapes or E.shapes(kind):
        prob = _open(kind, shape)
        try:
            tiled = E.tile(kind, shape, nh)
            for regime in E.REGIMES:
                raw = _score(prob, kind, tiled, E.thresholds(kind, shape, regime))
                bad += _mismatches(kind, shape, regime, nh, raw)
                cases += 1
        finally:
            prob.close()
    return cases, bad


def _report(cases, bad, want):
    assert cases == want
    assert not bad, f"{len(bad)} mismatches, first: " + "; ".join(bad[:8])


# ------------------------------------------------------------ child process --
def _child_main():
    # GCR_SCORER=split in the environment: nh = 2061 runs k_score_split<K, 16, 420>
    N.context(0)
    out = {}
    for kind in ALL_KINDS:
        cases, bad = _sweep(kind, E.NH[16])
        out[str(kind)] = [cases, bad]
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    _child_main()
    sys.exit(0)


@pytest.fixture(scope="module")
def split16():
    env = dict(os.environ)
    env["GCR_SCORER"] = "split"
    env["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p] + [env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout)


# ------------------------------------------------- per-hypothesis matrix ----
# (id, hypotheses, environment): the kernel launch_score picks for the rectification kinds
RECT_PATHS = [
    ("k_score_split<K,4,960>", E.NH[4], {}),
    ("k_score_fm<K,16,false>", E.NH[16], {}),
    ("k_score_split<K,64,120>", E.NH[64], {}),
    ("k_lo_resid+k_lo_fold", E.NMODELS, {"GCR_DEBUG_SCORER": "small"}),
    ("k_lo_chain<K,true>", E.NMODELS, {"GCR_DEBUG_SCORER": "small", "GCR_LO_SPLIT": "0"}),
    ("k_lo_chain<K,false>", E.NMODELS, {"GCR_DEBUG_SCORER": "small", "GCR_LO_FOLD": "seq"}),
]
# ... launch_score_geo and launch_score_small pick for the correspondence kinds
CORR_PATHS = [
    ("k_score_split<K,4,960>", E.NH[4], {}),
    ("k_score_fm<K,16,false>", E.NH[16], {}),
    ("k_score_fm<K,16,false>,16387", E.NH[64], {}),
    ("k_score_split<K,64,120>", E.NH[64], {"GCR_GEO_FM_LARGE": "0"}),
    ("k_lo_chain<K,true>", E.NMODELS, {"GCR_DEBUG_SCORER": "small"}),
]


@pytest.mark.parametrize("path", RECT_PATHS, ids=_pid)
@pytest.mark.parametrize("kind", E.RECT_KINDS, ids=_kid)
def test_rect_scorer_at_edges(kind, path, monkeypatch):
    """gcr_debug_score: every shape x regime through the kernel of the id."""
    _, nh, env = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases, bad = _sweep(kind, nh)
    _report(cases, bad, 3 * len(E.shapes(kind)))


@pytest.mark.parametrize("path", CORR_PATHS, ids=_pid)
@pytest.mark.parametrize("kind", E.CORR_KINDS, ids=_kid)
def test_corr_scorer_at_edges(kind, path, monkeypatch):
    """gcr_debug_score_h: every shape x regime through the kernel of the id."""
    _, nh, env = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases, bad = _sweep(kind, nh)
    _report(cases, bad, 3 * len(E.shapes(kind)))


@pytest.mark.parametrize("kind", ALL_KINDS, ids=_kid)
def test_split16_scorer_at_edges(kind, split16):
    """k_score_split<K,16,420>: nh = 2061 with GCR_SCORER=split (child process)."""
    cases, bad = split16[str(kind)]
    _report(cases, bad, 3 * len(E.shapes(kind)))


@pytest.mark.parametrize("path", [("k_lo_resid+k_lo_fold|k_lo_chain<K,true>", {}),
                                  ("k_lo_chain<K,true>", {"GCR_LO_SPLIT": "0"})], ids=_pid)
@pytest.mark.parametrize("kind", (0, 2), ids=_kid)
def test_small_scorer_limits(kind, path, monkeypatch):
    """The small scorer at its limits: padded pair totals of 16384 (the split
    scorer, k_lo_resid + k_lo_fold, holds every value in LDS) and above (one
    k_lo_chain workgroup per model, blocks of kLoBlock = 8192 features), and
    class sizes around one block.  13 models, typical and full."""
    monkeypatch.setenv("GCR_DEBUG_SCORER", "small")
    for k, v in path[1].items():
        monkeypatch.setenv(k, v)
    bad = []
    for shape in E.small_limit_shapes(kind):
        prob = _open(kind, shape)
        try:
            for regime in ("typical", "full"):
                raw = _score(prob, kind, E.models(kind, shape), E.thresholds(kind, shape, regime))
                bad += _mismatches(kind, shape, regime, E.NMODELS, raw)
        finally:
            prob.close()
    assert not bad, f"{len(bad)} mismatches, first: " + "; ".join(bad[:8])


# ----------------------------------------------------- masks and residuals --
def _rule2(r2, T, lam):
    # exact.h mask_rule, rule 2: the 1-class labeling of an empty neighbourhood graph
    with np.errstate(all="ignore"):
        q = np.clip(r2 / T, 0.0, 1.0)
        energy = 1.0 - q
        oml = 1.0 - lam
        tr = np.where(r2 <= T, 0.0 - oml * energy, oml * (1.0 - energy) - 0.0)
    return tr < 0.0


@pytest.mark.parametrize("kind", ALL_KINDS, ids=_kid)
def test_masks_at_block_edges(kind):
    """k_mask (gcr_debug_mask[_h]), blocks of kMaskBlock = 256 features: rule
    0 against the oracle's MSAC masks, rules 1 and 2 against its residuals."""
    lam = 0.3
    bad = []
    for shape in E.mask_shapes(kind):
        f0, f1, _ = E.problem(kind, shape)
        prob = _open(kind, shape)
        try:
            for regime in E.REGIMES:
                thr = E.thresholds(kind, shape, regime)
                masks = E.reference(kind, shape, regime)[3]
                for j, m in enumerate(E.models(kind, shape)):
                    for c, f in enumerate((f0, f1)[:len(E.SAMPLE[kind])]):
                        if kind in E.RECT_KINDS:
                            r2 = O.residuals(kind, c, f, m)
                            got = [prob.mask(m, c, rule, thr[0], thr[1], lam) for rule in (0, 1, 2)]
                        else:
                            r2 = (O.h_residuals if kind == 3 else O.f_residuals)(f, m)
                            got = [prob.mask(m, rule, thr[0], lam) for rule in (0, 1, 2)]
                        T = E.lo_T(thr[c])
                        with np.errstate(invalid="ignore"):
                            want = [masks[j][c], r2 <= T, _rule2(r2, T, lam)]
                        for rule in (0, 1, 2):
                            if not np.array_equal(got[rule], want[rule]):
                                i = int(np.flatnonzero(got[rule] != want[rule])[0])
                                bad.append(f"{E.shape_id(shape)}/{regime}: model {j} class {c} rule {rule} feature {i}")
        finally:
            prob.close()
    assert not bad, f"{len(bad)} mismatches, first: " + "; ".join(bad[:8])


# ------------------------------------------------- fused launch, per slot ----
def _replay_count(kind, shape):
    return NB * 3000 if shape in E.chained_shapes(kind) else E.NH[64]


@functools.lru_cache(maxsize=None)
def _rect_replay(kind, shape):
    """The oracle's slots SLOT0 ... of the shape (sampler seed E.SEED), scored
    in every regime: inc (n,), models (n, 7), and per regime counts (n, 2),
    values (n, 2), value (n,) -- zeros for a slot without a model.  Shared by
    the per-slot and the per-batch tests."""
    n = _replay_count(kind, shape)
    f0, f1, _ = E.problem(kind, shape)
    thr = [E.thresholds(kind, shape, r) for r in E.REGIMES]
    step = (n + 4 * THREADS - 1) // (4 * THREADS)

    def work(lo):
        return O.slots_scored(kind, f0, f1, E.SEED, SLOT0 + lo, min(step, n - lo), thr)

    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(work, range(0, n, step)))
    inc, models = (np.concatenate([p[q] for p in parts]) for q in (0, 1))
    counts, values, value = (np.concatenate([p[q] for p in parts], axis=1) for q in (2, 3, 4))
    return inc.astype(np.int64), models, counts.astype(np.int64), values, value


def _verify_slots(prob, thr, nslots):
    p = N.default_params()
    p.scale_residual_thresh, p.orientation_residual_thresh, p.seed = thr[0], thr[1], E.SEED
    inc = np.zeros(nslots, np.uint8)
    n0, n1 = np.zeros(nslots, np.uint32), np.zeros(nslots, np.uint32)
    v0, v1, tot = np.zeros(nslots), np.zeros(nslots), np.zeros(nslots)
    N.check(N.lib.gcr_debug_verify_slots(prob.h, C.byref(p), SLOT0, nslots, inc.ctypes.data_as(u8p),
                                         n0.ctypes.data_as(u32p), n1.ctypes.data_as(u32p), dp(v0), dp(v1), dp(tot)))
    return inc, (n0, n1, v0, v1, tot)


FUSED = [("k_score_split<K,4,960,true>", E.NH[4]), ("k_score_fm<K,16,true>", E.NH[16]),
         ("k_score_split<K,64,120,true>", E.NH[64])]


@pytest.mark.parametrize("path", FUSED, ids=_pid)
@pytest.mark.parametrize("kind", E.RECT_KINDS, ids=_kid)
def test_fused_launch_every_slot(kind, path):
    """gcr_debug_verify_slots: the fused generate + score launch of a
    one-batch gcr_problem_verify_batches call (at 2061 slots the bench's
    kernel, rounds of 896 features), every slot's attempt count and finished
    score against O.slot + O.score -- the batch record shows one slot only."""
    nslots = path[1]
    bad = []
    for shape in E.fused_shapes(kind):
        oinc, _, ocnt, ovals, oval = _rect_replay(kind, shape)
        assert (oinc[:nslots] <= 101).any()
        prob = _open(kind, shape)
        try:
            for r, regime in enumerate(E.REGIMES):
                thr = E.thresholds(kind, shape, regime)
                inc, raw = _verify_slots(prob, thr, nslots)
                tag = f"{E.shape_id(shape)}/{regime}"
                d = np.flatnonzero(inc != oinc[:nslots])
                if len(d):
                    bad.append(f"{tag}: inc of slot {int(d[0])}: {int(inc[d[0]])} != {int(oinc[d[0]])}, {len(d)} slots")
                    continue
                counts, values, value = E.finish(kind, *raw, thr)
                d = np.flatnonzero((counts != ocnt[r, :nslots]).any(axis=1) | (bits(value) != bits(oval[r, :nslots])) |
                                   (bits(values) != bits(ovals[r, :nslots])).any(axis=1))
                if len(d):
                    i = int(d[0])
                    bad.append(f"{tag}: slot {i} (position {i % 16} of 16, {i % 64} of 64) counts "
                               f"{counts[i].tolist()} value {float(value[i])!r} != {ocnt[r, i].tolist()} "
                               f"{float(oval[r, i])!r}, {len(d)} of {nslots} slots")
        finally:
            prob.close()
    assert not bad, f"{len(bad)} mismatches, first: " + "; ".join(bad[:8])


# ------------------------------------- fused launch, chained and grouped ----
def _records(prob, thr, nslots):
    p = N.default_params()
    p.scale_residual_thresh, p.orientation_residual_thresh, p.seed = thr[0], thr[1], E.SEED
    res = (N.BatchResult * NB)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, NB, res, None))
    return res


@pytest.mark.parametrize("nslots", [2048, 3000])
@pytest.mark.parametrize("kind", E.RECT_KINDS, ids=_kid)
def test_chained_grouped_batches_match_oracle_replay(kind, nslots):
    """gcr_problem_verify_batches, 11 batches, default knobs: k_score_fm<K,
    16, true> chained across launches and several batches a launch (3000
    slots: a partial last workgroup).  Every record against the oracle's
    replay of its slots: `best < score && isValidModel` in slot order."""
    bad = []
    for shape in E.chained_shapes(kind):
        oinc, omodels, ocnt, _, oval = _rect_replay(kind, shape)
        prob = _open(kind, shape)
        try:
            for regime in ("typical", "full"):
                r = E.REGIMES.index(regime)
                res = _records(prob, E.thresholds(kind, shape, regime), nslots)
                for b in range(NB):
                    lo = b * nslots
                    best, bj = 0.0, -1
                    for j in range(lo, lo + nslots):
                        if oinc[j] > 101 or not best < oval[r, j]:
                            continue
                        if kind == 2 and not max(abs(omodels[j, 3]), abs(omodels[j, 4])) < 1e-3:   # two_sift.hpp:45-61
                            continue
                        best, bj = oval[r, j], j
                    want = [int((oinc[lo:lo + nslots] <= 101).sum()), int(oinc[lo:lo + nslots].sum()),
                            SLOT0 + bj if bj >= 0 else -1, int(bits(best))]
                    rec = res[b]
                    got = [rec.models, rec.iterations, rec.best_slot, int(bits(rec.best_score))]
                    if bj >= 0:
                        want += ocnt[r, bj].tolist() + bits(omodels[bj]).tolist()
                        m = rec.best_model
                        got += [rec.best_inliers[0], rec.best_inliers[1]] + bits(
                            [m.x0, m.y0, m.s, m.h7, m.h8, m.alpha, m.phi]).tolist()
                    if got != want:
                        bad.append(f"{E.shape_id(shape)}/{regime}: batch {b}: {got[:6]} != {want[:6]}")
                assert any(res[b].best_slot >= 0 for b in range(NB)), (shape, regime)
        finally:
            prob.close()
    assert not bad, f"{len(bad)} mismatches, first: " + "; ".join(bad[:8])


@functools.lru_cache(maxsize=None)
def _corr_replay(kind, shape, nslots):
    """Per batch and regime (typical, full) of the oracle's slots: models,
    iterations, first strict best (slot, value, count)."""
    corr = E.problem(kind, shape)[0]
    thr = [E.thresholds(kind, shape, r)[0] for r in ("typical", "full")]
    L = O.lib()
    dpt = C.POINTER(C.c_double)
    pc, n = corr.ctypes.data_as(dpt), corr.shape[0]

    def work(b):
        buf = np.zeros((3, 9))
        pm = [buf[q].ctypes.data_as(dpt) for q in range(3)]
        k, cnt, val = C.c_int(), C.c_uint64(), C.c_double()
        models = iters = 0
        best = [[0.0, -1, 0], [0.0, -1, 0]]
        for s in range(SLOT0 + b * nslots, SLOT0 + (b + 1) * nslots):
            if kind == 3:
                inc = L.oracle_h_slot(pc, n, E.SEED, s, pm[0])
                nm = 1 if inc <= 101 else 0
            else:
                inc = L.oracle_f_slot(pc, n, E.SEED, s, pm[0], C.byref(k))
                nm = k.value
            iters += inc
            models += nm
            for q in range(nm):
                for r in range(2):
                    (L.oracle_h_score if kind == 3 else L.oracle_f_score)(pc, n, pm[q], thr[r], C.byref(cnt),
                                                                          C.byref(val), None)
                    if best[r][0] < val.value:
                        best[r] = [val.value, s, cnt.value]
        return models, iters, best

    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(work, range(NB)))


@pytest.mark.parametrize("kind", E.CORR_KINDS, ids=_kid)
def test_correspondence_batches_match_oracle_replay(kind):
    """gcr_problem_verify_batches of the homography and the fundamental
    matrix, 11 batches of 2048 slots through the two-stream pipeline
    (k_generate / k_generate_fw + k_compact + k_score_fm<K, 16, false>)."""
    nslots = 2048
    bad = []
    for shape in E.chained_shapes(kind):
        ref = _corr_replay(kind, shape, nslots)
        prob = _open(kind, shape)
        try:
            for r, regime in enumerate(("typical", "full")):
                res = _records(prob, E.thresholds(kind, shape, regime), nslots)
                for b in range(NB):
                    models, iters, best = ref[b]
                    value, slot, count = best[r]
                    rec = res[b]
                    got = [rec.models, rec.iterations, rec.best_slot, int(bits(rec.best_score))]
                    want = [models, iters, slot, int(bits(value))]
                    if slot >= 0:
                        got.append(rec.best_inliers[0])
                        want.append(count)
                    if got != want:
                        bad.append(f"{E.shape_id(shape)}/{regime}: batch {b}: {got} != {want}")
                assert any(res[b].best_slot >= 0 for b in range(NB)), (shape, regime)
        finally:
            prob.close()
    assert not bad, f"{len(bad)} mismatches, first: " + "; ".join(bad[:8])
