"""The value ring of the feature-major rectification scorers (k_score_fm,
KIND <= 2; csrc/fm_groups.h): a compute wave's survivor values go to
variable-size blocks of one ring, and the wave runs several rounds ahead of the
chain wave's fold (run on an MI355X: pytest -m gpu).

gcr_problem_verify_batches with GCR_VERIFY_GROUPS = 1 and 8 and with unchained
launches (GCR_VERIFY_CHAIN=0) must return the records of the same call with
GCR_SCORER=split (k_score_split: its own layout, no ring), field by field:
models, iterations, best slot, score bits, both inlier counts, model bits.
The scorer is chosen once per process, so the reference records of every case
come from one child process.

Shapes (seed 20251121).  A round is 14 waves x 64 = 896 features of one class:
  typical     M2 (1000, 900), 50 % outliers: blocks of a third of the ring,
              run-ahead over several rounds
  full        M2 (1000, 900), no outliers, thresholds (8.0, 0.75): nearly every
              wave-round needs more than half of the ring and many all of it
              (checked below from oracle residuals), so blocks start at 0, the
              tail is skipped and a wave waits for the fold of the round before
  empty       M2 (1000, 900), thresholds (1e-7, 1e-9): rounds without a block;
              the depth of the run-length rows limits the run-ahead
  two_rounds  M2 (300, 200): two rounds a batch, run-ahead across batches
  m1, m1orig  1000 features: one class
Slots: 2048 and 3000 (a partial last workgroup).  Batches: 11.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SEED = 20251121
SLOT0 = 7
THREADS = 16
NB = 11
SLOTS = (2048, 3000)

# shape: (solver name, scale features, orientation features, outlier ratio, thresholds or None)
SHAPES = {
    "typical": ("SOLVER_SIFT22", 1000, 900, 0.5, None),
    "full": ("SOLVER_SIFT22", 1000, 900, 0.0, (8.0, 0.75)),
    "empty": ("SOLVER_SIFT22", 1000, 900, 0.5, (1e-7, 1e-9)),
    "two_rounds": ("SOLVER_SIFT22", 300, 200, 0.5, None),
    "m1": ("SOLVER_SCALE3", 1000, 0, 0.5, None),
    "m1orig": ("SOLVER_SCALE3_ORIGINAL", 1000, 0, 0.5, None),
}
# (GCR_VERIFY_GROUPS, GCR_VERIFY_CHAIN)
RUNS = [("1", "1"), ("8", "1"), ("1", "0")]


@functools.lru_cache(maxsize=None)
def _problem(shape):
    from gcr_testutil import Problem
    from pygcransac import _native as N
    from pygcransac import synthetic as S

    solver, ns, no, outl, thr = SHAPES[shape]
    kind = getattr(N, solver)
    if kind == N.SOLVER_SIFT22:
        fs, fo, _, _, ts, to = S.problem_m2(ns, no, outlier_ratio=outl, seed=SEED)
        t0, t1 = thr if thr else (ts, to)
        return kind, Problem(kind, fs, fo), t0, t1
    f, _, t = S.problem_m1(ns, outlier_ratio=outl, seed=SEED)
    return kind, Problem(kind, f, None), t, 0.0


def _records(prob, thr0, thr1, nslots, nb):
    from pygcransac import _native as N

    p = N.default_params()
    p.scale_residual_thresh, p.orientation_residual_thresh, p.seed = thr0, thr1, SEED
    res = (N.BatchResult * nb)()
    N.check(N.lib.gcr_problem_verify_batches(prob.h, C.byref(p), SLOT0, nslots, nb, res, None))
    return res


def _fields(res):
    from gcr_testutil import bits

    return [[r.models, r.iterations, r.best_slot, int(bits(r.best_score).item()), r.best_inliers[0], r.best_inliers[1],
             [int(v) for v in bits([r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7,
                                    r.best_model.h8, r.best_model.alpha, r.best_model.phi]).tolist()]] for r in res]


def _reference_main():
    # child process (GCR_SCORER=split in its environment): every case's records
    out = {}
    for shape in SHAPES:
        _, prob, thr0, thr1 = _problem(shape)
        for nslots in SLOTS:
            out[f"{shape}/{nslots}"] = _fields(_records(prob, thr0, thr1, nslots, NB))
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    _reference_main()
    sys.exit(0)

import pytest  # noqa: E402

import oracle_ffi as O  # noqa: E402
from gcr_testutil import bits  # noqa: E402
from pygcransac import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if N.lib.gcr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    N.context(0)
    O.lib()


@pytest.fixture(scope="module")
def reference():
    env = {k: v for k, v in os.environ.items() if not k.startswith("GCR_VERIFY")}
    env["GCR_SCORER"] = "split"
    env["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p] + [env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout)


@pytest.mark.parametrize("nslots", SLOTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ring_scorer_equals_split_scorer(shape, nslots, reference, monkeypatch):
    _, prob, thr0, thr1 = _problem(shape)
    ref = reference[f"{shape}/{nslots}"]
    assert len(ref) == NB and sum(o[0] for o in ref) > 0          # models were generated and scored
    for groups, chain in RUNS:
        monkeypatch.setenv("GCR_VERIFY_GROUPS", groups)
        monkeypatch.setenv("GCR_VERIFY_CHAIN", chain)
        got = _fields(_records(prob, thr0, thr1, nslots, NB))
        for b in range(NB):
            assert got[b] == ref[b], (groups, chain, b)


def _oracle_slot(args):
    kind, f0, f1, thr0, thr1, s = args
    inc, m = O.slot(kind, f0, f1, SEED, s)
    if inc > 101:
        return inc, None, None
    return inc, m, O.score(kind, f0, f1, m, thr0, thr1)


def test_full_shape_fills_the_ring():
    # the premise of the "full" shape, from the oracle's residuals of the
    # first 64 slots (4 workgroups of 16): inliers are a subset of the band's
    # survivors, so a wave-round whose inlier runs already need the whole ring
    # (16 runs of 49 .. 64 values: 16 x 64 + 32 = 1056 doubles) needs it
    kind, prob, thr0, thr1 = _problem("full")
    T = [(2.25 * thr0) * thr0, (2.25 * thr1) * thr1]
    need = []
    for wg in range(4):
        per_q = []
        for q in range(16):
            inc, m = O.slot(kind, prob.f0, prob.f1, SEED, SLOT0 + 16 * wg + q)
            runs = []
            for cls, f in ((0, prob.f0), (1, prob.f1)):
                if inc > 101:
                    inl = np.zeros(f.shape[0], dtype=bool)
                else:
                    inl = O.residuals(kind, cls, f, m) <= T[cls]
                for r0 in range(0, f.shape[0], 896):
                    for w in range(14):
                        runs.append(int(inl[r0 + 64 * w:min(r0 + 64 * w + 64, r0 + 896)].sum()))
            per_q.append(runs)
        n = np.array(per_q)                                        # [q][wave-round]
        padded = ((n + 15) // 16 * 16).sum(axis=0)
        need += [int(p) + 32 if p else 0 for p in padded]
    need = np.array([x for x in need if x])
    print(f"full shape: {len(need)} wave-rounds with survivors, {np.mean(need == 1056):.2f} need 1056 doubles, "
          f"{np.mean(need >= 528):.2f} at least 528")
    assert (need == 1056).any(), "no wave-round of the full shape needs the whole ring"


def test_full_ring_matches_oracle_replay():
    # the full-ring shape, 2 batches of 2048 slots: every record against the
    # oracle's sampler, solver, twin-math MSAC score and `best < score &&
    # isValidModel` in slot order (as test_gpu_verify_groups.py replays)
    kind, prob, thr0, thr1 = _problem("full")
    nslots, nb = 2048, 2
    res = _records(prob, thr0, thr1, nslots, nb)
    with ThreadPoolExecutor(THREADS) as ex:
        outs = list(ex.map(_oracle_slot, [(kind, prob.f0, prob.f1, thr0, thr1, s)
                                          for s in range(SLOT0, SLOT0 + nb * nslots)], chunksize=64))
    for b in range(nb):
        s0 = SLOT0 + b * nslots
        models = iters = 0
        best, bslot, bcnt, bmodel = 0.0, -1, [0, 0], None
        for j, (inc, m, sc) in enumerate(outs[b * nslots:(b + 1) * nslots]):
            iters += inc
            if m is None:
                continue
            models += 1
            valid = max(abs(m[3]), abs(m[4])) < 1e-3            # two_sift.hpp:45-61
            if best < sc["value"] and valid:
                best, bslot, bcnt, bmodel = sc["value"], s0 + j, [int(c) for c in sc["counts"]], m
        r = res[b]
        assert (r.models, r.iterations, r.best_slot) == (models, iters, bslot), b
        assert bslot >= 0, b
        assert bits(r.best_score) == bits(best), b
        assert [r.best_inliers[0], r.best_inliers[1]] == bcnt, b
        got = [r.best_model.x0, r.best_model.y0, r.best_model.s, r.best_model.h7, r.best_model.h8,
               r.best_model.alpha, r.best_model.phi]
        assert np.array_equal(bits(got), bits(bmodel)), b
