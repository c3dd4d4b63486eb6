"""PROSAC sampling on the CPU (csrc/prosac.h): the growth table against its
restatement, the host sampler against the existing primitives, the Python
wrapper's ordering, and the conditions the GPU whole-run tests rest on."""
import ctypes as C

import numpy as np
import pytest

import prosac_cases as PC
import pygcransac
from pygcransac import _native as N
from pygcransac import pygcransac as P
from pygcransac import synthetic as S

SEED = 0x5EEDFACE12345678
MS = (2, 3, 4, 5, 7)


# ----------------------------------------------------------- growth table ----
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("convergence", (1, 1000, 100000, 1 << 40))
def test_growth_table_equals_restatement(m, convergence):
    for n in (m, m + 1, 257, 2000, 10007):
        g = PC.host_growth(n, m, convergence)
        assert np.array_equal(g, PC.growth_ref(n, m, convergence)), (n, m, convergence)
        assert not g[:m].any() and g[m] == 1
        assert np.all(np.diff(g[m:].astype(np.int64)) >= 1), (n, m, convergence)      # strictly increasing


def test_growth_table_known_values():
    assert PC.host_growth(10000, 7, 100000)[-1] == 106813
    assert PC.host_growth(7, 7, 100000)[-1] == 1


def test_pool_equals_restatement():
    for n, m, convergence in ((257, 4, 1000), (10007, 7, 100000), (5, 5, 1), (2000, 2, 1 << 40)):
        g = PC.growth_ref(n, m, convergence)
        gn = int(g[n])
        slots = sorted({0, 1, 2, 50, 255, 256, max(gn - 2, 0), gn - 1, gn, gn + 1, 1 << 40, (1 << 64) - 1})
        for slot in slots:
            want = PC.pool_ref(g, n, m, slot) if slot < (1 << 64) - 1 else 0
            assert PC.host_pool(n, m, convergence, slot) == want, (n, m, convergence, slot)
        assert PC.host_pool(n, m, convergence, 0) == m
        assert PC.host_pool(n, m, convergence, gn - 1) == n and PC.host_pool(n, m, convergence, gn) == 0


def test_host_argument_checks():
    g = np.zeros(16, dtype=np.uint64)
    gp = g.ctypes.data_as(PC.u64p)
    assert N.lib.gcr_host_prosac_growth(10, 4, (1 << 40) + 1, gp) == N.GCR_EINVAL
    assert "2^40" in N.last_error()
    assert N.lib.gcr_host_prosac_growth(10, 4, 0, gp) == N.GCR_EINVAL
    assert N.lib.gcr_host_prosac_growth(3, 4, 1000, gp) == N.GCR_EINVAL          # n < m
    assert N.lib.gcr_host_prosac_growth(10, 4, 1000, None) == N.GCR_EINVAL
    assert N.lib.gcr_problem_set_prosac(None, 1000) == N.GCR_EINVAL


# ----------------------------------------------------------- host sampler ----
@pytest.mark.parametrize("m", MS)
def test_host_sampler_equals_existing_primitives(m):
    for n in (m, m + 1, 257, 10007):
        for convergence in (1000, 100000):
            g = PC.growth_ref(n, m, convergence)
            gn = int(g[n])
            slots = sorted(set(range(40)) | {255, 256, 300, max(gn - 2, 0), gn - 1, gn, gn + 1, gn + 77, 1 << 40})
            for slot in slots:
                pool = PC.pool_ref(g, n, m, slot)
                for a in (0, 1, 100):
                    rc, got = PC.host_sample_prosac(SEED, slot, a, n, m, convergence)
                    wrc, want = PC.composed_sample(g, SEED, slot, a, n, m)
                    assert rc == wrc == 0, (n, m, slot, a)
                    assert np.array_equal(got, want), (n, m, convergence, slot, a)
                    assert len(set(got.tolist())) == m                           # distinct
                    if pool:                                                     # growth phase
                        assert slot < gn and got[-1] == pool - 1 and np.all(got[:-1] < pool - 1)
                    else:                                                        # the uniform sampler's own bits
                        assert slot >= gn
                        assert np.array_equal(got, PC.host_sample_uniform(SEED, slot, a, n, m)[1])


def test_all_attempts_of_a_slot_share_its_pool():
    n, m, convergence = 2000, 4, 100000
    for slot in (0, 7, 300):
        pool = PC.host_pool(n, m, convergence, slot)
        for a in range(0, 101, 10):
            assert PC.host_sample_prosac(SEED, slot, a, n, m, convergence)[1][-1] == pool - 1


# --------------------------------------------------------- Python wrapper ----
def test_order_is_stable_descending():
    assert P.prosac_order([1.0, 3.0, 3.0, 1.0, 3.0, 7.0]).tolist() == [5, 1, 2, 4, 0, 3]
    assert P.prosac_order(-np.arange(9)).tolist() == list(range(9))              # rows already in quality order


class FakeEngine:
    """Stands in for the resident-problem calls of the sampler=1 path: records
    what it was given and marks as inliers the ordered rows whose tag (column
    0, the caller's row number) is even."""

    def __init__(self, monkeypatch):
        self.rows = self.sift = self.convergence = None
        self.destroyed = 0
        monkeypatch.setattr(N, "context", lambda device=None: 1)
        monkeypatch.setattr(N.lib, "gcr_problem_create", self.create, raising=False)
        monkeypatch.setattr(N.lib, "gcr_problem_create_sift_homography", self.create_sift, raising=False)
        monkeypatch.setattr(N.lib, "gcr_problem_set_prosac", self.set_prosac, raising=False)
        monkeypatch.setattr(N.lib, "gcr_problem_run", self.run, raising=False)
        monkeypatch.setattr(N.lib, "gcr_problem_destroy", self.destroy, raising=False)

    @staticmethod
    def _array(ptr, n, cols):
        addr = ptr if isinstance(ptr, int) else C.cast(ptr, C.c_void_p).value
        return np.ctypeslib.as_array((C.c_double * (n * cols)).from_address(addr)).reshape(n, cols).copy()

    def create(self, ctx, solver, f0, n0, f1, n1, out):
        self.rows = self._array(f0, n0, 4)
        out._obj.value = 1234
        return 0

    def create_sift(self, ctx, f, sift, n, out):
        self.rows = self._array(f, n, 4)
        self.sift = self._array(sift, n, 4)
        out._obj.value = 1234
        return 0

    def set_prosac(self, h, convergence):
        assert h.value == 1234
        self.convergence = convergence
        return 0

    def run(self, h, params, mask0, mask1, H, model, stats):
        n = len(self.rows)
        even = (self.rows[:, 0].astype(np.int64) % 2 == 0)
        for i in range(n):
            mask0[i] = 1 if even[i] else 0
        for q in range(9):
            H[q] = float(q)
        return int(even.sum())

    def destroy(self, h):
        self.destroyed += 1


def tagged_rows(n, cols=4):
    rows = np.random.default_rng(5).uniform(0.0, 900.0, (n, cols))
    rows[:, 0] = np.arange(n)                       # the caller's row number
    return rows


def test_wrapper_sorts_rows_and_returns_the_mask_in_caller_order(monkeypatch):
    eng = FakeEngine(monkeypatch)
    n = 50
    rows = tagged_rows(n)
    scores = np.random.default_rng(6).integers(0, 8, n).astype(np.float64)       # many ties
    M, mask = pygcransac.findHomography(rows, 960, 1280, 960, 1280, probabilities=scores, sampler=1,
                                        prosac_convergence=777, neighborhood_size=0, spatial_coherence_weight=0.0)
    order = np.argsort(-scores, kind="stable")
    assert np.array_equal(eng.rows, rows[order])
    assert np.all(np.diff(scores[order]) <= 0)
    tags = eng.rows[:, 0].astype(int)
    for v in np.unique(scores):                     # ties keep the input order
        assert np.all(np.diff(tags[scores[order] == v]) > 0)
    assert eng.convergence == 777 and eng.destroyed == 1
    assert mask.dtype == bool and np.array_equal(mask, np.arange(n) % 2 == 0)
    assert np.array_equal(M.ravel(), np.arange(9.0))
    # the default convergence length is upstream's
    pygcransac.findFundamentalMatrix(rows, 960, 1280, 960, 1280, probabilities=-np.arange(n), sampler=1,
                                     neighborhood_size=0, spatial_coherence_weight=0.0)
    assert eng.convergence == 100000 and np.array_equal(eng.rows, rows)


def test_wrapper_sorts_the_sift_columns_with_their_rows(monkeypatch):
    eng = FakeEngine(monkeypatch)
    n = 40
    rows8 = tagged_rows(n, 8)
    rows8[:, 4:6] = np.abs(rows8[:, 4:6]) + 1.0     # sizes > 0
    rows8[:, 6:8] = rows8[:, 6:8] / 900.0           # angles
    scores = np.random.default_rng(7).normal(size=n)
    M, mask = pygcransac.findHomographySIFT(rows8, 960, 1280, 960, 1280, probabilities=scores, sampler=1,
                                            neighborhood_size=0, spatial_coherence_weight=0.0)
    order = np.argsort(-scores, kind="stable")
    assert np.array_equal(eng.rows, rows8[order, :4]) and np.array_equal(eng.sift, rows8[order, 4:8])
    assert np.array_equal(mask, np.arange(n) % 2 == 0)


@pytest.mark.parametrize("fn", (pygcransac.findHomography, pygcransac.findFundamentalMatrix))
def test_wrapper_errors(fn):
    rows = tagged_rows(30)
    kw = dict(neighborhood_size=0, spatial_coherence_weight=0.0)
    with pytest.raises(ValueError, match="probabilities"):
        fn(rows, 960, 1280, 960, 1280, sampler=1, **kw)
    bad = np.ones(30)
    bad[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        fn(rows, 960, 1280, 960, 1280, probabilities=bad, sampler=1, **kw)
    bad[3] = np.inf
    with pytest.raises(ValueError, match="finite"):
        fn(rows, 960, 1280, 960, 1280, probabilities=bad, sampler=1, **kw)
    for flat in (np.ones(30), np.zeros(30), np.full(30, -2.5)):                  # equal scores rank nothing
        with pytest.raises(ValueError, match="rank"):
            fn(rows, 960, 1280, 960, 1280, probabilities=flat, sampler=1, **kw)
    with pytest.raises(ValueError, match="one quality score per correspondence"):
        fn(rows, 960, 1280, 960, 1280, probabilities=np.ones(29), sampler=1, **kw)
    for t in (0, (1 << 40) + 1):
        with pytest.raises(ValueError, match="prosac_convergence"):
            fn(rows, 960, 1280, 960, 1280, probabilities=-np.arange(30), sampler=1, prosac_convergence=t, **kw)
    with pytest.raises(ValueError, match="guided_stop"):
        fn(rows, 960, 1280, 960, 1280, probabilities=np.ones(30), sampler=1, guided_stop=True, **kw)
    with pytest.raises(ValueError, match="Unsupported sampler"):
        fn(rows, 960, 1280, 960, 1280, probabilities=np.ones(30), sampler=2, **kw)


# ------------------------------------- what the GPU whole-run tests rest on ----
@pytest.mark.parametrize("solver", (PC.H4, PC.F7))
def test_whole_run_problem_conditions(solver):
    """Slot 0 alone does not solve the problem (an outlier among the first m
    ordered rows), yet every tested seed draws an all-truth-inlier sample
    within its budget of 32 iterations, the first of them within 32 slots."""
    corr, truth, thr, scores = PC.e2e_problem(solver)
    m = PC.M_OF[solver]
    assert int(truth.sum()) == round((1.0 - PC.E2E_OUTLIERS) * PC.E2E_N)
    order = PC.order_of(scores)
    ts, cs = truth[order], np.ascontiguousarray(corr[order])
    assert not ts[:m].all()
    for seed in PC.E2E_SEEDS:
        walk = PC.budget_walk(solver, cs, ts, seed)
        hits = [slot for slot, _, ok in walk if ok]
        print(f"solver {solver} seed {seed}: {len(walk)} slots with a model, all-inlier samples at slots {hits}")
        assert hits and hits[0] < 32, (seed, walk)
        assert walk[0][0] == 0 and not walk[0][2]   # slot 0 gives a model, from a sample with an outlier
