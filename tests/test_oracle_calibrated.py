"""The oracle's additions for calibrated and guided whole runs, on the CPU: its
restatements of csrc/guided.h and csrc/guided_stop.h against the product's host
entries bit for bit, its run loop around the 5-point and 3-point host solvers
against the synthetic truth and against its own final rule, minimal inputs and
the recorded runs of tests/golden/calib."""
import ctypes as C

import numpy as np
import pytest

import calibrated_cases as CC
import gravity_cases as GC
import guided_cases as G
from gcr_testutil import bits
from pygcransac import _native as N

u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
WORDS = (0, 1, 1 << 11, (1 << 11) - 1, 1 << 63, (1 << 63) - 1, 0x9E3779B97F4A7C15, (1 << 64) - (1 << 11) - 1,
         (1 << 64) - (1 << 11), (1 << 64) - 1)


def draw_weights(n, m):
    """name -> weights with at least m positive entries."""
    rng = np.random.default_rng(5 + 1000 * n + m)
    out = {}
    # leading, trailing and interior zeros around exactly max(m, n // 3) positive entries
    w = np.zeros(n)
    keep = max(m, n // 3)
    lead, trail = ((n - keep) // 3, (n - keep) // 3) if n - keep >= 3 else (0, 0)
    pos = np.sort(rng.choice(np.arange(lead, n - trail), keep, replace=False))
    w[pos] = rng.uniform(0.5, 2.0, keep)
    out["edge_zeros"] = w
    for pattern in ("zero_runs", "heavy", "heavy90", "loguniform"):
        v = G.weights(pattern, n, m)
        if int((v > 0).sum()) >= m:
            out[pattern] = v
    # sums that are no power of two and round at every step.  (r <= 1 - 2^-53, so r * total never rounds up
    # to total: the largest u, of W = 2^64 - 1, lies one ulp under it, and the definition's "c[i] == total"
    # clause cannot be reached through a word -- DESIGN section 6)
    out["rounding"] = rng.uniform(0.1, 1.0, n) * (1.0 + 2.0 ** -30)
    return out


def host_index(w, m, word):
    out = C.c_uint32()
    N.check(N.lib.gcr_host_guided_index(w.ctypes.data, len(w), m, word, C.byref(out)))
    return out.value


@pytest.mark.parametrize("n", G.NS)
def test_guided_draws_equal_the_host_sampler_bitwise(oracle, n):
    crossings = 0
    for m in (3, 7):
        for name, w in draw_weights(n, m).items():
            w = np.ascontiguousarray(w)
            if name == "edge_zeros" and n >= 255:
                assert w[0] == 0.0 and w[-1] == 0.0 and (w[np.flatnonzero(w)[0]:np.flatnonzero(w)[-1]] == 0.0).any()
            if name == "zero_runs" and n > 256:
                c = G.cdf_of(w)
                stride = (n + 255) // 256
                assert stride >= 2
                edges = np.arange(stride, n, stride)
                crossings += int((c[edges - 1] == c[edges]).sum())     # a run of equal values across a bucket boundary
            # a heavy entry exhausts the 4096-word budget: a few samples show the refusal on both sides
            slots = range(2) if name == "heavy" else range(24)
            exhausted = 0
            for index in slots:
                for sub in (0, 100):
                    got = oracle.sample_guided(77, (1 << 40) + index, sub, 0, 0, w, m)
                    rc, want = G.host_sample_guided(77, (1 << 40) + index, sub, w, m)
                    assert (got is None) == (rc != 0), (name, m, index, sub)
                    if got is None:
                        exhausted += 1
                        continue
                    assert np.array_equal(got, want), (name, m, index, sub)
                    assert np.all(w[got.astype(np.int64)] > 0) and len(set(got.tolist())) == m
            if name == "heavy":
                assert exhausted == 4
            elif name != "loguniform":                 # (a few of its weights dominate: some samples complete, some not)
                assert exhausted == 0, (name, exhausted)
            # single draws by their word, the extremes of r = (W >> 11) 2^-53 included
            c = G.cdf_of(w)
            for word in WORDS:
                i = oracle.guided_pick(w, word)
                assert i == host_index(w, m, word), (name, m, hex(word))
                assert w[i] > 0
                # ... and guided_cases' numpy statement of the same definition
                u = float(word >> 11) * 2.0 ** -53 * float(c[-1])
                k = int(np.searchsorted(c, u, side="right"))
                assert i == (k if k < n else int(np.searchsorted(c, c[-1], side="left"))), (name, m, hex(word))
            assert oracle.guided_pick(w, 0) == np.flatnonzero(w)[0]
            assert c[oracle.guided_pick(w, (1 << 64) - 1)] == c[-1]    # the last entry that still moves the CDF
    if n > 256:
        assert crossings > 0


@pytest.mark.parametrize("n", G.NS)
def test_guided_quanta_equal_the_host_quanta(oracle, n):
    for name, w in draw_weights(n, 3).items():
        w = np.ascontiguousarray(w)
        q = np.zeros(n, dtype=np.uint64)
        Q = C.c_uint64()
        N.check(N.lib.gcr_host_guided_quanta(w.ctypes.data, n, 3, q.ctypes.data_as(u64p), C.byref(Q)))
        oq, oQ = oracle.guided_quanta(w)
        assert np.array_equal(oq, q) and oQ == Q.value, name
        assert 0 < oQ < 2 ** 52 and not oq[w == 0].any(), name
        if name not in ("heavy", "loguniform"):               # (their small weights truncate to no quantum)
            assert oq[w > 0].all(), name


def test_guided_iterations_equal_the_host_stop(oracle):
    seen = set()
    for n in (7, 600, 10007):
        _, Q = oracle.guided_quanta(np.ones(n))
        for mass in (0, 1, Q // 2, Q - 1, Q):
            for m in (3, 4, 5, 7):
                for conf in (0.5, 0.99, 1.0 - 1e-12):
                    out = C.c_uint64()
                    N.check(N.lib.gcr_host_guided_iterations(mass, Q, m, conf, C.byref(out)))
                    got = oracle.guided_iterations(mass, Q, m, conf)
                    assert got == out.value, (n, mass, m, conf)
                    seen.add(got)
    # the guard's "never" (no inlier mass), 0 (all of it) and proper counts in between all occur
    assert 2 ** 64 - 1 in seen and 0 in seen and any(1 < v < 10 ** 6 for v in seen)


# ------------------------------------------------------------- whole runs ----
@pytest.fixture(scope="module")
def runs(oracle):
    out = {}
    for kind, seed in (("E", 61), ("G", 62)):
        p = CC.problem(kind, 600, 0.5, seed=seed)
        out[kind] = (p, CC.run_oracle(p, seed=7, lam=0.3))
    return out


@pytest.mark.parametrize("kind", ("E", "G"))
def test_oracle_run_finds_the_truth_and_returns_its_own_final_mask(runs, kind):
    p, r = runs[kind]
    truth, mask = p["truth"], r["mask"]
    assert r["num_inliers"] == mask.sum() > 0
    assert (mask & truth).sum() >= 0.9 * truth.sum()
    assert r["stats"]["local_optimization_number"] > 0 and r["stats"]["hypotheses"] > r["stats"]["slots"]
    E = r["H"]
    assert abs(np.linalg.norm(E) - 1.0) < 1e-12
    # the final rule on its own model: r^2 <= (2.25 thr) thr on the normalised rows
    T = (2.25 * r["thr"]) * r["thr"]
    assert np.array_equal(CC.sampson(r["rows"], E) <= T, mask)
    if kind == "G":
        assert GC.constrained_form(E, p["G1"], p["G2"]) < 1e-14
    again = CC.run_oracle(p, seed=7, lam=0.3)
    assert np.array_equal(again["mask"], mask) and np.array_equal(bits(again["H"]), bits(E))
    assert {k: again["stats"][k] for k in CC.COUNTS} == {k: r["stats"][k] for k in CC.COUNTS}
    assert bits(again["stats"]["score"]) == bits(r["stats"]["score"])
    other = CC.run_oracle(p, seed=8, lam=0.3)
    assert other["stats"]["slots"] != r["stats"]["slots"] or not np.array_equal(bits(other["H"]), bits(E))


@pytest.mark.parametrize("kind", ("E", "G"))
def test_minimal_input(oracle, kind):
    p = CC.problem(kind, 60, 0.0, seed=63)
    m = CC.M_OF[kind]
    exact = dict(p, corr=np.ascontiguousarray(p["corr"][:m]))
    r = CC.run_oracle(exact, seed=1, min_it=100, max_it=100)
    assert r["num_inliers"] == 0 and not r["mask"].any() and r["stats"]["iteration_number"] >= 100
    below = dict(p, corr=np.ascontiguousarray(p["corr"][:m - 1]))
    with pytest.raises(RuntimeError):
        CC.run_oracle(below, seed=1, min_it=100, max_it=100)


def test_a_raising_callback_fails_the_run(oracle, monkeypatch):
    p = CC.problem("E", 60, 0.0, seed=63)
    calls = []

    def broken(*args):
        calls.append(1)
        raise ValueError("solver callback broke")

    monkeypatch.setattr(N.lib, "gcr_host_solve_minimal", broken)
    with pytest.raises(RuntimeError):
        CC.run_oracle(p, seed=1, min_it=100, max_it=100)
    assert len(calls) == 1                                     # the run ended at the first failure


@pytest.mark.parametrize("kind", ("H", "F"))
def test_added_entries_leave_the_uniform_run_unchanged(oracle, kind):
    """Without weights the entries added for guided runs are the plain ones."""
    p = CC.problem(kind, 500, 0.5, seed=64)
    a = CC.run_oracle(p, seed=3, lam=0.3)
    from pygcransac import pygcransac as P

    plain = oracle.find_homography if kind == "H" else oracle.find_fundamental
    b = plain(p["corr"], p["thr"], min_it=50, max_it=5000, confidence=0.99, lam=0.3, lo=50, seed=3,
              cell_size=P.grid_cell_sizes(p["corr"], *CC.SIZE, 8), cell_number=8)
    assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(bits(a["H"]), bits(b["H"]))
    assert {k: a["stats"][k] for k in CC.COUNTS} == {k: b["stats"][k] for k in CC.COUNTS}
    assert a["stats"]["graph_cut_number"] > 0


@pytest.mark.parametrize("kind", ("H", "F", "E", "G"))
def test_guided_oracle_runs(oracle, kind):
    """Guided draws reach the run (a zero weight is never sampled into a
    minimal-size result), the mass stop differs from the count stop under
    informative weights and is the count stop under equal ones."""
    p = CC.problem(kind, 600, 0.5, seed=65)
    w = CC.guided_weights(p["truth"], seed=66)
    # the floor of 2 iterations lies under every bound: each run is ended by its own stop
    kw = dict(seed=4, min_it=2, max_it=5000, confidence=1.0 - 1e-12)
    uni = CC.run_oracle(p, **kw)
    off = CC.run_oracle(p, weights=w, guided_stop=False, **kw)
    on = CC.run_oracle(p, weights=w, guided_stop=True, **kw)
    assert kw["min_it"] < on["stats"]["iteration_number"] < off["stats"]["iteration_number"] < kw["max_it"]
    assert on["stats"]["iteration_number"] < uni["stats"]["iteration_number"] < kw["max_it"]
    assert not np.array_equal(bits(off["H"]), bits(uni["H"])) or off["stats"]["hypotheses"] != uni["stats"]["hypotheses"]
    for r in (off, on):
        assert (r["mask"] & p["truth"]).sum() >= 0.9 * p["truth"].sum()
    ones = np.ones(len(w))
    a = CC.run_oracle(p, weights=ones, guided_stop=False, **kw)
    b = CC.run_oracle(p, weights=ones, guided_stop=True, **kw)
    assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(bits(a["H"]), bits(b["H"]))
    assert {k: a["stats"][k] for k in CC.COUNTS} == {k: b["stats"][k] for k in CC.COUNTS}


@pytest.mark.parametrize("name", CC.CALIB_NAMES)
def test_calib_fixture_is_reproduced_bitwise(oracle, name):
    p, kw, want = CC.load_calib(name)
    assert np.array_equal(p["corr"], CC.calib_problem(name)["corr"])
    r = CC.run_oracle(p, **kw)
    assert np.array_equal(r["mask"], want["mask"]) and r["num_inliers"] == want["num_inliers"] > 0
    assert np.array_equal(bits(r["H"]), bits(want["H"]))
    assert {k: r["stats"][k] for k in CC.COUNTS} == {k: want["stats"][k] for k in CC.COUNTS}
    assert bits(r["stats"]["score"]) == bits(want["stats"]["score"])
    assert r["stats"]["local_optimization_number"] > 0
    if name.endswith("n500"):
        assert r["stats"]["graph_cut_number"] > 0 and kw["lam"] > 0
