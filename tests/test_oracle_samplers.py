"""The oracle's additions for PROSAC, NAPSAC and SIFT-homography whole runs, on
the CPU: its restatements of csrc/prosac.h, csrc/prosac_stop.h and
csrc/napsac.h against the product's host entries bit for bit, whole runs on the
oracle alone (what each run of test_gpu_oracle_samplers.py must do is asserted
here on the reference), and the recorded runs of tests/golden/samplers."""
import numpy as np
import pytest

import napsac_cases as NC
import prosac_cases as PC
import prosac_stop_cases as Q
import sampler_run_cases as SR
from gcr_testutil import bits

MS = (2, 3, 4, 5, 7)
SEED = 77


def same_result(a, b):
    return (np.array_equal(a["mask"], b["mask"]) and np.array_equal(bits(a["H"]), bits(b["H"]))
            and {k: a["stats"][k] for k in SR.COUNTS} == {k: b["stats"][k] for k in SR.COUNTS}
            and bits(a["stats"]["score"]) == bits(b["stats"]["score"]))


# ---------------------------------------------------------------- PROSAC ----
@pytest.mark.parametrize("m", MS)
def test_growth_table_equals_the_host_table(oracle, m):
    for n in (m, m + 1, 257, 10007):
        for convergence in SR.CONVERGENCES:
            g = oracle.prosac_growth(n, m, convergence)
            assert np.array_equal(g, PC.host_growth(n, m, convergence)), (n, m, convergence)
            assert np.array_equal(g, PC.growth_ref(n, m, convergence)), (n, m, convergence)
            assert not g[:m].any() and g[m] == 1 and np.all(np.diff(g[m:].astype(np.int64)) >= 1)


@pytest.mark.parametrize("m", MS)
def test_prosac_samples_equal_the_host_sampler(oracle, m):
    phases = set()
    for n in (m + 1, 257):
        for convergence in SR.CONVERGENCES:
            g = PC.host_growth(n, m, convergence)
            top = int(g[n])
            for slot in sorted({0, 1, top // 3, top - 1, top, top + 1, 1 << 40}):
                for attempt in (0, 100):
                    got, pool = oracle.sample_prosac(SEED, slot, attempt, n, m, convergence)
                    rc, want = PC.host_sample_prosac(SEED, slot, attempt, n, m, convergence)
                    assert rc == 0 and got is not None, (n, m, convergence, slot, attempt)
                    assert np.array_equal(got, want), (n, m, convergence, slot, attempt)
                    assert pool == PC.host_pool(n, m, convergence, slot) == PC.pool_ref(g, n, m, slot)
                    assert (pool == 0) == (slot >= top)
                    if pool:
                        assert got[-1] == pool - 1 and np.all(got[:-1] < pool - 1)
                    else:                                        # the uniform sampler's own bits
                        assert np.array_equal(got, oracle.sample(SEED, slot, attempt, 0, 0, n, m))
                    phases.add((pool == 0, slot))
    assert any(u for u, _ in phases) and any(not u and s > 1 for u, s in phases)


def test_the_smallest_pool_and_the_refusals(oracle):
    """Slot 0 draws m - 1 distinct indices out of exactly m - 1: the smallest
    pool there is.  pool - 1 >= m - 1 always holds, so the 4096-word budget
    cannot run out inside the growth phase (a duplicate is redrawn, and all
    m - 1 values are reachable); the refusal both sides share is the one for
    fewer rows than a sample."""
    for m in MS:
        for n in (m, m + 3):
            for attempt in (0, 1, 100):
                got, pool = oracle.sample_prosac(SEED, 0, attempt, n, m, 1000)
                rc, want = PC.host_sample_prosac(SEED, 0, attempt, n, m, 1000)
                assert rc == 0 and pool == m and np.array_equal(got, want)
                assert sorted(got.tolist()) == list(range(m))
        with pytest.raises(ValueError):
            oracle.sample_prosac(SEED, 0, 0, m - 1, m, 1000)
        assert PC.host_sample_prosac(SEED, 0, 0, m - 1, m, 1000)[0] != 0
        with pytest.raises(ValueError):
            oracle.prosac_growth(m - 1, m, 1000)


# ----------------------------------------------------------- PROSAC stop ----
@pytest.mark.parametrize("n", (7, 20, 21, 257, 2000))
def test_stop_tables_equal_the_host_tables(oracle, n):
    for m in MS:
        for convergence in SR.CONVERGENCES + (1 << 40,):
            for conf in (0.95, 0.99, 1.0 - 1e-12):
                imin, qmin = oracle.prosac_stop_tables(n, m, convergence, conf)
                want_i, want_q = Q.host_tables(n, m, convergence, conf)
                assert np.array_equal(imin, want_i), (n, m, convergence, conf)
                assert qmin.tobytes() == want_q.tobytes(), (n, m, convergence, conf)


def crafted_masks():
    """(n, m, convergence, mask, what) -- test_prosac_stop.py's crafted cases"""
    T = 1 << 40
    out = [(600, 4, T, Q.prefix_mask(600, 40), "share 1 up to 40"),
           (600, 4, T, Q.mask_of(600, list(range(1, 200, 2)) + list(range(300, 400))), "equal ratios at 200 and 400"),
           (2000, 4, 1000, Q.prefix_mask(2000, 12), "fails only coverage"),
           (2000, 4, T, Q.prefix_mask(2000, 12), "covered"),
           (2000, 4, T, Q.prefix_mask(2000, 5), "fails only non-randomness"),
           (2000, 4, T, Q.prefix_mask(2000, 7), "at Imin"),
           (20, 4, T, Q.prefix_mask(20, 18), "N = 20: only N"),
           (21, 4, T, Q.prefix_mask(21, 20), "N = 21: 20 is a candidate"),
           (21, 4, T, Q.prefix_mask(21, 19), "N = 21, 19 of 20")]
    for n in range(7, 20):
        out.append((n, 4, T, Q.prefix_mask(n, n - 2), "short problem"))
    return out


def test_stop_choice_equals_the_host_choice(oracle):
    expect = {"equal ratios at 200 and 400": (200, 400), "fails only coverage": (12, 2000), "covered": (12, 20),
              "fails only non-randomness": (5, 2000), "at Imin": (7, 20), "share 1 up to 40": (40, 40),
              "N = 20: only N": (18, 20), "N = 21: 20 is a candidate": (20, 20), "N = 21, 19 of 20": (19, 20)}
    for n, m, convergence, mask, what in crafted_masks():
        imin, qmin = Q.host_tables(n, m, convergence, 0.99)
        got = oracle.prosac_stop_choice(mask, m, convergence, 0.99)
        assert got == Q.host_choose(mask, m, imin, qmin) == Q.choose_ref(mask, m, imin, qmin), what
        if what in expect:
            assert got == expect[what], what
    rng = np.random.default_rng(3)
    below = 0
    for m in MS:
        for n in (m, 19, 20, 21, 257, 2000):
            if n < m:
                continue
            for convergence in (1000, 100000, 1 << 40):
                imin, qmin = Q.host_tables(n, m, convergence, 0.99)
                for share in (0.0, 0.05, 0.3, 0.9, 1.0):
                    p = np.clip(share * 3.0 * np.exp(-3.0 * np.arange(n) / n), 0.0, 1.0)
                    mask = (rng.random(n) < p).astype(np.uint8)
                    got = oracle.prosac_stop_choice(mask, m, convergence, 0.99)
                    assert got == Q.host_choose(mask, m, imin, qmin), (n, m, convergence, share)
                    below += got[1] < n
    assert below > 20


def test_stop_number_equals_the_host_number(oracle):
    seen = set()
    for best_n in (7, 20, 256, 10007):
        for best_i in sorted({0, 1, best_n // 3, best_n - 1, best_n}):
            for m in MS:
                for conf in (0.5, 0.99, 1.0 - 1e-12):
                    got = oracle.prosac_stop_number(best_i, best_n, m, conf)
                    assert got == Q.host_stop_number(best_i, best_n, m, conf), (best_i, best_n, m, conf)
                    seen.add(got)
    assert Q.U64_MAX in seen and 0 in seen and any(1 < v < 10 ** 6 for v in seen)     # "never", 0 and proper counts


# ---------------------------------------------------------------- NAPSAC ----
def one_cell_rows(n=50):
    """every row in the same cell of every layer"""
    rng = np.random.default_rng(8)
    return np.ascontiguousarray(np.array([100.0, 100.0, 700.0, 500.0]) + rng.uniform(0.0, 5.0, (n, 4)))


def lone_rows():
    """Eight rows, each alone in its cell even at 2 cells per axis: every grid
    layer has count 1 < m, so every local sample falls back to layer 4."""
    e = np.array(NC.EXTENT)
    corners = [(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)][::2]
    return np.ascontiguousarray(np.array([(np.array(c) * 0.5 + 0.25) * e for c in corners]))


def napsac_row_sets():
    rng = np.random.default_rng(6)
    return {"uniform": np.ascontiguousarray(rng.uniform(0.0, 1.0, (400, 4)) * np.array(NC.EXTENT)),
            "local structure": NC.e2e_problem(0)[0][:600],
            "edges and negatives": NC.edge_rows()[0],
            "one cell": one_cell_rows(),
            "lone rows": lone_rows()}


@pytest.mark.parametrize("name", ("uniform", "local structure", "edges and negatives", "one cell", "lone rows"))
def test_napsac_layers_equal_the_host_layers(oracle, name):
    rows = napsac_row_sets()[name]
    got = oracle.napsac_layers(rows, NC.EXTENT)
    want = NC.host_layers(rows, NC.EXTENT)
    ref = NC.layers_ref(rows, NC.EXTENT)
    for l in range(4):
        for a, b, c in zip(got[l], want[l], ref[l]):
            assert np.array_equal(a, b) and np.array_equal(a, c), (name, l)
    if name == "edges and negatives":
        assert (rows < 0).any()
    if name == "one cell":
        assert all(np.all(got[l][2] == len(rows)) for l in range(4))
    if name == "lone rows":
        assert all(np.all(got[l][2] == 1) for l in range(4))


@pytest.mark.parametrize("name", ("uniform", "local structure", "edges and negatives", "one cell", "lone rows"))
def test_napsac_samples_equal_the_host_sampler(oracle, name):
    rows = napsac_row_sets()[name]
    n = len(rows)
    layers = NC.layers_ref(rows, NC.EXTENT)
    picked = set()
    for m in (2, 4, 7):
        for T in (8, 200, 1001):
            edges = sorted({0, T - 1, T, T + 1, 1 << 40} | {q * T // 4 + d for q in (1, 2, 3) for d in (-1, 0, 1)}
                           | {-(-q * T // 4) + d for q in (1, 2, 3) for d in (-1, 0)})
            for slot in (s for s in edges if s >= 0):
                for attempt in (0, 100):
                    got = oracle.samples_napsac(SEED, slot, 3, attempt, rows, m, NC.EXTENT, T)
                    want = NC.host_samples(SEED, slot, 3, attempt, rows, m, NC.EXTENT, T)
                    assert np.array_equal(got, want), (name, m, T, slot, attempt)
                    assert not (got == NC.ALL_ONES).any()
                    for k in range(3):
                        s = slot + k
                        assert len(set(got[k].tolist())) == m
                        if s >= T:
                            assert np.array_equal(got[k], oracle.sample(SEED, s, attempt, 0, 0, n, m))
                        else:
                            picked.add((m, NC.pick_layer(layers, int(got[k][0]), s, T, m)))
    if name == "lone rows":
        assert {l for _, l in picked} == {4}                   # count < m at every grid layer
    if name == "one cell":
        assert {l for _, l in picked} == {0, 1, 2, 3}          # every layer's cell is all rows; l = l_min
    if name in ("uniform", "local structure"):
        used = {l for _, l in picked}
        assert len(used) >= 3                                    # the coarsening rule took several exits


# ------------------------------------------------ whole runs, oracle alone ----
@pytest.fixture(scope="module")
def main(oracle):
    """kind -> (problem, scores, run seed)"""
    return {k: (SR.main_problem(k), SR.main_scores(k), SR.PROSAC_SEEDS[k][1]) for k in SR.KINDS}


@pytest.mark.parametrize("kind", SR.KINDS)
def test_runs_are_deterministic_and_each_mode_differs_from_the_uniform_run(main, kind):
    p, q, seed = main[kind]
    modes = {"uniform": {}, "prosac": dict(sampler=1, scores=q), "napsac": dict(sampler=2)}
    runs = {}
    for name, kw in modes.items():
        runs[name] = SR.run_oracle(p, seed=seed, **kw)
        assert same_result(runs[name], SR.run_oracle(p, seed=seed, **kw)), name
        r = runs[name]
        assert r["num_inliers"] == r["mask"].sum() and (r["mask"] & p["truth"]).sum() >= 0.9 * p["truth"].sum(), name
        assert r["stats"]["local_optimization_number"] > 0, name
    for name in ("prosac", "napsac"):
        assert not same_result(runs[name], runs["uniform"]), name
    assert not same_result(runs["prosac"], runs["napsac"])
    if kind in ("F", "E", "G"):                                  # several models per sample, each scored
        assert all(r["stats"]["hypotheses"] > r["stats"]["slots"] for r in runs.values())
    if kind == "S":
        # the kind never had a whole-run reference: the final rule on its own model
        r = runs["uniform"]
        c = p["corr"]
        H = r["H"]
        w = (H[2, 0] * c[:, 0] + H[2, 1] * c[:, 1]) + H[2, 2]
        du = ((H[0, 0] * c[:, 0] + H[0, 1] * c[:, 1]) + H[0, 2]) / w - c[:, 2]
        dv = ((H[1, 0] * c[:, 0] + H[1, 1] * c[:, 1]) + H[1, 2]) / w - c[:, 3]
        assert np.array_equal(du * du + dv * dv <= (2.25 * p["thr"]) * p["thr"], r["mask"])
        assert H[2, 2] == 1.0


@pytest.mark.parametrize("kind", SR.KINDS)
def test_the_caller_order_comes_back(main, kind):
    """The oracle's PROSAC run is made on sorted rows; scattered back, its mask
    marks the same correspondences, and the sort is stable on the tied scores."""
    p, q, seed = main[kind]
    order = np.array(SR.quality_order(q))
    assert np.array_equal(order, np.argsort(-q, kind="stable"))
    ties = np.flatnonzero(np.diff(q[order]) == 0)
    assert len(ties) > 100 and np.all(order[ties] < order[ties + 1])
    r = SR.run_oracle(p, seed=seed, sampler=1, scores=q)
    assert np.array_equal(r["mask"][order], r["sorted_mask"]) and not np.array_equal(r["mask"], r["sorted_mask"])
    assert (r["mask"] & p["truth"]).sum() >= 0.9 * p["truth"].sum()


@pytest.mark.parametrize("kind", SR.KINDS)
def test_past_the_local_phase_the_run_shares_the_uniform_samples(main, kind):
    """NAPSAC with T = 1: only slot 0 is local, every later slot draws the
    uniform sampler's bits.  Without LO trials (lo = 0) the result of a run
    with a fixed count of iterations is a function of its best hypothesis
    alone, and that one lies among the hundreds of shared slots: the two runs
    return the same bytes.  (Slot 0's attempts shift the count of slots.)"""
    p, _, _ = main[kind]
    kw = dict(seed=5, min_it=600, max_it=600, lo=0)
    uni = SR.run_oracle(p, **kw)
    nap = SR.run_oracle(p, sampler=2, napsac_iterations=1, **kw)
    assert uni["num_inliers"] > SR.M_OF[kind]
    assert np.array_equal(uni["mask"], nap["mask"]) and np.array_equal(bits(uni["H"]), bits(nap["H"]))
    assert bits(uni["stats"]["score"]) == bits(nap["stats"]["score"])
    assert abs(uni["stats"]["slots"] - nap["stats"]["slots"]) <= 101
    # ... while a run that stays local differs
    loc = SR.run_oracle(p, sampler=2, napsac_iterations=1 << 40, **kw)
    assert not same_result(loc, uni)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_past_the_growth_phase_the_run_shares_the_uniform_samples(oracle, kind):
    """The same under PROSAC with convergence 1 (g[N] = N - m + 1) and scores
    that keep the rows' order: from slot g[N] on the samples are the uniform
    run's, and the best hypothesis of 8000 iterations lies there."""
    p = SR.problem(kind, 60, 0.3, seed=67)          # few rows: the growth phase is 60 - m + 1 slots of thousands
    n, m = len(p["corr"]), SR.M_OF[kind]
    top = int(SR.O.prosac_growth(n, m, 1)[-1])
    assert top == n - m + 1
    kw = dict(seed=5, min_it=8000, max_it=8000, lo=0)
    uni = SR.run_oracle(p, **kw)
    pro = SR.run_oracle(p, sampler=1, scores=SR.flat_scores(n), prosac_convergence=1, **kw)
    assert pro["stats"]["slots"] > 10 * top and uni["num_inliers"] > m
    assert np.array_equal(uni["mask"], pro["mask"]) and np.array_equal(bits(uni["H"]), bits(pro["H"]))
    assert bits(uni["stats"]["score"]) == bits(pro["stats"]["score"])


@pytest.mark.parametrize("kind", SR.KINDS)
def test_prosac_runs_do_what_the_gpu_test_is_about(main, kind):
    p, q, seed = main[kind]
    n, m = len(q), SR.M_OF[kind]
    stars = []
    for convergence in SR.CONVERGENCES:
        top = int(SR.O.prosac_growth(n, m, convergence)[-1])
        kw = dict(seed=seed, sampler=1, scores=q, prosac_convergence=convergence)
        plain = SR.run_oracle(p, **kw, **SR.PROSAC_KW)
        assert plain["stats"]["local_optimization_number"] > 0 and plain["num_inliers"] > m
        off = SR.run_oracle(p, prosac_stop=False, **kw, **SR.PSTOP_KW)
        on = SR.run_oracle(p, prosac_stop=True, **kw, **SR.PSTOP_KW)
        # the flagged run is ended by its own stop: not the floor, not the cap, and sooner than the clear run
        assert SR.PSTOP_KW["min_it"] < on["stats"]["iteration_number"] < off["stats"]["iteration_number"] \
            < SR.PSTOP_KW["max_it"]
        assert on["stats"]["slots"] > 2 * 5 and off["stats"]["slots"] > 2 * 64     # chunks of 5 and of 64 slots
        for r in (off, on):
            assert r["stats"]["local_optimization_number"] > 0
            assert (r["mask"] & p["truth"]).sum() >= 0.9 * p["truth"].sum()
        if kind in ("F", "E", "G"):
            assert off["stats"]["hypotheses"] > off["stats"]["slots"]
        stars.append(on["prosac_star"])
        cross = SR.run_oracle(p, **kw, **SR.CROSS_KW)
        if convergence == 1000:
            assert cross["stats"]["slots"] > top                   # crossed into the uniform phase
        else:
            assert cross["stats"]["slots"] < top and off["stats"]["slots"] < top     # ended inside the growth phase
    assert all(0 < i <= k < n for i, k in stars)                   # the stop chose a proper prefix


@pytest.mark.parametrize("kind", SR.KINDS)
def test_scores_without_order_make_the_flagged_run_the_clear_run(oracle, kind):
    """When every update chooses n* = N the flag changes nothing, bit for bit.
    The maximum over the prefixes is biased upward (prosac_stop.h's caveat), so
    under most random orders some prefix wins; sampler_run_cases.FLAT_CASES
    names orders and seeds under which none does."""
    p, q, seed = SR.flat_case(kind)
    n = len(p["corr"])
    assert len(np.unique(q)) == n and (n < 100 or abs(np.corrcoef(q, p["truth"])[0, 1]) < 0.15)   # no order in them
    kw = dict(seed=seed, sampler=1, scores=q, min_it=50, max_it=5000, confidence=0.99)
    off = SR.run_oracle(p, prosac_stop=False, **kw)
    on = SR.run_oracle(p, prosac_stop=True, **kw)
    assert on["prosac_star"][1] == n and on["prosac_star"][0] > SR.M_OF[kind]
    assert on["num_inliers"] > SR.M_OF[kind] and same_result(on, off)


def test_napsac_runs_do_what_the_gpu_test_is_about(main):
    T = SR.NAPSAC_T
    f = SR.run_oracle(main["F"][0], seed=main["F"][2], sampler=2, napsac_iterations=T)
    h = SR.run_oracle(main["H"][0], seed=main["H"][2], sampler=2, napsac_iterations=T)
    assert f["stats"]["slots"] > T > h["stats"]["slots"]           # F ends past T, H inside it
    assert f["stats"]["slots"] > 2 * 64 and h["stats"]["slots"] > 2 * 5
    loc = SR.local_problem()
    for kw in (dict(napsac_iterations=T), {}):
        r = SR.run_oracle(loc, seed=3, sampler=2, **kw)
        assert (r["mask"] & loc["truth"]).sum() >= 0.9 * loc["truth"].sum()
        assert r["stats"]["local_optimization_number"] > 0
    for kind in ("E", "G"):
        assert not np.array_equal(main[kind][0]["K"], np.eye(3))   # pixel rows and normalised rows differ


@pytest.mark.parametrize("kind", ("H", "F", "S"))
def test_added_arguments_leave_the_uniform_and_guided_runs_unchanged(oracle, kind):
    """Without sampler arguments the extended entries are the earlier ones:
    the plain entry's bytes for a uniform run, and a guided run is the same
    with sampler=0 spelled out."""
    from pygcransac import pygcransac as P

    p = SR.problem(kind, 500, 0.5, seed=64)
    a = SR.run_oracle(p, seed=3, lam=0.3)
    b = SR.run_oracle(p, seed=3, lam=0.3, sampler=0, prosac_convergence=7, napsac_iterations=3)
    assert same_result(a, b) and a["stats"]["graph_cut_number"] > 0
    if kind != "S":
        plain = oracle.find_homography if kind == "H" else oracle.find_fundamental
        c = plain(p["corr"], p["thr"], min_it=50, max_it=5000, confidence=0.99, lam=0.3, lo=50, seed=3,
                  cell_size=P.grid_cell_sizes(p["corr"], *SR.SIZE, 8), cell_number=8)
        assert same_result(a, c)
    w = np.where(p["truth"], 1.0, 0.05)
    g1 = SR.run_oracle(p, seed=3, weights=w, guided_stop=True, min_it=2, confidence=1.0 - 1e-12)
    assert not same_result(g1, a)
    # at most one draw may be set
    with pytest.raises(RuntimeError):
        SR.run_oracle(p, seed=3, weights=w, sampler=2)
    with pytest.raises(RuntimeError):
        SR.run_oracle(p, seed=3, weights=w, sampler=1, scores=w)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_small_problems_retry_their_slots(oracle, kind):
    p = SR.small_problem(kind)
    assert len(p["corr"]) == 40
    q = SR.quality_scores(p["truth"], 9)
    for kw in ({}, dict(sampler=1, scores=q, prosac_convergence=1000), dict(sampler=2)):
        r = SR.run_oracle(p, seed=11, max_it=2000, **kw)
        assert r["num_inliers"] > SR.M_OF[kind]
        assert r["stats"]["iteration_number"] > r["stats"]["slots"], (kind, kw.get("sampler"))


# ---------------------------------------------------------------- fixtures ----
@pytest.mark.parametrize("name", SR.GOLDEN_NAMES)
def test_sampler_fixture_is_reproduced_bitwise(oracle, name):
    p, kw, want = SR.load_golden(name)
    src, scores = SR.golden_problem(name)
    assert np.array_equal(p["corr"], src["corr"])
    assert (scores is None) == ("scores" not in kw) and (scores is None or np.array_equal(scores, kw["scores"]))
    r = SR.run_oracle(p, **kw)
    assert r["num_inliers"] == want["num_inliers"] > 0
    assert same_result(r, want)
    assert r["stats"]["local_optimization_number"] > 0
    if name.endswith("n500"):
        assert r["stats"]["graph_cut_number"] > 0 and kw["lam"] > 0
    else:
        assert r["stats"]["iteration_number"] > r["stats"]["slots"]          # duplicated rows: retried slots
