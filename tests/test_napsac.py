"""NAPSAC sampling (csrc/napsac.h) on the CPU: the layers against a numpy
restatement and against the graph cut's grid, the host sampler against the
definition restated from Philox words, a stand-alone C++ program under ASan +
UBSan, the wrapper's argument checks, and the conditions the GPU whole-run
test rests on.  (gcr_problem_set_napsac's own refusals need a resident
problem: test_gpu_napsac.py.)"""
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

import guided_cases as G
import napsac_cases as NC
import pygcransac
from pygcransac import _native as N
from pygcransac import pygcransac as P
from pygcransac import synthetic as S
from test_graphcut import product_edges

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
SEED = 0x5EEDFACE12345678
MS = (2, 3, 4, 5, 7)


# ------------------------------------------------------------------ layers ----
def test_layers_equal_the_numpy_restatement():
    rows, lone = NC.edge_rows()
    n = len(rows)
    ref, got = NC.layers_ref(rows, NC.EXTENT), NC.host_layers(rows, NC.EXTENT)
    for l in range(4):
        members, start, count, pos = got[l]
        for a, b in zip(ref[l], got[l]):
            assert np.array_equal(a, b), l
        # every row once; start / count / pos say where
        assert np.array_equal(np.sort(members), np.arange(n))
        assert np.array_equal(members[start + pos], np.arange(n))
        assert (pos < count).all() and (start.astype(np.int64) + count <= n).all()
        for i in range(n):
            cell = members[start[i]:start[i] + count[i]]
            assert (np.diff(cell.astype(np.int64)) > 0).all()              # rows ascending inside a cell
            assert (start[cell] == start[i]).all() and (count[cell] == count[i]).all()
        assert count[lone] == 1, l
    # the duplicates share a cell on every layer.  (Cells are keyed by the grid's index sum alone, as the graph
    # cut's: a point outside the extent may share a key with a cell inside it, so the layers need not nest.)
    for l in range(4):
        assert len(set(got[l][1][7:11])) == 1


def test_the_8_cell_layer_is_the_graph_cuts_grid():
    rows, _ = NC.edge_rows()
    members, start, count, _ = NC.host_layers(rows, NC.EXTENT)[1]
    edges = product_edges(rows, P.grid_cell_sizes(rows, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, 8), 8)
    want = []                                       # labeling()'s order: by a, then b, a < b inside a cell
    for i in range(len(rows)):
        cell = members[start[i]:start[i] + count[i]]
        want += [(i, int(j)) for j in cell if j > i]
    assert len(want) > 0 and np.array_equal(edges, np.array(want, dtype=np.uint32))


# ------------------------------------------------------------ host sampler ----
@pytest.mark.parametrize("m", MS)
def test_host_sampler_equals_the_definition(m):
    rows, _ = NC.edge_rows()
    n = len(rows)
    layers = NC.layers_ref(rows, NC.EXTENT)
    T = 1001                                        # not divisible by 4: quarters begin at 251, 501, 751
    quarter = [-(-k * T // 4) for k in (1, 2, 3)]
    assert quarter == [251, 501, 751]
    slots = list(range(12)) + [q + d for q in quarter for d in (-1, 0)] + [T - 1, T, T + 1, (1 << 32) + 5]
    seen_layers = set()
    for slot in slots:
        for a in (0, 1, 100):
            rc, idx = NC.host_sample(SEED, slot, a, rows, m, NC.EXTENT, T)
            assert rc == 0
            assert idx.tolist() == NC.ref_sample(layers, SEED, slot, a, n, m, T), (slot, a)
            uni = G.host_samples_uniform(SEED, slot, 1, a, n, m)[0]
            assert idx[0] == uni[0]
            assert len(set(idx.tolist())) == m
            if slot >= T:
                assert np.array_equal(idx, uni)
                continue
            l = NC.pick_layer(layers, int(idx[0]), slot, T, m)
            assert l >= 4 * slot // T
            seen_layers.add(l)
            assert set(idx.tolist()) <= set(NC.cell_rows(layers, l, int(idx[0]), n).tolist()), (slot, a, l)
    assert len(seen_layers) >= (3 if m <= 4 else 2)       # 300 rows: few cells hold 5 or 7 of them
    # T = 1: slot 0 is local (the finest layer), slot 1 uniform
    rc, idx = NC.host_sample(SEED, 0, 0, rows, m, NC.EXTENT, 1)
    assert rc == 0 and idx.tolist() == NC.ref_sample(layers, SEED, 0, 0, n, m, 1)
    rc, idx = NC.host_sample(SEED, 1, 0, rows, m, NC.EXTENT, 1)
    assert rc == 0 and np.array_equal(idx, G.host_samples_uniform(SEED, 1, 1, 0, n, m)[0])
    # the batch hook is the same function
    got = NC.host_samples(SEED, T - 20, 40, 1, rows, m, NC.EXTENT, T)
    for s in range(40):
        assert np.array_equal(got[s], NC.host_sample(SEED, T - 20 + s, 1, rows, m, NC.EXTENT, T)[1])


@pytest.mark.parametrize("m", MS)
def test_a_cell_of_exactly_m_rows_and_n_equal_m(m):
    """m rows in one cell of the finest layer, every other row alone in its
    cell: a local sample that starts in the cell is i0 plus the other m - 1
    rows, and over many slots every order of them occurs after every first
    row (all m! samples); one that starts elsewhere falls to all rows."""
    e = np.array(NC.EXTENT)
    n = 40
    rows = (np.arange(n)[:, None] * 7.0 + 1.0) * e        # far apart, outside the extent: all alone
    cell = np.arange(3, 3 + m)
    rows[cell] = e / 32.0 + np.arange(m)[:, None] * 0.25  # inside cell 0 of every layer
    layers = NC.host_layers(rows, NC.EXTENT)
    assert (layers[0][2][cell] == m).all() and (np.delete(layers[3][2], cell) == 1).all()
    T = 1 << 20
    got = NC.host_samples(SEED, 0, 6000, 0, rows, m, NC.EXTENT, T)
    inside = np.isin(got[:, 0], cell)
    assert inside.sum() >= 200
    assert (np.sort(got[inside], axis=1) == cell).all()
    for idx in got[~inside][:200]:                        # alone on every layer: layer 4
        assert len(set(idx.tolist())) == m
    # every order: the cell and one row outside it, so 7 of 8 local samples (m = 7) start inside; 24 m! slots
    # leave any one of the m! samples out with probability exp(-24 m / (m + 1)) < 2e-7 each
    few = np.ascontiguousarray(rows[2:3 + m])
    inner = np.arange(1, 1 + m)
    nslots = 24 * math.factorial(m) + 64
    assert nslots < T // 4                                # all in the first quarter
    got = NC.host_samples(SEED, 0, nslots, 0, few, m, NC.EXTENT, T)
    got = got[np.isin(got[:, 0], inner)]
    assert (np.sort(got, axis=1) == inner).all()
    assert len(np.unique(got, axis=0)) == math.factorial(m)
    # N = m: every sample is all rows
    rows_m = np.ascontiguousarray(rows[cell])
    for far in (rows_m, np.ascontiguousarray(rows[:m])):
        got = NC.host_samples(SEED, 0, 64, 0, far, m, NC.EXTENT, 16)
        assert (np.sort(got, axis=1) == np.arange(m)).all()
        assert np.array_equal(got[16:], G.host_samples_uniform(SEED, 16, 48, 0, m, m))


def test_host_hooks_refuse_bad_arguments():
    rows, _ = NC.edge_rows()
    for bad in ((0.0, 1, 1, 1), (1, -1.0, 1, 1), (1, 1, float("nan"), 1), (1, 1, 1, float("inf"))):
        rc, _ = NC.host_sample(SEED, 0, 0, rows, 4, bad, 100)
        assert rc == N.GCR_EINVAL and "extent" in N.last_error()
    for T in (0, (1 << 40) + 1):
        rc, _ = NC.host_sample(SEED, 0, 0, rows, 4, NC.EXTENT, T)
        assert rc == N.GCR_EINVAL and "2^40" in N.last_error()
    rc, _ = NC.host_sample(SEED, 0, 0, rows[:3], 4, NC.EXTENT, 100)
    assert rc == N.GCR_EINVAL
    rc, _ = NC.host_sample(SEED, 0, 0, rows, 4, NC.EXTENT, 1 << 40)
    assert rc == 0


# -------------------------------------------------- stand-alone C++ program ----
def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/napsac_host.cpp: the layers of rows with border, outside,
    non-finite and duplicated points and samples of every minimal size, a
    stand-alone host program built with ASan + UBSan."""
    exe = str(tmp_path / "napsac_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "napsac_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout


# ----------------------------------------------------------------- wrapper ----
FINDERS = (pygcransac.findHomography, pygcransac.findFundamentalMatrix)


@pytest.mark.parametrize("fn", FINDERS)
def test_wrapper_errors(fn):
    rows = np.random.default_rng(2).uniform(0.0, 900.0, (30, 4))
    kw = dict(neighborhood_size=0, spatial_coherence_weight=0.0)
    with pytest.raises(ValueError, match="Unsupported sampler 2 with probabilities"):
        fn(rows, 960, 1280, 960, 1280, probabilities=np.ones(30), sampler=2, **kw)
    for t in (0, (1 << 40) + 1):
        with pytest.raises(ValueError, match="napsac_iterations"):
            fn(rows, 960, 1280, 960, 1280, sampler=2, napsac_iterations=t, **kw)
    with pytest.raises(ValueError, match="guided_stop"):
        fn(rows, 960, 1280, 960, 1280, sampler=2, guided_stop=True, **kw)
    with pytest.raises(ValueError, match="prosac_stop"):
        fn(rows, 960, 1280, 960, 1280, sampler=2, prosac_stop=True, **kw)
    with pytest.raises(ValueError, match="Unsupported sampler"):
        fn(rows, 960, 1280, 960, 1280, sampler=4, **kw)


def test_signatures_and_defaults():
    for fn in (pygcransac.findHomography, pygcransac.findFundamentalMatrix, pygcransac.findEssentialMatrix,
               pygcransac.findGravityEssentialMatrix, pygcransac.findHomographySIFT):
        p = inspect.signature(fn).parameters["napsac_iterations"]
        assert p.default is None and p.kind == inspect.Parameter.KEYWORD_ONLY
    assert P._as_napsac_iterations(None, 2000) == 1000 and P._as_napsac_iterations(None, 7) == 4
    assert P._as_napsac_iterations(1 << 40, 10) == 1 << 40
    rows, _ = NC.edge_rows()
    assert P.napsac_extent(rows, 960, 1280, 960, 1280) == [1280.0, 960.0, 1280.0, 960.0]
    got = P.napsac_extent(rows, 0, 1280, -1, float("nan"))              # unknown sizes: from the data
    assert got == [1280.0, rows[:, 1].max() + 1.0, rows[:, 2].max() + 1.0, rows[:, 3].max() + 1.0]


def test_problem_h_local():
    corr, truth, H, thr = S.problem_h_local(2000, 0.9, seed=3)
    assert corr.shape == (2000, 4) and truth.sum() == 200 and thr == 2.0
    inl = corr[truth]
    assert np.ptp(inl[:, 0]) <= 0.25 * S.IMG_W and np.ptp(inl[:, 1]) <= 0.25 * S.IMG_H
    assert np.ptp(corr[~truth, 0]) > 0.9 * S.IMG_W and np.ptp(corr[~truth, 3]) > 0.9 * S.IMG_H
    p = H @ np.column_stack([inl[:, :2], np.ones(len(inl))]).T
    assert np.abs(p[:2] / p[2] - inl[:, 2:].T).max() < 5 * 0.5
    again = S.problem_h_local(2000, 0.9, seed=3)
    assert np.array_equal(corr, again[0]) and np.array_equal(truth, again[1])
    assert not np.array_equal(corr, S.problem_h_local(2000, 0.9, seed=4)[0])


# ------------------------------------- what the GPU whole-run test rests on ----
def test_whole_run_problem_conditions():
    """On every fixed seed the host generator's winning samples of the first 64
    slots include an all-truth-inlier one under NAPSAC -- the first of them
    inside the run's budget of 64 iterations -- and none under uniform
    sampling."""
    T = NC.e2e_iterations()
    for seed in NC.E2E_SEEDS:
        corr, truth, thr = NC.e2e_problem(seed)
        assert int(truth.sum()) == round((1.0 - NC.E2E_OUTLIERS) * NC.E2E_N)
        inc, _ = NC.host_generate(NC.H4, corr, NC.EXTENT, T, seed, 0, 64)
        hits, spent, first_cost = [], 0, None
        for s in range(64):
            a = int(inc[s, 0])
            spent += a
            if a > 101:
                continue
            idx = NC.host_samples(seed, s, 1, a - 1, corr, 4, NC.EXTENT, T)[0]
            assert len(G.solve_minimal(NC.H4, corr, idx)) == 1
            if truth[idx].all():
                hits.append(s)
                first_cost = spent if first_cost is None else first_cost
        uniform = [s for s, a, idx in NC.host_generate_uniform_h(corr, seed, 0, 64) if truth[idx].all()]
        print(f"seed {seed}: NAPSAC all-inlier winning samples at slots {hits[:8]} ... ({len(hits)} of 64), the first "
              f"after {first_cost} iterations; uniform: {uniform}")
        assert hits and first_cost <= NC.E2E_BUDGET, (seed, hits, first_cost)
        assert not uniform, (seed, uniform)
