"""NAPSAC sampling (csrc/napsac.h): the definition restated in numpy, the host
twins' wrappers and the whole-run problems shared by test_napsac.py (CPU) and
test_gpu_napsac.py."""
import ctypes as C

import numpy as np

import guided_cases as G
from pygcransac import _native as N
from pygcransac import synthetic as S

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
dpt = C.POINTER(C.c_double)
ALL_ONES = 0xFFFFFFFF

H4, F7, E5, G3, S2 = (N.SOLVER_HOMOGRAPHY4, N.SOLVER_FUNDAMENTAL7, N.SOLVER_ESSENTIAL5,
                      N.SOLVER_ESSENTIAL3_GRAVITY, N.SOLVER_HOMOGRAPHY2_SIFT)
SOLVERS = (H4, F7, E5, G3, S2)
M_OF = {H4: 4, F7: 7, E5: 5, G3: 3, S2: 2}
PER_OF = {H4: 1, F7: 3, E5: 10, G3: 4, S2: 3}
CELLS = (16, 8, 4, 2)
EXTENT = (S.IMG_W, S.IMG_H, S.IMG_W, S.IMG_H)
MAX_ITERATIONS = 1 << 40


def _extent(extent):
    return (C.c_double * 4)(*[float(v) for v in extent])


# ---- the definition, restated -------------------------------------------------
def axis_index(v):
    """graphcut.h grid_axis_index: floor(v) as a 64-bit two's-complement value,
    2^63 when out of range or not a number"""
    f = np.floor(v)
    ok = (f >= -9.2233720368547758e18) & (f < 9.2233720368547758e18)
    out = np.full(f.shape, 1 << 63, dtype=np.uint64)
    out[ok] = f[ok].astype(np.int64).view(np.uint64)
    return out


def layer_ref(rows, extent, cells):
    """One grid layer: (members, start, count, pos).  Keys floor(coord / size)
    combined in 64-bit wrapping arithmetic, a stable sort by key."""
    rows = np.asarray(rows, dtype=np.float64)
    n = len(rows)
    key = np.zeros(n, dtype=np.uint64)
    off = np.uint64(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for d in range(4):
            size = float(extent[d]) / float(cells)
            key = key + off * axis_index(rows[:, d] / size)
            off = off * np.uint64(cells)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    first = np.r_[True, ks[1:] != ks[:-1]]
    begin = np.flatnonzero(first)
    cell = np.cumsum(first) - 1
    size_of = np.diff(np.r_[begin, n])
    start, count, pos = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    start[order] = begin[cell]
    count[order] = size_of[cell]
    pos[order] = np.arange(n) - begin[cell]
    return order.astype(np.uint32), start, count, pos


def layers_ref(rows, extent):
    return [layer_ref(rows, extent, c) for c in CELLS]


def pick_layer(layers, i0, slot, T, m):
    """the finest layer >= floor(4 slot / T) whose cell of i0 holds >= m rows, else 4"""
    for l in range(4 * slot // T, 4):
        if layers[l][2][i0] >= m:
            return l
    return 4


def cell_rows(layers, l, i0, n):
    if l == 4:
        return np.arange(n, dtype=np.uint32)
    members, start, count, _ = layers[l]
    return members[start[i0]:start[i0] + count[i0]]


def ref_sample(layers, seed, slot, attempt, n, m, T):
    """napsac.h's sample from Philox words (the oracle's) and mulhi64, or None
    when the draw budget runs out"""
    words = G.words(seed, slot, attempt)
    drawn = 0

    def draw(k):
        nonlocal drawn
        if drawn >= G.K_MAX_DRAWS:
            return None
        drawn += 1
        return (next(words) * k) >> 64

    i0 = draw(n)
    if slot >= T:
        out = [i0]
        while len(out) < m:
            v = draw(n)
            if v is None:
                return None
            if v not in out:
                out.append(v)
        return out
    l = pick_layer(layers, i0, slot, T, m)
    cell = cell_rows(layers, l, i0, n)
    pos = int(layers[l][3][i0]) if l < 4 else i0
    rs = []
    while len(rs) < m - 1:
        v = draw(len(cell) - 1)
        if v is None:
            return None
        if v not in rs:
            rs.append(v)
    return [i0] + [int(cell[r + (1 if r >= pos else 0)]) for r in rs]


# ---- host twins ---------------------------------------------------------------
def host_layers(rows, extent):
    """gcr_host_napsac_layers: per layer (members, start, count, pos)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n = len(rows)
    mem, start, count, pos = (np.zeros((4, n), dtype=np.uint32) for _ in range(4))
    N.check(N.lib.gcr_host_napsac_layers(rows.ctypes.data_as(dpt), n, _extent(extent), mem.ctypes.data_as(u32p),
                                         start.ctypes.data_as(u32p), count.ctypes.data_as(u32p),
                                         pos.ctypes.data_as(u32p)))
    return [(mem[l], start[l], count[l], pos[l]) for l in range(4)]


def host_sample(seed, slot, attempt, rows, m, extent, T):
    """gcr_host_sample_napsac: (rc, indices)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    out = np.zeros(m, dtype=np.uint32)
    rc = N.lib.gcr_host_sample_napsac(seed, slot, attempt, rows.ctypes.data_as(dpt), len(rows), m, _extent(extent), T,
                                      out.ctypes.data_as(u32p))
    return rc, out


def host_samples(seed, slot0, nslots, attempt, rows, m, extent, T):
    """gcr_host_samples_napsac: (nslots, m), all-ones rows where the budget ran out"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    out = np.zeros((nslots, m), dtype=np.uint32)
    N.check(N.lib.gcr_host_samples_napsac(seed, slot0, nslots, attempt, rows.ctypes.data_as(dpt), len(rows), m,
                                          _extent(extent), T, out.ctypes.data_as(u32p)))
    return out


def host_generate(solver, rows, extent, T, seed, slot0, nslots, pixels=None, sift=None, G1=None, G2=None, threads=3):
    """gcr_host_generate_napsac: inc (nslots, per), models (nslots, per, 9).
    rows: what the solver reads; pixels: what the layers lie over (None: rows)"""
    per = PER_OF[solver]
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (pixels, sift, G1, G2)]
    ptr = [None if a is None else a.ctypes.data_as(dpt) for a in keep]
    inc = np.zeros((nslots, per), dtype=np.uint8)
    models = np.zeros((nslots, per, 9))
    N.check(N.lib.gcr_host_generate_napsac(solver, rows.ctypes.data_as(dpt), ptr[0], ptr[1], ptr[2], ptr[3], len(rows),
                                           _extent(extent), T, seed, slot0, nslots, threads,
                                           inc.ctypes.data_as(u8p), models.ctypes.data_as(dpt)))
    return inc, models


def host_generate_uniform_h(rows, seed, slot0, nslots):
    """The uniform homography generator on the host: the first attempt whose
    sample (gcr_host_sample) yields a model (gcr_host_solve_minimal);
    [(slot, attempt, indices)] of the slots that have one."""
    n = len(rows)
    out = []
    for s in range(slot0, slot0 + nslots):
        for a in range(101):
            idx = np.zeros(4, dtype=np.uint32)
            rc = N.lib.gcr_host_sample(seed, s, a, 0, 0, n, 4, idx.ctypes.data_as(u32p))
            if rc == 0 and len(G.solve_minimal(H4, rows, idx)) > 0:
                out.append((s, a, idx))
                break
    return out


# ---- the rows of the layer test -----------------------------------------------
def edge_rows(n=300, seed=5):
    """n rows over EXTENT with points exactly on cell borders and on the
    extent, negative and beyond it, duplicates, and row 0 alone in its cell on
    every grid layer.  Returns (rows, the lone row)."""
    rng = np.random.default_rng(seed)
    e = np.array(EXTENT)
    rows = rng.uniform(0.0, 1.0, (n, 4)) * e
    rows[0] = 5.0 * e + 3.0                         # far outside: nobody shares its cell
    rows[1] = e                                     # on the extent
    rows[2] = e / 16.0 * np.array([3, 5, 7, 9])     # on borders of the finest layer
    rows[3] = e / 2.0                               # on a border of every layer
    rows[4] = 0.0
    rows[5] = [-0.5, -300.0, 10.0, 20.0]            # negative
    rows[6] = [e[0] + 0.25, 10.0, 2.0 * e[2], 20.0]  # beyond the extent
    rows[7:10] = rows[10]                           # duplicates
    rows[20:23, :2] = rows[23, :2]                  # ... and of one image's point only
    return np.ascontiguousarray(rows), 0


# ---- whole runs ---------------------------------------------------------------
# problem_h_local(2000, 0.9, seed): 200 inliers in a quarter x quarter window of
# image 1 among 1800 outliers, 64 iterations.  The data seeds are chosen on the
# CPU (test_napsac.py asserts both) so that, with run seed = data seed,
#   - under NAPSAC the winning samples of the first 64 slots include an
#     all-truth-inlier one,
#   - under uniform sampling they include none.
E2E_N = 2000
E2E_OUTLIERS = 0.9
E2E_BUDGET = 64
E2E_SEEDS = (0, 1, 2, 3, 4)


def e2e_problem(seed):
    """corr, truth, thr"""
    corr, truth, _, thr = S.problem_h_local(E2E_N, E2E_OUTLIERS, seed)
    return corr, truth, thr


def e2e_iterations():
    return (E2E_N + 1) // 2                         # napsac_iterations=None
