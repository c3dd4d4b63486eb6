"""The guided stop (GCR_FLAG_GUIDED_STOP, csrc/guided_stop.h) on the host: the
weights' quanta and the stop function against Python restatements of the
header, and the errors of the Python keyword and the host entries."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import guided_cases as G
import pygcransac
from pygcransac import _native as N
from pygcransac import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
U64_MAX = 2 ** 64 - 1


def host_quanta(w, m):
    """gcr_host_guided_quanta: (rc, q as Python ints, Q)."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    q = np.zeros(len(w), dtype=np.uint64)
    Q = C.c_uint64()
    rc = N.lib.gcr_host_guided_quanta(w.ctypes.data, len(w), m, q.ctypes.data_as(u64p), C.byref(Q))
    return rc, [int(v) for v in q], Q.value


def host_iterations(mass, Q, m, conf):
    out = C.c_uint64()
    rc = N.lib.gcr_host_guided_iterations(mass, Q, m, conf, C.byref(out))
    return rc, out.value


def ref_quanta(w):
    """guided_stop.h restated with Python integers."""
    n = len(w)
    K = 52 - int(n).bit_length()
    total = float(G.cdf_of(w)[-1])              # the CDF's last entry, summed as build_guided sums it
    return [int(float(wi) / total * float(2 ** K)) for wi in w]


def ref_iteration_number(inliers, n, m, conf):
    """GCRANSAC::getIterationNumber (GCRANSAC.h:738-757) for one class."""
    ratio = inliers / n                         # int / int: correctly rounded
    q = 1.0 * math.pow(ratio, float(m))
    lg = math.log(1 - q) if 1 - q > 0 else -math.inf
    if abs(lg) < np.finfo(np.float64).eps:
        return U64_MAX
    return int(math.ceil(math.log(1 - conf) / lg))


# ---------------------------------------------------------------- quanta ----
@pytest.mark.parametrize("n", G.NS)
@pytest.mark.parametrize("pattern", G.PATTERNS)
def test_quanta_equal_the_restatement(pattern, n):
    for m in (4, 7):
        w = G.weights(pattern, n, m)
        rc, q, Q = host_quanta(w, m)
        if int((w > 0).sum()) < m:
            assert rc == N.GCR_EINVAL, (pattern, n, m)
            continue
        assert rc == N.GCR_OK, (pattern, n, m, N.last_error())
        want = ref_quanta(w)
        assert q == want, (pattern, n, m)
        assert Q == sum(want) and Q < 2 ** 52
        assert all(qi == 0 for qi, wi in zip(q, w) if wi == 0.0)          # a zero weight has no mass
        assert all(qi <= 2 ** (52 - int(n).bit_length()) for qi in q)
        if pattern == "ones":
            assert len(set(q)) == 1 and q[0] > 0                          # equal weights: equal quanta
        if pattern == "heavy90":                                          # ... also beside an unequal one
            rest = q[:n // 2] + q[n // 2 + 1:]
            assert len(set(rest)) == 1 and q[n // 2] > rest[0] > 0


def test_equal_quanta_for_equal_weights_of_any_value():
    for value in (1e-300, 0.05, 1.0, 3.0, 1e300 / 4096):
        w = np.full(1000, value)
        rc, q, Q = host_quanta(w, 7)
        assert rc == N.GCR_OK and len(set(q)) == 1 and Q == 1000 * q[0] and q[0] > 0, value


# --------------------------------------------------------- stop function ----
@pytest.mark.parametrize("n", (7, 256, 10007))
def test_equal_weights_give_the_uniform_stop(n):
    rc, q, Q = host_quanta(np.ones(n), 4)
    assert rc == N.GCR_OK and Q == n * q[0]
    q1 = q[0]
    for m in (4, 7):
        for conf in (0.95, 0.99):
            for inl in range(n + 1):
                rc, got = host_iterations(inl * q1, Q, m, conf)
                assert rc == N.GCR_OK
                assert got == ref_iteration_number(inl, n, m, conf), (n, m, conf, inl)


def test_stop_function_branches():
    rc, q, Q = host_quanta(np.ones(100), 4)
    for m in (4, 7):
        for conf in (0.95, 0.99):
            assert host_iterations(0, Q, m, conf) == (N.GCR_OK, U64_MAX)      # the epsilon guard
            assert host_iterations(Q, Q, m, conf) == (N.GCR_OK, 0)            # log(0): ceil(-0 ...) = 0
            assert host_iterations(q[0], Q, m, conf) == (N.GCR_OK, ref_iteration_number(1, 100, m, conf))
    # a ratio the guard does not catch is a finite count, decreasing in the mass
    its = [host_iterations(k * Q // 10, Q, 7, 0.99)[1] for k in range(1, 11)]
    assert all(a >= b for a, b in zip(its, its[1:])) and its[-1] == 0
    # the issue's arithmetic: a model holding 0.75 of the mass needs 33 iterations at m = 7
    assert host_iterations(3 * Q // 4, Q, 7, 0.99)[1] == ref_iteration_number(3, 4, 7, 0.99) == 33


def test_uniform_bounds_of_the_gpu_tests_shapes():
    """tests/test_gpu_guided_stop.py asserts that flag-clear runs reach
    max_iters = 5000: the reference's bound at each shape's inlier share."""
    assert ref_iteration_number(400, 2000, 7, 0.99) > 5000        # F, 80 % outliers: 3.6e5
    assert ref_iteration_number(400, 2000, 4, 0.99) < 5000        # H at 80 % would stop on its own (2876)
    assert ref_iteration_number(330, 2000, 4, 0.99) > 5000        # H, 85 % outliers (+10 % chance inliers)


def test_header_under_sanitizers(tmp_path):
    """tests/cpp/guided_stop_host.cpp: guided_stop.h's quanta and stop function
    in a stand-alone host program built with ASan + UBSan (float-cast-overflow
    included): every conversion in range at N up to 2^22 and weights from
    1e-300 to a sum near DBL_MAX, every partial sum exact in fp64, equal
    weights the uniform stop for every inlier count."""
    exe = str(tmp_path / "guided_stop_host")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "cpp", "guided_stop_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout


# ---------------------------------------------------------------- errors ----
def test_python_keyword_errors():
    corr, truth, _, thr = S.problem_h(200, 0.5, seed=5)
    for fn in (pygcransac.findHomography, pygcransac.findFundamentalMatrix):
        with pytest.raises(ValueError, match="guided_stop"):
            fn(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, threshold=thr, sampler=0, guided_stop=True)
        with pytest.raises(TypeError):                      # keyword-only
            fn(corr, S.IMG_H, S.IMG_W, S.IMG_H, S.IMG_W, None, thr, 0.99, 0.0, 100, 50, 0, 50, 8, 0, None, 0,
               False, True)


def test_host_entry_errors():
    w = np.ones(10)
    q = np.zeros(10, dtype=np.uint64)
    Q = C.c_uint64()
    qp = q.ctypes.data_as(u64p)
    assert N.lib.gcr_host_guided_quanta(None, 10, 4, qp, C.byref(Q)) == N.GCR_EINVAL
    assert N.lib.gcr_host_guided_quanta(w.ctypes.data, 10, 4, None, C.byref(Q)) == N.GCR_EINVAL
    assert N.lib.gcr_host_guided_quanta(w.ctypes.data, 10, 4, qp, None) == N.GCR_EINVAL
    assert N.lib.gcr_host_guided_quanta(w.ctypes.data, 0, 4, qp, C.byref(Q)) == N.GCR_EINVAL
    assert N.lib.gcr_host_guided_quanta(w.ctypes.data, 3, 4, qp, C.byref(Q)) == N.GCR_EINVAL     # fewer than m
    bad = w.copy()
    bad[3] = -1.0
    assert N.lib.gcr_host_guided_quanta(bad.ctypes.data, 10, 4, qp, C.byref(Q)) == N.GCR_EINVAL
    out = C.c_uint64()
    assert N.lib.gcr_host_guided_iterations(1, 2, 4, 0.99, None) == N.GCR_EINVAL
    assert N.lib.gcr_host_guided_iterations(1, 0, 4, 0.99, C.byref(out)) == N.GCR_EINVAL         # Q == 0
    assert N.lib.gcr_host_guided_iterations(3, 2, 4, 0.99, C.byref(out)) == N.GCR_EINVAL         # mass > Q
    assert N.lib.gcr_host_guided_iterations(1, 2 ** 52, 4, 0.99, C.byref(out)) == N.GCR_EINVAL
    assert "guided stop" in N.last_error()
    assert N.FLAG_GUIDED_STOP == 2 and N.FLAG_NO_LO == 1
