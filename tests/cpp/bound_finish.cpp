// The bound path's rounding guard (csrc/bound.h), restated on the host.
//
// A slot's raw accumulators are three sequential fp64 sums of -r^2 over its
// inliers (r^2 <= T_c): v0 over the scale inliers, v1 over the orientation
// inliers, tot over both (scale first).  Its finished score is
//   tot - v0 + (v0 / T0 + n0) - v1 + (v1 / T1 + n1),
// at most n0 + n1 in real arithmetic.  The bound path drops a slot whose
// pre-band count ub0 + ub1 >= n0 + n1 satisfies ub0 + ub1 + 1 <= S, so the
// computed finish must stay below n0 + n1 + 1 -- and, by the bound written in
// bound.h, within finish_excess(n0 + n1, T0, T1) of n0 + n1 -- wherever
// guard_holds() lets the path run.  Checked here over random accumulators
// and over the patterns that round worst: all-zero residuals, every residual
// at T, a long run of large values followed by values far below its ulp, and
// all of them at the largest N the guard admits for several T.  Past that N,
// and for thresholds that are zero, negative or not finite, guard_holds()
// must refuse (the call then takes the fused path).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "bound.h"

using gcr::bnd::finish;
using gcr::bnd::finish_excess;
using gcr::bnd::guard_holds;

static int failures = 0;
static double worst = 0.0;       // largest excess over n0 + n1 seen, as a share of finish_excess

// value generators: the i-th squared residual of a class
template <class F0, class F1>
static void check(const char* what, uint64_t n0, uint64_t n1, double T0, double T1, int classes, F0&& r0, F1&& r1) {
    double v0 = 0.0, v1 = 0.0, tot = 0.0;
    for (uint64_t i = 0; i < n0; ++i) {
        const double v = -r0(i);
        v0 += v;
        tot += v;
    }
    if (classes == 2)
        for (uint64_t i = 0; i < n1; ++i) {
            const double v = -r1(i);
            v1 += v;
            tot += v;
        }
    else
        n1 = 0;
    const double f = finish(tot, v0, v1, (uint32_t)n0, (uint32_t)n1, 0, 0, T0, T1, classes);
    const double N = (double)(n0 + n1);
    const double ex = finish_excess(n0 + n1, T0, classes == 2 ? T1 : T0);
    if (!(f <= N + 1.0) || !(f - N <= ex)) {
        std::printf("FAIL %s: n0 %llu n1 %llu T0 %a T1 %a finish %.17g excess %.3g bound %.3g\n", what,
                    (unsigned long long)n0, (unsigned long long)n1, T0, T1, f, f - N, ex);
        ++failures;
    }
    if (ex > 0.0 && (f - N) / ex > worst) worst = (f - N) / ex;
}

static uint64_t guard_edge(double T0, double T1, int classes) {
    uint64_t lo = 1, hi = (1ull << 31) - 1;             // guard_holds(lo), largest N that holds
    if (!guard_holds(lo, T0, T1, classes)) return 0;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (guard_holds(mid, T0, T1, classes)) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

static void patterns(const char* tag, uint64_t n0, uint64_t n1, double T0, double T1, int classes) {
    char what[96];
    auto name = [&](const char* p) {
        std::snprintf(what, sizeof what, "%s/%s", tag, p);
        return what;
    };
    check(name("zero"), n0, n1, T0, T1, classes, [](uint64_t) { return 0.0; }, [](uint64_t) { return 0.0; });
    check(name("at T"), n0, n1, T0, T1, classes, [&](uint64_t) { return T0; }, [&](uint64_t) { return T1; });
    check(name("just below T"), n0, n1, T0, T1, classes, [&](uint64_t) { return std::nextafter(T0, 0.0); },
          [&](uint64_t) { return std::nextafter(T1, 0.0); });
    // large values first, then values below the running sum's ulp: tot loses
    // them one by one, v1 keeps them
    for (int k : {30, 52, 53, 60}) {
        char p[32];
        std::snprintf(p, sizeof p, "T then T 2^-%d", k);
        check(name(p), n0, n1, T0, T1, classes, [&](uint64_t) { return T0; },
              [&](uint64_t) { return std::ldexp(T1, -k); });
        check(name(p), n0, n1, T0, T1, classes, [&](uint64_t i) { return i < n0 / 2 ? T0 : std::ldexp(T0, -k); },
              [&](uint64_t i) { return (i & 1) ? T1 : std::ldexp(T1, -k); });
    }
    // odd mantissas: every addition rounds
    check(name("odd"), n0, n1, T0, T1, classes, [&](uint64_t i) { return T0 * (0.5 + 0x1p-53 * (double)(2 * (i % 1000) + 1)); },
          [&](uint64_t i) { return T1 * (0.25 + 0x1p-53 * (double)(2 * (i % 977) + 1)); });
}

int main() {
    std::mt19937_64 rng(20251121);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    // random accumulators
    for (int it = 0; it < 4000; ++it) {
        const int classes = 1 + (int)(rng() & 1);
        const uint64_t n0 = rng() % 6000, n1 = rng() % 6000;
        const double T0 = std::exp((U(rng) * 2.0 - 1.0) * 30.0), T1 = std::exp((U(rng) * 2.0 - 1.0) * 30.0);
        if (!guard_holds(n0 + (classes == 2 ? n1 : 0), T0, T1, classes)) continue;
        const int mode = (int)(rng() % 3);
        auto draw = [&](double T) {
            const double u = U(rng);
            if (mode == 0) return u * T;
            if (mode == 1) return (u < 0.1 ? 0.0 : u < 0.2 ? T : u * u * u * T);
            return std::ldexp(T, -(int)(u * 60.0));
        };
        check("random", n0, n1, T0, T1, classes, [&](uint64_t) { return draw(T0); }, [&](uint64_t) { return draw(T1); });
    }
    // the bench's shape and the patterns at moderate sizes
    patterns("5000+5000", 5000, 5000, 2.25 * 0.05 * 0.05, 2.25 * 0.0174 * 0.0174, 2);
    patterns("10000", 10000, 0, 2.25 * 0.05 * 0.05, 0.0, 1);
    patterns("tiny T", 3000, 3000, 2.25e-320, 2.25e-320, 2);
    // N and T at the guard's edge
    for (double T : {1.0, 0x1p10, 0x1p20, 0x1p30}) {
        for (int classes = 1; classes <= 2; ++classes) {
            const uint64_t N = guard_edge(T, T, classes);
            char tag[64];
            std::snprintf(tag, sizeof tag, "edge T=%g K=%d N=%llu", T, classes, (unsigned long long)N);
            if (N == 0 || guard_holds(N + 1, T, T, classes) || !(finish_excess(N, T, T) <= 0.5)) {
                std::printf("FAIL %s: no edge\n", tag);
                ++failures;
                continue;
            }
            if (classes == 1) patterns(tag, N, 0, T, T, 1);
            else patterns(tag, N / 2, N - N / 2, T, T, 2);
            // unequal thresholds at the same N
            if (classes == 2 && guard_holds(N, T, T * 0x1p-12, 2)) patterns(tag, N / 2, N - N / 2, T, T * 0x1p-12, 2);
        }
    }
    // past the edge and outside the thresholds' range the host check refuses
    const uint64_t e1 = guard_edge(1.0, 1.0, 2);
    const double bad[] = {0.0, -1.0, NAN, INFINITY, -0.0};
    if (guard_holds(e1 + 1, 1.0, 1.0, 2) || guard_holds(e1, 4.0, 1.0, 2) || guard_holds(e1, 1.0, 4.0, 2) ||
        guard_holds(1ull << 31, 1e-300, 1e-300, 1) || !guard_holds(10000, 0.005625, 0.00068, 2)) {
        std::printf("FAIL guard edge\n");
        ++failures;
    }
    for (double b : bad) {
        if (guard_holds(100, b, 1.0, 1) || guard_holds(100, b, 1.0, 2) || guard_holds(100, 1.0, b, 2)) {
            std::printf("FAIL guard accepts threshold %g\n", b);
            ++failures;
        }
        if (!guard_holds(100, 1.0, b, 1)) {            // one class: T1 is not used
            std::printf("FAIL guard tests an unused threshold %g\n", b);
            ++failures;
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK worst excess / bound %.3g\n", worst);
    return 0;
}
