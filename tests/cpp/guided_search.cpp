// guided.h's two-level search against the flat search and (N <= 1000) against
// a linear scan of the definition, at the values of u that sampling itself
// almost never produces: every CDF entry and its two neighbours, 0, the total (u rounded up:
// the "smallest i with c[i] == total" rule) and the value below it.  Tables in
// exact-size heap blocks, so a sanitizer build sees any read past their ends.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../graph-cut-ransac_amd/csrc/guided.h"

using namespace gcr;

static uint32_t linear(const std::vector<double>& c, double total, double u) {
    for (uint32_t i = 0; i < c.size(); ++i)
        if (c[i] > u) return i;
    for (uint32_t i = 0; i < c.size(); ++i)
        if (c[i] == total) return i;
    return 0xffffffffu;
}

int main() {
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const uint32_t sizes[] = {1, 2, 7, 8, 255, 256, 257, 511, 512, 513, 1000, 10007, 70001};
    unsigned long long checks = 0, bad = 0;
    for (uint32_t n : sizes)
        for (int pat = 0; pat < 6; ++pat) {
            std::vector<double> w(n);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t run = n / 4 < 37 ? (n / 4 ? n / 4 : 1) : 37;
                switch (pat) {
                    case 0: w[i] = 1.0; break;
                    case 1: w[i] = ((i / run) & 1) ? 0.0 : 0.5 + U(rng); break;          // zero runs, maybe trailing
                    case 2: w[i] = ((i / run) & 1) ? 0.5 + U(rng) : 0.0; break;          // leading zeros
                    case 3: w[i] = std::pow(10.0, -300.0 + 600.0 * U(rng)) / n; break;   // absorbed increments
                    case 4: w[i] = i == n / 2 ? 1.0 : (i % 3 ? 0.0 : 1e-18); break;      // one heavy entry
                    default: w[i] = U(rng) < 0.9 ? 0.0 : U(rng); break;                  // sparse
                }
            }
            if (pat != 0) w[n - 1 - (n > 1 && pat == 1)] += 0.25;                       // total > 0
            // the engine's table (engine.cpp build_guided)
            std::vector<double> c(n);
            double acc = 0.0;
            for (uint32_t i = 0; i < n; ++i) { acc = acc + w[i]; c[i] = acc; }
            GuidedTable t;
            t.n = n;
            t.stride = guided_stride(n);
            t.buckets = guided_buckets(n);
            t.total = acc;
            std::vector<double> coarse(t.buckets);
            for (uint32_t k = 0; k < t.buckets; ++k) {
                const size_t e = (size_t)(k + 1) * t.stride;
                coarse[k] = c[(e < n ? e : n) - 1];
            }
            t.cdf = c.data();
            t.coarse = coarse.data();
            if (t.buckets == 0 || t.buckets > kGuidedCoarse || (size_t)t.stride * t.buckets < n ||
                (size_t)t.stride * (t.buckets - 1) >= n) {
                std::printf("bad table shape n=%u S=%u B=%u\n", n, t.stride, t.buckets);
                return 1;
            }
            std::vector<double> us = {0.0, acc, std::nextafter(acc, 0.0)};
            for (uint32_t i = 0; i < n; ++i) {
                us.push_back(c[i]);
                us.push_back(std::nextafter(c[i], 0.0));
                if (c[i] < acc) us.push_back(std::nextafter(c[i], INFINITY));
            }
            for (int k = 0; k < 4096; ++k) us.push_back(guided_u(rng(), acc));
            us.push_back(guided_u(~0ull, acc));
            for (double u : us) {
                if (!(u >= 0.0 && u <= acc)) continue;
                const uint32_t a = guided_index(t, t.coarse, u), b = guided_index_flat(c.data(), n, acc, u),
                               d = n <= 1000 ? linear(c, acc, u) : b;     // (the scan is O(n) per value)
                ++checks;
                if (a != b || a != d || a >= n || !(w[a] > 0.0)) {
                    if (bad++ < 10)
                        std::printf("n=%u pat=%d u=%a: two-level %u flat %u linear %u\n", n, pat, u, a, b, d);
                }
            }
        }
    std::printf("checks %llu mismatches %llu\n", checks, bad);
    return bad ? 1 : 0;
}
