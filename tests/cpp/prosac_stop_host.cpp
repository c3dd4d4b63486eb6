// prosac_stop.h on the host, for a sanitizer build: the tables stay in range
// (every conversion to uint32_t is of a small positive value, every table read
// inside its n + 1 entries), the choice agrees with a plain restatement at
// N = m, N = 20, n = N - 1 and under random masks, the order's products do
// not overflow at the largest counts, and n* = N gives the uniform stop.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../graph-cut-ransac_amd/csrc/prosac.h"
#include "../../graph-cut-ransac_amd/csrc/prosac_stop.h"

using namespace gcr;

// GCRANSAC::getIterationNumber (GCRANSAC.h:738-757), one class
static uint64_t uniform_number(uint64_t inl, uint64_t n, uint32_t m, double log_prob) {
    const double ratio = static_cast<double>(inl) / static_cast<double>(n);
    double q = 1.0;
    q *= std::pow(ratio, static_cast<double>(m));
    const double lg = std::log(1 - q);
    if (std::fabs(lg) < std::numeric_limits<double>::epsilon()) return std::numeric_limits<uint64_t>::max();
    return static_cast<uint64_t>(std::ceil(log_prob / lg));
}

// the definition again, candidates listed first and compared afterwards
static void choose_plain(const std::vector<uint8_t>& mask, uint32_t m, const std::vector<uint32_t>& imin,
                         const std::vector<double>& qmin, uint32_t* bi, uint32_t* bn) {
    const uint32_t n = (uint32_t)mask.size();
    std::vector<uint32_t> cum(n + 1, 0);
    for (uint32_t k = 1; k <= n; ++k) cum[k] = cum[k - 1] + (mask[k - 1] ? 1u : 0u);
    uint32_t I = cum[n], L = n;
    for (uint32_t k = m > kProsacStopMinLength ? m : kProsacStopMinLength; k < n; ++k) {
        if (cum[k] < imin.at(k)) continue;
        const double r = (double)cum[k] / (double)k;
        double q = r;
        for (uint32_t j = 1; j < m; ++j) q = q * r;
        if (!(q >= qmin.at(k))) continue;
        const unsigned __int128 l = (unsigned __int128)cum[k] * L, rr = (unsigned __int128)I * k;
        if (l > rr || (l == rr && k > L)) {
            I = cum[k];
            L = k;
        }
    }
    *bi = I;
    *bn = L;
}

int main() {
    std::mt19937_64 rng(13);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    unsigned long long checks = 0, bad = 0;
    const double confs[] = {0.95, 0.99};
    const uint64_t convs[] = {1, 1000, 100000, kProsacMaxConvergence};
    for (uint32_t m : {2u, 3u, 4u, 5u, 7u})
        for (uint32_t n : {m, 19u, 20u, 21u, 63u, 64u, 65u, 257u, 2000u, 10007u}) {
            if (n < m) continue;
            for (uint64_t conv : convs)
                for (double conf : confs) {
                    const double lp = std::log(1.0 - conf);
                    std::vector<uint64_t> g(n + 1);
                    prosac_growth(n, m, conv, g.data());
                    std::vector<uint32_t> imin(n + 1, 77);
                    std::vector<double> qmin(n + 1, 77.0);
                    prosac_stop_tables(g.data(), n, m, lp, imin.data(), qmin.data());
                    for (uint32_t k = 0; k <= n; ++k) {
                        if (k < m) {
                            bad += imin[k] != 0 || qmin[k] != 0.0;
                        } else {
                            bad += imin[k] <= m || imin[k] > m + k;          // at most every row and the sample
                            bad += !(qmin[k] > 0.0 && qmin[k] < 1.0);
                            bad += k > m && (imin[k] < imin[k - 1] || qmin[k] > qmin[k - 1]);
                        }
                        checks += 3;
                    }
                    // masks: none, all, all but the last row (n* = N - 1 where it
                    // qualifies), the first row only, random ones crowding the top
                    for (int pat = 0; pat < 8; ++pat) {
                        std::vector<uint8_t> mask(n, 0);
                        for (uint32_t i = 0; i < n; ++i) {
                            switch (pat) {
                                case 0: mask[i] = 0; break;
                                case 1: mask[i] = 1; break;
                                case 2: mask[i] = i + 1 < n; break;
                                case 3: mask[i] = i == 0; break;
                                default: mask[i] = U(rng) < 0.3 * pat * std::exp(-3.0 * i / n); break;
                            }
                        }
                        uint32_t bi = 0, bn = 0, wi = 0, wn = 0;
                        prosac_stop_choose(mask.data(), n, m, imin.data(), qmin.data(), &bi, &bn);
                        choose_plain(mask, m, imin, qmin, &wi, &wn);
                        bad += bi != wi || bn != wn;
                        bad += bn == 0 || bn > n || bi > bn;
                        if (pat == 2 && n > kProsacStopMinLength && n - 1 >= m)
                            bad += bn != n - 1 || bi != n - 1;                // share 1 over the first N - 1 rows
                        if (n <= kProsacStopMinLength) bad += bn != n;       // N <= 20: only n = N
                        // never above the uniform stop
                        uint32_t I = 0;
                        for (uint8_t b : mask) I += b;
                        const uint64_t u = uniform_number(I, n, m, lp);
                        bad += iteration_number_prosac(bi, bn, m, lp) > u;
                        bad += iteration_number_prosac(I, n, m, lp) != u;
                        checks += 6;
                    }
                }
        }
    // the order at the largest counts: products near 2^64 stay exact
    const uint32_t big = 0xfffffffeu;
    bad += !prosac_stop_better(big, big, big - 1, big);                     // a larger share
    bad += prosac_stop_better(big - 1, big, big, big);
    bad += !prosac_stop_better(big, big, big - 1, big - 1);                 // equal shares: the larger length
    bad += prosac_stop_better(big - 1, big - 1, big, big);
    bad += prosac_stop_better(big, big, big, big);                          // irreflexive
    bad += !prosac_stop_better(1, 2, 0, 1) || prosac_stop_better(0, 1, 0, 2);
    bad += !prosac_stop_feasible(big, big, 32, big, 1.0);                   // share 1 meets any qmin <= 1
    bad += prosac_stop_feasible(big - 1, big, 2, big, 0.0);                 // below Imin
    bad += prosac_stop_imin(big, 32) <= 32;
    checks += 9;
    std::printf("checks %llu mismatches %llu\n", checks, bad);
    return bad == 0 ? 0 : 1;
}
