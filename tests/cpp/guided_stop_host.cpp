// guided_stop.h on the host, for a sanitizer build: the quanta of extreme
// weight vectors stay in range (every conversion to uint64_t is of a value in
// [0, 2^K], every partial sum below 2^52, so (double) of it is exact), and with
// equal weights the guided stop is the uniform stop for every inlier count.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../graph-cut-ransac_amd/csrc/guided_stop.h"

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

int main() {
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    unsigned long long checks = 0, bad = 0;
    const uint64_t sizes[] = {1, 7, 255, 256, 10007, (1ull << 20) - 1, 1ull << 20, (1ull << 22) + 3};
    for (uint64_t n : sizes)
        for (int pat = 0; pat < 6; ++pat) {
            std::vector<double> w(n);
            for (uint64_t i = 0; i < n; ++i) {
                switch (pat) {
                    case 0: w[i] = 1.0; break;
                    case 1: w[i] = U(rng); break;
                    case 2: w[i] = (i % 5 == 0) ? 1.0 : 0.05; break;
                    case 3: w[i] = (i == n / 2) ? 1.0 : 1e-300; break;                    // one weight dominates
                    case 4: w[i] = (i % 3 == 0) ? 0.0 : 1e300 / (double)n; break;          // zeros, a sum near DBL_MAX
                    default: w[i] = std::pow(10.0, -300.0 + 600.0 * U(rng)) / (double)n; break;
                }
            }
            double total = 0.0;
            for (double x : w) total = total + x;                                       // as build_guided sums it
            if (!(total > 0.0) || !std::isfinite(total)) continue;      // weights the engine refuses (build_guided)
            const int K = guided_quanta_shift(n);
            const uint64_t cap = 1ull << K;
            uint64_t Q = 0, first = 0;
            bool equal = true;
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t q = guided_quantum(w[i], total, K);
                if (i == 0) first = q;
                equal = equal && q == first;
                bad += q > cap;
                bad += w[i] == 0.0 && q != 0;                                          // no weight, no mass
                bad += q == 0 && w[i] / total >= std::ldexp(1.0, -K);                  // zero only below one quantum
                Q += q;
                bad += Q >= (1ull << 52);
                bad += static_cast<uint64_t>(static_cast<double>(Q)) != Q;              // exact in fp64
                checks += 5;
            }
            if (pat == 0) {
                bad += !equal || first == 0 || Q != n * first;
                // equal weights: the uniform stop, bit for bit, for every inlier count
                // (every 97th at the large sizes)
                const uint64_t step = n > 20000 ? 97 : 1;
                for (uint32_t m : {4u, 7u})
                    for (double conf : {0.95, 0.99}) {
                        const double lp = std::log(1.0 - conf);
                        for (uint64_t inl = 0; inl <= n; inl += (inl + step > n && inl < n) ? n - inl : step) {
                            bad += iteration_number_guided(inl * first, Q, m, lp) != uniform_number(inl, n, m, lp);
                            ++checks;
                        }
                    }
            }
        }
    std::printf("checks %llu mismatches %llu\n", checks, bad);
    return bad == 0 ? 0 : 1;
}
