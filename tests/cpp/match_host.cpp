// Stand-alone host program over csrc/match.h (built with ASan + UBSan by
// tests/test_match_descriptors.py): the plain-loop definition on the crafted
// inputs, against a second formulation (sort of all (d, j) keys), and the
// argument check and the split planner at their edges.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "match.h"

using namespace gcr;

namespace {

int g_fail = 0;
#define EXPECT(c)                                                   \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                               \
        }                                                           \
    } while (0)

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

struct Out {
    std::vector<uint32_t> idx, dist, idx2, dist2;
    explicit Out(size_t n) : idx(n), dist(n), idx2(n), dist2(n) {}
};

void run(const std::vector<uint8_t>& d1, size_t n1, const std::vector<uint8_t>& d2, size_t n2, uint32_t dim, Out& o) {
    // exact-size copies: a read past either array is the sanitizer's to see
    std::vector<uint8_t> a(d1.begin(), d1.begin() + n1 * dim), b(d2.begin(), d2.begin() + n2 * dim);
    host_match_rows(a.data(), b.data(), n2, dim, 0, n1, o.idx.data(), o.dist.data(), o.idx2.data(), o.dist2.data());
}

// the same by sorting every row's keys
void check_sorted(const std::vector<uint8_t>& d1, size_t n1, const std::vector<uint8_t>& d2, size_t n2, uint32_t dim,
                  const Out& o) {
    for (size_t i = 0; i < n1; ++i) {
        std::vector<uint64_t> keys(n2);
        for (size_t j = 0; j < n2; ++j) {
            int64_t d = 0;
            for (uint32_t k = 0; k < dim; ++k) {
                const int64_t t = (int64_t)d1[i * dim + k] - (int64_t)d2[j * dim + k];
                d += t * t;
            }
            keys[j] = match_key((uint32_t)d, (uint32_t)j);
        }
        std::sort(keys.begin(), keys.end());
        EXPECT(o.idx[i] == (uint32_t)keys[0] && o.dist[i] == (uint32_t)(keys[0] >> 32));
        if (n2 > 1) EXPECT(o.idx2[i] == (uint32_t)keys[1] && o.dist2[i] == (uint32_t)(keys[1] >> 32));
        else EXPECT(o.idx2[i] == kMatchNone && o.dist2[i] == kMatchNone);
        // any split of the columns merged in any order gives the same pair
        for (size_t cut = 1; cut < n2; cut += 1 + n2 / 5) {
            auto top2 = [&](size_t lo, size_t hi, uint64_t& k1, uint64_t& k2) {
                k1 = k2 = ~0ull;
                for (size_t j = lo; j < hi; ++j) {
                    uint64_t one = ~0ull;
                    for (size_t q = 0; q < n2; ++q)
                        if ((uint32_t)keys[q] == j) one = keys[q];
                    match_merge(k1, k2, one, ~0ull);
                }
            };
            uint64_t a1, a2, b1, b2;
            top2(0, cut, a1, a2);
            top2(cut, n2, b1, b2);
            uint64_t x1 = a1, x2 = a2, y1 = b1, y2 = b2;
            match_merge(x1, x2, b1, b2);
            match_merge(y1, y2, a1, a2);
            EXPECT(x1 == keys[0] && y1 == keys[0]);
            EXPECT(x2 == (n2 > 1 ? keys[1] : ~0ull) && y2 == x2);
        }
    }
}

}  // namespace

int main() {
    for (uint32_t dim : {32u, 128u, 512u}) {
        // values around the sign shift only
        {
            const size_t n1 = 9, n2 = 21;
            const uint8_t vals[4] = {0, 127, 128, 255};
            std::vector<uint8_t> d1(n1 * dim), d2(n2 * dim);
            for (auto& v : d1) v = vals[rnd() & 3];
            for (auto& v : d2) v = vals[rnd() & 3];
            Out o(n1);
            run(d1, n1, d2, n2, dim, o);
            check_sorted(d1, n1, d2, n2, dim, o);
        }
        // all 0 against all 255: dist = dim * 255^2, first two indices
        {
            const size_t n1 = 3, n2 = 33;
            std::vector<uint8_t> d1(n1 * dim, 0), d2(n2 * dim, 255);
            Out o(n1);
            run(d1, n1, d2, n2, dim, o);
            for (size_t i = 0; i < n1; ++i) {
                EXPECT(o.idx[i] == 0 && o.idx2[i] == 1);
                EXPECT(o.dist[i] == dim * 255u * 255u && o.dist2[i] == dim * 255u * 255u);
            }
        }
        // duplicate rows in D2
        {
            const size_t n1 = 6, n2 = 18;
            std::vector<uint8_t> d1(n1 * dim), d2(n2 * dim);
            for (size_t j = 0; j < 6 * dim; ++j) d2[j] = d2[6 * dim + j] = d2[12 * dim + j] = (uint8_t)rnd();
            for (size_t j = 0; j < n1 * dim; ++j) d1[j] = d2[j];
            Out o(n1);
            run(d1, n1, d2, n2, dim, o);
            check_sorted(d1, n1, d2, n2, dim, o);
            for (size_t i = 0; i < n1; ++i) EXPECT(o.idx[i] == i && o.idx2[i] == i + 6 && o.dist[i] == 0 && o.dist2[i] == 0);
        }
        // D2 a rotation of D1; one column only
        {
            const size_t n = 11;
            std::vector<uint8_t> d1(n * dim), d2(n * dim);
            for (auto& v : d1) v = (uint8_t)rnd();
            for (size_t j = 0; j < n; ++j)
                for (uint32_t k = 0; k < dim; ++k) d2[j * dim + k] = d1[((j + 4) % n) * dim + k];
            Out o(n);
            run(d1, n, d2, n, dim, o);
            for (size_t i = 0; i < n; ++i) EXPECT(o.dist[i] == 0 && o.idx[i] == (i + n - 4) % n);
            Out o1(n);
            run(d1, n, d2, 1, dim, o1);
            check_sorted(d1, n, d2, 1, dim, o1);
        }
    }
    // arguments
    uint8_t b = 0;
    uint32_t u = 0;
    EXPECT(match_check_args(&b, 1, &b, 1, 32, &u, &u, &u, &u) == nullptr);
    EXPECT(match_check_args(nullptr, 1, &b, 1, 32, &u, &u, &u, &u) != nullptr);
    EXPECT(match_check_args(&b, 0, &b, 1, 32, &u, &u, &u, &u) != nullptr);
    EXPECT(match_check_args(&b, 1, &b, ((size_t)1 << 24) + 1, 32, &u, &u, &u, &u) != nullptr);
    EXPECT(match_check_args(&b, 1, &b, (size_t)1 << 24, 512, &u, &u, &u, &u) == nullptr);
    for (uint32_t dim : {0u, 16u, 33u, 48u, 544u}) EXPECT(match_check_args(&b, 1, &b, 1, dim, &u, &u, &u, &u) != nullptr);
    EXPECT(match_check_args(&b, 1, &b, 1, 32, &u, &u, &u, nullptr) != nullptr);
    // the planner: every column in exactly one split, splits of whole steps
    for (size_t n2 : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)255, (size_t)256, (size_t)257,
                      (size_t)10000, (size_t)1 << 24})
        for (size_t n1 : {(size_t)1, (size_t)129, (size_t)10000, (size_t)1 << 24})
            for (int pin : {0, 1, 3, 1024}) {
                uint32_t cols = 0;
                const uint32_t s = match_plan(n1, n2, 256, pin, &cols);
                EXPECT(s >= 1 && cols % kMatchStepCols == 0 && (size_t)s * cols >= n2 && (size_t)(s - 1) * cols < n2);
                if (pin > 0) EXPECT(s <= (uint32_t)pin);
            }
    if (g_fail) return 1;
    std::printf("OK\n");
    return 0;
}
