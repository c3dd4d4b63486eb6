// Stand-alone host program over csrc/match_knn.h (built with ASan + UBSan by
// tests/test_match_knn.py): the plain-loop definition against a sort of all
// (d, j) keys, k = 2 against match.h's definition, the merge's independence of
// the split points and of the merge order, and the argument check.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "match_knn.h"

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

std::vector<uint64_t> row_keys(const std::vector<uint8_t>& d1, size_t i, const std::vector<uint8_t>& d2, size_t n2,
                               uint32_t dim) {
    std::vector<uint64_t> keys(n2);
    for (size_t j = 0; j < n2; ++j) {
        int64_t d = 0;
        for (uint32_t q = 0; q < dim; ++q) {
            const int64_t t = (int64_t)d1[i * dim + q] - (int64_t)d2[j * dim + q];
            d += t * t;
        }
        keys[j] = match_key((uint32_t)d, (uint32_t)j);
    }
    return keys;
}

// the definition on exact-size copies (a read past either array is the sanitizer's to see) against the sort
void check_rows(const std::vector<uint8_t>& d1, size_t n1, const std::vector<uint8_t>& d2, size_t n2, uint32_t dim) {
    std::vector<uint8_t> a(d1.begin(), d1.begin() + n1 * dim), b(d2.begin(), d2.begin() + n2 * dim);
    for (uint32_t k = 1; k <= kKnnMaxK; ++k) {
        std::vector<uint32_t> idx(n1 * k, 7u), dist(n1 * k, 7u);
        // two row ranges: the output rows are addressed by i, not by i - i0
        host_knn_rows(a.data(), b.data(), n2, dim, k, 0, n1 / 2, idx.data(), dist.data());
        host_knn_rows(a.data(), b.data(), n2, dim, k, n1 / 2, n1, idx.data(), dist.data());
        for (size_t i = 0; i < n1; ++i) {
            std::vector<uint64_t> keys = row_keys(a, i, b, n2, dim);
            std::sort(keys.begin(), keys.end());
            for (uint32_t r = 0; r < k; ++r) {
                const uint64_t want = r < n2 ? keys[r] : kKnnPad;
                EXPECT(idx[i * k + r] == (uint32_t)want && dist[i * k + r] == (uint32_t)(want >> 32));
            }
        }
        if (k == 2) {
            std::vector<uint32_t> o[4];
            for (auto& v : o) v.resize(n1);
            host_match_rows(a.data(), b.data(), n2, dim, 0, n1, o[0].data(), o[1].data(), o[2].data(), o[3].data());
            for (size_t i = 0; i < n1; ++i) {
                EXPECT(idx[2 * i] == o[0][i] && dist[2 * i] == o[1][i]);
                EXPECT(idx[2 * i + 1] == o[2][i] && dist[2 * i + 1] == o[3][i]);
            }
        }
    }
}

// the first K of keys[lo, hi), ascending, padded
template <int K>
void top(const std::vector<uint64_t>& keys, size_t lo, size_t hi, uint64_t (&out)[K]) {
    std::vector<uint64_t> part(keys.begin() + lo, keys.begin() + hi);
    std::sort(part.begin(), part.end());
    for (int r = 0; r < K; ++r) out[r] = (size_t)r < part.size() ? part[r] : kKnnPad;
}

template <int K>
bool equal(const uint64_t (&a)[K], const uint64_t (&b)[K]) {
    for (int r = 0; r < K; ++r)
        if (a[r] != b[r]) return false;
    return true;
}

template <int K>
void copy(uint64_t (&dst)[K], const uint64_t (&src)[K]) {
    for (int r = 0; r < K; ++r) dst[r] = src[r];
}

// every pair of split points of the columns and every order and shape of merging the three parts
template <int K>
void check_merge(const std::vector<uint64_t>& keys) {
    const size_t n = keys.size();
    uint64_t want[K];
    top<K>(keys, 0, n, want);
    for (size_t c1 = 0; c1 <= n; ++c1)
        for (size_t c2 = c1; c2 <= n; ++c2) {
            uint64_t part[3][K];
            top<K>(keys, 0, c1, part[0]);
            top<K>(keys, c1, c2, part[1]);
            top<K>(keys, c2, n, part[2]);
            int perm[3] = {0, 1, 2};
            do {
                // (x + y) + z
                uint64_t acc[K];
                copy<K>(acc, part[perm[0]]);
                knn_merge<K>(acc, part[perm[1]]);
                knn_merge<K>(acc, part[perm[2]]);
                EXPECT(equal<K>(acc, want));
                // x + (y + z)
                uint64_t right[K], left[K];
                copy<K>(right, part[perm[1]]);
                knn_merge<K>(right, part[perm[2]]);
                copy<K>(left, part[perm[0]]);
                knn_merge<K>(left, right);
                EXPECT(equal<K>(left, want));
            } while (std::next_permutation(perm, perm + 3));
            // from the empty list, as k_knn_merge starts
            uint64_t acc[K];
            for (int r = 0; r < K; ++r) acc[r] = kKnnPad;
            for (int q = 0; q < 3; ++q) knn_merge<K>(acc, part[q]);
            EXPECT(equal<K>(acc, want));
        }
}

}  // namespace

int main() {
    for (uint32_t dim : {32u, 128u}) {
        // a two-letter alphabet: few distinct distances, many ties
        {
            const size_t n1 = 7, n2 = 21;
            const uint8_t vals[2] = {3, 250};
            std::vector<uint8_t> d1(n1 * dim), d2(n2 * dim);
            for (auto& v : d1) v = vals[rnd() & 1];
            for (auto& v : d2) v = vals[rnd() & 1];
            check_rows(d1, n1, d2, n2, dim);
            check_rows(d1, n1, d2, 1, dim);               // the pad from position 1 on
            check_rows(d1, n1, d2, 5, dim);               // n2 < k, n2 == k, n2 > k
            check_rows(d1, 1, d2, n2, dim);               // an empty first row range
            const std::vector<uint64_t> keys = row_keys(d1, 0, d2, 13, dim);
            check_merge<1>(keys);
            check_merge<2>(keys);
            check_merge<4>(keys);
            check_merge<8>(keys);
        }
        // random bytes, all columns equal, distances falling and rising with j
        {
            const size_t n1 = 5, n2 = 40;
            std::vector<uint8_t> d1(n1 * dim), d2(n2 * dim), eq(n2 * dim, 77), down(n2 * dim), up(n2 * dim);
            for (auto& v : d1) v = (uint8_t)rnd();
            for (auto& v : d2) v = (uint8_t)rnd();
            for (size_t j = 0; j < n2; ++j)
                for (uint32_t q = 0; q < dim; ++q) {
                    down[j * dim + q] = (uint8_t)(255 - j);
                    up[j * dim + q] = (uint8_t)j;
                }
            check_rows(d1, n1, d2, n2, dim);
            check_rows(d1, n1, eq, n2, dim);
            const std::vector<uint8_t> zero(n1 * dim, 0);
            check_rows(zero, n1, down, n2, dim);
            check_rows(zero, n1, up, n2, dim);
            check_merge<4>(row_keys(d1, 1, d2, 11, dim));
            check_merge<8>(row_keys(d1, 1, eq, 11, dim));
            check_merge<8>(row_keys(zero, 0, down, 9, dim));
        }
    }
    // fewer keys than the capacity, and none
    check_merge<8>({match_key(5, 0), match_key(5, 1), match_key(2, 2)});
    check_merge<4>({});
    EXPECT(knn_capacity(1) == 4 && knn_capacity(4) == 4 && knn_capacity(5) == 8 && knn_capacity(8) == 8);
    EXPECT(kKnnPad == match_key(kMatchNone, kMatchNone));
    // arguments
    uint8_t b = 0;
    uint32_t u = 0;
    EXPECT(knn_check_args(&b, 1, &b, 1, 32, 1, &u, &u) == nullptr);
    EXPECT(knn_check_args(&b, 1, &b, (size_t)1 << 24, 512, 8, &u, &u) == nullptr);
    EXPECT(knn_check_args(nullptr, 1, &b, 1, 32, 1, &u, &u) != nullptr);
    EXPECT(knn_check_args(&b, 1, nullptr, 1, 32, 1, &u, &u) != nullptr);
    EXPECT(knn_check_args(&b, 1, &b, 1, 32, 1, nullptr, &u) != nullptr);
    EXPECT(knn_check_args(&b, 1, &b, 1, 32, 1, &u, nullptr) != nullptr);
    EXPECT(knn_check_args(&b, 0, &b, 1, 32, 1, &u, &u) != nullptr);
    EXPECT(knn_check_args(&b, 1, &b, ((size_t)1 << 24) + 1, 32, 1, &u, &u) != nullptr);
    for (uint32_t dim : {0u, 16u, 33u, 48u, 544u}) EXPECT(knn_check_args(&b, 1, &b, 1, dim, 1, &u, &u) != nullptr);
    for (uint32_t k : {0u, 9u, 0xFFFFFFFFu}) EXPECT(knn_check_args(&b, 1, &b, 1, 32, k, &u, &u) != nullptr);
    if (g_fail) return 1;
    std::printf("OK\n");
    return 0;
}
