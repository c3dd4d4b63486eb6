// napsac_host.cpp -- NAPSAC sampling (csrc/napsac.h, napsac_layers.h) as a
// stand-alone host program: the layers of seeded rows with points on cell
// borders, outside the extent, non-finite and duplicated, and samples of every
// minimal size across the quarters and past the local length.  Built by
// tests/test_napsac.py with ASan + UBSan; prints OK or the first failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "napsac_layers.h"

using namespace gcr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform01() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
            return 1;                         \
        }                                     \
    } while (0)

static int check_layers(const NapsacLayers& L, size_t n) {
    for (int l = 0; l < kNapsacLayers; ++l) {
        const uint32_t* mem = L.members.data() + (size_t)l * n;
        std::vector<int> seen(n, 0);
        for (size_t q = 0; q < n; ++q) {
            CHECK(mem[q] < n, "layer %d member %zu out of range", l, q);
            ++seen[mem[q]];
        }
        for (size_t i = 0; i < n; ++i) {
            const NapsacRecord& r = L.rec[i];
            CHECK(seen[i] == 1, "layer %d row %zu appears %d times", l, i, seen[i]);
            CHECK(r.count[l] >= 1 && r.pos[l] < r.count[l] && (size_t)r.start[l] + r.count[l] <= n,
                  "layer %d row %zu: start %u count %u pos %u", l, i, r.start[l], r.count[l], r.pos[l]);
            CHECK(mem[r.start[l] + r.pos[l]] == i, "layer %d row %zu is not at its position", l, i);
            for (uint32_t q = 1; q < r.count[l]; ++q)
                CHECK(mem[r.start[l] + q - 1] < mem[r.start[l] + q], "layer %d: a cell's rows are not ascending", l);
        }
    }
    return 0;
}

template <int M>
static int check_samples(const NapsacLayers& L, size_t n, uint64_t T, uint64_t slot0, uint32_t nslots) {
    const NapsacTable t = napsac_host_table(L, n, M, T);
    for (uint32_t s = 0; s < nslots; ++s)
        for (uint32_t a = 0; a < 3; ++a) {
            const uint64_t slot = slot0 + s;
            uint32_t idx[M], uni[M];
            WordStream ws(77, slot, a, kStreamMain, 0), wu(77, slot, a, kStreamMain, 0);
            CHECK(sample_napsac<M>(ws, t, M, idx), "m %d slot %llu: no sample", M, (unsigned long long)slot);
            CHECK(sample_distinct<M>(wu, n, M, uni), "uniform sample");
            CHECK(idx[0] == uni[0], "m %d slot %llu: the first index is not the uniform one", M,
                  (unsigned long long)slot);
            for (int j = 0; j < M; ++j) {
                CHECK(idx[j] < n, "index out of range");
                for (int k = 0; k < j; ++k) CHECK(idx[j] != idx[k], "repeated index");
            }
            if (slot >= T) {
                for (int j = 0; j < M; ++j) CHECK(idx[j] == uni[j], "past T the sample is not the uniform one");
                continue;
            }
            int layer = 4;
            const NapsacRecord& r = L.rec[idx[0]];
            for (int l = kNapsacLayers - 1; l >= napsac_min_layer(slot, T); --l)
                if (r.count[l] >= (uint32_t)M) layer = l;
            CHECK(napsac_min_layer(slot, T) == (int)(4 * slot / T), "the quarter of slot %llu",
                  (unsigned long long)slot);
            if (layer < 4)
                for (int j = 1; j < M; ++j) {
                    const NapsacRecord& q = L.rec[idx[j]];
                    CHECK(q.start[layer] == r.start[layer], "m %d slot %llu: index %d outside the first row's cell", M,
                          (unsigned long long)slot, j);
                }
        }
    return 0;
}

int main() {
    const double extent[4] = {1280.0, 960.0, 1280.0, 960.0};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (size_t n : {(size_t)7, (size_t)64, (size_t)301, (size_t)2000}) {
        std::vector<double> col[4];
        for (int d = 0; d < 4; ++d) col[d].resize(n);
        for (size_t i = 0; i < n; ++i)
            for (int d = 0; d < 4; ++d) col[d][i] = uniform01() * extent[d];
        // borders, the extent itself, outside, non-finite, duplicates
        if (n >= 64) {
            for (int d = 0; d < 4; ++d) {
                col[d][1] = extent[d];
                col[d][2] = extent[d] / 16.0 * 3.0;
                col[d][3] = -17.5;
                col[d][4] = 3.0 * extent[d] + 1.0;
                col[d][5] = 1e300;
                col[d][8] = col[d][9] = col[d][10] = col[d][11];
            }
            col[0][6] = nan;
            col[1][7] = -inf;
            col[2][12] = inf;
        }
        const double* cols[4] = {col[0].data(), col[1].data(), col[2].data(), col[3].data()};
        NapsacLayers L;
        napsac_layers(cols, n, extent, L);
        if (check_layers(L, n)) return 1;
        for (uint64_t T : {(uint64_t)1, (uint64_t)1001, (uint64_t)1 << 40}) {
            const uint64_t starts[3] = {0, T > 300 ? T - 300 : 0, T > 300 ? T / 4 - 200 : 0};
            for (uint64_t slot0 : starts) {
                if (check_samples<2>(L, n, T, slot0, 600)) return 1;
                if (check_samples<3>(L, n, T, slot0, 600)) return 1;
                if (check_samples<4>(L, n, T, slot0, 600)) return 1;
                if (check_samples<5>(L, n, T, slot0, 600)) return 1;
                if (check_samples<7>(L, n, T, slot0, 600)) return 1;
            }
        }
    }
    const double zero[4] = {1.0, 0.0, 1.0, 1.0}, bad[4] = {1.0, 1.0, nan, 1.0}, big[4] = {1.0, 1.0, 1.0, inf};
    CHECK(!napsac_extent_ok(zero) && !napsac_extent_ok(bad) && !napsac_extent_ok(big) && napsac_extent_ok(extent),
          "napsac_extent_ok");
    std::printf("OK\n");
    return 0;
}
