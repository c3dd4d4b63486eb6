// Stand-alone host program over csrc/match_geo.h (built with ASan + UBSan by
// tests/test_match_guided.py): the factorised evaluation of the residual
// against geo_sq_residual bit for bit on random and lattice pairs, the
// plain-loop definition against a second formulation (sort of the admissible
// (d, index) keys) in both directions, the crafted cases and the argument
// check.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "match_geo.h"

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
double uni(double lo, double hi) { return lo + (hi - lo) * (rnd() / 2147483648.0); }

const double kInf = std::numeric_limits<double>::infinity();
const double kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
const double kHGeneric[9] = {0.92, -0.08, 35.0, 0.06, 0.97, -18.0, 4.0e-5, -3.0e-5, 1.0};

void skew_times(const double e[3], const double* m, double* out) {
    const double s[9] = {0, -e[2], e[1], e[2], 0, -e[0], -e[1], e[0], 0};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (s[3 * r] * m[c] + s[3 * r + 1] * m[3 + c]) + s[3 * r + 2] * m[6 + c];
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the factorised value is the definition's, bit for bit: n1 x n2 pairs
template <int KIND>
size_t factorised(const std::vector<double>& p1, const std::vector<double>& p2, const double* h) {
    const size_t n1 = p1.size() / 2, n2 = p2.size() / 2;
    std::vector<double> t1(n1 * kMatchGeoTerms), t2(n2 * kMatchGeoTerms);
    for (size_t i = 0; i < n1; ++i) match_geo_terms1<KIND>(p1[2 * i], p1[2 * i + 1], h, &t1[i * kMatchGeoTerms]);
    for (size_t j = 0; j < n2; ++j) match_geo_terms2<KIND>(p2[2 * j], p2[2 * j + 1], h, &t2[j * kMatchGeoTerms]);
    size_t bad = 0;
    for (size_t i = 0; i < n1; ++i)
        for (size_t j = 0; j < n2; ++j) {
            const double def = geo_sq_residual<KIND>(p1[2 * i], p1[2 * i + 1], p2[2 * j], p2[2 * j + 1], h);
            const double fac = match_geo_sq<KIND>(&t1[i * kMatchGeoTerms], &t2[j * kMatchGeoTerms]);
            // every NaN is one value here: the sign and payload of a NaN decide nothing
            if (!(same_bits(def, fac) || (def != def && fac != fac))) ++bad;
            for (double T : {0.0, 1.0, 9.0, kInf})
                if ((def <= T) != match_geo_adm<KIND>(&t1[i * kMatchGeoTerms], &t2[j * kMatchGeoTerms], T)) ++bad;
        }
    return bad;
}

struct Case {
    std::vector<uint8_t> d1, d2;
    std::vector<double> p1, p2;
    uint32_t dim = 32;
    int kind = kMatchGeoHomography;
    double h[9];
    double T = 1.0;
    size_t n1() const { return p1.size() / 2; }
    size_t n2() const { return p2.size() / 2; }
};

struct Out {
    std::vector<uint32_t> idx, dist, idx2, dist2;
    explicit Out(size_t n) : idx(n), dist(n), idx2(n), dist2(n) {}
};

Out run(const Case& c, int reverse) {
    // exact-size copies: a read past any array is the sanitizer's to see
    std::vector<uint8_t> a(c.d1), b(c.d2);
    std::vector<double> p(c.p1), q(c.p2);
    Out o(reverse ? c.n2() : c.n1());
    // in two row ranges, as the threaded entry calls it
    const size_t nr = o.idx.size(), mid = nr / 2;
    host_match_rows_guided(a.data(), c.n1(), p.data(), b.data(), c.n2(), q.data(), c.dim, c.kind, c.h, c.T, reverse, 0,
                           mid, o.idx.data(), o.dist.data(), o.idx2.data(), o.dist2.data());
    host_match_rows_guided(a.data(), c.n1(), p.data(), b.data(), c.n2(), q.data(), c.dim, c.kind, c.h, c.T, reverse,
                           mid, nr, o.idx.data(), o.dist.data(), o.idx2.data(), o.dist2.data());
    return o;
}

double residual(const Case& c, size_t i, size_t j) {
    return c.kind == kMatchGeoFundamental
               ? f_sq_sampson(c.p1[2 * i], c.p1[2 * i + 1], c.p2[2 * j], c.p2[2 * j + 1], c.h)
               : h_sq_residual(c.p1[2 * i], c.p1[2 * i + 1], c.p2[2 * j], c.p2[2 * j + 1], c.h);
}

// the same by sorting every row's admissible keys; returns the admissible pairs
size_t check_sorted(const Case& c, int reverse, const Out& o) {
    const size_t nr = reverse ? c.n2() : c.n1(), nc = reverse ? c.n1() : c.n2();
    size_t total = 0;
    for (size_t r = 0; r < nr; ++r) {
        std::vector<uint64_t> keys;
        for (size_t q = 0; q < nc; ++q) {
            const size_t i = reverse ? q : r, j = reverse ? r : q;
            if (!(residual(c, i, j) <= c.T)) continue;
            int64_t d = 0;
            for (uint32_t k = 0; k < c.dim; ++k) {
                const int64_t t = (int64_t)c.d1[i * c.dim + k] - (int64_t)c.d2[j * c.dim + k];
                d += t * t;
            }
            keys.push_back(match_key((uint32_t)d, (uint32_t)q));
        }
        std::sort(keys.begin(), keys.end());
        total += keys.size();
        const uint64_t k1 = keys.size() > 0 ? keys[0] : ~0ull, k2 = keys.size() > 1 ? keys[1] : ~0ull;
        EXPECT(match_key(o.dist[r], o.idx[r]) == k1);
        EXPECT(match_key(o.dist2[r], o.idx2[r]) == k2);
    }
    return total;
}

Case lattice(size_t n1, size_t n2, uint32_t dim, int kind, double T) {
    Case c;
    c.dim = dim;
    c.kind = kind;
    c.T = T;
    c.d1.resize(n1 * dim);
    c.d2.resize(n2 * dim);
    for (auto& v : c.d1) v = (uint8_t)rnd();
    for (auto& v : c.d2) v = (uint8_t)rnd();
    for (size_t k = 0; k < 2 * n1; ++k) c.p1.push_back((double)(rnd() & 15));
    for (size_t k = 0; k < 2 * n2; ++k) c.p2.push_back((double)(rnd() & 15));
    const double shift[9] = {1, 0, 2, 0, 1, -1, 0, 0, 1};
    const double e[3] = {3, -2, 1};
    if (kind == kMatchGeoFundamental) skew_times(e, shift, c.h);
    else std::memcpy(c.h, shift, sizeof shift);
    return c;
}

}  // namespace

int main() {
    // ---- the factorised evaluation: 2 x (1200 x 1200) random + 2 x (600 x 600) lattice pairs, > 3.5 million
    {
        std::vector<double> p1, p2, l1, l2;
        for (int k = 0; k < 1200; ++k) {
            p1.push_back(uni(0, 1280));
            p1.push_back(uni(0, 960));
            p2.push_back(uni(0, 1280));
            p2.push_back(uni(0, 960));
        }
        for (int k = 0; k < 1200; ++k) {
            l1.push_back((double)(rnd() & 15));
            l2.push_back((double)(rnd() & 15));
        }
        double fg[9], fl[9];
        const double eg[3] = {2560.0, 480.0, 1.0}, el[3] = {3, -2, 1};
        const double shift[9] = {1, 0, 2, 0, 1, -1, 0, 0, 1};
        // w = 0 on the lattice column x = 5: infinite and NaN residuals
        const double wz[9] = {1, 0, 0, 0, 1, 0, 1, 0, -5};
        skew_times(eg, kHGeneric, fg);
        skew_times(el, shift, fl);
        EXPECT(factorised<kMatchGeoHomography>(p1, p2, kHGeneric) == 0);
        EXPECT(factorised<kMatchGeoFundamental>(p1, p2, fg) == 0);
        EXPECT(factorised<kMatchGeoHomography>(l1, l2, shift) == 0);
        EXPECT(factorised<kMatchGeoFundamental>(l1, l2, fl) == 0);
        EXPECT(factorised<kMatchGeoHomography>(l1, l2, wz) == 0);
        // a rank-deficient F whose denominators vanish at the origin: 0 / 0
        const double fz[9] = {0, 0, 0, 0, 0, 1, 0, -1, 0};
        EXPECT(factorised<kMatchGeoFundamental>(l1, l2, fz) == 0);
    }
    // ---- the definition, both kinds, both directions, three dims
    for (uint32_t dim : {32u, 128u, 512u})
        for (int kind : {kMatchGeoHomography, kMatchGeoFundamental})
            for (double T : {1.0, 9.0, 64.0}) {
                const Case c = lattice(37, 53, dim, kind, T);
                for (int reverse : {0, 1}) {
                    const size_t adm = check_sorted(c, reverse, run(c, reverse));
                    EXPECT(adm > 0 && adm < 37 * 53);
                }
            }
    // ---- crafted
    {
        // nothing admissible: four sentinels
        Case c = lattice(9, 21, 32, kMatchGeoHomography, 1.0);
        c.h[2] = 100.0;
        for (int reverse : {0, 1}) {
            const Out o = run(c, reverse);
            EXPECT(check_sorted(c, reverse, o) == 0);
            for (size_t r = 0; r < o.idx.size(); ++r)
                EXPECT(o.idx[r] == kMatchNone && o.dist[r] == kMatchNone && o.idx2[r] == kMatchNone &&
                       o.dist2[r] == kMatchNone);
        }
    }
    {
        // exactly one admissible column per row; in reverse the rows have one or none
        Case c = lattice(9, 21, 32, kMatchGeoHomography, 1.0);
        std::memcpy(c.h, kIdentity, sizeof kIdentity);
        for (size_t i = 0; i < 9; ++i) c.p1[2 * i] = 10.0 * i, c.p1[2 * i + 1] = 0.0;
        for (size_t j = 0; j < 21; ++j) c.p2[2 * j] = 10.0 * ((j * 8) % 21), c.p2[2 * j + 1] = 0.0;
        const Out f = run(c, 0);
        EXPECT(check_sorted(c, 0, f) == 9);
        for (size_t i = 0; i < 9; ++i) {
            EXPECT(f.idx[i] != kMatchNone && c.p2[2 * f.idx[i]] == c.p1[2 * i]);
            EXPECT(f.dist[i] != kMatchNone && f.idx2[i] == kMatchNone && f.dist2[i] == kMatchNone);
        }
        const Out b = run(c, 1);
        EXPECT(check_sorted(c, 1, b) == 9);
        for (size_t i = 0; i < 9; ++i) EXPECT(b.idx[f.idx[i]] == i);
    }
    {
        // T = +inf, identity: the unguided definition's bytes
        Case c = lattice(13, 40, 128, kMatchGeoHomography, kInf);
        std::memcpy(c.h, kIdentity, sizeof kIdentity);
        const Out g = run(c, 0);
        Out u(13);
        host_match_rows(c.d1.data(), c.d2.data(), 40, 128, 0, 13, u.idx.data(), u.dist.data(), u.idx2.data(),
                        u.dist2.data());
        EXPECT(g.idx == u.idx && g.dist == u.dist && g.idx2 == u.idx2 && g.dist2 == u.dist2);
        const Out gr = run(c, 1);
        Out ur(40);
        host_match_rows(c.d2.data(), c.d1.data(), 13, 128, 0, 40, ur.idx.data(), ur.dist.data(), ur.idx2.data(),
                        ur.dist2.data());
        EXPECT(gr.idx == ur.idx && gr.dist == ur.dist && gr.idx2 == ur.idx2 && gr.dist2 == ur.dist2);
    }
    {
        // w = 0 rows: infinite residuals are admissible under T = +inf only, NaN ones never
        Case c = lattice(12, 20, 32, kMatchGeoHomography, 4.0);
        const double wz[9] = {1, 0, 0, 0, 1, 0, 1, 0, -5};
        std::memcpy(c.h, wz, sizeof wz);
        c.p1[0] = 5.0, c.p1[1] = 3.0;                     // row 0: u = inf, v = inf
        c.p1[2] = 5.0, c.p1[3] = 0.0;                     // row 1: v = 0 / 0 = NaN
        EXPECT(std::isinf(residual(c, 0, 0)) && std::isnan(residual(c, 1, 0)));
        Out o = run(c, 0);
        check_sorted(c, 0, o);
        EXPECT(o.idx[0] == kMatchNone && o.idx[1] == kMatchNone);
        c.T = kInf;
        o = run(c, 0);
        check_sorted(c, 0, o);
        EXPECT(o.idx[0] != kMatchNone && o.idx2[0] != kMatchNone && o.idx[1] == kMatchNone);
        check_sorted(c, 1, run(c, 1));
    }
    {
        // r == T is admissible; duplicates keep the lower index first; all 0 against all 255
        Case c = lattice(6, 18, 64, kMatchGeoHomography, 0.0);
        std::memcpy(c.h, kIdentity, sizeof kIdentity);
        std::fill(c.p1.begin(), c.p1.end(), 3.0);
        std::fill(c.p2.begin(), c.p2.end(), 3.0);
        for (size_t j = 0; j < 6 * 64; ++j) c.d2[6 * 64 + j] = c.d2[12 * 64 + j] = c.d1[j] = c.d2[j];
        Out o = run(c, 0);
        EXPECT(check_sorted(c, 0, o) == 6 * 18);
        for (size_t i = 0; i < 6; ++i) EXPECT(o.idx[i] == i && o.idx2[i] == i + 6 && o.dist[i] == 0 && o.dist2[i] == 0);
        std::fill(c.d1.begin(), c.d1.end(), 0);
        std::fill(c.d2.begin(), c.d2.end(), 255);
        o = run(c, 0);
        for (size_t i = 0; i < 6; ++i)
            EXPECT(o.idx[i] == 0 && o.idx2[i] == 1 && o.dist[i] == 64u * 255u * 255u && o.dist2[i] == o.dist[i]);
        c.p2[2 * 0] = 4.0;                                // column 0 leaves: r = 1 > 0
        o = run(c, 0);
        for (size_t i = 0; i < 6; ++i) EXPECT(o.idx[i] == 1 && o.idx2[i] == 2);
    }
    // ---- arguments
    {
        uint8_t b = 0;
        uint32_t u = 0;
        double p[2] = {0, 0};
        auto chk = [&](const void* p1, const void* p2, int kind, const double* m, double T, int rev) {
            return match_geo_check_args(&b, 1, p1, &b, 1, p2, 32, kind, m, T, rev, &u, &u, &u, &u);
        };
        EXPECT(chk(p, p, kMatchGeoHomography, kIdentity, 1.0, 0) == nullptr);
        EXPECT(chk(p, p, kMatchGeoFundamental, kIdentity, kInf, 1) == nullptr);
        EXPECT(chk(p, p, kMatchGeoHomography, kIdentity, 0.0, 0) == nullptr);
        EXPECT(chk(nullptr, p, kMatchGeoHomography, kIdentity, 1.0, 0) != nullptr);
        EXPECT(chk(p, nullptr, kMatchGeoHomography, kIdentity, 1.0, 0) != nullptr);
        EXPECT(chk(p, p, kMatchGeoHomography, nullptr, 1.0, 0) != nullptr);
        for (int kind : {-1, 0, 2, 5, 7}) EXPECT(chk(p, p, kind, kIdentity, 1.0, 0) != nullptr);
        EXPECT(chk(p, p, kMatchGeoHomography, kIdentity, -1.0, 0) != nullptr);
        EXPECT(chk(p, p, kMatchGeoHomography, kIdentity, std::nan(""), 0) != nullptr);
        EXPECT(chk(p, p, kMatchGeoHomography, kIdentity, 1.0, 2) != nullptr);
        double m[9];
        for (double v : {kInf, -kInf, (double)std::nan("")}) {
            std::memcpy(m, kIdentity, sizeof m);
            m[4] = v;
            EXPECT(chk(p, p, kMatchGeoHomography, m, 1.0, 0) != nullptr);
        }
        EXPECT(match_geo_check_args(&b, 0, p, &b, 1, p, 32, 3, kIdentity, 1.0, 0, &u, &u, &u, &u) != nullptr);
        EXPECT(match_geo_check_args(&b, 1, p, &b, 1, p, 48, 3, kIdentity, 1.0, 0, &u, &u, &u, &u) != nullptr);
    }
    if (g_fail) return 1;
    std::printf("OK\n");
    return 0;
}
