// Stand-alone host program over csrc/match_select.h and csrc/match.h (built
// with ASan + UBSan by tests/test_match_sets.py): the front-end rule on search
// results of the plain-loop definition and on crafted rows, against a second
// formulation written row by row from the rule's text, and the argument check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "match.h"
#include "match_select.h"

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

struct Search {
    std::vector<uint32_t> idx, dist, idx2, dist2;
    explicit Search(size_t n) : idx(n), dist(n), idx2(n), dist2(n) {}
};

struct Picked {
    std::vector<uint32_t> matches;
    std::vector<double> ratios;
    size_t m = 0;
};

// exact-size outputs: a write past the kept rows' cap is the sanitizer's to see
Picked select(const Search& s, const std::vector<uint32_t>* back, const MatchSelectRule& rule) {
    const size_t n = s.idx.size();
    Picked p;
    p.matches.assign(2 * n, 0xABABABABu);
    p.ratios.assign(n, -1.0);
    p.m = host_match_select(s.idx.data(), s.dist.data(), s.idx2.data(), s.dist2.data(), n, back ? back->data() : nullptr,
                            back ? back->size() : 0, rule, p.matches.data(), p.ratios.data());
    return p;
}

// the rule's text, one statement per line of it
Picked restate(const Search& s, const std::vector<uint32_t>* back, const MatchSelectRule& rule) {
    Picked p;
    for (size_t i = 0; i < s.idx.size(); ++i) {
        const bool found = rule.guided ? s.idx[i] != kMatchNone : true;
        const bool none2 = s.idx2[i] == kMatchNone;
        double ratio = 1.0;
        if (found && !none2 && s.dist2[i] > 0) ratio = std::sqrt((double)s.dist[i] / (double)s.dist2[i]);
        if (!found) continue;
        if (rule.has_ratio) {
            const bool below = (double)s.dist[i] < rule.rr * (double)s.dist2[i];
            if (rule.guided ? !(none2 || below) : !(!none2 && below)) continue;
        }
        if (rule.guided && rule.has_max_distance && !((double)s.dist[i] <= rule.max_distance)) continue;
        if (back && (*back)[s.idx[i]] != (uint32_t)i) continue;
        p.matches.push_back((uint32_t)i);
        p.matches.push_back(s.idx[i]);
        p.ratios.push_back(ratio);
        ++p.m;
    }
    return p;
}

void expect_same(const Picked& got, const Picked& exp) {
    EXPECT(got.m == exp.m);
    if (got.m != exp.m) return;
    for (size_t k = 0; k < exp.m; ++k) {
        EXPECT(got.matches[2 * k] == exp.matches[2 * k] && got.matches[2 * k + 1] == exp.matches[2 * k + 1]);
        EXPECT(got.ratios[k] == exp.ratios[k]);
        if (k) EXPECT(got.matches[2 * k] > got.matches[2 * k - 2]);     // ascending rows
    }
    // nothing written past the kept rows
    for (size_t k = exp.m; k < got.ratios.size(); ++k)
        EXPECT(got.ratios[k] == -1.0 && got.matches[2 * k] == 0xABABABABu && got.matches[2 * k + 1] == 0xABABABABu);
}

MatchSelectRule rule_of(int guided, bool has_ratio, double ratio, bool has_max, double max_distance) {
    MatchSelectRule r{};
    r.guided = guided;
    r.has_ratio = has_ratio;
    r.rr = has_ratio ? ratio * ratio : 0.0;
    r.has_max_distance = has_max;
    r.max_distance = has_max ? max_distance : 0.0;
    return r;
}

void all_rules(const Search& s, const std::vector<uint32_t>& back, int guided) {
    const double ratios[] = {0.0, 0.8, 1e-9, 1e9};                  // 0.0: no ratio test
    for (double ratio : ratios)
        for (int mutual = 0; mutual < 2; ++mutual)
            for (int cap = 0; cap < (guided ? 3 : 1); ++cap) {
                const MatchSelectRule r = rule_of(guided, ratio != 0.0, ratio, cap != 0, cap == 1 ? 0.0 : 40000.0);
                expect_same(select(s, mutual ? &back : nullptr, r), restate(s, mutual ? &back : nullptr, r));
            }
}

void searched_inputs() {
    const size_t shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 1}, {31, 33}, {70, 97}, {300, 40}};
    const uint32_t dim = 32;
    for (const auto& sh : shapes) {
        const size_t n1 = sh[0], n2 = sh[1];
        std::vector<uint8_t> d1(n1 * dim), d2(n2 * dim);
        for (auto& v : d1) v = (uint8_t)(rnd() & 3u);               // few values: ties and 0 / 0
        for (auto& v : d2) v = (uint8_t)(rnd() & 3u);
        Search f(n1), b(n2);
        host_match_rows(d1.data(), d2.data(), n2, dim, 0, n1, f.idx.data(), f.dist.data(), f.idx2.data(),
                        f.dist2.data());
        host_match_rows(d2.data(), d1.data(), n1, dim, 0, n2, b.idx.data(), b.dist.data(), b.idx2.data(),
                        b.dist2.data());
        all_rules(f, b.idx, 0);
        all_rules(f, b.idx, 1);
    }
}

void crafted_rows() {
    // row 0: a plain match; 1: 0 / 0; 2: no second neighbour; 3: no candidate at all (guided);
    // 4: dist2 == 0 cannot happen with dist > 0, but dist == dist2 can; 5: the largest distance
    Search s(6);
    const uint32_t idx[] = {2, 0, 1, kMatchNone, 3, 0}, dist[] = {100, 0, 50, kMatchNone, 77, 33292800};
    const uint32_t idx2[] = {1, 3, kMatchNone, kMatchNone, 2, 1}, dist2[] = {400, 0, kMatchNone, kMatchNone, 77, 33292800};
    for (int k = 0; k < 6; ++k) s.idx[k] = idx[k], s.dist[k] = dist[k], s.idx2[k] = idx2[k], s.dist2[k] = dist2[k];
    const std::vector<uint32_t> back = {1, 2, 0, 4};                // exactly four rows on the other side

    // guided, no tests: every row with a candidate, ratios by the rule
    Picked p = select(s, nullptr, rule_of(1, false, 0, false, 0));
    EXPECT(p.m == 5 && p.matches[0] == 0 && p.matches[6] == 4 && p.matches[8] == 5);
    EXPECT(p.ratios[0] == 0.5 && p.ratios[1] == 1.0 && p.ratios[2] == 1.0 && p.ratios[3] == 1.0 && p.ratios[4] == 1.0);
    // plain, no tests: every row kept (a plain search has no row without a candidate, the rule does not look)
    Search q(5);
    for (int k = 0, o = 0; k < 6; ++k)
        if (k != 3) q.idx[o] = idx[k], q.dist[o] = dist[k], q.idx2[o] = idx2[k], q.dist2[o] = dist2[k], ++o;
    p = select(q, nullptr, rule_of(0, false, 0, false, 0));
    EXPECT(p.m == 5);
    for (size_t k = 0; k < 5; ++k) EXPECT(p.matches[2 * k] == k && p.matches[2 * k + 1] == q.idx[k]);
    // ratio 0.8: plain drops the row without a second neighbour, guided keeps it
    p = select(q, nullptr, rule_of(0, true, 0.8, false, 0));
    EXPECT(p.m == 1 && p.matches[0] == 0 && p.matches[1] == 2 && p.ratios[0] == 0.5);
    p = select(s, nullptr, rule_of(1, true, 0.8, false, 0));
    EXPECT(p.m == 2 && p.matches[0] == 0 && p.matches[2] == 2 && p.matches[3] == 1 && p.ratios[1] == 1.0);
    // no row kept
    p = select(s, nullptr, rule_of(1, true, 1e-9, true, 0.0));
    EXPECT(p.m == 0);
    expect_same(p, restate(s, nullptr, rule_of(1, true, 1e-9, true, 0.0)));
    // the cap: dist <= max_distance, the bound itself included
    p = select(s, nullptr, rule_of(1, false, 0, true, 77.0));
    EXPECT(p.m == 3 && p.matches[0] == 1 && p.matches[2] == 2 && p.matches[4] == 4);
    // mutual with a row whose idx is kMatchNone: back has FOUR entries, so reading back[idx] there is out of
    // bounds and the sanitizer's to see.  back[2] == 0, back[0] == 1: rows 0 and 1 are mutual; row 2's idx 1 has
    // back 2; row 4's idx 3 has back 4; row 5's idx 0 has back 1
    p = select(s, &back, rule_of(1, false, 0, false, 0));
    EXPECT(p.m == 4 && p.matches[0] == 0 && p.matches[2] == 1 && p.matches[4] == 2 && p.matches[6] == 4);
    expect_same(p, restate(s, &back, rule_of(1, false, 0, false, 0)));
    // every combination on the crafted rows
    all_rules(s, back, 1);
}

void argument_check() {
    uint32_t a[4] = {};
    double r[4] = {};
    size_t m = 0;
    MatchSelectRule rule = rule_of(0, true, 0.8, false, 0);
    auto bad = [&](const char* msg, const char* word) {
        EXPECT(msg != nullptr);
        if (msg) EXPECT(std::string(msg).find(word) != std::string::npos);
    };
    EXPECT(match_select_check_args(a, a, a, a, 4, nullptr, 0, &rule, a, r, 4, &m) == nullptr);
    EXPECT(match_select_check_args(a, a, a, a, 4, a, 4, &rule, a, r, 9, &m) == nullptr);
    bad(match_select_check_args(nullptr, a, a, a, 4, nullptr, 0, &rule, a, r, 4, &m), "idx");
    bad(match_select_check_args(a, nullptr, a, a, 4, nullptr, 0, &rule, a, r, 4, &m), "dist");
    bad(match_select_check_args(a, a, nullptr, a, 4, nullptr, 0, &rule, a, r, 4, &m), "idx2");
    bad(match_select_check_args(a, a, a, nullptr, 4, nullptr, 0, &rule, a, r, 4, &m), "dist2");
    bad(match_select_check_args(a, a, a, a, 4, nullptr, 0, nullptr, a, r, 4, &m), "rule");
    bad(match_select_check_args(a, a, a, a, 4, nullptr, 0, &rule, nullptr, r, 4, &m), "matches_out");
    bad(match_select_check_args(a, a, a, a, 4, nullptr, 0, &rule, a, nullptr, 4, &m), "ratios_out");
    bad(match_select_check_args(a, a, a, a, 4, nullptr, 0, &rule, a, r, 4, nullptr), "m_out");
    bad(match_select_check_args(a, a, a, a, 0, nullptr, 0, &rule, a, r, 4, &m), " n ");
    bad(match_select_check_args(a, a, a, a, kMatchMaxRows + 1, nullptr, 0, &rule, a, r, kMatchMaxRows + 1, &m), " n ");
    bad(match_select_check_args(a, a, a, a, 4, a, 0, &rule, a, r, 4, &m), "nb");
    bad(match_select_check_args(a, a, a, a, 4, nullptr, 0, &rule, a, r, 3, &m), "cap");
    for (double rr : {0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
        MatchSelectRule rb = rule;
        rb.rr = rr;
        bad(match_select_check_args(a, a, a, a, 4, nullptr, 0, &rb, a, r, 4, &m), "rr");
    }
    for (double md : {-1.0, std::numeric_limits<double>::quiet_NaN()}) {
        MatchSelectRule rb = rule_of(1, false, 0, true, md);
        bad(match_select_check_args(a, a, a, a, 4, nullptr, 0, &rb, a, r, 4, &m), "max_distance");
    }
}

}  // namespace

int main() {
    searched_inputs();
    crafted_rows();
    argument_check();
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("OK match_select_host\n");
    return 0;
}
