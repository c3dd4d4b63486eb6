// verify_many_host.cpp -- csrc/verify_many.h's host twin as a stand-alone
// program (built with -fsanitize=address,undefined by tests/test_verify_many.py):
//   * a few hundred random problems of both kinds, the degenerate ones (all
//     rows one point, exactly m rows) included, in packed calls: every
//     problem's record and mask equal the same problem run alone, for 1 and
//     for many threads;
//   * the packed-offset arithmetic: problems of m rows at both ends of a
//     buffer that is exactly as long as the rows (the sanitizer sees any
//     access past either end), masks in an exact buffer too;
//   * the argument checks;
//   * many_better: folding candidates in any order and any blocking gives the
//     first strict maximum of the sequential rule.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "verify_many.h"

using namespace gcr;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            ++fails;                                                    \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
        }                                                               \
    } while (0)

struct Call {
    std::vector<double> rows;
    std::vector<uint64_t> off{0};
    std::vector<double> thr;
    std::vector<uint64_t> seeds;
};

static void add_problem(Call& c, std::mt19937_64& rng, int solver, int shape) {
    const uint32_t m = (uint32_t)solver_row(solver).m;
    std::uniform_real_distribution<double> u(0.0, 1000.0), noise(-0.7, 0.7);
    uint32_t n = shape == 1 ? m : m + (uint32_t)(rng() % 40);
    const double H[9] = {1.02, 0.03, 5.0, -0.02, 0.98, -3.0, 1e-5, -2e-5, 1.0};
    for (uint32_t i = 0; i < n; ++i) {
        double x = u(rng), y = u(rng), x2, y2;
        if (shape == 2) {                     // all rows one point
            x = 100.0; y = 200.0; x2 = 110.0; y2 = 190.0;
        } else if (i % 3 == 2) {              // an outlier
            x2 = u(rng); y2 = u(rng);
        } else {
            const double w = H[6] * x + H[7] * y + H[8];
            x2 = (H[0] * x + H[1] * y + H[2]) / w + noise(rng);
            y2 = (H[3] * x + H[4] * y + H[5]) / w + noise(rng);
        }
        const double r[4] = {x, y, x2, y2};
        c.rows.insert(c.rows.end(), r, r + 4);
    }
    c.off.push_back(c.off.back() + n);
    c.thr.push_back(0.5 + (double)(rng() % 5));
    c.seeds.push_back(rng());
}

static void check_call(const Call& c, int solver, uint32_t S) {
    const size_t P = c.thr.size(), total = (size_t)c.off.back();
    // exact-size heap buffers: one byte or row past either end is a sanitizer report
    std::vector<double> rows(c.rows);
    rows.shrink_to_fit();
    CHECK(many_check_shape(solver, rows.data(), c.off.data(), P, c.thr.data(), c.seeds.data(), S, rows.data()).empty());
    CHECK(many_first_nonfinite(rows.data(), rows.size()) == -1);
    std::vector<gcr_many_result> out1(P), outN(P);
    std::vector<uint8_t> mask1(total, 9), maskN(total, 9);
    host_verify_many(solver, rows.data(), c.off.data(), P, c.thr.data(), c.seeds.data(), S, 1, out1.data(), mask1.data());
    host_verify_many(solver, rows.data(), c.off.data(), P, c.thr.data(), c.seeds.data(), S, 7, outN.data(), maskN.data());
    CHECK(std::memcmp(out1.data(), outN.data(), P * sizeof(gcr_many_result)) == 0);
    CHECK(mask1 == maskN);
    for (size_t p = 0; p < P; ++p) {
        const size_t n = (size_t)(c.off[p + 1] - c.off[p]);
        std::vector<double> own(rows.begin() + 4 * c.off[p], rows.begin() + 4 * c.off[p + 1]);
        const uint64_t off[2] = {0, n};
        gcr_many_result r;
        std::vector<uint8_t> mk(n, 9);
        host_verify_many(solver, own.data(), off, 1, &c.thr[p], &c.seeds[p], S, 1, &r, mk.data());
        CHECK(std::memcmp(&r, &out1[p], sizeof(r)) == 0);
        CHECK(std::memcmp(mk.data(), mask1.data() + c.off[p], n) == 0);
        size_t inl = 0;
        for (size_t i = 0; i < n; ++i) {
            CHECK(mk[i] <= 1);
            inl += mk[i];
        }
        CHECK(inl == r.best_inliers);
        CHECK((r.best_slot == -1) == (r.best_score == 0.0));
        CHECK(r.best_slot < (int64_t)S && r.best_hypothesis < (uint32_t)solver_row(solver).per);
        CHECK(r.iterations >= S && r.iterations <= 102ull * S && r.models <= (uint64_t)S * solver_row(solver).per);
        // without a mask buffer the record is the same
        gcr_many_result r2;
        host_verify_many(solver, own.data(), off, 1, &c.thr[p], &c.seeds[p], S, 1, &r2, nullptr);
        CHECK(std::memcmp(&r, &r2, sizeof(r)) == 0);
    }
}

static void check_degenerate(int solver, uint32_t S) {
    std::mt19937_64 rng(5);
    Call c;
    add_problem(c, rng, solver, 2);
    gcr_many_result r;
    std::vector<uint8_t> mk((size_t)c.off[1], 9);
    host_verify_many(solver, c.rows.data(), c.off.data(), 1, c.thr.data(), c.seeds.data(), S, 1, &r, mk.data());
    CHECK(r.models == 0 && r.iterations == 102ull * S && r.best_slot == -1 && r.best_inliers == 0);
    for (uint8_t b : mk) CHECK(b == 0);
}

static void check_args() {
    const double rows[8 * 4] = {};
    const uint64_t good[3] = {0, 4, 8}, desc[3] = {0, 5, 4}, shortp[3] = {0, 3, 8}, first[3] = {1, 5, 9};
    const double thr[2] = {1.0, 2.0}, bad_thr[2] = {1.0, 0.0};
    const uint64_t seeds[2] = {1, 2};
    gcr_many_result out[2];
    auto ok = [&](int solver, const uint64_t* off, size_t P, const double* t, uint32_t S) {
        return many_check_shape(solver, rows, off, P, t, seeds, S, out).empty();
    };
    CHECK(ok(GCR_SOLVER_HOMOGRAPHY4, good, 2, thr, 1));
    CHECK(ok(GCR_SOLVER_HOMOGRAPHY4, good, 2, thr, kManyMaxSlots));
    CHECK(!ok(GCR_SOLVER_FUNDAMENTAL7, good, 2, thr, 8));           // 4 rows < 7
    CHECK(!ok(GCR_SOLVER_ESSENTIAL5, good, 2, thr, 8));
    CHECK(!ok(GCR_SOLVER_HOMOGRAPHY4, good, 0, thr, 8));
    CHECK(!ok(GCR_SOLVER_HOMOGRAPHY4, desc, 2, thr, 8));
    CHECK(!ok(GCR_SOLVER_HOMOGRAPHY4, shortp, 2, thr, 8));
    CHECK(!ok(GCR_SOLVER_HOMOGRAPHY4, first, 2, thr, 8));
    CHECK(!ok(GCR_SOLVER_HOMOGRAPHY4, good, 2, bad_thr, 8));
    CHECK(!ok(GCR_SOLVER_HOMOGRAPHY4, good, 2, thr, 0));
    CHECK(!ok(GCR_SOLVER_HOMOGRAPHY4, good, 2, thr, kManyMaxSlots + 1));
    double v[5] = {0.0, 1.0, 2.0, 3.0, 4.0};
    CHECK(many_first_nonfinite(v, 5) == -1);
    v[3] = 0.0 / 0.0;
    CHECK(many_first_nonfinite(v, 5) == 3);
    v[1] = 1.0 / 0.0;
    CHECK(many_first_nonfinite(v, 5) == 1);
}

// the sequential rule over candidates in hypothesis order against folds of
// shuffled blocks: scores with many exact ties
static void check_merge() {
    std::mt19937_64 rng(9);
    for (int round = 0; round < 200; ++round) {
        const uint32_t n = 1 + (uint32_t)(rng() % 60);
        std::vector<double> sc(n);
        std::vector<uint32_t> hyp(n);
        for (uint32_t i = 0; i < n; ++i) {
            sc[i] = (double)(rng() % 4);           // 0 = not a candidate; ties among 1 .. 3
            hyp[i] = i;
        }
        double best = 0.0;
        uint32_t bh = kManyNone;
        for (uint32_t i = 0; i < n; ++i)
            if (best < sc[i]) {
                best = sc[i];
                bh = i;
            }
        // blocks of a random size, each folded in a shuffled order, then the blocks in a shuffled order
        const uint32_t bs = 1 + (uint32_t)(rng() % 9);
        std::vector<std::pair<double, uint32_t>> parts;
        for (uint32_t lo = 0; lo < n; lo += bs) {
            std::vector<uint32_t> ord;
            for (uint32_t i = lo; i < n && i < lo + bs; ++i) ord.push_back(i);
            std::shuffle(ord.begin(), ord.end(), rng);
            double s = 0.0;
            uint32_t h = kManyNone;
            for (uint32_t i : ord) {
                const uint32_t cand = sc[i] > 0.0 ? hyp[i] : kManyNone;
                if (many_better(s, h, sc[i], cand)) {
                    s = sc[i];
                    h = cand;
                }
            }
            parts.emplace_back(s, h);
        }
        std::shuffle(parts.begin(), parts.end(), rng);
        double s = 0.0;
        uint32_t h = kManyNone;
        for (auto& p : parts)
            if (many_better(s, h, p.first, p.second)) {
                s = p.first;
                h = p.second;
            }
        CHECK(h == bh);
        CHECK(h == kManyNone || s == best);
    }
    CHECK(!many_better(1.0, 3, 0.0, kManyNone) && many_better(0.0, kManyNone, 1.0, 3));
    CHECK(many_better(1.0, 3, 1.0, 2) && !many_better(1.0, 2, 1.0, 3) && !many_better(1.0, 2, 1.0, 2));
}

int main() {
    std::mt19937_64 rng(1);
    int problems = 0;
    for (int solver : {GCR_SOLVER_HOMOGRAPHY4, GCR_SOLVER_FUNDAMENTAL7}) {
        const uint32_t S = solver == GCR_SOLVER_HOMOGRAPHY4 ? 24 : 6;
        for (int call = 0; call < 8; ++call) {
            Call c;
            const int P = 1 + (int)(rng() % 24);
            add_problem(c, rng, solver, 1);                        // m rows at the front of the buffer
            for (int p = 1; p + 1 < P; ++p) add_problem(c, rng, solver, (int)(rng() % 8 == 0 ? 2 : rng() % 5 == 0 ? 1 : 0));
            add_problem(c, rng, solver, 1);                        // ... and at its end
            check_call(c, solver, S);
            problems += (int)c.thr.size();
        }
        check_degenerate(solver, 5);
    }
    check_args();
    check_merge();
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("OK %d problems\n", problems);
    return 0;
}
