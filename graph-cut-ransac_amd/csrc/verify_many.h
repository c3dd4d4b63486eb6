// verify_many.h -- the best RANSAC hypothesis of many small problems per call
// (gcr_verify_many; the kernels are k_many / k_many_merge / k_many_mask at the
// end of kernels.hip).  This header is the definition: the rule, and its host
// twin as plain loops over the GCR_HD functions the kernels call.
//
// A call has one kind (GCR_SOLVER_HOMOGRAPHY4 or GCR_SOLVER_FUNDAMENTAL7, m = 4
// or 7 rows per sample, per = 1 or 3 hypotheses per slot) and one slot count S
// (1 .. 65536).  Problem p has n_p >= m rows (x1, y1, x2, y2), a threshold
// thr_p in pixels and a seed.  Its result is what
// gcr_problem_verify_batch(prob, params, 0, S) gives for those rows alone with
// the uniform sampler, params.seed = seed_p and the threshold in params:
//
//   generation  slot s tries attempts a = 0 .. 100 in order and keeps the
//               first that yields a model: the uniform draw of m rows from
//               Philox (seed_p, s, a), then valid_sample_h4 + solve_h4 (one
//               model), or fund.h's 7-point solver (0 .. 3 models, hypotheses
//               3 s + k).  inc = a + 1, or 102 when all 101 fail; the
//               fundamental matrix's extra / absent hypotheses carry the
//               markers 0 / 255, which add no iterations.
//   score       per hypothesis, over the rows in order: r2 =
//               geo_sq_residual<KIND>(row, model); if (r2 <= T) { n0 += 1;
//               v0 += -r2; } from n0 = 0, v0 = +0.0, T = msac_sq_threshold(thr_p).
//   selection   sum = v0; if (n0 < m) sum = 0; else { msac = v0 / T +
//               double(n0); sum -= v0; sum += msac; }; the first strict
//               maximum above 0 in hypothesis order (many_better: the higher
//               score, on equal scores the lower hypothesis, "none" loses --
//               associative and commutative, so partial bests merge in any
//               order and blocking).  models = live hypotheses, iterations =
//               the sum of inc.
//   mask        row i: r2 <= T under the best hypothesis' own model
//               (mask_rule 0, what gcr_debug_mask_h computes); all zero without
//               a best.  Its sum is best_inliers: the same residual, the same T.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "exact.h"
#include "fund.h"
#include "geo.h"
#include "philox.h"
#include "solver.h"

namespace gcr {

constexpr uint32_t kManyMaxSlots = 65536;
constexpr uint32_t kManyNone = 0xffffffffu;     // hypothesis index of "no best"

// The MSAC threshold on r^2 that the scorers get (MSAC_scoring_function.hpp:64):
// the runner of gcr_problem_verify_batch(es) takes it from here too.
GCR_HD double msac_sq_threshold(double thr) { return (2.25 * thr) * thr; }

// k_select's finish of one hypothesis' raw accumulators (one class, tot = v0)
GCR_HD double many_finish_score(uint32_t n0, double v0, uint32_t m, double Tm) {
    double sum = v0;
    if (n0 < m) {
        sum = 0.0;
    } else {
        const double msac = v0 / Tm + static_cast<double>(n0);
        sum -= v0;
        sum += msac;
    }
    return sum;
}

// Is candidate b (score sb, hypothesis hb) better than a?  A candidate is a
// hypothesis whose score is above 0, or none (kManyNone).  The order is total
// on distinct hypotheses, so the merge is associative and commutative.
GCR_HD bool many_better(double sa, uint32_t ha, double sb, uint32_t hb) {
    return hb != kManyNone && (ha == kManyNone || sb > sa || (sb == sa && hb < ha));
}

// The generators' uniform draw (kernels.hip draw_sample<M> with UniformDraw):
// m <= 32 distinct rows of n for (seed, index, sub, stream, class).
inline bool host_sample_uniform(uint64_t seed, uint64_t index, uint32_t sub, uint32_t stream, uint32_t cls,
                                uint64_t n, uint32_t m, uint32_t* out) {
    WordStream ws(seed, index, sub, stream, cls);
    return sample_distinct<32>(ws, n, (int)m, out);
}

// What an attempt does with its sample (kernels.hip attempt<3> / attempt_f and
// the winning lane's models): 0 .. 3 models of 9 doubles each in models_out.
inline uint32_t host_solve_minimal_hf(int solver, const double* x1, const double* y1, const double* x2,
                                      const double* y2, double* models_out) {
    if (solver == GCR_SOLVER_HOMOGRAPHY4) {
        GeoModel g = default_geo();
        if (!valid_sample_h4(x1, y1, x2, y2) || !solve_h4(x1, y1, x2, y2, g)) return 0;
        for (int q = 0; q < 9; ++q) models_out[q] = g.h[q];
        return 1;
    }
    F7Basis b;
    if (solve_f7_basis(x1, y1, x2, y2, b) == 0) return 0;
    uint32_t k = 0;
    for (int q = 0; q < 3; ++q)
        if (b.valid & (1u << q)) {
            f7_model(b, f7_root(b, q), models_out + 9 * k);
            ++k;
        }
    return k;
}

// Every argument but the rows' values; an empty string if they are good.
inline std::string many_check_shape(int solver, const double* rows, const uint64_t* row_offset, size_t nproblems,
                                    const double* thresholds, const uint64_t* seeds, uint32_t nslots,
                                    const void* out) {
    char buf[200];
    if (solver != GCR_SOLVER_HOMOGRAPHY4 && solver != GCR_SOLVER_FUNDAMENTAL7)
        return "verify_many: solver must be GCR_SOLVER_HOMOGRAPHY4 or GCR_SOLVER_FUNDAMENTAL7";
    if (nproblems == 0) return "verify_many: nproblems is 0";
    if (!rows) return "verify_many: rows is NULL";
    if (!row_offset) return "verify_many: row_offset is NULL";
    if (!thresholds) return "verify_many: thresholds is NULL";
    if (!seeds) return "verify_many: seeds is NULL";
    if (!out) return "verify_many: out is NULL";
    if (nslots < 1 || nslots > kManyMaxSlots) {
        snprintf(buf, sizeof(buf), "verify_many: nslots = %u is outside 1 .. %u", nslots, kManyMaxSlots);
        return buf;
    }
    if (row_offset[0] != 0) return "verify_many: row_offset[0] is not 0";
    const uint64_t m = (uint64_t)solver_row(solver).m;
    for (size_t p = 0; p < nproblems; ++p) {
        if (row_offset[p + 1] < row_offset[p]) {
            snprintf(buf, sizeof(buf), "verify_many: row_offset[%zu] descends", p + 1);
            return buf;
        }
        if (row_offset[p + 1] - row_offset[p] < m) {
            snprintf(buf, sizeof(buf), "verify_many: problem %zu has %llu rows, fewer than a sample of %llu", p,
                     (unsigned long long)(row_offset[p + 1] - row_offset[p]), (unsigned long long)m);
            return buf;
        }
        if (row_offset[p + 1] >= (1ull << 32)) return "verify_many: 2^32 rows or more in one call";
        if (!(thresholds[p] > 0.0) || !(thresholds[p] < HUGE_VAL)) {
            snprintf(buf, sizeof(buf), "verify_many: thresholds[%zu] is not finite and > 0", p);
            return buf;
        }
    }
    return std::string();
}

// the first of `count` doubles that is not finite, or -1
inline ptrdiff_t many_first_nonfinite(const double* v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!(v[i] - v[i] == 0.0)) return (ptrdiff_t)i;
    return -1;
}

inline std::string many_bad_row(size_t p, size_t i) {
    char buf[120];
    snprintf(buf, sizeof(buf), "verify_many: row %zu of problem %zu is not finite", i, p);
    return buf;
}

// One problem by plain loops.  mask: n bytes or null.
template <int KIND>
inline void host_verify_one(const double* rows, size_t n, double thr, uint64_t seed, uint32_t nslots,
                            gcr_many_result* out, uint8_t* mask) {
    constexpr uint32_t kM = KIND == 4 ? 7 : 4;
    constexpr uint32_t kPer = KIND == 4 ? (uint32_t)kFModels : 1u;
    const double T = msac_sq_threshold(thr);
    gcr_many_result r{};
    r.best_slot = -1;
    const GeoModel def = default_geo();
    for (int q = 0; q < 9; ++q) r.best_model[q] = def.h[q];
    double best = 0.0;
    uint32_t bh = kManyNone;
    for (uint32_t s = 0; s < nslots; ++s) {
        uint32_t inc = 102, cnt = 0;
        double ms[9 * 3];
        for (uint32_t a = 0; a < 101 && cnt == 0; ++a) {
            uint32_t idx[kM];
            if (!host_sample_uniform(seed, s, a, kStreamMain, 0, n, kM, idx)) continue;
            double x1[kM], y1[kM], x2[kM], y2[kM];
            for (uint32_t j = 0; j < kM; ++j) {
                const double* row = rows + 4 * (size_t)idx[j];
                x1[j] = row[0];
                y1[j] = row[1];
                x2[j] = row[2];
                y2[j] = row[3];
            }
            cnt = host_solve_minimal_hf(KIND, x1, y1, x2, y2, ms);
            if (cnt) inc = a + 1;
        }
        r.iterations += inc;            // the markers 0 / 255 of hypotheses 3 s + 1, 3 s + 2 add nothing
        for (uint32_t k = 0; k < cnt; ++k) {
            ++r.models;
            const double* h = ms + 9 * k;
            uint32_t n0 = 0;
            double v0 = 0.0;
            for (size_t i = 0; i < n; ++i) {
                const double* row = rows + 4 * i;
                const double r2 = geo_sq_residual<KIND>(row[0], row[1], row[2], row[3], h);
                if (r2 <= T) {
                    n0 += 1;
                    v0 += -r2;
                }
            }
            const double sum = many_finish_score(n0, v0, kM, T);
            if (best < sum) {           // first strict maximum above 0, hypotheses in order
                best = sum;
                bh = s * kPer + k;
                r.best_inliers = n0;
                for (int q = 0; q < 9; ++q) r.best_model[q] = h[q];
            }
        }
    }
    if (bh != kManyNone) {
        r.best_slot = (int64_t)(bh / kPer);
        r.best_hypothesis = bh % kPer;
        r.best_score = best;
    }
    *out = r;
    if (mask != nullptr)
        for (size_t i = 0; i < n; ++i) {
            const double* row = rows + 4 * i;
            mask[i] = bh != kManyNone &&
                              mask_rule(geo_sq_residual<KIND>(row[0], row[1], row[2], row[3], r.best_model), 0, T, 0.0)
                          ? 1
                          : 0;
        }
}

// The host twin of gcr_verify_many: arguments already checked
// (many_check_shape, many_first_nonfinite).  Up to 16 threads over problems.
inline void host_verify_many(int solver, const double* rows, const uint64_t* row_offset, size_t nproblems,
                             const double* thresholds, const uint64_t* seeds, uint32_t nslots, int threads,
                             gcr_many_result* out, uint8_t* masks_out) {
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t p; (p = next.fetch_add(1)) < nproblems;) {
            const double* r = rows + 4 * row_offset[p];
            const size_t n = (size_t)(row_offset[p + 1] - row_offset[p]);
            uint8_t* mk = masks_out ? masks_out + row_offset[p] : nullptr;
            if (solver == GCR_SOLVER_FUNDAMENTAL7) host_verify_one<4>(r, n, thresholds[p], seeds[p], nslots, out + p, mk);
            else host_verify_one<3>(r, n, thresholds[p], seeds[p], nslots, out + p, mk);
        }
    };
    size_t nt = (size_t)(threads < 1 ? 1 : (threads > 16 ? 16 : threads));
    if (nt > nproblems) nt = nproblems;
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
}

}  // namespace gcr
