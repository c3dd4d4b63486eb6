// prosac_stop.h -- the adaptive stop of a PROSAC run (GCR_FLAG_PROSAC_STOP).
// The reference's bound log(1 - conf) / log(1 - (I / N)^m) (GCRANSAC.h:738-757)
// assumes every sample is drawn from all N rows.  prosac.h draws the early
// slots from the best-ranked rows, so a model whose inliers crowd the top of
// the order is hit far sooner than I / N says: PROSAC's own stop (Chum & Matas,
// CVPR 2005, section 2.2) looks for the prefix length n* whose inlier share
// I_n / n is the largest one the samples drawn so far can answer for.  There is
// no reference for it (the reference has its PROSAC sampler commented out), so
// this is the definition:
//
//   I_n      of a model: the number of its inliers among the first n rows, the
//            rows in quality order as gcr_problem_set_prosac requires.  The
//            inlier decision is the scorer's own (r^2 <= (2.25 thr) thr with
//            fund.h's geo_sq_residual, k_inlier_mass's test); I_N equals the
//            scorer's n0 of that model.
//   candidates  n = N always.  n in [max(m, kProsacStopMinLength), N) when both
//            hold:
//     non-randomness  I_n >= Imin[n], Imin[n] = m + (uint32_t)ceil(n b + z
//            sqrt(n b (1 - b))), b = kProsacStopBeta = 0.05, z =
//            kProsacStopZ = 1.6448536269514722: the normal approximation of
//            the paper's binomial tail at 5 %.  A uint32_t table built once on
//            the host in fp64 (prosac_stop_imin: nb = n * b, v = nb * (1 - b),
//            s = sqrt(v), zs = z * s, t = nb + zs, every operation rounded
//            singly and in this order, sqrt correctly rounded on both sides).
//     coverage  the bound for the top n rows may only count samples drawn from
//            the top n rows.  Slot s has pool <= n exactly when s < g[n]
//            (prosac.h), so the bound k_n must not exceed g[n].  Without
//            transcendentals on the device: r = (double)I_n / (double)n (one
//            IEEE division), q = r multiplied by r another m - 1 times, left
//            to right (plain multiplications: no FMA can arise), and the
//            condition is q >= qmin[n], qmin[n] = 1.0 - exp(log_prob /
//            (double)g[n]) -- a host table, glibc exp, one call per n, for the
//            run's log_prob = log(1 - confidence).  Device and host twin run
//            the same function (prosac_stop_feasible), so feasibility is the
//            same bit on both sides.
//   choice   among the candidates the largest I_n / n, compared exactly as
//            I_a n_b against I_b n_a in uint64_t (N < 2^32); on equal ratios
//            the larger n.  A total order: any reduction tree gives the same
//            (I*, n*).
//   stop     iteration_number_prosac: the reference's formula with ratio =
//            (double)I* / (double)n* in place of I / N, otherwise line for
//            line the same (pow, log(1 - q), the epsilon guard, ceil).
//
//   when     wherever the uniform run updates max_iteration, with the model
//            that is the best at that point: a generated hypothesis that
//            becomes the best takes its own (I*, n*), and after a local
//            optimisation the best it leaves (the LO model if it won, else the
//            model that went in) takes its own again.  A hypothesis that does
//            not become the best never moves the stop.  The oracle's run loop
//            (oracle/gcr_oracle.cpp, stopNumber) states this independently, and
//            tests/test_gpu_oracle_samplers.py compares whole flagged runs
//            with it bitwise.
//
// With n* = N the formula is the uniform stop bit for bit, and (I_N, N) is
// always a candidate, so I* / n* >= I_N / N: the flag can only lower
// max_iteration, never raise it.  The result is a function of the model and
// the problem's tables alone, so replay, batch_slots independence and sharding
// hold as they do for the guided stop's mass.
//
// Caveats, left as they are.  The maximum over n is biased upward, as PROSAC's
// own n* is: a simulation with scores that carry no information gave 2357-3086
// against the uniform 3062-3144 iterations at 80 % outliers, m = 4; without
// the coverage condition it was 56 010 against 402 780 at m = 7.  b is a fixed
// constant, not estimated from the data.  (I / n)^m ignores the rejection of
// repeated indices inside a sample, as (I / N)^m does everywhere else.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#include "gcr_hd.h"

namespace gcr {

constexpr uint32_t kProsacStopMinLength = 20;
constexpr double kProsacStopBeta = 0.05;
constexpr double kProsacStopZ = 1.6448536269514722;

// Imin[n] (host; n >= 1)
inline uint32_t prosac_stop_imin(uint32_t n, uint32_t m) {
    const double nb = (double)n * kProsacStopBeta;
    const double v = nb * (1.0 - kProsacStopBeta);
    const double s = std::sqrt(v);
    const double zs = kProsacStopZ * s;
    const double t = nb + zs;
    return m + (uint32_t)std::ceil(t);
}

// qmin[n] of growth entry g_n >= 1 (host)
inline double prosac_stop_qmin(uint64_t g_n, double log_prob) { return 1.0 - std::exp(log_prob / (double)g_n); }

// the tables of a problem of n rows with growth table g (n + 1 entries);
// imin_out / qmin_out: n + 1 entries each, those below m are 0.  Either
// output may be null.
inline void prosac_stop_tables(const uint64_t* g, uint32_t n, uint32_t m, double log_prob, uint32_t* imin_out,
                               double* qmin_out) {
    for (uint32_t k = 0; k <= n; ++k) {
        if (imin_out) imin_out[k] = k < m ? 0u : prosac_stop_imin(k, m);
        if (qmin_out) qmin_out[k] = k < m ? 0.0 : prosac_stop_qmin(g[k], log_prob);
    }
}

// first prefix length that can be a candidate besides N
GCR_HD uint32_t prosac_stop_first(uint32_t m) { return m > kProsacStopMinLength ? m : kProsacStopMinLength; }

// both conditions of prefix length n (prosac_stop_first(m) <= n < N) holding
// I of the model's inliers
GCR_HD bool prosac_stop_feasible(uint32_t I, uint32_t n, uint32_t m, uint32_t imin, double qmin) {
    if (I < imin) return false;
    const double r = (double)I / (double)n;
    double q = r;
    for (uint32_t k = 1; k < m; ++k) q = q * r;
    return q >= qmin;
}

// the choice's order: (Ia, na) before (Ib, nb)
GCR_HD bool prosac_stop_better(uint32_t Ia, uint32_t na, uint32_t Ib, uint32_t nb) {
    const uint64_t l = (uint64_t)Ia * (uint64_t)nb, r = (uint64_t)Ib * (uint64_t)na;
    return l > r || (l == r && na > nb);
}

// the host twin of k_prosac_stop: (I*, n*) of the inlier mask (n entries,
// nonzero: inlier) in row order
inline void prosac_stop_choose(const uint8_t* mask, uint32_t n, uint32_t m, const uint32_t* imin, const double* qmin,
                               uint32_t* best_i, uint32_t* best_n) {
    uint32_t I = 0, bi = 0, bn = 0;
    bool have = false;
    const uint32_t first = prosac_stop_first(m);
    for (uint32_t k = 1; k <= n; ++k) {
        I += mask[k - 1] ? 1u : 0u;
        const bool cand = k == n || (k >= first && prosac_stop_feasible(I, k, m, imin[k], qmin[k]));
        if (cand && (!have || prosac_stop_better(I, k, bi, bn))) {
            bi = I;
            bn = k;
            have = true;
        }
    }
    *best_i = bi;
    *best_n = bn;
}

// GCRANSAC::getIterationNumber (GCRANSAC.h:738-757) on the chosen prefix;
// log_prob = log(1 - confidence)
inline uint64_t iteration_number_prosac(uint32_t best_i, uint32_t best_n, uint32_t m, double log_prob) {
    const double ratio = static_cast<double>(best_i) / static_cast<double>(best_n);
    const double q = 1.0 * std::pow(ratio, static_cast<double>(m));
    const double lg = std::log(1 - q);
    if (std::fabs(lg) < std::numeric_limits<double>::epsilon()) return std::numeric_limits<uint64_t>::max();
    return static_cast<uint64_t>(std::ceil(log_prob / lg));
}

}  // namespace gcr
