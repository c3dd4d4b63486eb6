// guided_stop.h -- the adaptive stop of a guided run (GCR_FLAG_GUIDED_STOP).
// The reference's bound log(1 - conf) / log(1 - (I / N)^m) (GCRANSAC.h:738-757)
// assumes every correspondence is drawn with probability 1 / N.  guided.h
// draws correspondence i with probability w[i] / W, so a sample is all-inlier
// with probability (W_I / W)^m, W_I the weight of the best model's inliers:
// the inlier MASS takes the place of the inlier count.  There is no reference
// for it, so this is the definition:
//
//   quanta  the weights as unsigned integers, fixed once on the host when the
//           weights are accepted: b = bit_length(N), K = 52 - b, total = the
//           CDF's last entry (guided.h), r_i = w_i / total (one fp64 division,
//           r_i <= 1), q_i = (uint64_t)(r_i * 2^K) (an exact scaling, then
//           truncation), Q = sum q_i.  q_i <= 2^K and N < 2^b, so Q < 2^52:
//           every partial sum of quanta is an exact integer below 2^53, a
//           reduction in any order gives the same bits and (double) of it is
//           exact.  w_i == 0 gives q_i == 0; equal weights give equal quanta.
//           Q == 0 (every r_i < 2^-K: possible only for N >= 2^26) leaves
//           nothing to measure, and the flag is refused.
//   mass    of a model: sum of q_i over the correspondences the scorer counts
//           as inliers (r^2 <= (2.25 thr) thr with the scorer's own residual,
//           fund.h geo_sq_residual); count is their number and equals the
//           scorer's n0 of that model.
//   stop    iteration_number_guided: the reference's formula with ratio =
//           (double)mass / (double)Q in place of I / N, otherwise line for
//           line the same (pow, log(1 - q), the epsilon guard, ceil).
//
// With all-equal weights mass / Q = (I q_1) / (N q_1); both products are exact,
// so the correctly rounded quotient equals I / N bit for bit: the guided stop
// with equal weights IS the uniform stop.
//
// (W_I / W)^m ignores the rejection of repeated indices inside a sample,
// exactly as (I / N)^m does (a sample is m DISTINCT draws in both).  Under
// uniform sampling that error is O(m^2 / N); here it is of the order of m^2
// times the largest single share w_i / W, so the bound is meaningful when no
// single weight dominates W -- a correspondence holding most of the weight
// is drawn once per sample at most, however large its share makes the ratio.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#include "gcr_hd.h"

namespace gcr {

// b = bit_length(n), K = 52 - b (n < 2^33: K >= 19)
GCR_HD int guided_quanta_shift(uint64_t n) {
    int b = 0;
    while (n) {
        ++b;
        n >>= 1;
    }
    return 52 - b;
}

// q_i of weight w (finite, 0 <= w <= total, total > 0)
GCR_HD uint64_t guided_quantum(double w, double total, int K) {
    const double r = w / total;
    return (uint64_t)(r * (double)(1ull << K));
}

// GCRANSAC::getIterationNumber (GCRANSAC.h:738-757) on the inlier mass;
// log_prob = log(1 - confidence)
inline uint64_t iteration_number_guided(uint64_t mass, uint64_t Q, uint32_t m, double log_prob) {
    const double ratio = static_cast<double>(mass) / static_cast<double>(Q);
    const double q = 1.0 * std::pow(ratio, static_cast<double>(m));
    const double lg = std::log(1 - q);
    if (std::fabs(lg) < std::numeric_limits<double>::epsilon()) return std::numeric_limits<uint64_t>::max();
    return static_cast<uint64_t>(std::ceil(log_prob / lg));
}

}  // namespace gcr
