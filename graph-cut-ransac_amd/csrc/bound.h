// The bound path of gcr_problem_verify_batches ("k_bound"): the
// finish of a slot's raw MSAC accumulators, the rounding guard under which a
// slot's pre-band survivor count bounds that finish, and the list layout the
// kernels and the engine share.  Host and device; tests/cpp/bound_finish.cpp
// restates the sums around these functions.
#pragma once
#include <cstdint>

#include "gcr_hd.h"

namespace gcr {
namespace bnd {

// MSACScoringFunction::getScore's finish of the raw accumulators (tot, v0, v1:
// the sequential sums of -r^2 over all inliers, the scale and the orientation
// inliers), operation for operation what k_select and the fused scorer's chain
// wave compute.  classes = 1: the scale class alone.
GCR_HD double finish(double tot, double v0, double v1, uint32_t n0, uint32_t n1, uint32_t m0, uint32_t m1,
                            double T0, double T1, int classes) {
    if (n0 < m0 || (classes == 2 && n1 < m1)) return 0.0;
    double sum = tot;
    const double ms0 = v0 / T0 + static_cast<double>(n0);
    sum -= v0;
    sum += ms0;
    if (classes == 2) {
        const double ms1 = v1 / T1 + static_cast<double>(n1);
        sum -= v1;
        sum += ms1;
    }
    return sum;
}

// Largest excess of the computed finish over n0 + n1 for a slot of at most N
// inliers ("the bound path's rounding guard"):
//   (3 Tmax + 1) N^2 u (1 + N u)  from the three sequential sums, the v_c / T_c
//                                 terms included, and
//   16 N max(Tmax, 1) u           from the finish's eight operations,
// u = 2^-53, Tmax = max(T0, T1).  Bounded here by 4 (N^2 + 4 N) max(Tmax, 1) u,
// which needs N u <= 1 / 4 -- implied by the guard below.
GCR_HD double finish_excess(uint64_t N, double T0, double T1) {
    double tm = T0 > T1 ? T0 : T1;
    if (!(tm > 1.0)) tm = 1.0;
    const double n = static_cast<double>(N);
    return 4.0 * (n * n + 4.0 * n) * tm * 0x1p-53;
}

// The host's condition for the bound path: thresholds finite and positive and
// the excess at N = every feature of the problem at most 1/2, so that a slot
// whose bound ub0 + ub1 satisfies ub0 + ub1 + 1 <= S scores strictly below S.
// (!(x <= 0.5) also refuses NaN and infinity.)
GCR_HD bool guard_holds(uint64_t nfeatures, double T0, double T1, int classes) {
    if (!(T0 > 0.0) || !(T0 < 0x1p1000)) return false;
    if (classes == 2 && (!(T1 > 0.0) || !(T1 < 0x1p1000))) return false;
    if (nfeatures >= (1ull << 31)) return false;
    return finish_excess(nfeatures, T0, classes == 2 ? T1 : T0) <= 0.5;
}

// Per batch the two lists share one map / score array of list_stride(n, cap1)
// entries: the seeds at [0, cap1), the contenders from cap1 on.
GCR_HD uint32_t seed_cap(uint32_t seeds) {
    uint32_t c = 2u * seeds;
    if (c < 16u) c = 16u;
    return (c + 3u) & ~3u;
}
GCR_HD uint32_t list_stride(uint32_t nslots, uint32_t cap1) { return ((nslots + 3u) & ~3u) + cap1; }

// per-slot state the seed kernel leaves for the contender kernel
constexpr uint8_t kDead = 0, kLive = 1, kSeed = 2;

}  // namespace bnd
}  // namespace gcr
