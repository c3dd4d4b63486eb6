// match_geo.h -- guided matching: match.h's 2-nearest-neighbour search among
// the pairs a two-view model admits.  The definition (host and device) and the
// host twin.
//
// D1 (n1 x dim) and D2 (n2 x dim) are uint8 descriptors under match.h's rules;
// P1 (n1 x 2) and P2 (n2 x 2) are the keypoint positions, row-major doubles
// (x, y).  `kind` is one of the two residual kinds of solver.h, the homography
// (GCR_SOLVER_HOMOGRAPHY4 = 3, h_sq_residual of geo.h) or the fundamental
// matrix (GCR_SOLVER_FUNDAMENTAL7 = 4, f_sq_sampson of fund.h); h[9] is the
// model, row-major, T >= 0 a squared bound (+inf allowed).
//
//   adm(i, j) = geo_sq_residual<kind>(P1[i].x, P1[i].y, P2[j].x, P2[j].y, h) <= T
//
// in IEEE fp64 by exactly that operation tree: a NaN residual is not
// admissible, an infinite one only under T = +inf.  i is always a row of image
// 1 and j a row of image 2, so the admissible set does not depend on the
// search direction.
//   forward (reverse = 0): for every i the first two elements of match.h's
//     total order (d(i, j), j) among the admissible j; n1 results.
//   reverse (reverse = 1): for every j the first two elements of the order
//     (d(i, j), i) among the admissible i; n2 results.
// kMatchNone in idx and dist where a row has no admissible candidate, in idx2
// and dist2 where it has one.
//
// The kernels (match.hip) evaluate the residual FACTORISED: the terms that
// depend on one point only are computed once per point (match_geo_terms1 /
// match_geo_terms2), the rest per pair (match_geo_adm).  This is the one
// operation tree split where it stops depending on one side: every operation
// keeps its operands and its order, and the build has -ffp-contract=off, so
// the factorised value is the definition's, bit for bit
// (tests/cpp/match_geo_host.cpp holds the two against each other).
//
// Plain C++: tests/cpp/match_geo_host.cpp includes this header alone.
#pragma once

#include "fund.h"
#include "match.h"

namespace gcr {

constexpr int kMatchGeoHomography = 3;           // GCR_SOLVER_HOMOGRAPHY4 (held to it in engine.cpp)
constexpr int kMatchGeoFundamental = 4;          // GCR_SOLVER_FUNDAMENTAL7
constexpr int kMatchGeoTerms = 4;                // doubles per point of the factorised evaluation

// The terms of an image-1 point.  F: fx0, fx1, fx2, fx0^2 + fx1^2.  H: u, v
// (the transferred point), 0, 0.
template <int KIND>
GCR_HD void match_geo_terms1(double x1, double y1, const double* h, double* t) {
    if constexpr (KIND == kMatchGeoFundamental) {
        const double fx0 = (h[0] * x1 + h[1] * y1) + h[2];
        const double fx1 = (h[3] * x1 + h[4] * y1) + h[5];
        const double fx2 = (h[6] * x1 + h[7] * y1) + h[8];
        t[0] = fx0;
        t[1] = fx1;
        t[2] = fx2;
        t[3] = fx0 * fx0 + fx1 * fx1;
    } else {
        const double w = (h[6] * x1 + h[7] * y1) + h[8];
        t[0] = ((h[0] * x1 + h[1] * y1) + h[2]) / w;
        t[1] = ((h[3] * x1 + h[4] * y1) + h[5]) / w;
        t[2] = 0.0;
        t[3] = 0.0;
    }
}

// The terms of an image-2 point.  F: x2, y2, ft0^2, ft1^2.  H: x2, y2, 0, 0.
template <int KIND>
GCR_HD void match_geo_terms2(double x2, double y2, const double* h, double* t) {
    t[0] = x2;
    t[1] = y2;
    if constexpr (KIND == kMatchGeoFundamental) {
        const double ft0 = (h[0] * x2 + h[3] * y2) + h[6];
        const double ft1 = (h[1] * x2 + h[4] * y2) + h[7];
        t[2] = ft0 * ft0;
        t[3] = ft1 * ft1;
    } else {
        t[2] = 0.0;
        t[3] = 0.0;
    }
}

// geo_sq_residual<KIND> of the pair from the terms of P1[i] (one) and P2[j] (two)
template <int KIND>
GCR_HD double match_geo_sq(const double* one, const double* two) {
    if constexpr (KIND == kMatchGeoFundamental) {
        const double num = (two[0] * one[0] + two[1] * one[1]) + one[2];
        const double den = (one[3] + two[2]) + two[3];
        return (num * num) / den;
    } else {
        const double du = one[0] - two[0], dv = one[1] - two[1];
        return du * du + dv * dv;
    }
}

// adm(i, j); false for a NaN residual
template <int KIND>
GCR_HD bool match_geo_adm(const double* one, const double* two, double T) {
    return match_geo_sq<KIND>(one, two) <= T;
}

// nullptr, or the message naming the first bad one of kind, model and sq_threshold
// (the array entries and the resident sets' guided entry share it)
inline const char* match_geo_check_model(int kind, const double* model, double sq_threshold) {
    if (!model) return "match_descriptors_guided: model is NULL";
    if (kind != kMatchGeoHomography && kind != kMatchGeoFundamental)
        return "match_descriptors_guided: kind must be GCR_SOLVER_HOMOGRAPHY4 or GCR_SOLVER_FUNDAMENTAL7";
    if (!(sq_threshold >= 0.0)) return "match_descriptors_guided: sq_threshold must be >= 0 (+inf allowed), not NaN";
    for (int k = 0; k < 9; ++k)
        if (!(__builtin_fabs(model[k]) <= DBL_MAX)) return "match_descriptors_guided: model has a non-finite entry";
    return nullptr;
}

// nullptr, or the message naming the first bad argument
inline const char* match_geo_check_args(const void* d1, size_t n1, const void* p1, const void* d2, size_t n2,
                                        const void* p2, uint32_t dim, int kind, const double* model,
                                        double sq_threshold, int reverse, const void* idx, const void* dist,
                                        const void* idx2, const void* dist2) {
    if (const char* bad = match_check_args(d1, n1, d2, n2, dim, idx, dist, idx2, dist2)) return bad;
    if (!p1) return "match_descriptors_guided: p1 is NULL";
    if (!p2) return "match_descriptors_guided: p2 is NULL";
    if (const char* bad = match_geo_check_model(kind, model, sq_threshold)) return bad;
    if (reverse != 0 && reverse != 1) return "match_descriptors_guided: reverse must be 0 or 1";
    return nullptr;
}

// The definition: result rows [r0, r1) -- rows of image 1 forward, of image 2
// in reverse -- by plain loops.
template <int KIND>
inline void host_match_rows_guided_kind(const uint8_t* d1, size_t n1, const double* p1, const uint8_t* d2, size_t n2,
                                        const double* p2, uint32_t dim, const double* h, double T, int reverse,
                                        size_t r0, size_t r1, uint32_t* idx, uint32_t* dist, uint32_t* idx2,
                                        uint32_t* dist2) {
    const size_t ncols = reverse ? n1 : n2;
    for (size_t r = r0; r < r1; ++r) {
        uint32_t bd = kMatchNone, bc = kMatchNone, sd = kMatchNone, sc = kMatchNone;
        for (size_t c = 0; c < ncols; ++c) {
            const size_t i = reverse ? c : r, j = reverse ? r : c;
            if (!(geo_sq_residual<KIND>(p1[2 * i], p1[2 * i + 1], p2[2 * j], p2[2 * j + 1], h) <= T)) continue;
            const uint8_t* a = d1 + i * dim;
            const uint8_t* b = d2 + j * dim;
            uint32_t d = 0;
            for (uint32_t k = 0; k < dim; ++k) {
                const int32_t t = (int32_t)a[k] - (int32_t)b[k];
                d += (uint32_t)(t * t);
            }
            // c ascends, so an equal distance never displaces an earlier index
            if (d < bd) {
                sd = bd;
                sc = bc;
                bd = d;
                bc = (uint32_t)c;
            } else if (d < sd) {
                sd = d;
                sc = (uint32_t)c;
            }
        }
        idx[r] = bc;
        dist[r] = bd;
        idx2[r] = sc;
        dist2[r] = sd;
    }
}

inline void host_match_rows_guided(const uint8_t* d1, size_t n1, const double* p1, const uint8_t* d2, size_t n2,
                                   const double* p2, uint32_t dim, int kind, const double* h, double T, int reverse,
                                   size_t r0, size_t r1, uint32_t* idx, uint32_t* dist, uint32_t* idx2,
                                   uint32_t* dist2) {
    if (kind == kMatchGeoFundamental)
        host_match_rows_guided_kind<kMatchGeoFundamental>(d1, n1, p1, d2, n2, p2, dim, h, T, reverse, r0, r1, idx, dist,
                                                          idx2, dist2);
    else
        host_match_rows_guided_kind<kMatchGeoHomography>(d1, n1, p1, d2, n2, p2, dim, h, T, reverse, r0, r1, idx, dist,
                                                         idx2, dist2);
}

#if defined(__HIPCC__)
// One guided search on device memory (match.hip), as MatchDev: m.d1 / norm1 /
// n1 are the image of the RESULT rows (image 2 in reverse), m.d2 / norm2 / n2
// the other image; the terms are match_geo_terms_enqueue's.
struct MatchGeoDev {
    MatchDev m;
    const double* row_terms;    // [m.n1][kMatchGeoTerms]
    const double* col_terms;    // [m.n2][kMatchGeoTerms]
    double T;
    int kind, reverse;
};
// the factorised residual's per-point terms of image 1 (p1, n1 -> t1) and image 2 (p2, n2 -> t2)
void match_geo_terms_enqueue(hipStream_t stream, const double* p1, size_t n1, const double* p2, size_t n2,
                             const double* model, int kind, double* t1, double* t2);
// k_match_geo<dim / 32>, then k_match_merge for m.splits > 1
void match_geo_enqueue(hipStream_t stream, const MatchGeoDev& g);

// match.hip: uploads (descriptors, positions, model), runs the kernels on
// `stream`, downloads n1 (forward) or n2 (reverse) results.  ms_kernel (may be
// null): HIP-event time of the kernels alone.
hipError_t match_geo_device(hipStream_t stream, int n_cu, const uint8_t* d1, size_t n1, const double* p1,
                            const uint8_t* d2, size_t n2, const double* p2, uint32_t dim, int kind, const double* model,
                            double sq_threshold, int reverse, uint32_t* idx, uint32_t* dist, uint32_t* idx2,
                            uint32_t* dist2, double* ms_kernel);
#endif

}  // namespace gcr
