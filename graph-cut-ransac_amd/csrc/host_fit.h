// host_fit.h -- host-side model fitting for local optimisation and the final
// refit (the parts north_star keeps in host C++).  Per-feature constants come
// from the problem's precomputed SoA arrays; hypothesis-dependent angles use
// glibc, as the reference's fits do (models are never twin arithmetic).
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <type_traits>
#include <vector>

#include "ess.h"
#include "fund.h"
#include "geo.h"
#include "gram.h"
#include "grav.h"
#include "rect.h"
#include "solver.h"

namespace gcr {

// Per-class host copy of the features plus the precomputed per-feature
// constants (same values the GPU holds):
//   scale class:       c0 = pow(s, kScalePower)      (glibc, +1/3 or -1/3)
//   orientation class: c0 = cos(theta), c1 = sin(theta)
// std::vector storage that default-initialises (no zero fill on resize): the
// feature columns are filled in parallel right after sizing
template <class T>
struct DefaultInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = DefaultInitAlloc<U>;
    };
    DefaultInitAlloc() = default;
    template <class U>
    DefaultInitAlloc(const DefaultInitAlloc<U>&) noexcept {}
    template <class U>
    void construct(U* p) noexcept(std::is_nothrow_default_constructible<U>::value) {
        ::new (static_cast<void*>(p)) U;
    }
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};
using HVec = std::vector<double, DefaultInitAlloc<double>>;

struct HostClass {
    HVec x, y, a, c0, c1;
    size_t n = 0;
};

// Eigen ColPivHouseholderQR<MatrixX3d>::compute(A).solve(b) restated for an
// m x 3 column-major matrix (A and b are overwritten); qr3.h, blocked sums.
void colpiv_qr_solve3(std::vector<double>& A, size_t m, std::vector<double>& b, double x[3]);

// Another backend for the hybrid fit's least-squares system (the GPU refit):
// builds the ns scale rows + C(no, 2) vanishing-point pair rows of the index
// lists itself and solves them with qr3_solve; must be op-identical to the
// host path (rows as in fit_sift22, blocked sums).
struct SiftSystemSolver {
    virtual ~SiftSystemSolver() = default;
    virtual void solve(const std::vector<uint32_t>& si, const std::vector<uint32_t>& oi, size_t rows,
                       double x[3]) = 0;
    // the double-double Gram matrix of the same rows (gram.h order), ten
    // entries; false: not available here (the host computes it)
    virtual bool gram(const std::vector<uint32_t>& si, const std::vector<uint32_t>& oi, size_t rows,
                      DD g[kGramN]) { return false; }
    // fn(lo, hi) over [0, n) in disjoint ranges, possibly in parallel (the
    // per-inlier work around a big solve); the default runs it in one piece
    virtual void for_ranges(size_t n, const std::function<void(size_t, size_t)>& fn) { fn(0, n); }
};

// RectifyingHomographyEstimator::estimateModelNonminimal for the three solvers
// (rectifying_homography_estimator.h:164-227): normalisation check, then the
// minimal solver when the subset is exactly minimal, else weighted LS (+ mode).
// Hybrid systems with at least `big_rows` rows go to `big` when given.
bool fit_nonminimal(int solver, const HostClass* cls, const std::vector<uint32_t>* idx, RectModel& out,
                    SiftSystemSolver* big = nullptr, size_t big_rows = 0);

// Non-minimal homography fit (LO and final refit; geo.h): exactly 4 points ->
// the minimal solver; more -> Hartley-normalised DLT, h33 = 1, solved by the
// 8-column pivoted QR of qr3.h, denormalised and scaled to h33 = 1.
// Correspondences: c.x = x1, c.y = y1, c.a = x2, c.c0 = y2.
bool fit_h4_nonminimal(const HostClass& c, const std::vector<uint32_t>& idx, GeoModel& out);

// Non-minimal fundamental-matrix fit (LO and final refit; fund.h): exactly 7
// points -> the 7-point solver's first model; more -> normalised 8-point
// (smallest eigenvector of A^T A by cyclic Jacobi, rank-2 projection), unit
// Frobenius norm.  Blocked-order sums (qr3.h), restated by the oracle.
bool fit_f8_nonminimal(const HostClass& c, const std::vector<uint32_t>& idx, GeoModel& out);

// Non-minimal essential-matrix fit (LO and final refit; ess.h), on normalised
// correspondences: exactly 5 points -> the 5-point solver's first model; more
// -> the four eigenvectors of A^T A (rows in index order, sequential sums) with
// the smallest eigenvalues by cyclic Jacobi, as W (smallest), Z, Y, X; ess.h's
// steps 3-7 without the oriented test; of the up to kEModels candidates the
// one with the smallest sum of squared Sampson residuals over the listed
// points (sequential, the first on ties).
bool fit_e5_nonminimal(const HostClass& c, const std::vector<uint32_t>& idx, GeoModel& out);

// Non-minimal fit of the essential matrix with known gravity (LO and final
// refit; grav.h), on normalised correspondences.  3 or 4 points -> the
// 3-point solver's first model on the first three.  5 or more: in the aligned
// frames E' = [[a, b, d], [f, 0, g], [-d, h, a]], so q^T E' p is linear in
// v = (a, b, d, f, g, h) with the row (qx px + qz pz, qx py, qx pz - qz px,
// qy px, qy pz, qz py); v = the eigenvector of A^T A (rows in index order,
// sequential sums) with the smallest eigenvalue by cyclic Jacobi, the lowest
// index on ties.  v is projected onto {[t]x R_y} by this rule:
//   a = -ty sn, d = ty c, b = -tz, h = tx, f = tz c + tx sn, g = tz sn - tx c;
//   tx0 = h, tz0 = -b, nc = tz0 f - tx0 g, ns = tx0 f + tz0 g
//     (= (c, sn) (tx^2 + tz^2) on the set);
//   ty and theta from (a, d): (c, sn) = (d, -a) / sqrt(a^2 + d^2), or its
//     negative where that leaves the smaller residual in (f, g), which is
//     where c nc + sn ns < 0;
//   but where (a, d) is lost in v's own error, a^2 + d^2 <=
//     max(lambda_min / lambda_next of A^T A, 1e-12) (no vertical translation,
//     or one small against the noise: (a, d) carries no angle), theta from
//     (b, f, g, h): (c, sn) = (nc, ns) over its norm, if that is > 0;
//   a zero norm of whichever pair is used: no model;
//   ty = d c - a sn, tx = (tx0 + (sn f - c g)) / 2, tz = (tz0 + (c f + sn g)) / 2
//     (the least-squares t given the angle).
// E = G2^T E' G1 at unit Frobenius norm by grav.h's step 7, without the
// oriented test.  The returned model always has the constrained form.
bool fit_g3_nonminimal(const HostClass& c, const std::vector<uint32_t>& idx, const GravRot& rot, GeoModel& out);

// Cyclic Jacobi eigen-decomposition of a symmetric N x N matrix (a is
// destroyed); eigenvalues d[k] with eigenvectors in the COLUMNS of v.
template <int N>
void jacobi_eigen(double (&a)[N][N], double (&v)[N][N], double (&d)[N]);

// findWeightedMode (two_sift.hpp:354-394), libstdc++ unordered_map order.
double weighted_mode(const std::vector<double>& angles, const std::vector<double>& weights, double bin_width);

// The hybrid system's Gram matrix on the host, in gram.h's order (tiles,
// 256 lanes, halving tree, tiles in order): bit-identical to the GPU kernel.
void gram_sift_host(const HostClass& sc, const HostClass& oc, const std::vector<uint32_t>& si,
                    const std::vector<uint32_t>& oi, size_t rows, DD g[kGramN]);
// min |A x - b| from the Gram matrix of [A | b] (gram.h): column-pivoted
// Cholesky in double-double with Eigen's pivot rule and rank threshold.
void gram_solve3(const DD g[kGramN], size_t rows, double x[3]);
// GCR_REFIT=qr: big hybrid systems by Householder QR (round 2) instead
bool gram_refit_on();

// RectifyingHomography::getHomography (model.h:211-226), row-major, / H22.
void homography_of(const RectModel& m, double H[9]);

}  // namespace gcr
