// sifth.h -- homography from two SIFT correspondences (point, feature size,
// orientation in both images): the minimal solver of the hot path, host and
// device (GCR_HD).
//
// Upstream GC-RANSAC ships a SIFT-based homography solver; it is not part of
// this project's sources and parity with it is unpinned.  As with fund.h,
// ess.h and grav.h this header is the definition.  The same code runs on both
// sides with -ffp-contract=off and uses +, -, *, / and sqrt only, in one
// fixed order; trig is evaluated once on the host when a problem is created
// (sift_row) and both sides read the stored doubles.
//
// Input per correspondence: x1, y1, x2, y2 in pixels and the stored columns
// r = (q2 / q1)^2, cos / sin of alpha1 and of alpha2 (q: feature sizes as
// lengths, alpha: orientations in radians).
//
// Constraints: with X = (x1, y1, 1), s = h3 . X and
//   B = [[h11 - x2 h31, h12 - x2 h32], [h21 - y2 h31, h22 - y2 h32]]
// the local affine map of H at X is B / s.  d_k = (cos alpha_k, sin alpha_k),
// n2 = (-sin alpha2, cos alpha2).  Per correspondence
//   1. h1 . X - x2 (h3 . X) = 0, h2 . X - y2 (h3 . X) = 0      (the DLT rows)
//   2. n2^T B d1 = 0                                           (linear in h)
//   3. det B - r (h3 . X)^2 = 0                                (quadratic)
// Two correspondences: 6 linear and 2 quadratic equations in 9 entries.
//
//   (a) normalise: each image is translated to the midpoint of the sample's
//       two points and scaled by k = 1 / (half their distance); orientations
//       stay, r becomes r (k2 / k1)^2.  A sample whose half distance in either
//       image is not above kSCoincide (1 + |mx| + |my|), m the midpoint, is
//       rejected (coincident points);
//   (b) the 6 x 9 system (rows: the DLT x rows of correspondences 0 and 1,
//       their DLT y rows, their orientation rows; columns h11 .. h33 row-
//       major) is eliminated on columns 0..5 with partial (row)
//       pivoting, fund.h's manner for its 7 x 9 basis; a pivot not above
//       kSRankTol rejects the sample.  The free entries are h31, h32, h33:
//       h = a n1 + b n2 + n3 with (h31, h32, h33) = (1, 0, 0), (0, 1, 0),
//       (0, 0, 1) for n1, n2, n3.  Homographies with h33 = 0 in the normalised
//       frames (the midpoint of image 1 goes to infinity) and samples whose
//       first six columns are dependent (parallel orientations in image 2, an
//       orientation in image 1 along the line between the points) are
//       outside this chart and are not found;
//   (c) every entry of B and s is a linear form in (a, b, 1); the quadratic of
//       correspondence i is the conic A_i a^2 + P_i(b) a + R_i(b), deg P = 1,
//       deg R = 2 (conic()).  u = A1 R2 - A2 R1, v = A1 P2 - A2 P1,
//       w = P1 R2 - P2 R1, and the resultant in b is u^2 - v w, each
//       coefficient summed as written below.  Its b^4 coefficient
//       u2^2 - v1 w3 is zero in exact arithmetic: after (a) the two points of
//       image 1 are X and (-x, -y, 1), and the rank-one matrix
//       (alpha, beta, gamma)^T (y, -x, 0) satisfies all eight equations with
//       h33 = 0 (s = 0 and B of rank one at both points; the two orientation
//       rows fix (alpha, beta, gamma)), so one of the four solutions always
//       lies at infinity of the chart.  What the computed coefficient holds
//       is rounding, and it is dropped: the polynomial is a cubic, a sample
//       yields up to three models;
//   (d) real roots b in ascending order: fund.h's real_roots_cubic, the path
//       the 7-point solver's cubic takes.  a = -u(b) / v(b); the root is
//       dropped when |v(b)| is not above kSVTol (|v0| + |v1 b|);
//   (e) h = (n1 a + n2 b) + n3.  The candidate is dropped when an entry is not
//       finite, when s_0 s_1 <= 0, or when (d2^T B d1) s <= 0 for either
//       correspondence (the first orientation must map onto the second, not
//       its opposite).  H = T2^-1 h T1; dropped when |H33| is not above
//       kSH33Tol max |H_jk|; then H / H33 with H33 = 1 exactly, and solve_h4's
//       validity: every entry finite and below 1e300 in magnitude.
// Survivors are returned in ascending root order.  On synthetic scenes all but
// about 1e-5 of the samples that yield a model yield exactly one: of the
// three finite solutions the sign tests of (e) keep the one whose affine maps
// preserve both orientations.  The exceptions are pairs of nearly rank-one
// matrices next to the solution at infinity (s of order 1e-5 |h3| |X|), which
// score nothing.
#pragma once

#include "gcr_hd.h"
#include "fund.h"
#include "geo.h"

namespace gcr {

constexpr int kSModels = 3;              // real roots of the cubic, models per sample
constexpr double kSCoincide = 1e-10;     // (a): half distance over 1 + |midpoint|
constexpr double kSRankTol = 1e-10;      // (b): smallest pivot of the normalised system
constexpr double kSVTol = 1e-12;         // (d): |v(b)| over |v0| + |v1 b|
constexpr double kSH33Tol = 1e-12;       // (e): |H33| over the largest entry

// The stored SIFT columns of a problem, one entry per correspondence: device
// pointers for the generator launches, host pointers for the host twin.
// DevProblem does not carry them.
struct SiftCols {
    const double* r;      // (q2 / q1)^2
    const double* c1;     // cos alpha1
    const double* s1;     // sin alpha1
    const double* c2;     // cos alpha2
    const double* s2;     // sin alpha2
};

// the SIFT side of a two-correspondence sample
struct SiftPair {
    double r[2], c1[2], s1[2], c2[2], s2[2];
};

namespace sifth {

// product of the linear forms l and m in (a, b, 1), added to the conic
// (aa, ab, bb, a, b, 1) with sign sg
GCR_HD void add_prod(double (&q)[6], const double (&l)[3], const double (&m)[3], double sg) {
    q[0] = q[0] + sg * (l[0] * m[0]);
    q[1] = q[1] + sg * (l[0] * m[1] + l[1] * m[0]);
    q[2] = q[2] + sg * (l[1] * m[1]);
    q[3] = q[3] + sg * (l[0] * m[2] + l[2] * m[0]);
    q[4] = q[4] + sg * (l[1] * m[2] + l[2] * m[1]);
    q[5] = q[5] + sg * (l[2] * m[2]);
}

// Step (c), one correspondence: det B - r s^2 as a conic, the products added
// in the order B11 B22, - B12 B21, - r s s.  n1 / n2 / n3: the basis' first six
// entries; (x, y) -> (x2, y2) normalised.
GCR_HD void conic(const double (&n1)[6], const double (&n2)[6], const double (&n3)[6], double x, double y, double x2,
                  double y2, double r, double (&q)[6]) {
    const double b11[3] = {n1[0] - x2, n2[0], n3[0]};
    const double b12[3] = {n1[1], n2[1] - x2, n3[1]};
    const double b21[3] = {n1[3] - y2, n2[3], n3[3]};
    const double b22[3] = {n1[4], n2[4] - y2, n3[4]};
    const double s[3] = {x, y, 1.0};
    const double rs[3] = {r * x, r * y, r};
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = 0.0;
    add_prod(q, b11, b22, 1.0);
    add_prod(q, b12, b21, -1.0);
    add_prod(q, rs, s, -1.0);
}

}  // namespace sifth

// The 2-point solver with every model in a fixed position: ms[t] is the model
// of root position t where bit t of the result is set (ascending roots over
// the set bits).  No array is indexed at run time.
GCR_HD unsigned solve_s2_slots(const double x1[2], const double y1[2], const double x2[2], const double y2[2],
                               const SiftPair& sp, GeoModel (&ms)[kSModels]) {
    using namespace sifth;
    // (a)
    const double m1x = 0.5 * (x1[0] + x1[1]), m1y = 0.5 * (y1[0] + y1[1]);
    const double m2x = 0.5 * (x2[0] + x2[1]), m2y = 0.5 * (y2[0] + y2[1]);
    const double e1x = x1[1] - x1[0], e1y = y1[1] - y1[0];
    const double e2x = x2[1] - x2[0], e2y = y2[1] - y2[0];
    const double d1 = 0.5 * sqrt(e1x * e1x + e1y * e1y);
    const double d2 = 0.5 * sqrt(e2x * e2x + e2y * e2y);
    if (!(d1 > kSCoincide * ((1.0 + __builtin_fabs(m1x)) + __builtin_fabs(m1y)))) return 0;
    if (!(d2 > kSCoincide * ((1.0 + __builtin_fabs(m2x)) + __builtin_fabs(m2y)))) return 0;
    if (!(d1 < 1e150) || !(d2 < 1e150)) return 0;
    const double k1 = 1.0 / d1, k2 = 1.0 / d2;
    const double kk = k2 / k1;
    double u1[2], v1[2], u2[2], v2[2], rn[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        u1[i] = (x1[i] - m1x) * k1;
        v1[i] = (y1[i] - m1y) * k1;
        u2[i] = (x2[i] - m2x) * k2;
        v2[i] = (y2[i] - m2y) * k2;
        rn[i] = sp.r[i] * (kk * kk);
    }
    // (b)
    double a[6][9];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        double* r0 = a[i];
        double* r1 = a[2 + i];
        double* r2 = a[4 + i];
        r0[0] = u1[i]; r0[1] = v1[i]; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0;
        r0[6] = -(u2[i] * u1[i]); r0[7] = -(u2[i] * v1[i]); r0[8] = -u2[i];
        r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = u1[i]; r1[4] = v1[i]; r1[5] = 1.0;
        r1[6] = -(v2[i] * u1[i]); r1[7] = -(v2[i] * v1[i]); r1[8] = -v2[i];
        const double g = sp.s2[i] * u2[i] - sp.c2[i] * v2[i];
        r2[0] = -(sp.s2[i] * sp.c1[i]); r2[1] = -(sp.s2[i] * sp.s1[i]); r2[2] = 0.0;
        r2[3] = sp.c2[i] * sp.c1[i];    r2[4] = sp.c2[i] * sp.s1[i];    r2[5] = 0.0;
        r2[6] = g * sp.c1[i];           r2[7] = g * sp.s1[i];           r2[8] = 0.0;
    }
    // forward elimination, partial pivoting on columns 0..5, fully unrolled:
    // the row swap is a compare-select per row (fund.h)
    bool rank = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double pm = __builtin_fabs(a[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
            if (__builtin_fabs(a[i][k]) > pm) { pm = __builtin_fabs(a[i][k]); p = i; }
        rank = rank && (pm > kSRankTol);             // false for a NaN too
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const bool sw = i == p;
#pragma unroll
            for (int j = k; j < 9; ++j) {
                const double u = a[k][j], v = a[i][j];
                a[k][j] = sw ? v : u;
                a[i][j] = sw ? u : v;
            }
        }
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double fct = a[i][k] / a[k][k];
#pragma unroll
            for (int j = k + 1; j < 9; ++j) a[i][j] = a[i][j] - fct * a[k][j];
            a[i][k] = 0.0;
        }
    }
    if (!rank) return 0;
    // null-space basis: entries 0..5 of n1, n2, n3 (entries 6..8 are unit vectors)
    double n1[6], n2[6], n3[6];
    auto back_substitute = [&](double (&fv)[6], int col) {
#pragma unroll
        for (int r = 5; r >= 0; --r) {
            double acc = a[r][col];
#pragma unroll
            for (int cc = r + 1; cc < 6; ++cc) acc = acc + a[r][cc] * fv[cc];
            fv[r] = -acc / a[r][r];
        }
    };
    back_substitute(n1, 6);
    back_substitute(n2, 7);
    back_substitute(n3, 8);
    // (c)
    double q1[6], q2[6];
    conic(n1, n2, n3, u1[0], v1[0], u2[0], v2[0], rn[0], q1);
    conic(n1, n2, n3, u1[1], v1[1], u2[1], v2[1], rn[1], q2);
    // A = q[0]; P(b) = q[3] + q[1] b; R(b) = q[5] + q[4] b + q[2] b^2
    const double uc[3] = {q1[0] * q2[5] - q2[0] * q1[5], q1[0] * q2[4] - q2[0] * q1[4], q1[0] * q2[2] - q2[0] * q1[2]};
    const double vc[2] = {q1[0] * q2[3] - q2[0] * q1[3], q1[0] * q2[1] - q2[0] * q1[1]};
    const double wc[4] = {q1[3] * q2[5] - q2[3] * q1[5],
                          (q1[3] * q2[4] + q1[1] * q2[5]) - (q2[3] * q1[4] + q2[1] * q1[5]),
                          (q1[3] * q2[2] + q1[1] * q2[4]) - (q2[3] * q1[2] + q2[1] * q1[4]),
                          q1[1] * q2[2] - q2[1] * q1[2]};
    const double Q0 = uc[0] * uc[0] - vc[0] * wc[0];
    const double Q1 = 2.0 * (uc[0] * uc[1]) - (vc[0] * wc[1] + vc[1] * wc[0]);
    const double Q2 = (2.0 * (uc[0] * uc[2]) + uc[1] * uc[1]) - (vc[0] * wc[2] + vc[1] * wc[1]);
    const double Q3 = 2.0 * (uc[1] * uc[2]) - (vc[0] * wc[3] + vc[1] * wc[2]);
    // (d)
    double root[3];
    const int nr = real_roots_cubic(Q3, Q2, Q1, Q0, root[0], root[1], root[2]);
    // T1 = [[k1, 0, t1x], [0, k1, t1y], [0, 0, 1]]
    const double t1x = -(k1 * m1x), t1y = -(k1 * m1y);
    unsigned valid = 0;
#pragma unroll
    for (int t = 0; t < kSModels; ++t) {
        const double b = root[t];
        const double ub = (uc[2] * b + uc[1]) * b + uc[0];
        const double vb = vc[1] * b + vc[0];
        bool ok = t < nr;
        ok = ok && (__builtin_fabs(vb) > kSVTol * (__builtin_fabs(vc[0]) + __builtin_fabs(vc[1] * b)));
        const double av = -ub / vb;
        // (e)
        double h[9];
#pragma unroll
        for (int k = 0; k < 6; ++k) h[k] = (n1[k] * av + n2[k] * b) + n3[k];
        h[6] = av;
        h[7] = b;
        h[8] = 1.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) ok = ok && (__builtin_fabs(h[k]) < 1e300);    // false for a NaN too
        double sv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            sv[i] = (av * u1[i] + b * v1[i]) + 1.0;
            const double l3 = h[6] * sp.c1[i] + h[7] * sp.s1[i];
            const double bx = (h[0] * sp.c1[i] + h[1] * sp.s1[i]) - u2[i] * l3;
            const double by = (h[3] * sp.c1[i] + h[4] * sp.s1[i]) - v2[i] * l3;
            const double along = sp.c2[i] * bx + sp.s2[i] * by;
            ok = ok && (along * sv[i] > 0.0);
        }
        ok = ok && (sv[0] * sv[1] > 0.0);
        // H = T2^-1 (h T1)
        double m[9], H[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            m[3 * r] = h[3 * r] * k1;
            m[3 * r + 1] = h[3 * r + 1] * k1;
            m[3 * r + 2] = (h[3 * r] * t1x + h[3 * r + 1] * t1y) + h[3 * r + 2];
        }
        double big = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            H[j] = m[j] * d2 + m2x * m[6 + j];
            H[3 + j] = m[3 + j] * d2 + m2y * m[6 + j];
            H[6 + j] = m[6 + j];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) big = __builtin_fmax(big, __builtin_fabs(H[k]));
        ok = ok && (__builtin_fabs(H[8]) > kSH33Tol * big) && (big < 1e300);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double v = H[k] / H[8];
            ms[t].h[k] = v;
            ok = ok && (__builtin_fabs(v) < 1e300);
        }
        ms[t].h[8] = 1.0;
        if (ok) valid |= 1u << t;
    }
    return valid;
}

// The 2-point minimal solver: up to kSModels models packed to the front of
// `out` in ascending root order; returns their number
GCR_HD int solve_s2(const double x1[2], const double y1[2], const double x2[2], const double y2[2],
                    const SiftPair& sp, GeoModel* out) {
    GeoModel ms[kSModels];
    const unsigned valid = solve_s2_slots(x1, y1, x2, y2, sp, ms);
    int cnt = 0;
#pragma unroll
    for (int t = 0; t < kSModels; ++t)
        if ((valid >> t) & 1u) out[cnt++] = ms[t];
    return cnt;
}

}  // namespace gcr
