// grav.h -- essential matrix from three correspondences and the gravity
// direction of both cameras: the minimal solver of the hot path and the
// shared pieces of its non-minimal fit, host and device (GCR_HD).
//
// Upstream GC-RANSAC is not part of this project's sources, and parity with
// its gravity solver is unpinned; as with fund.h, guided.h and ess.h this
// header is the definition.  The same code runs on both sides with
// -ffp-contract=off and uses +, -, *, / and sqrt only, in one fixed order.
//
// Input: three K-normalised correspondences (x^1, x^2) and two
// gravity-alignment rotations G1, G2 (row-major 3 x 3): Gi takes a direction
// in camera i to a frame whose y axis is the gravity direction.  In the
// aligned frames the relative pose is a rotation about y and a translation:
// E' = [t]x R_y(theta), R_y = [[c, 0, sn], [0, 1, 0], [-sn, 0, c]], and the
// essential matrix of the normalised frames is E = G2^T E' G1.
//
//   1. aligned rays p = G1 (x^1, 1)^T, q = G2 (x^2, 1)^T.  They stay
//      3-vectors and are never dehomogenised (their third component may be
//      <= 0);
//   2. q^T E' p = t . ((R_y p) x q).  With s = tan(theta / 2),
//      (1 + s^2) R_y p = P0 + P1 s + P2 s^2, P0 = (px, py, pz),
//      P1 = (2 pz, 0, -2 px), P2 = (-px, py, -pz); row i of M(s) is
//      A_i + B_i s + C_i s^2 with A = P0 x q, B = P1 x q, C = P2 x q, and
//      M(s) t = 0;
//   3. det M(s) = row0 . (row1 x row2), a sextic: the quartic vector
//      W = row1 x row2 and the seven coefficients D0..D6 in closed form, the
//      products of each coefficient added in ascending order of the first
//      factor's degree;
//   4. in exact arithmetic the sextic is divisible by 1 + s^2 (at s = +-i the
//      three polynomials P0 + P1 s + P2 s^2 are multiples of one vector):
//      Q4 = D6, Q3 = D5, Q2 = D4 - Q4, Q1 = D3 - Q3, Q0 = D2 - Q2; the
//      remainder (D1 - Q1) s + (D0 - Q0) is rounding and is dropped;
//   5. real roots of the quartic in ascending order: Q is made monic (a
//      leading coefficient that is zero or not finite fails the attempt: two
//      equal rows make the determinant vanish identically), all real roots of
//      Q and of its derivatives lie inside the Cauchy bound R, and the roots
//      of each derivative bracket those of the one above it, from the linear
//      third derivative down to Q: ess.h's safeguarded Newton (root_in) per
//      sign change, an exact zero at a bracket's lower end counted once.  The
//      brackets are held in fixed positions (an interval without a root hands
//      its lower end down as the next level's bracket point, which makes an
//      empty interval there), so nothing is indexed at run time.  A root of
//      even multiplicity changes no sign and may be missed;
//   6. per root s: rows m_i = (C_i s + B_i) s + A_i; t is the cross product
//      of the row pairs (0, 1), (0, 2), (1, 2), in this order, the first with
//      the largest squared norm.  The root is rejected when that squared norm
//      is not above kGRankTol (|m_0|^2 + |m_1|^2 + |m_2|^2)^2: M(s) has rank
//      below two (pure rotation, repeated or collinear rays);
//   7. c = (1 - s^2) / (1 + s^2), sn = 2 s / (1 + s^2),
//      E' = [[-ty sn, -tz, ty c], [tz c + tx sn, 0, tz sn - tx c],
//            [-ty c, tx, -ty sn]], E = G2^T (E' G1) over its Frobenius norm.
//      Models with a non-finite entry and (minimal solver only) models that
//      fail fund.h's oriented_ok<3> on the sample are dropped, as ess.h drops
//      them; the others are returned in ascending root order.
//
// theta = pi (s infinite) is outside the parametrisation: such a pose is not
// found, and a root whose s^2 overflows yields a non-finite model, which is
// dropped.
#pragma once

#include "ess.h"
#include "fund.h"
#include "gcr_hd.h"
#include "geo.h"

namespace gcr {

constexpr int kGModels = 4;          // real roots of the quartic, models per sample
constexpr double kGRankTol = 1e-20;  // step 6: squared sine of the rows' angle, about (1e-10)^2

// The two gravity-alignment rotations, row-major.  Passed to the generator
// kernel by value (wave-uniform: scalar registers).
struct GravRot {
    double g1[9];
    double g2[9];
};

namespace grav {

GCR_HD void vcross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

GCR_HD double vdot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// g (x, y, 1)^T
GCR_HD void align(const double* g, double x, double y, double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = (g[3 * r] * x + g[3 * r + 1] * y) + g[3 * r + 2];
}

// One level of step 5: q has degree D and derivative dq; in[0 .. D - 1) are
// the bracket points handed down by the level above (ascending); out[0 .. D)
// are this level's: the root of interval t where it has one (bit t of the
// result), else the interval's lower end.
template <int D>
GCR_HD unsigned root_level(const double* q, const double* dq, const double* in, double* out, double R) {
    unsigned live = 0;
    bool any = false;
    double last = 0.0;
    double lo = -R, flo = ess::horner<D>(q, lo);
#pragma unroll
    for (int t = 0; t < D; ++t) {
        const double hi = t < D - 1 ? in[t] : R;
        const double fhi = ess::horner<D>(q, hi);
        double r = lo;
        bool got = false;
        if (flo == 0.0) {
            got = !(any && last == lo);
        } else if (((flo < 0.0) != (fhi < 0.0)) && !(fhi == 0.0) && fhi == fhi) {
            r = ess::root_in<D>(q, dq, lo, hi, flo);
            got = true;
        }
        out[t] = r;
        if (got) {
            live |= 1u << t;
            any = true;
            last = r;
        }
        lo = hi;
        flo = fhi;
    }
    return live;
}

// Real roots of c[0] + ... + c[4] s^4 (step 5): root[t] is a root where bit t
// of the result is set, ascending over the set bits; 0 also for a leading
// coefficient that is zero or not finite.
GCR_HD unsigned quartic_roots(const double (&c)[5], double (&root)[4]) {
    const double lead = c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) root[t] = 0.0;
    if (!(__builtin_fabs(lead) > 0.0) || !(__builtin_fabs(lead) < 1e300)) return 0;
    double m[5], d1[4], d2[3], d3[2];
    double R = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = c[j] / lead;
        R = __builtin_fmax(R, __builtin_fabs(m[j]));
    }
    m[4] = 1.0;
    R = 1.0 + R;
    if (!(R < 1e300)) return 0;                     // also a NaN coefficient
#pragma unroll
    for (int j = 0; j < 4; ++j) d1[j] = m[j + 1] * (double)(j + 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) d2[j] = d1[j + 1] * (double)(j + 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) d3[j] = d2[j + 1] * (double)(j + 1);
    double b1[1], b2[2], b3[3];
    {
        const double r = -d3[0] / d3[1];            // the third derivative is linear
        b1[0] = (r > -R && r < R) ? r : -R;
    }
    root_level<2>(d2, d3, b1, b2, R);
    root_level<3>(d1, d2, b2, b3, R);
    return root_level<4>(m, d1, b3, root, R);
}

// Step 7: E of (t, c, sn) and the rotations, unit Frobenius norm; false for
// a model with a non-finite entry
GCR_HD bool compose(const GravRot& rot, double tx, double ty, double tz, double c, double sn, double* e) {
    const double ep[9] = {-(ty * sn),        -tz, ty * c,
                          tz * c + tx * sn,  0.0, tz * sn - tx * c,
                          -(ty * c),         tx,  -(ty * sn)};
    double tm[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            tm[3 * r + k] = (ep[3 * r] * rot.g1[k] + ep[3 * r + 1] * rot.g1[3 + k]) + ep[3 * r + 2] * rot.g1[6 + k];
    double nn = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = (rot.g2[r] * tm[k] + rot.g2[3 + r] * tm[3 + k]) + rot.g2[6 + r] * tm[6 + k];
            e[3 * r + k] = v;
            nn = nn + v * v;
        }
    const double nrm = sqrt(nn);
    bool ok = (nrm > 0.0) && (nrm < 1e300);          // false for a NaN too
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        e[k] = e[k] / nrm;
        ok = ok && (__builtin_fabs(e[k]) <= 2.0);    // finite (unit norm: at most 1 + rounding)
    }
    return ok;
}

}  // namespace grav

// The 3-point solver with every model in a fixed position: ms[t] is the model
// of root position t where bit t of the result is set (ascending roots over
// the set bits).  The generator kernel calls this form: no array is indexed at
// run time, so samples, polynomials and models stay in registers.
GCR_HD unsigned solve_g3_slots(const double x1[3], const double y1[3], const double x2[3], const double y2[3],
                               const GravRot& rot, GeoModel (&ms)[kGModels]) {
    using namespace grav;
    // steps 1 and 2
    double A[3][3], B[3][3], C[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double p[3], q[3];
        align(rot.g1, x1[i], y1[i], p);
        align(rot.g2, x2[i], y2[i], q);
        const double p1[3] = {2.0 * p[2], 0.0, -(2.0 * p[0])};
        const double p2[3] = {-p[0], p[1], -p[2]};
        vcross(p, q, A[i]);
        vcross(p1, q, B[i]);
        vcross(p2, q, C[i]);
    }
    // step 3
    double W[5][3], u[3], v[3], w[3];
    vcross(A[1], A[2], W[0]);
    vcross(A[1], B[2], u);
    vcross(B[1], A[2], v);
#pragma unroll
    for (int k = 0; k < 3; ++k) W[1][k] = u[k] + v[k];
    vcross(A[1], C[2], u);
    vcross(B[1], B[2], v);
    vcross(C[1], A[2], w);
#pragma unroll
    for (int k = 0; k < 3; ++k) W[2][k] = (u[k] + v[k]) + w[k];
    vcross(B[1], C[2], u);
    vcross(C[1], B[2], v);
#pragma unroll
    for (int k = 0; k < 3; ++k) W[3][k] = u[k] + v[k];
    vcross(C[1], C[2], W[4]);
    // (D0 and D1 enter the dropped remainder only)
    const double D2 = (vdot(A[0], W[2]) + vdot(B[0], W[1])) + vdot(C[0], W[0]);
    const double D3 = (vdot(A[0], W[3]) + vdot(B[0], W[2])) + vdot(C[0], W[1]);
    const double D4 = (vdot(A[0], W[4]) + vdot(B[0], W[3])) + vdot(C[0], W[2]);
    const double D5 = vdot(B[0], W[4]) + vdot(C[0], W[3]);
    const double D6 = vdot(C[0], W[4]);
    // step 4
    double Q[5];
    Q[4] = D6;
    Q[3] = D5;
    Q[2] = D4 - Q[4];
    Q[1] = D3 - Q[3];
    Q[0] = D2 - Q[2];
    // step 5
    double root[4];
    const unsigned live = quartic_roots(Q, root);
    unsigned valid = 0;
#pragma unroll
    for (int t = 0; t < kGModels; ++t) {
        if (((live >> t) & 1u) == 0) continue;
        const double s = root[t];
        // step 6
        double m[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) m[i][k] = (C[i][k] * s + B[i][k]) * s + A[i][k];
        double c01[3], c02[3], c12[3];
        vcross(m[0], m[1], c01);
        vcross(m[0], m[2], c02);
        vcross(m[1], m[2], c12);
        const double n01 = vdot(c01, c01), n02 = vdot(c02, c02), n12 = vdot(c12, c12);
        double best = n01, tx = c01[0], ty = c01[1], tz = c01[2];
        if (n02 > best) { best = n02; tx = c02[0]; ty = c02[1]; tz = c02[2]; }
        if (n12 > best) { best = n12; tx = c12[0]; ty = c12[1]; tz = c12[2]; }
        const double S = (vdot(m[0], m[0]) + vdot(m[1], m[1])) + vdot(m[2], m[2]);
        bool ok = best > kGRankTol * (S * S);   // false for a NaN too
        // step 7
        const double ss = s * s, den = 1.0 + ss;
        const double c = (1.0 - ss) / den, sn = (2.0 * s) / den;
        ok = compose(rot, tx, ty, tz, c, sn, ms[t].h) && ok;
        ok = oriented_ok<3>(ms[t].h, x1, y1, x2, y2) && ok;
        if (ok) valid |= 1u << t;
    }
    return valid;
}

// The 3-point minimal solver: up to kGModels models packed to the front of
// `out` in ascending root order; returns their number
GCR_HD int solve_g3(const double x1[3], const double y1[3], const double x2[3], const double y2[3],
                    const GravRot& rot, GeoModel* out) {
    GeoModel ms[kGModels];
    const unsigned valid = solve_g3_slots(x1, y1, x2, y2, rot, ms);
    int cnt = 0;
#pragma unroll
    for (int t = 0; t < kGModels; ++t)
        if ((valid >> t) & 1u) out[cnt++] = ms[t];
    return cnt;
}

}  // namespace gcr
