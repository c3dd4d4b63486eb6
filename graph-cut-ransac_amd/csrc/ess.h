// ess.h -- essential-matrix estimator of the hot path: the 5-point minimal
// solver (Nister's formulation) and the shared core of the non-minimal fit,
// host and device (GCR_HD).
//
// Neither the fork nor the oracle has this estimator, so, as with fund.h and
// guided.h, this header is the definition: the same code runs on both sides
// with -ffp-contract=off and uses +, -, *, / and sqrt only.  Correspondences
// are K-normalised (x^ = K^-1 x); a model is a 9-double GeoModel of unit
// Frobenius norm with x^2^T E x^1 = 0, and its residual is fund.h's squared
// Sampson distance in normalised coordinates.
//
//   1. epipolar system: five rows (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1);
//   2. null space: forward elimination with partial pivoting on columns 0..4
//      (a pivot <= 1e-10 fails the attempt), back substitution with
//      (e5..e8) = the four unit vectors, then modified Gram-Schmidt in two
//      passes: X, Y, Z, W.  The orthonormalisation is required: the raw
//      elimination basis loses the true E in a sixth of random samples;
//   3. E = x X + y Y + z Z + W; det E = 0 (row 0) and the nine entries of
//      (2 E E^T - tr(E E^T) I) E = 0 (rows 1..9, row-major) as a 10 x 20
//      matrix over the monomials
//        x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1;
//   4. Gauss-Jordan with partial pivoting on the first ten columns (a pivot
//      <= 1e-10 fails the attempt: the basis is orthonormal, so the entries
//      are of order one and such a pivot means a family of solutions, e.g.
//      collinear points);
//   5. rows e..j (led by x^2z, x^2, y^2z, y^2, xyz, xy): e - z f, g - z h and
//      i - z j are the rows of B(z), whose columns multiply (x, y, 1) and have
//      degrees 3, 3, 4; n(z) = det B(z), expanded along the third column, has
//      degree 10;
//   6. real roots of n(z) in ascending order: n is made monic (a leading
//      coefficient that is zero or not finite fails the attempt), all real
//      roots of n and of its derivatives lie inside the Cauchy bound R of n
//      (Gauss-Lucas), and the roots of the (m)-th derivative are bracketed by
//      -R, the roots of the (m+1)-th and R, from the linear ninth derivative
//      down to n itself: one safeguarded-Newton root (cubic_root_in's
//      iteration on Horner values) per sign change, an exact zero at a
//      bracket's lower end counted once.  A root of even multiplicity changes
//      no sign and may be missed;
//   7. per root, the rows (a_r, b_r, c_r) of B(z): among the row pairs (0, 1),
//      (0, 2), (1, 2), in this order, the first with the largest
//      |a_i b_j - a_j b_i| gives x and y by Cramer's rule; E = xX + yY + zZ + W
//      over its Frobenius norm.  Models with a non-finite entry and (minimal
//      solver only) models that fail oriented_ok<5> on the sample are dropped;
//      the others are packed to the front in root order.
#pragma once

#include "fund.h"
#include "gcr_hd.h"
#include "geo.h"

namespace gcr {

constexpr int kEModels = 10;         // real roots of n(z), models per sample

namespace ess {

// variables 0 = x, 1 = y, 2 = z, 3 = 1.  Quadratic monomial of the pair i <= j.
constexpr int pair_idx(int i, int j) { return (i == 0 ? 0 : i == 1 ? 4 : i == 2 ? 7 : 9) + (j - i); }

// column of the cubic monomial i <= j <= k in the order of step 3
constexpr int tri_col(int i, int j, int k) {
    switch (i * 16 + j * 4 + k) {
        case 0x00: return 0;    // x^3
        case 0x15: return 1;    // y^3
        case 0x01: return 2;    // x^2 y
        case 0x05: return 3;    // x y^2
        case 0x02: return 4;    // x^2 z
        case 0x03: return 5;    // x^2
        case 0x16: return 6;    // y^2 z
        case 0x17: return 7;    // y^2
        case 0x06: return 8;    // x y z
        case 0x07: return 9;    // x y
        case 0x0a: return 10;   // x z^2
        case 0x0b: return 11;   // x z
        case 0x0f: return 12;   // x
        case 0x1a: return 13;   // y z^2
        case 0x1b: return 14;   // y z
        case 0x1f: return 15;   // y
        case 0x2a: return 16;   // z^3
        case 0x2b: return 17;   // z^2
        case 0x2f: return 18;   // z
        default: return 19;     // 1
    }
}
// ... of the quadratic monomial (i <= j) times the variable k
constexpr int tri_of(int i, int j, int k) {
    return k <= i ? tri_col(k, i, j) : (k <= j ? tri_col(i, k, j) : tri_col(i, j, k));
}

// q += a * b: linear x linear, products added in (i, j) order
GCR_HD void acc11(double (&q)[10], const double* a, const double* b) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = i <= j ? pair_idx(i, j) : pair_idx(j, i);
            q[p] = q[p] + a[i] * b[j];
        }
}

// c += q * l: quadratic x linear, products added in (i <= j, k) order
GCR_HD void acc21(double (&c)[20], const double (&q)[10], const double* l) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = tri_of(i, j, k);
                c[t] = c[t] + q[pair_idx(i, j)] * l[k];
            }
}

// a * b - c * d for linear polynomials
GCR_HD void minor11(double (&q)[10], const double* a, const double* b, const double* c, const double* d) {
    double u[10], v[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) u[t] = v[t] = 0.0;
    acc11(u, a, b);
    acc11(v, c, d);
#pragma unroll
    for (int t = 0; t < 10; ++t) q[t] = u[t] - v[t];
}

// Horner value of c[0] + c[1] z + ... + c[D] z^D.  The degree is a template
// argument and the loop unrolled, so every coefficient index is a constant
// and, on the device, the derivative triangle below needs no run-time
// indexed (scratch) storage.
template <int D>
GCR_HD double horner(const double* c, double z) {
    double v = c[D];
#pragma unroll
    for (int j = D - 1; j >= 0; --j) v = v * z + c[j];
    return v;
}

// cubic_root_in for a polynomial of degree D (q) and its derivative (dq):
// the root in [lo, hi], q(lo) q(hi) < 0, flo = q(lo)
template <int D>
GCR_HD double root_in(const double* q, const double* dq, double lo, double hi, double flo) {
    double xl = lo, xh = hi;                       // q(xl) < 0 < q(xh)
    if (!(flo < 0.0)) { xl = hi; xh = lo; }
    double rts = 0.5 * (lo + hi);
    double dxold = __builtin_fabs(hi - lo), dx = dxold;
    double f = horner<D>(q, rts), df = horner<D - 1>(dq, rts);
    for (int it = 0; it < 100; ++it) {
        if (f == 0.0) break;
        if ((((rts - xh) * df - f) * ((rts - xl) * df - f) > 0.0) ||
            (__builtin_fabs(2.0 * f) > __builtin_fabs(dxold * df))) {
            dxold = dx;
            dx = 0.5 * (xh - xl);
            rts = xl + dx;
            if (xl == rts) break;
        } else {
            dxold = dx;
            dx = f / df;
            const double prev = rts;
            rts = rts - dx;
            if (prev == rts) break;
        }
        if (__builtin_fabs(dx) < 1e-14 * (1.0 + __builtin_fabs(rts))) break;
        f = horner<D>(q, rts);
        df = horner<D - 1>(dq, rts);
        if (f < 0.0) xl = rts;
        else xh = rts;
    }
    return rts;
}

// One level of step 6 and the levels below it: cur[0 .. k) are the roots of
// row M + 1 of the derivative triangle (the (M+1)-th derivative) in ascending
// order; on return they are the roots of row 0.
template <int M>
GCR_HD void root_levels(const double (&tri)[10][11], double (&cur)[10], int& k, double R) {
    constexpr int D = 10 - M;                      // degree of row M
    const double* q = tri[M];
    const double* dq = tri[M + 1];
    double nxt[10];
    int no = 0;
    double lo = -R, flo = horner<D>(q, lo);
    for (int t = 0; t <= k; ++t) {
        const double hi = t < k ? cur[t] : R;
        const double fhi = horner<D>(q, hi);
        if (flo == 0.0) {
            if (no == 0 || nxt[no - 1] != lo) {
                if (no < D) nxt[no++] = lo;
            }
        } else if (((flo < 0.0) != (fhi < 0.0)) && !(fhi == 0.0) && fhi == fhi) {
            if (no < D) nxt[no++] = root_in<D>(q, dq, lo, hi, flo);
        }
        lo = hi;
        flo = fhi;
    }
    k = no;
    for (int t = 0; t < k; ++t) cur[t] = nxt[t];
    if constexpr (M > 0) root_levels<M - 1>(tri, cur, k, R);
}

// Real roots of n[0] + ... + n[10] z^10 in ascending order (step 6); returns
// the count, -1 if the leading coefficient is zero or not finite.
GCR_HD int real_roots_deg10(const double (&n)[11], double (&roots)[10]) {
    const double lead = n[10];
    if (!(__builtin_fabs(lead) > 0.0) || !(__builtin_fabs(lead) < 1e300)) return -1;
    // the derivative triangle: row m is the m-th derivative of the monic
    // polynomial, degree 10 - m (entries past it unused)
    double tri[10][11];
    double R = 0.0;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        tri[0][j] = n[j] / lead;
        R = __builtin_fmax(R, __builtin_fabs(tri[0][j]));
    }
    tri[0][10] = 1.0;
    R = 1.0 + R;
    if (!(R < 1e300)) return -1;                   // also a NaN coefficient
#pragma unroll
    for (int m = 1; m <= 9; ++m)
#pragma unroll
        for (int j = 0; j <= 10 - m; ++j) tri[m][j] = tri[m - 1][j + 1] * (double)(j + 1);
    int k = 0;
    {
        const double r = -tri[9][0] / tri[9][1];   // row 9 is linear
        if (r > -R && r < R) roots[k++] = r;
    }
    root_levels<8>(tri, roots, k, R);
    return k;
}

}  // namespace ess

// Step 2: the orthonormal null-space basis X, Y, Z, W of the five epipolar rows
GCR_HD bool e5_basis(const double x1[5], const double y1[5], const double x2[5], const double y2[5],
                     double (&bs)[4][9]) {
    double a[5][9];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        a[i][0] = x2[i] * x1[i]; a[i][1] = x2[i] * y1[i]; a[i][2] = x2[i];
        a[i][3] = y2[i] * x1[i]; a[i][4] = y2[i] * y1[i]; a[i][5] = y2[i];
        a[i][6] = x1[i];         a[i][7] = y1[i];         a[i][8] = 1.0;
    }
    // as solve_f7_basis: unrolled, the row swap a compare-select per row
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        int p = k;
        double pm = __builtin_fabs(a[k][k]);
#pragma unroll
        for (int i = k + 1; i < 5; ++i)
            if (__builtin_fabs(a[i][k]) > pm) { pm = __builtin_fabs(a[i][k]); p = i; }
        if (!(pm > 1e-10)) return false;             // rank < 5: degenerate sample
#pragma unroll
        for (int i = k + 1; i < 5; ++i) {
            const bool sw = i == p;
#pragma unroll
            for (int j = k; j < 9; ++j) {
                const double u = a[k][j], v = a[i][j];
                a[k][j] = sw ? v : u;
                a[i][j] = sw ? u : v;
            }
        }
#pragma unroll
        for (int i = k + 1; i < 5; ++i) {
            const double fct = a[i][k] / a[k][k];
#pragma unroll
            for (int j = k + 1; j < 9; ++j) a[i][j] = a[i][j] - fct * a[k][j];
            a[i][k] = 0.0;
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int c = 5; c < 9; ++c) bs[v][c] = c == 5 + v ? 1.0 : 0.0;
#pragma unroll
        for (int r = 4; r >= 0; --r) {
            double acc = 0.0;
#pragma unroll
            for (int c = r + 1; c < 9; ++c) acc = acc + a[r][c] * bs[v][c];
            bs[v][r] = -acc / a[r][r];
        }
    }
    // modified Gram-Schmidt, two passes per vector
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass)
#pragma unroll
            for (int u = 0; u < v; ++u) {
                double dot = 0.0;
#pragma unroll
                for (int c = 0; c < 9; ++c) dot = dot + bs[u][c] * bs[v][c];
#pragma unroll
                for (int c = 0; c < 9; ++c) bs[v][c] = bs[v][c] - dot * bs[u][c];
            }
        double nn = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) nn = nn + bs[v][c] * bs[v][c];
        const double nrm = sqrt(nn);
        if (!(nrm > 1e-10) || !(nrm < 1e300)) return false;
#pragma unroll
        for (int c = 0; c < 9; ++c) bs[v][c] = bs[v][c] / nrm;
    }
    return true;
}

// Steps 3..7 on an orthonormal basis bs = (X, Y, Z, W).  kOriented: models
// must pass oriented_ok<5> on the sample (x1 .. y2, five entries each; unused
// otherwise).  Returns the number of models written to the front of `out`
// (room for kEModels), in ascending root order; 0: a failed attempt.
template <bool kOriented>
GCR_HD int e5_models(const double (&bs)[4][9], const double* x1, const double* y1, const double* x2,
                     const double* y2, GeoModel* out) {
    using namespace ess;
    // entry e of E as a linear polynomial: (X[e], Y[e], Z[e], W[e])
    double E[9][4];
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
        for (int v = 0; v < 4; ++v) E[e][v] = bs[v][e];
    double M[10][20];
    // row 0: det E, expanded along the first row
    {
        double m0[10], m1[10], m2[10], row[20];
        minor11(m0, E[4], E[8], E[5], E[7]);
        minor11(m1, E[5], E[6], E[3], E[8]);
        minor11(m2, E[3], E[7], E[4], E[6]);
#pragma unroll
        for (int t = 0; t < 20; ++t) row[t] = 0.0;
        acc21(row, m0, E[0]);
        acc21(row, m1, E[1]);
        acc21(row, m2, E[2]);
#pragma unroll
        for (int t = 0; t < 20; ++t) M[0][t] = row[t];
    }
    // rows 1..9: (2 E E^T - tr(E E^T) I) E
    {
        double eet[6][10];                           // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        int s = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) {
#pragma unroll
                for (int t = 0; t < 10; ++t) eet[s][t] = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) acc11(eet[s], E[3 * r + k], E[3 * c + k]);
                ++s;
            }
        double tr[10];
#pragma unroll
        for (int t = 0; t < 10; ++t) tr[t] = (eet[0][t] + eet[3][t]) + eet[5][t];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double row[20];
#pragma unroll
                for (int t = 0; t < 20; ++t) row[t] = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int lo = r < k ? r : k, hi = r < k ? k : r;
                    const int sidx = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
                    double lam[10];
#pragma unroll
                    for (int t = 0; t < 10; ++t)
                        lam[t] = r == k ? 2.0 * eet[sidx][t] - tr[t] : 2.0 * eet[sidx][t];
                    acc21(row, lam, E[3 * k + c]);
                }
#pragma unroll
                for (int t = 0; t < 20; ++t) M[1 + 3 * r + c][t] = row[t];
            }
    }
    // step 4: Gauss-Jordan, partial pivoting, on columns 0..9
    for (int k = 0; k < 10; ++k) {
        int p = k;
        double pm = __builtin_fabs(M[k][k]);
        for (int i = k + 1; i < 10; ++i) {
            const double v = __builtin_fabs(M[i][k]);
            if (v > pm) { pm = v; p = i; }
        }
        if (!(pm > 1e-10) || !(pm < 1e300)) return 0;
        for (int j = k; j < 20; ++j) {
            const double u = M[k][j], v = M[p][j];
            M[k][j] = v;
            M[p][j] = u;
        }
        const double piv = M[k][k];
        for (int j = k + 1; j < 20; ++j) M[k][j] = M[k][j] / piv;
        M[k][k] = 1.0;
        for (int i = 0; i < 10; ++i) {
            if (i == k) continue;
            const double fct = M[i][k];
            for (int j = k + 1; j < 20; ++j) M[i][j] = M[i][j] - fct * M[k][j];
            M[i][k] = 0.0;
        }
    }
    // step 5: B(z), coefficients in ascending powers of z
    double bx[3][4], by[3][4], b1[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double* A = &M[4 + 2 * r][10];
        const double* B = &M[5 + 2 * r][10];
        bx[r][0] = A[2]; bx[r][1] = A[1] - B[2]; bx[r][2] = A[0] - B[1]; bx[r][3] = -B[0];
        by[r][0] = A[5]; by[r][1] = A[4] - B[5]; by[r][2] = A[3] - B[4]; by[r][3] = -B[3];
        b1[r][0] = A[9]; b1[r][1] = A[8] - B[9]; b1[r][2] = A[7] - B[8]; b1[r][3] = A[6] - B[7];
        b1[r][4] = -B[6];
    }
    double n[11];
#pragma unroll
    for (int t = 0; t < 11; ++t) n[t] = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        // minor of b1[r]: rows (i, j) = (1, 2), (0, 2), (0, 1), sign + - +
        const int i = r == 0 ? 1 : 0, j = r == 2 ? 1 : 2;
        double u[7], v[7];
#pragma unroll
        for (int t = 0; t < 7; ++t) u[t] = v[t] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                u[a + b] = u[a + b] + bx[i][a] * by[j][b];
                v[a + b] = v[a + b] + bx[j][a] * by[i][b];
            }
#pragma unroll
        for (int t = 0; t < 7; ++t) u[t] = r == 1 ? v[t] - u[t] : u[t] - v[t];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 7; ++b) n[a + b] = n[a + b] + b1[r][a] * u[b];
    }
    // step 6
    double roots[10];
    const int nr = real_roots_deg10(n, roots);
    if (nr <= 0) return 0;
    // step 7
    int cnt = 0;
    for (int q = 0; q < nr; ++q) {
        const double z = roots[q];
        double a[3], b[3], c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[r] = horner<3>(bx[r], z);
            b[r] = horner<3>(by[r], z);
            c[r] = horner<4>(b1[r], z);
        }
        const double d01 = a[0] * b[1] - a[1] * b[0];
        const double d02 = a[0] * b[2] - a[2] * b[0];
        const double d12 = a[1] * b[2] - a[2] * b[1];
        int i = 0, j = 1;
        double det = d01;
        if (__builtin_fabs(d02) > __builtin_fabs(det)) { det = d02; i = 0; j = 2; }
        if (__builtin_fabs(d12) > __builtin_fabs(det)) { det = d12; i = 1; j = 2; }
        const double ai = i == 0 ? a[0] : a[1], bi = i == 0 ? b[0] : b[1], ci = i == 0 ? c[0] : c[1];
        const double aj = j == 1 ? a[1] : a[2], bj = j == 1 ? b[1] : b[2], cj = j == 1 ? c[1] : c[2];
        const double x = (bi * cj - bj * ci) / det;
        const double y = (aj * ci - ai * cj) / det;
        GeoModel m;
        double nn = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            m.h[e] = ((x * bs[0][e] + y * bs[1][e]) + z * bs[2][e]) + bs[3][e];
            nn = nn + m.h[e] * m.h[e];
        }
        const double nrm = sqrt(nn);
        bool ok = (nrm > 0.0) && (nrm < 1e300);      // false for a NaN too
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            m.h[e] = m.h[e] / nrm;
            ok = ok && (__builtin_fabs(m.h[e]) <= 2.0);   // finite (unit norm: at most 1 + rounding)
        }
        if (!ok) continue;
        if constexpr (kOriented) {
            if (!oriented_ok<5>(m.h, x1, y1, x2, y2)) continue;
        }
        out[cnt++] = m;
    }
    return cnt;
}

// The 5-point minimal solver: up to kEModels models in ascending root order
GCR_HD int solve_e5(const double x1[5], const double y1[5], const double x2[5], const double y2[5],
                    GeoModel* out) {
    double bs[4][9];
    if (!e5_basis(x1, y1, x2, y2, bs)) return 0;
    return e5_models<true>(bs, x1, y1, x2, y2, out);
}

}  // namespace gcr
