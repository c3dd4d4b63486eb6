// The 2-point SIFT homography solver (csrc/sifth.h) as a stand-alone host
// program, meant to be built with ASan + UBSan (tests/test_sift_homography.py):
// random homographies with exact SIFT columns, then degenerate and non-finite
// samples.  Prints "OK ..." and returns 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>

#include "sifth.h"

using namespace gcr;

namespace {

struct Sample {
    double x1[2], y1[2], x2[2], y2[2];
    SiftPair sp;
};

// the point, direction and size of (x, y, alpha, q) under H
void transfer(const double* H, double x, double y, double alpha, double q, double& x2, double& y2, double& alpha2,
              double& q2) {
    const double s = H[6] * x + H[7] * y + H[8];
    x2 = (H[0] * x + H[1] * y + H[2]) / s;
    y2 = (H[3] * x + H[4] * y + H[5]) / s;
    const double a = (H[0] - x2 * H[6]) / s, b = (H[1] - x2 * H[7]) / s;
    const double c = (H[3] - y2 * H[6]) / s, d = (H[4] - y2 * H[7]) / s;
    const double dx = std::cos(alpha), dy = std::sin(alpha);
    alpha2 = std::atan2(c * dx + d * dy, a * dx + b * dy);
    q2 = q * std::sqrt(std::fabs(a * d - b * c));
}

void set_row(Sample& s, int i, double x, double y, double x2, double y2, double q1, double q2, double a1, double a2) {
    s.x1[i] = x; s.y1[i] = y; s.x2[i] = x2; s.y2[i] = y2;
    const double r = q2 / q1;
    s.sp.r[i] = r * r;
    s.sp.c1[i] = std::cos(a1); s.sp.s1[i] = std::sin(a1);
    s.sp.c2[i] = std::cos(a2); s.sp.s2[i] = std::sin(a2);
}

bool all_finite(const GeoModel& m) {
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(m.h[k])) return false;
    return m.h[8] == 1.0;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> small(-0.1, 0.1), proj(-5e-5, 5e-5), shift(-40.0, 40.0);
    std::uniform_real_distribution<double> px(0.0, 1280.0), py(0.0, 960.0), ang(-3.14159, 3.14159), size(2.0, 30.0);
    int solved = 0, tried = 0;
    double worst = 0.0;
    for (int c = 0; c < 400; ++c) {
        const double H[9] = {1.0 + small(rng), small(rng), shift(rng), small(rng), 1.0 + small(rng), shift(rng),
                             proj(rng), proj(rng), 1.0};
        Sample s;
        for (int i = 0; i < 2; ++i) {
            const double x = px(rng), y = py(rng), a1 = ang(rng), q1 = size(rng);
            double x2, y2, a2, q2;
            transfer(H, x, y, a1, q1, x2, y2, a2, q2);
            set_row(s, i, x, y, x2, y2, q1, q2, a1, a2);
        }
        GeoModel out[kSModels];
        const int n = solve_s2(s.x1, s.y1, s.x2, s.y2, s.sp, out);
        ++tried;
        if (n < 0 || n > kSModels) { printf("FAIL: count %d\n", n); return 1; }
        double best = 1e300;
        for (int k = 0; k < n; ++k) {
            if (!all_finite(out[k])) { printf("FAIL: non-finite model, case %d\n", c); return 1; }
            double d = 0.0;
            for (int q = 0; q < 9; ++q) d = std::fmax(d, std::fabs(out[k].h[q] - H[q]));
            best = std::fmin(best, d / 40.0);
        }
        if (n > 0) {
            ++solved;
            worst = std::fmax(worst, best);
        }
    }
    if (solved < tried * 9 / 10 || !(worst < 1e-6)) { printf("FAIL: solved %d of %d, worst %g\n", solved, tried, worst); return 1; }
    // degenerate and non-finite samples: no model, or finite ones, and nothing undefined
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double bad[] = {nan, inf, -inf, 0.0, 1e308, -1e308, 1e-320};
    int degenerate = 0;
    for (double v : bad)
        for (int at = 0; at < 14; ++at) {
            Sample s;
            set_row(s, 0, 100.0, 200.0, 130.0, 190.0, 5.0, 6.0, 0.3, 0.5);
            set_row(s, 1, 700.0, 500.0, 720.0, 480.0, 9.0, 8.0, -1.2, -1.0);
            double* field[14] = {&s.x1[0], &s.y1[1], &s.x2[0], &s.y2[1], &s.sp.r[0], &s.sp.r[1], &s.sp.c1[0],
                                 &s.sp.s1[1], &s.sp.c2[0], &s.sp.s2[1], &s.x1[1], &s.y1[0], &s.x2[1], &s.y2[0]};
            *field[at] = v;
            GeoModel out[kSModels];
            const int n = solve_s2(s.x1, s.y1, s.x2, s.y2, s.sp, out);
            for (int k = 0; k < n; ++k)
                if (!all_finite(out[k])) { printf("FAIL: non-finite model from a bad sample (%g at %d)\n", v, at); return 1; }
            ++degenerate;
        }
    {
        Sample s;                                   // coincident points, parallel orientations
        set_row(s, 0, 100.0, 200.0, 130.0, 190.0, 5.0, 6.0, 0.3, 0.5);
        set_row(s, 1, 100.0, 200.0, 130.0, 190.0, 9.0, 8.0, -1.2, -1.0);
        GeoModel out[kSModels];
        if (solve_s2(s.x1, s.y1, s.x2, s.y2, s.sp, out) != 0) { printf("FAIL: coincident points gave a model\n"); return 1; }
        set_row(s, 1, 700.0, 500.0, 720.0, 480.0, 9.0, 8.0, -1.2, 0.5);
        if (solve_s2(s.x1, s.y1, s.x2, s.y2, s.sp, out) != 0) { printf("FAIL: parallel orientations gave a model\n"); return 1; }
    }
    printf("OK solved %d of %d, worst distance %.3g, %d bad samples\n", solved, tried, worst, degenerate);
    return 0;
}
