// The 5-point solver (csrc/ess.h) and the non-minimal essential-matrix fit
// (csrc/host_fit.cpp) as a stand-alone host program, meant to be built with
// ASan + UBSan (tests/test_essential.py): random noise-free two-view poses,
// then degenerate and non-finite samples.  Prints "OK ..." and returns 0 when
// every structural check holds.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <limits>
#include <random>
#include <vector>

#include "ess.h"
#include "host_fit.h"

using namespace gcr;

namespace {

struct Scene {
    std::vector<double> x1, y1, x2, y2;
    double E[9];
};

// rotation vector components ~ N(0, 0.2) rad, unit baseline, depths 4..8,
// lateral coordinates in +-2
Scene make_scene(std::mt19937_64& rng, int n) {
    std::normal_distribution<double> nd(0.0, 0.2), n1(0.0, 1.0);
    std::uniform_real_distribution<double> lat(-2.0, 2.0), dep(4.0, 8.0);
    const double w[3] = {nd(rng), nd(rng), nd(rng)};
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th > 0.0) {
        const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
        const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
        double K2[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
        for (int e = 0; e < 9; ++e) R[e] += std::sin(th) * K[e] + (1.0 - std::cos(th)) * K2[e];
    }
    double t[3] = {n1(rng), n1(rng), n1(rng)};
    const double tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (double& v : t) v /= tn;
    const double T[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    Scene s;
    double nn = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            s.E[3 * r + c] = T[3 * r] * R[c] + T[3 * r + 1] * R[3 + c] + T[3 * r + 2] * R[6 + c];
            nn += s.E[3 * r + c] * s.E[3 * r + c];
        }
    for (double& v : s.E) v /= std::sqrt(nn);
    for (int i = 0; i < n; ++i) {
        const double P[3] = {lat(rng), lat(rng), dep(rng)};
        double Q[3];
        for (int r = 0; r < 3; ++r) Q[r] = R[3 * r] * P[0] + R[3 * r + 1] * P[1] + R[3 * r + 2] * P[2] + t[r];
        s.x1.push_back(P[0] / P[2]);
        s.y1.push_back(P[1] / P[2]);
        s.x2.push_back(Q[0] / Q[2]);
        s.y2.push_back(Q[1] / Q[2]);
    }
    return s;
}

double dist_pm(const double* a, const double* b) {
    double dp = 0.0, dm = 0.0;
    for (int e = 0; e < 9; ++e) {
        dp += (a[e] - b[e]) * (a[e] - b[e]);
        dm += (a[e] + b[e]) * (a[e] + b[e]);
    }
    return std::sqrt(std::min(dp, dm));
}

int g_bad = 0;
void check(bool ok, const char* what, int id) {
    if (!ok) {
        if (g_bad < 20) std::printf("FAIL case %d: %s\n", id, what);
        ++g_bad;
    }
}

// count, order, finiteness, unit norm, the five epipolar equations
void check_models(const GeoModel* ms, int cnt, const double* x1, const double* y1, const double* x2, const double* y2,
                  int id) {
    check(cnt >= 0 && cnt <= kEModels, "model count", id);
    for (int q = 0; q < cnt; ++q) {
        double nn = 0.0;
        for (int e = 0; e < 9; ++e) {
            check(std::isfinite(ms[q].h[e]), "finite entry", id);
            nn += ms[q].h[e] * ms[q].h[e];
        }
        check(std::fabs(std::sqrt(nn) - 1.0) < 1e-12, "unit norm", id);
        for (int i = 0; i < 5; ++i) {
            const double* h = ms[q].h;
            const double r = x2[i] * (h[0] * x1[i] + h[1] * y1[i] + h[2]) + y2[i] * (h[3] * x1[i] + h[4] * y1[i] + h[5]) +
                             (h[6] * x1[i] + h[7] * y1[i] + h[8]);
            check(std::fabs(r) < 1e-6, "epipolar equation", id);
        }
    }
}

int solve_rows(const double rows[5][4], GeoModel* ms) {
    double x1[5], y1[5], x2[5], y2[5];
    for (int i = 0; i < 5; ++i) { x1[i] = rows[i][0]; y1[i] = rows[i][1]; x2[i] = rows[i][2]; y2[i] = rows[i][3]; }
    return solve_e5(x1, y1, x2, y2, ms);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261019);
    const int kCases = 400;
    int hit = 0, models = 0;
    for (int id = 0; id < kCases; ++id) {
        const Scene s = make_scene(rng, 5);
        GeoModel ms[kEModels];
        const int cnt = solve_e5(s.x1.data(), s.y1.data(), s.x2.data(), s.y2.data(), ms);
        check_models(ms, cnt, s.x1.data(), s.y1.data(), s.x2.data(), s.y2.data(), id);
        double best = 1e300;
        for (int q = 0; q < cnt; ++q) best = std::min(best, dist_pm(ms[q].h, s.E));
        hit += best < 1e-6;
        models += cnt;
        // k = 5 of the fit: the minimal solver's first model, bit for bit
        HostClass c;
        c.n = 5;
        c.x.assign(s.x1.begin(), s.x1.end()); c.y.assign(s.y1.begin(), s.y1.end());
        c.a.assign(s.x2.begin(), s.x2.end()); c.c0.assign(s.y2.begin(), s.y2.end());
        c.c1.assign(5, 0.0);
        GeoModel f;
        const bool ok = fit_e5_nonminimal(c, {0, 1, 2, 3, 4}, f);
        check(ok == (cnt > 0), "fit(k = 5) succeeds with the solver", id);
        if (ok && cnt > 0)
            for (int e = 0; e < 9; ++e) check(as_u64(f.h[e]) == as_u64(ms[0].h[e]), "fit(k = 5) bits", id);
    }
    // the truth is among the models for most samples (a numpy restatement with
    // an SVD basis and companion-matrix roots reaches 95-98 %)
    check(hit >= kCases * 85 / 100, "true E recovered in >= 85 % of the samples", -1);

    int fit_hit = 0;
    const int kFits = 100;
    for (int id = 0; id < kFits; ++id) {
        const Scene s = make_scene(rng, 35);
        HostClass c;
        c.n = 35;
        c.x.assign(s.x1.begin(), s.x1.end()); c.y.assign(s.y1.begin(), s.y1.end());
        c.a.assign(s.x2.begin(), s.x2.end()); c.c0.assign(s.y2.begin(), s.y2.end());
        c.c1.assign(35, 0.0);
        std::vector<uint32_t> idx(35);
        for (uint32_t i = 0; i < 35; ++i) idx[i] = 34 - i;
        GeoModel f;
        if (fit_e5_nonminimal(c, idx, f)) fit_hit += dist_pm(f.h, s.E) < 1e-6;
    }
    check(fit_hit >= kFits * 85 / 100, "35-point fit recovers E in >= 85 % of the scenes", -2);

    // degenerate and non-finite samples: no model, no trap, and an end
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    GeoModel ms[kEModels];
    {
        double rows[5][4];
        for (auto& r : rows) { r[0] = 0.25; r[1] = -0.5; r[2] = 0.125; r[3] = 0.75; }
        check(solve_rows(rows, ms) == 0, "five identical rows", -3);
    }
    {
        double rows[5][4];
        for (int i = 0; i < 5; ++i) {
            const double t = 0.1 * i - 0.2;
            rows[i][0] = 0.3 + t; rows[i][1] = -0.1 + 2.0 * t; rows[i][2] = 0.05 + 1.5 * t; rows[i][3] = 0.2 - 0.5 * t;
        }
        check(solve_rows(rows, ms) == 0, "collinear points", -4);
    }
    for (double bad : {nan, inf, -inf}) {
        for (int at = 0; at < 20; ++at) {
            const Scene s = make_scene(rng, 5);
            double rows[5][4];
            for (int i = 0; i < 5; ++i) { rows[i][0] = s.x1[i]; rows[i][1] = s.y1[i]; rows[i][2] = s.x2[i]; rows[i][3] = s.y2[i]; }
            rows[at / 4][at % 4] = bad;
            check(solve_rows(rows, ms) == 0, "non-finite coordinate", -5);
        }
    }
    if (g_bad) {
        std::printf("%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("OK minimal %d/%d recovered, %.2f models per sample, fit %d/%d recovered\n", hit, kCases,
                (double)models / kCases, fit_hit, kFits);
    return 0;
}
