// The 3-point solver with known gravity (csrc/grav.h) and its constrained
// non-minimal fit (csrc/host_fit.cpp) as a stand-alone host program, meant to
// be built with ASan + UBSan (tests/test_gravity_essential.py): random
// noise-free poses with random gravity-alignment rotations, then degenerate
// and non-finite samples.  Prints "OK ..." and returns 0 when every structural
// check holds.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <limits>
#include <random>
#include <vector>

#include "grav.h"
#include "host_fit.h"

using namespace gcr;

namespace {

void mul3(const double* a, const double* b, double* c) {
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) c[3 * r + k] = a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k] + a[3 * r + 2] * b[6 + k];
}

void transpose3(const double* a, double* t) {
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) t[3 * r + k] = a[3 * k + r];
}

// Rz(roll) Rx(pitch) Ry(yaw)
void euler(double yaw, double pitch, double roll, double* R) {
    const double cy = std::cos(yaw), sy = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch);
    const double cr = std::cos(roll), sr = std::sin(roll);
    const double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp};
    const double Rz[9] = {cr, -sr, 0, sr, cr, 0, 0, 0, 1};
    double t[9];
    mul3(Rx, Ry, t);
    mul3(Rz, t, R);
}

struct Scene {
    std::vector<double> x1, y1, x2, y2;
    GravRot rot;
    double E[9];
};

// rotations of up to 0.5 rad about each axis, a turn of up to 0.6 rad about the
// vertical, unit baseline, depths 4..8, lateral coordinates in +-2
Scene make_scene(std::mt19937_64& rng, int n) {
    std::uniform_real_distribution<double> ang(-0.5, 0.5), turn(-0.6, 0.6), lat(-2.0, 2.0), dep(4.0, 8.0);
    std::normal_distribution<double> n1(0.0, 1.0);
    Scene s;
    euler(ang(rng), ang(rng), ang(rng), s.rot.g1);
    euler(ang(rng), ang(rng), ang(rng), s.rot.g2);
    double Ry[9], G2t[9], tmp[9], R[9];
    euler(turn(rng), 0.0, 0.0, Ry);
    transpose3(s.rot.g2, G2t);
    mul3(Ry, s.rot.g1, tmp);
    mul3(G2t, tmp, R);
    double ta[3] = {n1(rng), n1(rng), n1(rng)}, t[3];
    const double tn = std::sqrt(ta[0] * ta[0] + ta[1] * ta[1] + ta[2] * ta[2]);
    for (double& v : ta) v /= tn;
    for (int r = 0; r < 3; ++r) t[r] = G2t[3 * r] * ta[0] + G2t[3 * r + 1] * ta[1] + G2t[3 * r + 2] * ta[2];
    const double T[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    mul3(T, R, s.E);
    double nn = 0.0;
    for (double v : s.E) nn += v * v;
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

// finite, unit norm, and the constrained form of G2 E G1^T
void check_model(const GeoModel& m, const GravRot& rot, int id) {
    double nn = 0.0;
    for (int e = 0; e < 9; ++e) {
        check(std::isfinite(m.h[e]), "finite entry", id);
        nn += m.h[e] * m.h[e];
    }
    check(std::fabs(std::sqrt(nn) - 1.0) < 1e-12, "unit norm", id);
    double G1t[9], tmp[9], Ep[9];
    transpose3(rot.g1, G1t);
    mul3(m.h, G1t, tmp);
    mul3(rot.g2, tmp, Ep);
    check(std::fabs(Ep[4]) < 1e-12 && std::fabs(Ep[0] - Ep[8]) < 1e-12 && std::fabs(Ep[2] + Ep[6]) < 1e-12,
          "constrained form", id);
}

HostClass host_class(const std::vector<double>& x1, const std::vector<double>& y1, const std::vector<double>& x2,
                     const std::vector<double>& y2) {
    HostClass c;
    c.n = x1.size();
    c.x.assign(x1.begin(), x1.end()); c.y.assign(y1.begin(), y1.end());
    c.a.assign(x2.begin(), x2.end()); c.c0.assign(y2.begin(), y2.end());
    c.c1.assign(x1.size(), 0.0);
    return c;
}

GravRot identity_rot() {
    GravRot r{};
    for (int k = 0; k < 9; ++k) r.g1[k] = r.g2[k] = (k % 4 == 0) ? 1.0 : 0.0;
    return r;
}

// the solver and the fit (k = 3, 4, 6 with the rows repeated) on three rows: no trap, finite models
int run_rows(const double rows[3][4], const GravRot& rot, int id) {
    std::vector<double> x1, y1, x2, y2;
    for (int rep = 0; rep < 2; ++rep)
        for (int i = 0; i < 3; ++i) {
            x1.push_back(rows[i][0]); y1.push_back(rows[i][1]); x2.push_back(rows[i][2]); y2.push_back(rows[i][3]);
        }
    GeoModel ms[kGModels];
    const int cnt = solve_g3(x1.data(), y1.data(), x2.data(), y2.data(), rot, ms);
    check(cnt >= 0 && cnt <= kGModels, "model count", id);
    for (int q = 0; q < cnt; ++q) check_model(ms[q], rot, id);
    const HostClass c = host_class(x1, y1, x2, y2);
    GeoModel f;
    for (std::vector<uint32_t> idx : {std::vector<uint32_t>{0, 1, 2}, std::vector<uint32_t>{0, 1, 2, 3},
                                      std::vector<uint32_t>{0, 1, 2, 3, 4, 5}})
        if (fit_g3_nonminimal(c, idx, rot, f)) check_model(f, rot, id);
    return cnt;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261020);
    const int kCases = 400;
    int hit = 0, models = 0;
    for (int id = 0; id < kCases; ++id) {
        const Scene s = make_scene(rng, 4);
        GeoModel ms[kGModels];
        const int cnt = solve_g3(s.x1.data(), s.y1.data(), s.x2.data(), s.y2.data(), s.rot, ms);
        check(cnt >= 0 && cnt <= kGModels, "model count", id);
        double best = 1e300;
        for (int q = 0; q < cnt; ++q) {
            check_model(ms[q], s.rot, id);
            for (int i = 0; i < 3; ++i) {
                const double* h = ms[q].h;
                const double r = s.x2[i] * (h[0] * s.x1[i] + h[1] * s.y1[i] + h[2]) +
                                 s.y2[i] * (h[3] * s.x1[i] + h[4] * s.y1[i] + h[5]) +
                                 (h[6] * s.x1[i] + h[7] * s.y1[i] + h[8]);
                check(std::fabs(r) < 1e-6, "epipolar equation", id);
            }
            best = std::min(best, dist_pm(ms[q].h, s.E));
        }
        hit += best < 1e-6;
        models += cnt;
        // k = 3 and k = 4 of the fit: the minimal solver's first model, bit for bit
        const HostClass c = host_class(s.x1, s.y1, s.x2, s.y2);
        for (std::vector<uint32_t> idx : {std::vector<uint32_t>{0, 1, 2}, std::vector<uint32_t>{0, 1, 2, 3}}) {
            GeoModel f;
            const bool ok = fit_g3_nonminimal(c, idx, s.rot, f);
            check(ok == (cnt > 0), "fit(k < 5) succeeds with the solver", id);
            if (ok && cnt > 0)
                for (int e = 0; e < 9; ++e) check(as_u64(f.h[e]) == as_u64(ms[0].h[e]), "fit(k < 5) bits", id);
        }
        GeoModel f;
        check(!fit_g3_nonminimal(c, {0, 1}, s.rot, f), "fit(k = 2) has no model", id);
    }
    check(hit >= kCases * 95 / 100, "true E recovered in >= 95 % of the samples", -1);

    int fit_hit = 0;
    const int kFits = 100;
    for (int id = 0; id < kFits; ++id) {
        const Scene s = make_scene(rng, 35);
        const HostClass c = host_class(s.x1, s.y1, s.x2, s.y2);
        std::vector<uint32_t> idx(35);
        for (uint32_t i = 0; i < 35; ++i) idx[i] = 34 - i;
        GeoModel f;
        if (fit_g3_nonminimal(c, idx, s.rot, f)) {
            check_model(f, s.rot, 1000 + id);
            fit_hit += dist_pm(f.h, s.E) < 1e-6;
        }
    }
    check(fit_hit >= kFits * 95 / 100, "35-point fit recovers E in >= 95 % of the scenes", -2);

    // degenerate and non-finite samples: 0 models or finite ones, no trap, and an end
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const GravRot eye = identity_rot();
    {
        double rows[3][4];
        for (auto& r : rows) { r[0] = 0.25; r[1] = -0.5; r[2] = 0.125; r[3] = 0.75; }
        check(run_rows(rows, eye, -3) == 0, "three identical rows", -3);
    }
    {
        double rows[3][4] = {};
        check(run_rows(rows, eye, -4) == 0, "all-zero rows", -4);
    }
    {
        double rows[3][4];
        for (int i = 0; i < 3; ++i) {
            const double t = 0.1 * i - 0.1;
            rows[i][0] = 0.3 + t; rows[i][1] = -0.1 + 2.0 * t; rows[i][2] = 0.05 + 1.5 * t; rows[i][3] = 0.2 - 0.5 * t;
        }
        run_rows(rows, eye, -5);                                   // collinear rays
    }
    for (int id = 0; id < 50; ++id) {
        // pure rotation about the vertical: x2 = R x1, every row of M vanishes at the true angle
        Scene s = make_scene(rng, 3);
        double Ry[9], G2t[9], tmp[9], R[9];
        euler(0.1 + 0.01 * id, 0.0, 0.0, Ry);
        transpose3(s.rot.g2, G2t);
        mul3(Ry, s.rot.g1, tmp);
        mul3(G2t, tmp, R);
        double rows[3][4];
        for (int i = 0; i < 3; ++i) {
            const double P[3] = {s.x1[i], s.y1[i], 1.0};
            double Q[3];
            for (int r = 0; r < 3; ++r) Q[r] = R[3 * r] * P[0] + R[3 * r + 1] * P[1] + R[3 * r + 2] * P[2];
            rows[i][0] = P[0]; rows[i][1] = P[1]; rows[i][2] = Q[0] / Q[2]; rows[i][3] = Q[1] / Q[2];
        }
        run_rows(rows, s.rot, -6);
        for (int i = 0; i < 3; ++i) { rows[i][2] = rows[i][0]; rows[i][3] = rows[i][1]; }
        run_rows(rows, eye, -7);                                   // no motion at all
    }
    for (double bad : {nan, inf, -inf}) {
        for (int at = 0; at < 12; ++at) {
            const Scene s = make_scene(rng, 3);
            double rows[3][4];
            for (int i = 0; i < 3; ++i) { rows[i][0] = s.x1[i]; rows[i][1] = s.y1[i]; rows[i][2] = s.x2[i]; rows[i][3] = s.y2[i]; }
            rows[at / 4][at % 4] = bad;
            check(run_rows(rows, s.rot, -8) == 0, "non-finite coordinate", -8);
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
