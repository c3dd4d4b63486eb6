// solver.h -- the solver table: what the engine and the launchers need to know
// about each estimator (GCR_SOLVER_*, include/gcr.h), one row each.
//
// SOLVER and KIND are two things.  The solver is the estimator: it decides the
// sample size, the generator kernel, the models per sample and what a problem
// must carry (calibration, gravity rotations, SIFT columns).  The kind is the
// residual: the layout of the device classes and the KIND the scorers, masks,
// residual and inlier-mass kernels are templated on.  The rectification solvers
// and the plain homography / fundamental matrix are their own kind; both
// essential-matrix solvers run on K-normalised rows with the fundamental
// matrix's Sampson distance, the SIFT homography with the homography's
// transfer error.  DevProblem (kernels.h) carries the kind; a launcher that
// needs the estimator takes it as an argument.
#pragma once

#include "ess.h"
#include "fund.h"
#include "gcr.h"
#include "gcr_hd.h"
#include "grav.h"
#include "sifth.h"

namespace gcr {

constexpr int kSolverCount = 8;                     // GCR_SOLVER_* are 0 .. kSolverCount - 1
// the kinds that are not a rectification solver's own
constexpr int kKindHomography = GCR_SOLVER_HOMOGRAPHY4;
constexpr int kKindFundamental = GCR_SOLVER_FUNDAMENTAL7;

struct SolverRow {
    int m;                  // minimal sample size of class 0 (class 1, SIFT22 only: 2)
    int per;                // models per sample = hypotheses per slot
    int classes;            // feature classes
    int kind;               // residual kind (above)
    bool rect;              // rectification solver: RectModel, N x 3 features
    bool corr;              // correspondence estimator: GeoModel, N x 4 rows
    bool calibrated;        // K-normalised rows, pixel grid, pixel threshold
    bool needs_gravity;     // the generator takes the two gravity rotations (grav.h)
    bool needs_sift;        // the generator takes the stored SIFT columns (sifth.h)
};

constexpr SolverRow kSolverTable[kSolverCount] = {
    // m, per, classes, kind | rect, corr, calibrated, needs_gravity, needs_sift
    {3, 1, 1, GCR_SOLVER_SCALE3, true, false, false, false, false},
    {3, 1, 1, GCR_SOLVER_SCALE3_ORIGINAL, true, false, false, false, false},
    {2, 1, 2, GCR_SOLVER_SIFT22, true, false, false, false, false},
    {4, 1, 1, kKindHomography, false, true, false, false, false},
    {7, kFModels, 1, kKindFundamental, false, true, false, false, false},
    {5, kEModels, 1, kKindFundamental, false, true, true, false, false},
    {3, kGModels, 1, kKindFundamental, false, true, true, true, false},
    {2, kSModels, 1, kKindHomography, false, true, false, false, true},
};
static_assert(GCR_SOLVER_SCALE3 == 0 && GCR_SOLVER_SCALE3_ORIGINAL == 1 && GCR_SOLVER_SIFT22 == 2 &&
                  GCR_SOLVER_HOMOGRAPHY4 == 3 && GCR_SOLVER_FUNDAMENTAL7 == 4 && GCR_SOLVER_ESSENTIAL5 == 5 &&
                  GCR_SOLVER_ESSENTIAL3_GRAVITY == 6 && GCR_SOLVER_HOMOGRAPHY2_SIFT == 7,
              "kSolverTable's rows are in GCR_SOLVER_* order");

constexpr bool solver_known(int solver) { return solver >= 0 && solver < kSolverCount; }

// The row of a solver; an unknown value gets a row without any property (host
// code: the entry points test their argument with it before the range check).
constexpr SolverRow solver_row(int solver) {
    return solver_known(solver) ? kSolverTable[solver] : SolverRow{0, 0, 0, -1, false, false, false, false, false};
}

// The class count in closed form, for device code (a table read there would be
// a load from constant memory); held to the table below.
GCR_HD constexpr int solver_classes(int solver) { return solver == GCR_SOLVER_SIFT22 ? 2 : 1; }

constexpr bool solver_table_consistent() {
    for (int s = 0; s < kSolverCount; ++s) {
        const SolverRow r = kSolverTable[s];
        if (r.classes != solver_classes(s) || r.rect == r.corr || kSolverTable[r.kind].kind != r.kind) return false;
    }
    return true;
}
static_assert(solver_table_consistent(), "solver_classes and the kinds agree with kSolverTable");

}  // namespace gcr
