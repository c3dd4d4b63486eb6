// Prints csrc/solver.h's table, one line per GCR_SOLVER_* value:
//   solver m per classes kind rect corr calibrated needs_gravity needs_sift
// tests/test_solver_table.py compares the lines with the expected rows.
#include <cstdio>

#include "solver.h"

int main() {
    for (int s = 0; s < gcr::kSolverCount; ++s) {
        const gcr::SolverRow r = gcr::solver_row(s);
        std::printf("%d %d %d %d %d %d %d %d %d %d\n", s, r.m, r.per, r.classes, r.kind, (int)r.rect, (int)r.corr,
                    (int)r.calibrated, (int)r.needs_gravity, (int)r.needs_sift);
    }
    // values outside the table have no property
    const gcr::SolverRow lo = gcr::solver_row(-1), hi = gcr::solver_row(gcr::kSolverCount);
    std::printf("unknown %d %d\n", (int)(lo.rect || lo.corr || lo.calibrated || lo.needs_gravity || lo.needs_sift),
                (int)(hi.rect || hi.corr || hi.calibrated || hi.needs_gravity || hi.needs_sift));
    return 0;
}
