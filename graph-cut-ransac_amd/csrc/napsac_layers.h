// napsac_layers.h -- the host side of napsac.h: the four grid layers of a
// problem's rows, grouped by graphcut.h's grid (grid_sorted_cells: one key
// function for the graph cut's neighbourhood grid and for these layers).
#pragma once

#include <cmath>
#include <vector>

#include "graphcut.h"
#include "napsac.h"

namespace gcr {

struct NapsacLayers {
    std::vector<NapsacRecord> rec;       // N
    std::vector<uint32_t> members;       // 4 N: layer l's member list at l * N
};

// extent = {w1, h1, w2, h2}
inline bool napsac_extent_ok(const double extent[4]) {
    for (int d = 0; d < 4; ++d)
        if (!(extent[d] > 0.0) || !std::isfinite(extent[d])) return false;
    return true;
}

// cols: the four columns x1, y1, x2, y2 of n rows (n < 2^32 - 1)
inline void napsac_layers(const double* const* cols, size_t n, const double extent[4], NapsacLayers& out) {
    out.rec.assign(n, NapsacRecord{});
    out.members.assign((size_t)kNapsacLayers * n, 0u);
    for (int l = 0; l < kNapsacLayers; ++l) {
        const uint32_t c = kNapsacCells[l];
        double cs[4];
        for (int d = 0; d < 4; ++d) cs[d] = extent[d] / static_cast<double>(c);
        const auto kp = grid_sorted_cells(cols, 4, n, cs, c);
        uint32_t* mem = out.members.data() + (size_t)l * n;
        for (size_t s0 = 0; s0 < n;) {
            size_t e = s0;
            while (e < n && kp[e].first == kp[s0].first) ++e;
            for (size_t q = s0; q < e; ++q) {
                const uint32_t row = kp[q].second;
                mem[q] = row;
                out.rec[row].start[l] = (uint32_t)s0;
                out.rec[row].count[l] = (uint32_t)(e - s0);
                out.rec[row].pos[l] = (uint32_t)(q - s0);
            }
            s0 = e;
        }
    }
}

inline NapsacTable napsac_host_table(const NapsacLayers& L, size_t n, uint32_t m, uint64_t T) {
    NapsacTable t;
    t.rec = L.rec.data();
    t.members = L.members.data();
    t.n = (uint32_t)n;
    t.m = m;
    t.T = T;
    return t;
}

}  // namespace gcr
