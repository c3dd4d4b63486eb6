// napsac.h -- NAPSAC sampling of minimal samples: upstream GC-RANSAC's
// sampler 2, progressive NAPSAC (Barath et al., "MAGSAC++, a fast, reliable
// and accurate robust estimator", CVPR 2020; Myatt et al., "NAPSAC", BMVC
// 2002).  A sample is drawn from the neighbourhood of its first point, and
// the neighbourhood widens until the sampler is the uniform one.  It needs no
// scores, only the positions, and suits inliers that are a local structure (a
// small plane, one object) among outliers spread over the images.
//
// Upstream widens a point's neighbourhood by a hit counter per point, which is
// sequential state.  Here a slot's sample is a function of (seed, slot,
// attempt) alone, as everywhere in this engine (replay, batch_slots, shards),
// so the growth is by the slot index.  There is no reference for it: this is
// the definition.
//
//   layers  l = 0..3 are grids over (x1, y1, x2, y2) with c = 16, 8, 4, 2
//           cells per axis (upstream's layer sizes), cell size extent / c per
//           axis, the four extents given by the caller.  A row's cell is
//           graphcut.h's grid cell with cell_number = c (grid_sorted_cells: the
//           same key, rows with equal key share a cell); cells in key order,
//           rows ascending inside a cell: the layer's member list.  Layer 4 is
//           all N rows as one cell, row r at position r.  Per row and layer:
//           start (where its cell begins in the member list), count (rows in
//           the cell) and pos (the row's position in the cell).  Built on the
//           host (napsac_layers.h); the 8-cell layer is the graph-cut grid of
//           neighborhood_size = 8.
//   sample  slot s, local length T (1 <= T <= 2^40), minimal sample m.
//           s >= T: sample_distinct over N with m indices, the uniform
//           sampler's own bits for that slot.
//           s < T:  l_min = floor(4 s / T): four equal quarters, the finest
//           admissible layer coarsens from 16 cells to 2.  The first index i0
//           is one draw over N from the attempt's ordinary WordStream (the
//           uniform sampler's first index of that slot and attempt).  l is the
//           smallest layer >= l_min whose count[i0] >= m, or 4.  The other
//           m - 1 indices: distinct values of [0, count - 1) in draw order,
//           continuing the same stream under the same draw budget; a value r
//           is position r + (r >= pos) of the cell's member list (the cell
//           without i0).  The sample is i0, then these rows in draw order.
//           Every attempt of a slot shares l_min and draws its own i0.
//
// For the essential-matrix estimators the layers lie over the PIXEL rows, as
// the graph cut's neighbourhood grid does, not over the K-normalised rows the
// solver reads.  Local optimisation's inner samples stay the uniform
// sampler's on its own stream (kStreamLO).
//
// Pinned: the oracle (oracle/gcr_oracle.cpp) restates this block without
// including this header, its layers grouped by its own grid index;
// tests/test_oracle_samplers.py holds layers and samples to the host entries
// bit for bit, and tests/test_gpu_oracle_samplers.py compares whole NAPSAC
// runs of all five correspondence estimators with the oracle's run loop
// bitwise.
//
// Only the sampler changes: the stop is the reference's uniform bound.  From
// slot T on every sample is the uniform sampler's, which is what that bound
// describes.  The engine applies the same bound before T as well, where the
// samples are not uniform: there it is a heuristic, and a run whose bound
// falls below T ends inside the local phase.
//
// The generators pay two dependent loads per local attempt: the row's record
// (one 64-byte line holds all four layers) and then the m - 1 members.
#pragma once

#include "philox.h"
#include "prosac.h"

namespace gcr {

constexpr int kNapsacLayers = 4;                                  // grid layers; layer 4 is all rows
constexpr uint32_t kNapsacCells[kNapsacLayers] = {16, 8, 4, 2};   // cells per axis
constexpr uint64_t kNapsacMaxIterations = 1ull << 40;

// one row's cell in each grid layer: one cache line
struct alignas(64) NapsacRecord {
    uint32_t start[kNapsacLayers];
    uint32_t count[kNapsacLayers];
    uint32_t pos[kNapsacLayers];
    uint32_t pad[4];
};
static_assert(sizeof(NapsacRecord) == 64, "one cache line per row");

// What a generator launch gets (never part of DevProblem).
struct NapsacTable {
    const NapsacRecord* rec = nullptr;    // N records
    const uint32_t* members = nullptr;    // 4 N rows: layer l's member list at l * N
    uint32_t n = 0;                       // N
    uint32_t m = 0;
    uint64_t T = 0;                       // local length: slots >= T are uniform
};

// floor(4 s / T) for s < T <= 2^40, without a division
GCR_HD int napsac_min_layer(uint64_t slot, uint64_t T) {
    const uint64_t s4 = 4 * slot;
    return (int)(s4 >= T) + (int)(s4 >= 2 * T) + (int)(s4 >= 3 * T);
}

// sample_distinct's loop entered with out[0 .. j0) already drawn: indices j0 ..
// m - 1 distinct from one another and from out[q0 .. j0), the same budget and
// the same constant-index stores (philox.h)
template <int MAXM>
GCR_HD bool sample_distinct_from(WordStream& ws, uint64_t n, int q0, int j0, int m, uint32_t* out) {
    int j = j0;
    while (j < m) {
        if (ws.next >= kMaxSampleDraws) return false;
        const uint32_t v = (uint32_t)mulhi64(ws.word(), n);
        bool dup = false;
#pragma unroll
        for (int q = 0; q < MAXM; ++q)
            if (q >= q0 && q < j && out[q] == v) dup = true;
#pragma unroll
        for (int q = 0; q < MAXM; ++q)
            if (!dup && q == j) out[q] = v;
        j += dup ? 0 : 1;
    }
    return true;
}

// One sample of the stream's slot.  One draw loop serves both phases (past T
// it continues the uniform sample whose first index i0 is), so a generator
// holds one copy of it.
template <int MAXM>
GCR_HD bool sample_napsac(WordStream& ws, const NapsacTable& t, int m, uint32_t* out) {
    const uint64_t slot = prosac_slot(ws);
    const bool local = slot < t.T;
    if (!sample_distinct<1>(ws, t.n, 1, out)) return false;
    const uint32_t i0 = out[0];
    // layer 4: every row, row r at position r
    bool grid = false;
    uint64_t base = 0;
    uint32_t count = t.n, pos = i0;
    if (local) {
        const int lmin = napsac_min_layer(slot, t.T);
        const NapsacRecord r = t.rec[i0];
#pragma unroll
        for (int l = kNapsacLayers - 1; l >= 0; --l)
            if (l >= lmin && r.count[l] >= (uint32_t)m) {
                grid = true;
                base = (uint64_t)l * t.n + r.start[l];
                count = r.count[l];
                pos = r.pos[l];
            }
    }
    if (!sample_distinct_from<MAXM>(ws, local ? (uint64_t)(count - 1u) : (uint64_t)t.n, local ? 1 : 0, 1, m, out))
        return false;
#pragma unroll
    for (int q = 1; q < MAXM; ++q)
        if (local && q < m) {
            const uint32_t p = out[q] + (out[q] >= pos ? 1u : 0u);
            out[q] = grid ? t.members[base + p] : p;
        }
    return true;
}

}  // namespace gcr
