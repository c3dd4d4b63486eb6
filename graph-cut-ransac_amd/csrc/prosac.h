// prosac.h -- PROSAC sampling of minimal samples: upstream GC-RANSAC's
// sampler 1 (Chum & Matas, "Matching with PROSAC", CVPR 2005).  The rows are
// in quality order, best first; early slots draw from the best-ranked rows
// and the pool widens on a fixed schedule until the sampler is the uniform
// one.  Everything else of a sample (distinct indices in draw order, the draw
// budget, the word addressing) is philox.h's.  There is no reference for it
// (the reference has its PROSAC sampler commented out), so this is the
// definition:
//
//   growth  N rows, minimal sample m, convergence length T_N (1 <= T_N <=
//           2^40).  g[m..N] is built once on the host in fp64, in exactly this
//           order, every operation rounded singly (no FMA can arise in
//           T * a / b or in a subtraction):
//             T = (double)T_N;  for i = 0 .. m-1: T = T * (double)(m - i) / (double)(N - i)
//             g[m] = 1
//             for n = m .. N-1:  T1 = T * (double)(n + 1) / (double)(n + 1 - m)
//                                g[n+1] = g[n] + (uint64_t)ceil(T1 - T);  T = T1
//           g is strictly increasing (every step adds at least 1).  The
//           device never rebuilds it.
//   pool    of slot s: t = s + 1, n(t) = the smallest n in [m, N] with
//           g[n] >= t.  A pure function of the slot index: all attempts of a
//           slot share it, and any lane, chunk, shard or rank finds the same.
//   sample  growth phase (there is such an n): m - 1 distinct indices of
//           [0, n - 1) in draw order by sample_distinct from the slot's
//           ordinary WordStream, the same draw budget, then index n - 1 in the
//           last position.  Past it (t > g[N]): sample_distinct over N with m
//           indices, the uniform sampler's own bits for that slot.
//
// Only the main loop's sampler changes.  Local optimisation's inner samples
// stay the uniform sampler's on its own stream (kStreamLO), drawn from the
// graph cut's inliers whatever their rank.  The stop is the reference's
// uniform bound (valid, since the sampler becomes the uniform one).  PROSAC's
// own non-randomness / maximality stop is opt-in (GCR_FLAG_PROSAC_STOP) and
// defined in prosac_stop.h; it reads this table's g[n] as the number of slots
// whose pool lies within the first n rows.
//
// Pinned: the oracle (oracle/gcr_oracle.cpp) restates this block without
// including this header; tests/test_oracle_samplers.py holds the restatement
// to the host entries bit for bit, and tests/test_gpu_oracle_samplers.py
// compares whole PROSAC runs of all five correspondence estimators with the
// oracle's run loop bitwise, through the Python wrapper's sort and unsort.
//
// The generators do not search g in global memory per attempt.  A workgroup
// covers at most kProsacWindow consecutive slots and g is strictly increasing,
// so its slots need at most the entries g[n_lo .. n_lo + kProsacWindow - 1],
// n_lo = n(first slot + 1): g[n_lo + k] >= g[n_lo] + k > first slot + k.  The
// workgroup finds n_lo once and copies that window to LDS (entries past N
// read as all-ones); each attempt searches the window, which returns the flat
// search's index for every slot of the workgroup.
#pragma once

#include "philox.h"

namespace gcr {

constexpr uint32_t kProsacWindow = 256;              // growth entries per workgroup (2 KB of LDS)
constexpr uint64_t kProsacMaxConvergence = 1ull << 40;
constexpr uint64_t kProsacDefaultConvergence = 100000;   // upstream's PROSAC sampler

// What a generator launch gets (never part of DevProblem): the growth table
// in device memory and where the launch's workgroups start.
struct ProsacTable {
    const uint64_t* g = nullptr;      // N + 1 entries, those below m are 0
    uint32_t n = 0;                   // N
    uint32_t m = 0;
    uint64_t g_n = 0;                 // g[N]: slots >= g_n are uniform
    // filled per launch: the launch's first slot and its lanes per slot (a
    // workgroup of B threads starts at slot0 + blockIdx.x * B / lanes)
    uint64_t slot0 = 0;
    uint32_t lanes = 1;
};

// the growth table (host; g_out: n + 1 entries, n >= m >= 1)
inline void prosac_growth(uint32_t n, uint32_t m, uint64_t convergence, uint64_t* g_out) {
    for (uint32_t i = 0; i < m; ++i) g_out[i] = 0;
    double T = (double)convergence;
    for (uint32_t i = 0; i < m; ++i) T = T * (double)(m - i) / (double)(n - i);
    g_out[m] = 1;
    for (uint32_t k = m; k < n; ++k) {
        const double T1 = T * (double)(k + 1) / (double)(k + 1 - m);
        g_out[k + 1] = g_out[k] + (uint64_t)ceil(T1 - T);
        T = T1;
    }
}

// smallest i in [lo, hi) with g[i] > slot (that is g[i] >= t, t = slot + 1);
// hi if there is none
template <class PTR>
GCR_HD uint32_t prosac_first(PTR g, uint32_t lo, uint32_t hi, uint64_t slot) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const bool hit = g[mid] > slot;
        hi = hit ? mid : hi;
        lo = hit ? lo : mid + 1;
    }
    return lo;
}

// the definition: the slot's pool size n by one search over the whole table;
// 0 past g[N] (the uniform phase)
GCR_HD uint32_t prosac_pool_flat(const uint64_t* g, uint32_t n, uint32_t m, uint64_t slot) {
    if (slot >= g[n]) return 0;
    return prosac_first(g, m, n, slot);              // none in [m, N): N itself
}

// the stream's slot, read back from its counter words
GCR_HD uint64_t prosac_slot(const WordStream& ws) { return (uint64_t)ws.ctr[0] | ((uint64_t)ws.ctr[1] << 32); }

// One sample of a slot whose pool is `pool` (0: uniform over n).  One
// sample_distinct serves both phases, so a generator holds one copy of the
// draw loop.
template <int MAXM>
GCR_HD bool sample_prosac(WordStream& ws, uint64_t n, int m, uint32_t pool, uint32_t* out) {
    const bool grow = pool != 0;
    if (!sample_distinct<MAXM>(ws, grow ? (uint64_t)(pool - 1u) : n, grow ? m - 1 : m, out)) return false;
    // constant-index store, as in sample_distinct
#pragma unroll
    for (int q = 0; q < MAXM; ++q)
        if (grow && q == m - 1) out[q] = pool - 1u;
    return true;
}

}  // namespace gcr
