// guided.h -- guided (importance) sampling of minimal samples: upstream
// GC-RANSAC's sampler 3.  Correspondence i is drawn with probability
// w[i] / sum(w) instead of 1 / N; everything else of a sample (distinct
// indices in draw order, the draw budget, the word addressing) is philox.h's.
// There is no reference for it, so this is the definition:
//
//   CDF     built once on the host, sequentially in index order in fp64:
//           c[i] = c[i-1] + w[i], c[-1] = 0, total = c[N-1].  w[i] is finite
//           and >= 0, at least m of them are > 0 and the running sum stays
//           finite.  The device never re-sums.
//   draw    one 64-bit word W of the WordStream:
//           r = (double)(W >> 11) * 2^-53 (exact), u = r * total (one
//           rounding, no FMA); the index is the smallest i with c[i] > u, or,
//           if u rounded up to total, the smallest i with c[i] == total.
//           An entry with w[i] == 0 has c[i] == c[i-1] (c[0] == 0 for i = 0):
//           whenever it satisfies either condition so does its predecessor
//           (and 0 > u, 0 == total never hold), so it is never the smallest:
//           a zero-weight entry is never drawn.
//   sample  m distinct indices in draw order, repeats rejected exactly as
//           sample_distinct rejects them, the same budget (kMaxSampleDraws).
//
// The search runs in two levels.  The host cuts the CDF into at most
// kGuidedCoarse buckets of S = ceil(N / kGuidedCoarse) entries and keeps each
// bucket's last (largest) value in a coarse table: coarse[k] = c[min((k+1)S,
// N) - 1].  The CDF is non-decreasing, so a bucket holds an entry > u exactly
// when its last value is > u, and the first such bucket holds the smallest
// such entry: the coarse search (the generators keep the table in LDS)
// followed by at most ceil(log2 S) CDF loads inside the bucket returns the
// flat search's index for every u, whatever runs of equal values cross a
// bucket boundary.
#pragma once

#include "philox.h"

namespace gcr {

constexpr uint32_t kGuidedCoarse = 256;      // coarse table entries (2 KB of LDS)

GCR_HD uint32_t guided_stride(uint32_t n) { return (uint32_t)(((uint64_t)n + kGuidedCoarse - 1) / kGuidedCoarse); }
GCR_HD uint32_t guided_buckets(uint32_t n) {
    const uint32_t s = guided_stride(n);
    return s == 0 ? 0 : (uint32_t)(((uint64_t)n + s - 1) / s);
}

// What a generator launch gets (never part of DevProblem): the CDF and its
// coarse table in device memory.
struct GuidedTable {
    const double* cdf = nullptr;      // N entries
    const double* coarse = nullptr;   // guided_buckets(N) entries
    uint32_t n = 0;
    uint32_t stride = 0;              // S
    uint32_t buckets = 0;
    double total = 0.0;
};

// the position in the CDF's range that word W selects
GCR_HD double guided_u(uint64_t W, double total) {
    const double r = (double)(W >> 11) * 0x1p-53;
    return r * total;
}

// smallest i in [lo, hi) with c[i] > u (kGE: c[i] >= u); hi if there is none
template <bool kGE, class PTR>
GCR_HD uint32_t guided_first(PTR c, uint32_t lo, uint32_t hi, double u) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const double v = c[mid];
        const bool hit = kGE ? v >= u : v > u;
        hi = hit ? mid : hi;
        lo = hit ? lo : mid + 1;
    }
    return lo;
}

// the definition: one search over the whole CDF
GCR_HD uint32_t guided_index_flat(const double* cdf, uint32_t n, double total, double u) {
    const uint32_t i = guided_first<false>(cdf, 0u, n, u);
    return i < n ? i : guided_first<true>(cdf, 0u, n, total);
}

// the same index through the coarse table (`coarse`: t.coarse or a copy of it)
template <class PTR>
GCR_HD uint32_t guided_index(const GuidedTable& t, PTR coarse, double u) {
    uint32_t k = guided_first<false>(coarse, 0u, t.buckets, u);
    const bool top = k == t.buckets;                 // u rounded up to total
    if (top) k = guided_first<true>(coarse, 0u, t.buckets, t.total);
    k = k < t.buckets ? k : t.buckets - 1u;          // (a consistent table never needs it: reads stay in bounds)
    // the bucket's last entry satisfies the predicate: search the ones before it
    const uint32_t lo = k * t.stride;
    const uint32_t rem = t.n - lo;
    const uint32_t last = lo + (rem < t.stride ? rem : t.stride) - 1u;
    return top ? guided_first<true>(t.cdf, lo, last, t.total) : guided_first<false>(t.cdf, lo, last, u);
}

// sample_distinct with guided draws: m distinct indices in draw order
template <int MAXM, class PTR>
GCR_HD bool sample_guided(WordStream& ws, const GuidedTable& t, PTR coarse, int m, uint32_t* out) {
    int j = 0;
    while (j < m) {
        if (ws.next >= kMaxSampleDraws) return false;
        const uint32_t v = guided_index(t, coarse, guided_u(ws.word(), t.total));
        bool dup = false;
#pragma unroll
        for (int q = 0; q < MAXM; ++q)
            if (q < j && out[q] == v) dup = true;
        // constant-index stores, as in sample_distinct
#pragma unroll
        for (int q = 0; q < MAXM; ++q)
            if (!dup && q == j) out[q] = v;
        j += dup ? 0 : 1;
    }
    return true;
}

}  // namespace gcr
