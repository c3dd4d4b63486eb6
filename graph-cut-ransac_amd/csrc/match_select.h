// match_select.h -- the matchers' front-end rule: which rows of a 2-nearest-
// neighbour search are matches, and their ratios.  The definition (host and
// device) and the host twin.
//
// The inputs are a forward search's idx / dist / idx2 / dist2 (match.h, or
// match_geo.h's guided search), one per result row i, and optionally back[]:
// the first neighbour of every row of the other set from the reverse search.
// Everything is + - * / sqrt on doubles in one fixed order, which the host and
// gfx950 round identically (-ffp-contract=off), so the kernels
// (match_sets.hip) and host_match_select give the same bytes -- the bytes of
// features.match_descriptors / match_descriptors_guided's numpy statements.
//
//   found    plain: always.  guided: idx != kMatchNone.
//   none2    idx2 == kMatchNone.
//   ratio_i  sqrt((double)dist / (double)dist2) where found && !none2 &&
//            dist2 > 0, else exactly 1.0.
//   ratio test (has_ratio; rr = ratio * ratio, a double of the caller's)
//            plain:  !none2 && (double)dist < rr * (double)dist2
//            guided:  none2 || (double)dist < rr * (double)dist2
//   distance cap (guided and has_max_distance): (double)dist <= max_distance
//   mutual (back != nullptr): back[idx] == i, evaluated ONLY where found:
//            back[kMatchNone] would be read out of bounds.
//   keep     found and every enabled rule.
// The output is the kept rows in ascending i: the pairs (i, idx), ratio_i, and
// their count M.
//
// Plain C++: tests/cpp/match_select_host.cpp includes this header and match.h
// alone.
#pragma once

#include "gcr_hd.h"
#include "match.h"

namespace gcr {

// the select kernels' tiling (match_sets.hip): rows per workgroup, one per
// thread; gcr_match_select_tiling() reports it to tests
constexpr uint32_t kMatchSelectRows = 256;

struct MatchSelectRule {
    int guided;                 // match_geo.h's search: rows without a candidate exist
    int has_ratio;
    double rr;                  // ratio * ratio
    int has_max_distance;       // guided only
    double max_distance;
};

// The rule of one row.  nb: the length of back[] (the other set's rows); an
// idx past it never reaches back[].  *ratio_out is written whether or not the
// row is kept.
GCR_HD bool match_select_row(const MatchSelectRule& r, uint32_t i, uint32_t idx, uint32_t dist, uint32_t idx2,
                             uint32_t dist2, const uint32_t* back, uint32_t nb, double* ratio_out) {
    const bool found = r.guided ? idx != kMatchNone : true;
    const bool none2 = idx2 == kMatchNone;
    const double fd = (double)dist, fd2 = (double)dist2;
    *ratio_out = (found && !none2 && dist2 > 0u) ? sqrt(fd / fd2) : 1.0;
    bool keep = found;
    if (r.has_ratio) {
        const bool below = fd < r.rr * fd2;
        keep = keep && (r.guided ? (none2 || below) : (!none2 && below));
    }
    if (r.guided && r.has_max_distance) keep = keep && fd <= r.max_distance;
    if (back != nullptr && keep) keep = idx < nb && back[idx] == i;
    return keep;
}

// nullptr, or the message naming the first bad argument
inline const char* match_select_check_args(const void* idx, const void* dist, const void* idx2, const void* dist2,
                                           size_t n, const void* back, size_t nb, const MatchSelectRule* rule,
                                           const void* matches, const void* ratios, size_t cap, const void* m_out) {
    if (!idx) return "match_select: idx is NULL";
    if (!dist) return "match_select: dist is NULL";
    if (!idx2) return "match_select: idx2 is NULL";
    if (!dist2) return "match_select: dist2 is NULL";
    if (!rule) return "match_select: rule is NULL";
    if (!matches) return "match_select: matches_out is NULL";
    if (!ratios) return "match_select: ratios_out is NULL";
    if (!m_out) return "match_select: m_out is NULL";
    if (n == 0 || n > kMatchMaxRows) return "match_select: n must be in 1 .. 2^24";
    if (back && (nb == 0 || nb > kMatchMaxRows)) return "match_select: nb must be in 1 .. 2^24 with back";
    if (cap < n) return "match_select: cap must be at least n";
    if (rule->has_ratio && !(rule->rr > 0.0 && rule->rr <= DBL_MAX))
        return "match_select: rr must be finite and > 0";
    if (rule->has_max_distance && !(rule->max_distance >= 0.0))
        return "match_select: max_distance must be >= 0, not NaN";
    return nullptr;
}

// The definition by plain loops.  matches: (i, idx) pairs, ratios: one per
// pair; returns M.
inline size_t host_match_select(const uint32_t* idx, const uint32_t* dist, const uint32_t* idx2, const uint32_t* dist2,
                                size_t n, const uint32_t* back, size_t nb, const MatchSelectRule& rule,
                                uint32_t* matches, double* ratios) {
    size_t m = 0;
    for (size_t i = 0; i < n; ++i) {
        double ratio;
        if (!match_select_row(rule, (uint32_t)i, idx[i], dist[i], idx2[i], dist2[i], back, (uint32_t)nb, &ratio))
            continue;
        matches[2 * m] = (uint32_t)i;
        matches[2 * m + 1] = idx[i];
        ratios[m] = ratio;
        ++m;
    }
    return m;
}

}  // namespace gcr
