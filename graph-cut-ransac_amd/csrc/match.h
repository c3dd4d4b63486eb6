// match.h -- exact 2-nearest-neighbour matching of uint8 descriptors: the
// definition (host and device) and the host twin.
//
// D1 is n1 x dim, D2 is n2 x dim, uint8, row-major; dim is a multiple of 32 in
// 32..512.  d(i, j) = sum_k (D1[i,k] - D2[j,k])^2 as a uint32 (at most
// 512 * 255^2 = 33 292 800).  For every row i the neighbours are ordered by
// the TOTAL order (d(i, j), j): on equal distances the lower index is nearer.
// idx / dist are the first element of that order, idx2 / dist2 the second
// (kMatchNone for both where n2 == 1).  Because the order is total the result
// does not depend on how the columns are partitioned or in which order
// partial results are merged: the kernels (match.hip) split the columns over
// lanes, waves and workgroups and still give the host loop's bytes.
//
// Plain C++: tests/cpp/match_host.cpp includes this header alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gcr {

constexpr uint32_t kMatchNone = 0xFFFFFFFFu;     // no second neighbour (n2 == 1)
constexpr uint32_t kMatchDimStep = 32, kMatchDimMax = 512;
constexpr size_t kMatchMaxRows = (size_t)1 << 24;

// the kernels' tiling (match.hip); gcr_match_tiling() reports them to tests
constexpr uint32_t kMatchRowsPerWg = 128;        // D1 rows per workgroup: four waves of 32
constexpr uint32_t kMatchStepCols = 64;          // D2 rows staged per step: two 32 x 32 tiles
constexpr uint32_t kMatchSplitMinCols = 256;     // a column split is never planned narrower

// One candidate of the order: (d, j) packed so that integer comparison is the
// lexicographic one.  kMatchNone / kMatchNone is the largest key.
inline constexpr uint64_t match_key(uint32_t d, uint32_t j) { return ((uint64_t)d << 32) | j; }

// The two best of the union of two sorted pairs (a1 <= a2, b1 <= b2, all
// distinct or the sentinel): associative and commutative, so any merge tree
// gives the same pair.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void match_merge(uint64_t& a1, uint64_t& a2, uint64_t b1, uint64_t b2) {
    if (b1 < a1) {
        const uint64_t s = a1 < b2 ? a1 : b2;
        a1 = b1;
        a2 = s;
    } else if (b1 < a2) {
        a2 = b1;
    }
}

// nullptr, or the message naming the first bad argument
inline const char* match_check_args(const void* d1, size_t n1, const void* d2, size_t n2, uint32_t dim,
                                    const void* idx, const void* dist, const void* idx2, const void* dist2) {
    if (!d1) return "match_descriptors: d1 is NULL";
    if (!d2) return "match_descriptors: d2 is NULL";
    if (!idx) return "match_descriptors: idx_out is NULL";
    if (!dist) return "match_descriptors: dist_out is NULL";
    if (!idx2) return "match_descriptors: idx2_out is NULL";
    if (!dist2) return "match_descriptors: dist2_out is NULL";
    if (n1 == 0 || n1 > kMatchMaxRows) return "match_descriptors: n1 must be in 1 .. 2^24";
    if (n2 == 0 || n2 > kMatchMaxRows) return "match_descriptors: n2 must be in 1 .. 2^24";
    if (dim < kMatchDimStep || dim > kMatchDimMax || dim % kMatchDimStep != 0)
        return "match_descriptors: dim must be a multiple of 32 in 32 .. 512";
    return nullptr;
}

// The definition: rows [i0, i1) of D1 against all of D2, by plain loops.
inline void host_match_rows(const uint8_t* d1, const uint8_t* d2, size_t n2, uint32_t dim, size_t i0, size_t i1,
                            uint32_t* idx, uint32_t* dist, uint32_t* idx2, uint32_t* dist2) {
    for (size_t i = i0; i < i1; ++i) {
        const uint8_t* a = d1 + i * dim;
        uint32_t bd = kMatchNone, bj = kMatchNone, sd = kMatchNone, sj = kMatchNone;
        for (size_t j = 0; j < n2; ++j) {
            const uint8_t* b = d2 + j * dim;
            uint32_t d = 0;
            for (uint32_t k = 0; k < dim; ++k) {
                const int32_t t = (int32_t)a[k] - (int32_t)b[k];
                d += (uint32_t)(t * t);
            }
            // j ascends, so an equal distance never displaces an earlier index
            if (d < bd) {
                sd = bd;
                sj = bj;
                bd = d;
                bj = (uint32_t)j;
            } else if (d < sd) {
                sd = d;
                sj = (uint32_t)j;
            }
        }
        idx[i] = bj;
        dist[i] = bd;
        idx2[i] = sj;
        dist2[i] = sd;
    }
}

// The column split the kernels use for n1 x n2 on a device of n_cu compute
// units; `pin` > 0 is GCR_MATCH_SPLIT.  cols_out: columns per split (a
// multiple of kMatchStepCols); returns the number of splits (>= 1).
inline uint32_t match_plan(size_t n1, size_t n2, int n_cu, int pin, uint32_t* cols_out) {
    const size_t row_blocks = (n1 + kMatchRowsPerWg - 1) / kMatchRowsPerWg;
    const size_t steps = (n2 + kMatchStepCols - 1) / kMatchStepCols;
    size_t want;
    if (pin > 0) {
        want = (size_t)pin < steps ? (size_t)pin : steps;
    } else {
        // four workgroups (16 waves) per compute unit: measured at 10 000 x 10 000 x 128 the
        // kernels take 0.32 / 0.18 / 0.10 / 0.074 / 0.060 ms at 1 / 2 / 4 / 7 / 16 splits
        // (79 row blocks); no split narrower than kMatchSplitMinCols
        const size_t target = 4 * (size_t)(n_cu > 0 ? n_cu : 1);
        want = (target + row_blocks - 1) / row_blocks;
        const size_t cap = (n2 + kMatchSplitMinCols - 1) / kMatchSplitMinCols;
        if (want > cap) want = cap;
        if (want < 1) want = 1;
    }
    size_t cols = (n2 + want - 1) / want;
    cols = (cols + kMatchStepCols - 1) / kMatchStepCols * kMatchStepCols;
    *cols_out = (uint32_t)cols;
    return (uint32_t)((n2 + cols - 1) / cols);
}

#if defined(__HIPCC__)
// One search on device memory (match.hip): the plan, the launch and the merge.
// Nothing here allocates, copies or synchronises.
struct MatchDev {
    const uint8_t* d1;          // n1 x dim, rows 16-byte aligned; no padding: every read is clamped by index
    const uint8_t* d2;          // n2 x dim
    const uint32_t* norm1;      // match_norms_enqueue's, n1
    const uint32_t* norm2;      // n2
    size_t n1, n2;
    uint32_t dim;
    uint32_t splits, cols;      // match_plan_env's
    uint32_t* out[4];           // idx, dist, idx2, dist2: n1 each
    uint32_t* part[4];          // [splits][n1] each; not read for splits == 1
};
// match_plan under GCR_MATCH_SPLIT=k (1 .. 1024, read per call): the number of column splits
uint32_t match_plan_env(size_t n1, size_t n2, int n_cu, uint32_t* cols_out);
// |row - 128|^2 of every row of d1 and of d2 (n2 may be 0) in one launch
void match_norms_enqueue(hipStream_t stream, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2, uint32_t dim,
                         uint32_t* norm1, uint32_t* norm2);
// k_match<dim / 32>, then k_match_merge for splits > 1; errors through hipGetLastError
void match_enqueue(hipStream_t stream, const MatchDev& m);

// match.hip: uploads, runs the kernels on `stream`, downloads.  ms_kernel
// (may be null): HIP-event time of the kernels alone.
hipError_t match_device(hipStream_t stream, int n_cu, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2,
                        uint32_t dim, uint32_t* idx, uint32_t* dist, uint32_t* idx2, uint32_t* dist2,
                        double* ms_kernel);
#endif

}  // namespace gcr
