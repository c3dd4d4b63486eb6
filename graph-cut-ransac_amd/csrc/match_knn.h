// match_knn.h -- exact k-nearest-neighbour search over uint8 descriptors: the
// definition (host and device), the host twin and the merge.
//
// D1, D2, dim, d(i, j) and the TOTAL order (d(i, j), j) are match.h's.  For
// every row i and 1 <= k <= kKnnMaxK, idx[i][r] / dist[i][r], r = 0 .. k - 1,
// are the first k elements of that order, row-major n1 x k; positions from n2
// on (n2 < k) are kMatchNone / kMatchNone.  For k = 2 the columns are
// host_match_rows' idx / idx2 and dist / dist2, byte for byte.
//
// A candidate is match.h's key (d, j); kMatchNone / kMatchNone is the largest
// key and pads every list.  The first k of a union do not depend on how the
// union was partitioned, and knn_merge is a fixed network of minima and maxima
// over distinct keys (or the pad): any merge tree gives the same bytes.  The
// kernels (match_knn.hip) split the columns over lane halves and workgroups
// and still give the host loop's bytes.
//
// Plain C++: tests/cpp/match_knn_host.cpp includes this header alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "match.h"

namespace gcr {

constexpr uint32_t kKnnMaxK = 8;
constexpr uint64_t kKnnPad = ~0ull;              // match_key(kMatchNone, kMatchNone)

// the kernels' list capacities: k is rounded up to one of them (match_knn.hip)
constexpr uint32_t kKnnCapSmall = 4, kKnnCapLarge = 8;
inline constexpr uint32_t knn_capacity(uint32_t k) { return k <= kKnnCapSmall ? kKnnCapSmall : kKnnCapLarge; }

#if defined(__HIPCC__)
#define GCR_KNN_HD __host__ __device__
#else
#define GCR_KNN_HD
#endif

// The first K (a power of two) of the union of two ascending K-lists, ascending,
// into a.  min(a[r], b[K - 1 - r]) over r are the K smallest of the union and
// form a bitonic sequence; log2 K compare-exchange stages sort it.  Every index
// is a constant once unrolled: on the device the lists stay in registers.
template <int K>
GCR_KNN_HD inline void knn_merge(uint64_t (&a)[K], const uint64_t (&b)[K]) {
    static_assert(K >= 1 && (K & (K - 1)) == 0, "K is a power of two");
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = a[r] < b[K - 1 - r] ? a[r] : b[K - 1 - r];
#pragma unroll
    for (int s = K / 2; s >= 1; s /= 2) {
#pragma unroll
        for (int r = 0; r < K; ++r) {
            if ((r & s) == 0) {
                const uint64_t lo = a[r] < a[r + s] ? a[r] : a[r + s];
                const uint64_t hi = a[r] < a[r + s] ? a[r + s] : a[r];
                a[r] = lo;
                a[r + s] = hi;
            }
        }
    }
}

// nullptr, or the message naming the first bad argument
inline const char* knn_check_args(const void* d1, size_t n1, const void* d2, size_t n2, uint32_t dim, uint32_t k,
                                  const void* idx, const void* dist) {
    if (!d1) return "knn_descriptors: d1 is NULL";
    if (!d2) return "knn_descriptors: d2 is NULL";
    if (!idx) return "knn_descriptors: idx_out is NULL";
    if (!dist) return "knn_descriptors: dist_out is NULL";
    if (n1 == 0 || n1 > kMatchMaxRows) return "knn_descriptors: n1 must be in 1 .. 2^24";
    if (n2 == 0 || n2 > kMatchMaxRows) return "knn_descriptors: n2 must be in 1 .. 2^24";
    if (dim < kMatchDimStep || dim > kMatchDimMax || dim % kMatchDimStep != 0)
        return "knn_descriptors: dim must be a multiple of 32 in 32 .. 512";
    if (k == 0 || k > kKnnMaxK) return "knn_descriptors: k must be in 1 .. 8";
    return nullptr;
}

// The definition: rows [i0, i1) of D1 against all of D2, by plain loops.
inline void host_knn_rows(const uint8_t* d1, const uint8_t* d2, size_t n2, uint32_t dim, uint32_t k, size_t i0,
                          size_t i1, uint32_t* idx, uint32_t* dist) {
    for (size_t i = i0; i < i1; ++i) {
        const uint8_t* a = d1 + i * dim;
        uint32_t bd[kKnnMaxK], bj[kKnnMaxK];
        for (uint32_t r = 0; r < k; ++r) bd[r] = bj[r] = kMatchNone;
        for (size_t j = 0; j < n2; ++j) {
            const uint8_t* b = d2 + j * dim;
            uint32_t d = 0;
            for (uint32_t q = 0; q < dim; ++q) {
                const int32_t t = (int32_t)a[q] - (int32_t)b[q];
                d += (uint32_t)(t * t);
            }
            // j ascends, so an equal distance never displaces an earlier index
            if (!(d < bd[k - 1])) continue;
            uint32_t p = k - 1;
            for (; p > 0 && d < bd[p - 1]; --p) {
                bd[p] = bd[p - 1];
                bj[p] = bj[p - 1];
            }
            bd[p] = d;
            bj[p] = (uint32_t)j;
        }
        for (uint32_t r = 0; r < k; ++r) {
            idx[i * k + r] = bj[r];
            dist[i * k + r] = bd[r];
        }
    }
}

}  // namespace gcr

#if defined(__HIPCC__)
struct gcr_descriptors;

namespace gcr {
struct MatchWorkspace;

// One search on device memory (match_knn.hip): the launch and the merge.
// Nothing here allocates, copies or synchronises.
struct KnnDev {
    const uint8_t* d1;          // as MatchDev's
    const uint8_t* d2;
    const uint32_t* norm1;
    const uint32_t* norm2;
    size_t n1, n2;
    uint32_t dim, k;
    uint32_t splits, cols;      // match_plan_env's
    uint32_t* out[2];           // idx, dist: n1 x k each
    uint32_t* part[2];          // [splits][n1][k] each; not read for splits == 1
};
// k_knn<dim / 32, knn_capacity(k)>, then k_knn_merge for splits > 1; errors through hipGetLastError
void knn_enqueue(hipStream_t stream, const KnnDev& m);

// The array entry: uploads, runs the kernels on `stream`, downloads.
// ms_kernel (may be null): HIP-event time of the kernels alone.
hipError_t knn_device(hipStream_t stream, int n_cu, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2,
                      uint32_t dim, uint32_t k, uint32_t* idx, uint32_t* dist, double* ms_kernel);
// The rows of resident set a against b: the sets' buffers and norms, the
// workspace's device block and staging; one synchronisation, one download.
hipError_t knn_sets_run(hipStream_t stream, int n_cu, MatchWorkspace& ws, const gcr_descriptors* a,
                        const gcr_descriptors* b, uint32_t k, uint32_t* idx, uint32_t* dist, double* ms_kernel);
}  // namespace gcr
#endif
