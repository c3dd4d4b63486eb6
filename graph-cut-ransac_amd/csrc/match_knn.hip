// match_knn.hip -- exact k-nearest-neighbour descriptor search on the int8
// matrix cores (match_knn.h is the definition; gcr_knn_descriptors and
// gcr_knn_sets the entries).
//
// The tiling is k_match's (match.hip): a workgroup is four waves, each wave
// owns 32 rows of D1 in registers as the B operand of
// v_mfma_i32_32x32x32_i8; per step the workgroup stages kMatchStepCols rows of
// D2 in the LDS (row stride dim + 16 bytes); the columns are split over
// workgroups by match_plan_env; padded columns are masked by INDEX; the row's
// |a|^2 is added at the end.  The norms are match.hip's (match_norms_enqueue).
//
// What differs is the selection.
//   k_knn<NK, KC>   A lane keeps its KC best candidates as 2 KC registers: e[r]
//                   ascending with the column j[r].  A lane meets its columns
//                   in ascending order, so inserting with `ev < e[r]` keeps the
//                   lower index first on a tie.  The insertion is one fully
//                   unrolled chain over constant register indices -- position r
//                   takes its left neighbour, the new candidate or itself --
//                   so the list is never indexed dynamically and nothing goes
//                   to scratch.  A tile is skipped when no lane's minimum of
//                   its 16 values beats that lane's KC-th best, and inside a
//                   tile a column (one result register) that no lane of the
//                   wave takes; both tests are wave-uniform branches.  At the end
//                   the two lane halves (disjoint columns of one row) are
//                   merged by knn_merge<KC> on the keys (d, j), and the first
//                   k columns are written.  k is rounded up to the capacity
//                   KC in {4, 8}: 16 dim classes x 2 capacities.
//   k_knn_merge<KC> the splits' partial lists of a row merged by the same
//                   knn_merge.  Not launched for one split.
// Device memory beyond the descriptors and norms: the results and the
// partials, O(n1 * k * splits).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "match_knn.h"
#include "match_sets.h"

namespace gcr {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kKnnThreads = 256;
constexpr uint32_t kSignFlip = 0x80808080u;
static_assert(kKnnThreads == (int)(kMatchRowsPerWg / 32u) * 64, "four waves of 32 rows");

struct KnnArgs {
    const uint8_t* d1;
    const uint8_t* d2;
    const uint32_t* norm1;      // |D1[i] - 128|^2
    const uint32_t* norm2;
    uint32_t n1, n2;
    uint32_t splits, cols;      // column splits, columns per split (multiple of kMatchStepCols)
    uint32_t k;                 // columns written, <= the kernel's capacity
    // [splits][n1][k] partials; the results themselves for splits == 1
    uint32_t *p_idx, *p_dist;
    uint32_t *idx, *dist;       // n1 x k
};

template <int NK, int KC>
__global__ __launch_bounds__(kKnnThreads) void k_knn(KnnArgs a) {
    constexpr uint32_t DIM = NK * 32;
    constexpr uint32_t STRIDE = DIM + 16;                 // LDS row stride, bytes
    constexpr uint32_t CHUNKS = DIM / 16;                 // 16-byte chunks of a row
    __shared__ __attribute__((aligned(16))) uint8_t s_d2[kMatchStepCols * STRIDE];
    __shared__ __attribute__((aligned(16))) int s_nb[kMatchStepCols];

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t rb = blockIdx.x / a.splits, sp = blockIdx.x % a.splits;
    const uint32_t i = rb * kMatchRowsPerWg + wave * 32u + r;
    const uint32_t ic = i < a.n1 ? i : a.n1 - 1;          // rows past the end read the last row, never written

    v4i breg[NK];
    {
        const uint4* p = reinterpret_cast<const uint4*>(a.d1 + (size_t)ic * DIM + h * 16u);
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            const uint4 v = p[2 * ks];
            breg[ks] = v4i{(int)(v.x ^ kSignFlip), (int)(v.y ^ kSignFlip), (int)(v.z ^ kSignFlip),
                           (int)(v.w ^ kSignFlip)};
        }
    }
    const uint32_t jbeg = sp * a.cols;
    const uint32_t jend = jbeg + a.cols < a.n2 ? jbeg + a.cols : a.n2;

    // the lane's KC best of e = |b|^2 - 2 a.b, ascending (the row's |a|^2 is added at the end)
    int be[KC];
    uint32_t bj[KC];
#pragma unroll
    for (int p = 0; p < KC; ++p) {
        be[p] = INT_MAX;
        bj[p] = kMatchNone;
    }

    for (uint32_t j0 = jbeg; j0 < jend; j0 += kMatchStepCols) {
        __syncthreads();                                  // the previous step's operand reads are done
        for (uint32_t c = tid; c < kMatchStepCols * CHUNKS; c += kKnnThreads) {
            const uint32_t col = c / CHUNKS, off = (c % CHUNKS) * 16u;
            const uint32_t j = j0 + col < a.n2 ? j0 + col : a.n2 - 1;
            uint4 v = *reinterpret_cast<const uint4*>(a.d2 + (size_t)j * DIM + off);
            v.x ^= kSignFlip;
            v.y ^= kSignFlip;
            v.z ^= kSignFlip;
            v.w ^= kSignFlip;
            *reinterpret_cast<uint4*>(&s_d2[col * STRIDE + off]) = v;
        }
        if (tid < kMatchStepCols) {
            const uint32_t j = j0 + tid < a.n2 ? j0 + tid : a.n2 - 1;
            s_nb[tid] = (int)a.norm2[j];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < kMatchStepCols / 32u; ++q) {
            const uint32_t jt = j0 + q * 32u;             // wave-uniform
            if (jt >= jend) break;
            v16i acc = {};
            const uint8_t* arow = &s_d2[(q * 32u + r) * STRIDE + h * 16u];
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                const v4i av = *reinterpret_cast<const v4i*>(arow + ks * 32);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, breg[ks], acc, 0, 0, 0);
            }
            int e[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i nb = *reinterpret_cast<const v4i*>(&s_nb[q * 32u + 8u * g + 4u * h]);
#pragma unroll
                for (int k = 0; k < 4; ++k) e[4 * g + k] = nb[k] - 2 * acc[4 * g + k];
            }
            const uint32_t jl = jt + 4u * h;              // the lane's first column of the tile
            if (jt + 32u > jend) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if (jl + (reg & 3) + 8 * (reg >> 2) >= jend) e[reg] = INT_MAX;
            }
            int m = e[0];
#pragma unroll
            for (int reg = 1; reg < 16; ++reg) m = e[reg] < m ? e[reg] : m;
            if (__any(m < be[KC - 1])) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int ev = e[reg];
                    const uint32_t jj = jl + (reg & 3) + 8 * (reg >> 2);
                    if (!__any(ev < be[KC - 1])) continue;     // wave-uniform: no lane takes this column
                    // lt[p]: the candidate goes before position p (a masked INT_MAX never does)
                    bool lt[KC];
#pragma unroll
                    for (int p = 0; p < KC; ++p) lt[p] = ev < be[p];
#pragma unroll
                    for (int p = KC - 1; p >= 1; --p) {
                        be[p] = lt[p - 1] ? be[p - 1] : (lt[p] ? ev : be[p]);
                        bj[p] = lt[p - 1] ? bj[p - 1] : (lt[p] ? jj : bj[p]);
                    }
                    be[0] = lt[0] ? ev : be[0];
                    bj[0] = lt[0] ? jj : bj[0];
                }
            }
        }
    }

    // the two lane halves hold disjoint columns of the same row
    const int na = (int)a.norm1[ic];
    uint64_t mine[KC], other[KC];
#pragma unroll
    for (int p = 0; p < KC; ++p) {
        const uint32_t d = be[p] == INT_MAX ? kMatchNone : (uint32_t)(be[p] + na);
        mine[p] = match_key(d, bj[p]);
        other[p] = match_key((uint32_t)__shfl_xor((int)d, 32), (uint32_t)__shfl_xor((int)bj[p], 32));
    }
    knn_merge<KC>(mine, other);
    if (h == 0 && i < a.n1) {
        const size_t o = ((size_t)sp * a.n1 + i) * a.k;
#pragma unroll
        for (int p = 0; p < KC; ++p) {
            if ((uint32_t)p < a.k) {
                a.p_idx[o + p] = (uint32_t)mine[p];
                a.p_dist[o + p] = (uint32_t)(mine[p] >> 32);
            }
        }
    }
}

template <int KC>
__global__ __launch_bounds__(kKnnThreads) void k_knn_merge(KnnArgs a) {
    const uint32_t i = blockIdx.x * kKnnThreads + threadIdx.x;
    if (i >= a.n1) return;
    uint64_t best[KC];
#pragma unroll
    for (int p = 0; p < KC; ++p) best[p] = kKnnPad;
    for (uint32_t s = 0; s < a.splits; ++s) {
        const size_t o = ((size_t)s * a.n1 + i) * a.k;
        uint64_t part[KC];
#pragma unroll
        for (int p = 0; p < KC; ++p)
            part[p] = (uint32_t)p < a.k ? match_key(a.p_dist[o + p], a.p_idx[o + p]) : kKnnPad;
        knn_merge<KC>(best, part);
    }
    const size_t o = (size_t)i * a.k;
#pragma unroll
    for (int p = 0; p < KC; ++p) {
        if ((uint32_t)p < a.k) {
            a.idx[o + p] = (uint32_t)best[p];
            a.dist[o + p] = (uint32_t)(best[p] >> 32);
        }
    }
}

template <int NK, int KC>
void launch_k_knn(const KnnArgs& a, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL((k_knn<NK, KC>), dim3(blocks), dim3(kKnnThreads), 0, stream, a);
}

using LaunchFn = void (*)(const KnnArgs&, uint32_t, hipStream_t);
#define GCR_KNN_ROW(KC)                                                                                     \
    {launch_k_knn<1, KC>,  launch_k_knn<2, KC>,  launch_k_knn<3, KC>,  launch_k_knn<4, KC>,                 \
     launch_k_knn<5, KC>,  launch_k_knn<6, KC>,  launch_k_knn<7, KC>,  launch_k_knn<8, KC>,                 \
     launch_k_knn<9, KC>,  launch_k_knn<10, KC>, launch_k_knn<11, KC>, launch_k_knn<12, KC>,                \
     launch_k_knn<13, KC>, launch_k_knn<14, KC>, launch_k_knn<15, KC>, launch_k_knn<16, KC>}
constexpr LaunchFn kLaunch[2][16] = {GCR_KNN_ROW((int)kKnnCapSmall), GCR_KNN_ROW((int)kKnnCapLarge)};
#undef GCR_KNN_ROW

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

void knn_enqueue(hipStream_t stream, const KnnDev& m) {
    KnnArgs a{};
    a.d1 = m.d1;
    a.d2 = m.d2;
    a.norm1 = m.norm1;
    a.norm2 = m.norm2;
    a.n1 = (uint32_t)m.n1;
    a.n2 = (uint32_t)m.n2;
    a.splits = m.splits;
    a.cols = m.cols;
    a.k = m.k;
    a.idx = m.out[0];
    a.dist = m.out[1];
    const bool split = m.splits > 1;
    a.p_idx = split ? m.part[0] : a.idx;
    a.p_dist = split ? m.part[1] : a.dist;
    const bool large = knn_capacity(m.k) == kKnnCapLarge;
    const size_t row_blocks = (m.n1 + kMatchRowsPerWg - 1) / kMatchRowsPerWg;
    kLaunch[large ? 1 : 0][m.dim / 32 - 1](a, (uint32_t)(row_blocks * m.splits), stream);
    if (!split) return;
    const dim3 grid((uint32_t)((m.n1 + kKnnThreads - 1) / kKnnThreads));
    if (large) hipLaunchKernelGGL(k_knn_merge<(int)kKnnCapLarge>, grid, dim3(kKnnThreads), 0, stream, a);
    else hipLaunchKernelGGL(k_knn_merge<(int)kKnnCapSmall>, grid, dim3(kKnnThreads), 0, stream, a);
}

// The array entry: allocate, upload, norms, the device search, download, free.
hipError_t knn_device(hipStream_t stream, int n_cu, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2,
                      uint32_t dim, uint32_t k, uint32_t* idx, uint32_t* dist, double* ms_kernel) {
    KnnDev m{};
    m.n1 = n1;
    m.n2 = n2;
    m.dim = dim;
    m.k = k;
    m.splits = match_plan_env(n1, n2, n_cu, &m.cols);
    const size_t b_d1 = up256(n1 * dim), b_d2 = up256(n2 * dim), b_n1 = up256(n1 * 4), b_n2 = up256(n2 * 4);
    const size_t b_out = up256(n1 * k * 4), b_part = m.splits > 1 ? up256((size_t)m.splits * n1 * k * 4) : 0;
    char* base = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), b_d1 + b_d2 + b_n1 + b_n2 + 2 * b_out + 2 * b_part);
    if (e != hipSuccess) return e;
    char* p = base;
    uint8_t* dd1 = reinterpret_cast<uint8_t*>(p);
    p += b_d1;
    uint8_t* dd2 = reinterpret_cast<uint8_t*>(p);
    p += b_d2;
    uint32_t* norm1 = reinterpret_cast<uint32_t*>(p);
    p += b_n1;
    uint32_t* norm2 = reinterpret_cast<uint32_t*>(p);
    p += b_n2;
    for (int q = 0; q < 2; ++q) m.out[q] = reinterpret_cast<uint32_t*>(p), p += b_out;
    for (int q = 0; q < 2; ++q) m.part[q] = reinterpret_cast<uint32_t*>(p), p += b_part;
    m.d1 = dd1;
    m.d2 = dd2;
    m.norm1 = norm1;
    m.norm2 = norm2;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipMemcpyAsync(dd1, d1, n1 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dd2, d2, n2 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(ev0, stream);
    if (e == hipSuccess) {
        match_norms_enqueue(stream, dd1, n1, dd2, n2, dim, norm1, norm2);
        knn_enqueue(stream, m);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev1, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(idx, m.out[0], n1 * k * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dist, m.out[1], n1 * k * 4, hipMemcpyDeviceToHost, stream);
    const hipError_t s = hipStreamSynchronize(stream);    // also after an error: nothing in flight reads `base`
    if (e == hipSuccess) e = s;
    if (e == hipSuccess && ms_kernel) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, ev0, ev1);
        *ms_kernel = (double)ms;
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipFree(base);
    return e;
}

hipError_t knn_sets_run(hipStream_t stream, int n_cu, MatchWorkspace& ws, const gcr_descriptors* a,
                        const gcr_descriptors* b, uint32_t k, uint32_t* idx, uint32_t* dist, double* ms_kernel) {
    std::lock_guard<std::mutex> lk(ws.mu);
    KnnDev m{};
    m.d1 = a->d;
    m.norm1 = a->norm;
    m.n1 = a->n;
    m.d2 = b->d;
    m.norm2 = b->norm;
    m.n2 = b->n;
    m.dim = a->dim;
    m.k = k;
    m.splits = match_plan_env(m.n1, m.n2, n_cu, &m.cols);
    // the workspace: the partials, then idx | dist, which one copy brings down
    const size_t b_out = up256(m.n1 * k * 4), b_part = m.splits > 1 ? up256((size_t)m.splits * m.n1 * k * 4) : 0;
    hipError_t e = match_workspace_grow(stream, ws, 2 * b_part + 2 * b_out, 2 * b_out, false);
    if (e != hipSuccess) return e;
    if (ms_kernel)
        for (int q = 0; q < 2; ++q)
            if (!ws.ev[q] && (e = hipEventCreate(&ws.ev[q])) != hipSuccess) return e;
    char* p = ws.dev;
    for (int q = 0; q < 2; ++q) m.part[q] = reinterpret_cast<uint32_t*>(p), p += b_part;
    char* out_base = p;
    for (int q = 0; q < 2; ++q) m.out[q] = reinterpret_cast<uint32_t*>(p), p += b_out;
    if (ms_kernel) e = hipEventRecord(ws.ev[0], stream);
    if (e == hipSuccess) {
        knn_enqueue(stream, m);
        e = hipGetLastError();
    }
    if (ms_kernel && e == hipSuccess) e = hipEventRecord(ws.ev[1], stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ws.pinned, out_base, 2 * b_out, hipMemcpyDeviceToHost, stream);
    const hipError_t s = hipStreamSynchronize(stream);    // the one synchronisation; also after an error
    if (e == hipSuccess) e = s;
    if (e != hipSuccess) return e;
    std::memcpy(idx, ws.pinned, m.n1 * k * 4);
    std::memcpy(dist, ws.pinned + b_out, m.n1 * k * 4);
    if (ms_kernel) {
        float t = 0.f;
        e = hipEventElapsedTime(&t, ws.ev[0], ws.ev[1]);
        *ms_kernel = (double)t;
    }
    return e;
}

}  // namespace gcr
