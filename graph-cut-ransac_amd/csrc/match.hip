// match.hip -- exact 2-nearest-neighbour descriptor matching on the int8
// matrix cores (match.h is the definition; gcr_match_descriptors the entry).
//
// d(i, j) = |a|^2 + |b|^2 - 2 a.b with a = D1[i] - 128, b = D2[j] - 128 as int8
// (the distance is translation invariant; x - 128 is x ^ 0x80 reinterpreted).
// Every intermediate fits int32, so the result is exact.
//
// Three launches:
//   k_match_norms  |a|^2 and |b|^2, one thread per row.
//   k_match<NK>    grid = row blocks x column splits (NK = dim / 32).  A
//                  workgroup is four waves; each wave owns 32 rows of D1, kept
//                  in registers as the B operand for the whole kernel.  Per
//                  step the workgroup stages kMatchStepCols rows of D2 into
//                  the LDS (row stride dim + 16 bytes: the 16-byte operand
//                  reads of 32 rows then fall on distinct banks) and every
//                  wave runs v_mfma_i32_32x32x32_i8 over dim with the D2 tile
//                  as the A operand.  The 32 x 32 result tile therefore has
//                  the D1 row i on the lane (C/D map: column = lane & 31) and
//                  16 D2 rows j = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in
//                  its registers: a lane's running top-2 is four registers.
//                  The k order inside an operand does not matter (a sum), only
//                  that both operands pair the same k: both read the same 16
//                  bytes of their row.
//                  A lane meets its j in ascending order, so `d < best` keeps
//                  the lower index on a tie.  A tile whose 16 values all lose
//                  against every lane's second best is skipped after 16
//                  minima.  Columns past the split's end are masked by INDEX
//                  (a padded column's distance can beat real ones).  The two
//                  lane halves are merged once at the end, lexicographically.
//   k_match_merge  the splits' partial top-2 of a row merged (match_merge:
//                  order-independent).  Not launched for one split: k_match
//                  then writes the result itself.
// Device memory beyond the descriptors: norms, results and the partials,
// O(n1 * splits + n2).  The n1 x n2 matrix never exists.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>

#include "match.h"

namespace gcr {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kMatchThreads = 256;
constexpr uint32_t kSignFlip = 0x80808080u;

struct MatchArgs {
    const uint8_t* d1;
    const uint8_t* d2;
    const uint32_t* norm1;      // |D1[i] - 128|^2
    const uint32_t* norm2;
    uint32_t n1, n2;
    uint32_t splits, cols;      // column splits, columns per split (multiple of kMatchStepCols)
    // [splits][n1] partials; the results themselves for splits == 1
    uint32_t *p_idx, *p_dist, *p_idx2, *p_dist2;
    uint32_t *idx, *dist, *idx2, *dist2;
};

__device__ __forceinline__ uint32_t sq_bytes(uint32_t w) {
    uint32_t s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int v = (int)((w >> (8 * b)) & 0xffu) - 128;
        s += (uint32_t)(v * v);
    }
    return s;
}

__global__ __launch_bounds__(kMatchThreads) void k_match_norms(const uint8_t* d1, uint32_t n1, const uint8_t* d2,
                                                               uint32_t n2, uint32_t dim, uint32_t* norm1,
                                                               uint32_t* norm2) {
    const uint32_t t = blockIdx.x * kMatchThreads + threadIdx.x;
    if (t >= n1 + n2) return;
    const uint8_t* row = t < n1 ? d1 + (size_t)t * dim : d2 + (size_t)(t - n1) * dim;
    const uint4* p = reinterpret_cast<const uint4*>(row);
    uint32_t s = 0;
    for (uint32_t k = 0; k < dim / 16; ++k) {
        const uint4 v = p[k];
        s += sq_bytes(v.x) + sq_bytes(v.y) + sq_bytes(v.z) + sq_bytes(v.w);
    }
    if (t < n1) norm1[t] = s;
    else norm2[t - n1] = s;
}

template <int NK>
__global__ __launch_bounds__(kMatchThreads) void k_match(MatchArgs a) {
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

    // running top-2 of e = |b|^2 - 2 a.b (the row's |a|^2 is added at the end)
    int e1 = INT_MAX, e2 = INT_MAX;
    uint32_t j1 = kMatchNone, j2 = kMatchNone;

    for (uint32_t j0 = jbeg; j0 < jend; j0 += kMatchStepCols) {
        __syncthreads();                                  // the previous step's operand reads are done
        for (uint32_t c = tid; c < kMatchStepCols * CHUNKS; c += kMatchThreads) {
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
            if (__any(m < e2)) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int ev = e[reg];
                    const uint32_t jj = jl + (reg & 3) + 8 * (reg >> 2);
                    if (ev < e1) {
                        e2 = e1;
                        j2 = j1;
                        e1 = ev;
                        j1 = jj;
                    } else if (ev < e2) {
                        e2 = ev;
                        j2 = jj;
                    }
                }
            }
        }
    }

    // the two lane halves hold disjoint columns of the same row
    const int na = (int)a.norm1[ic];
    const uint32_t da = e1 == INT_MAX ? kMatchNone : (uint32_t)(e1 + na);
    const uint32_t db = e2 == INT_MAX ? kMatchNone : (uint32_t)(e2 + na);
    uint64_t k1 = match_key(da, j1), k2 = match_key(db, j2);
    const uint64_t o1 = match_key((uint32_t)__shfl_xor((int)da, 32), (uint32_t)__shfl_xor((int)j1, 32));
    const uint64_t o2 = match_key((uint32_t)__shfl_xor((int)db, 32), (uint32_t)__shfl_xor((int)j2, 32));
    match_merge(k1, k2, o1, o2);
    if (h == 0 && i < a.n1) {
        const size_t o = (size_t)sp * a.n1 + i;
        a.p_idx[o] = (uint32_t)k1;
        a.p_dist[o] = (uint32_t)(k1 >> 32);
        a.p_idx2[o] = (uint32_t)k2;
        a.p_dist2[o] = (uint32_t)(k2 >> 32);
    }
}

__global__ __launch_bounds__(kMatchThreads) void k_match_merge(MatchArgs a) {
    const uint32_t i = blockIdx.x * kMatchThreads + threadIdx.x;
    if (i >= a.n1) return;
    uint64_t k1 = ~0ull, k2 = ~0ull;
    for (uint32_t s = 0; s < a.splits; ++s) {
        const size_t o = (size_t)s * a.n1 + i;
        match_merge(k1, k2, match_key(a.p_dist[o], a.p_idx[o]), match_key(a.p_dist2[o], a.p_idx2[o]));
    }
    a.idx[i] = (uint32_t)k1;
    a.dist[i] = (uint32_t)(k1 >> 32);
    a.idx2[i] = (uint32_t)k2;
    a.dist2[i] = (uint32_t)(k2 >> 32);
}

template <int NK>
void launch_k_match(const MatchArgs& a, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(k_match<NK>, dim3(blocks), dim3(kMatchThreads), 0, stream, a);
}

using LaunchFn = void (*)(const MatchArgs&, uint32_t, hipStream_t);
constexpr LaunchFn kLaunch[16] = {
    launch_k_match<1>,  launch_k_match<2>,  launch_k_match<3>,  launch_k_match<4>,
    launch_k_match<5>,  launch_k_match<6>,  launch_k_match<7>,  launch_k_match<8>,
    launch_k_match<9>,  launch_k_match<10>, launch_k_match<11>, launch_k_match<12>,
    launch_k_match<13>, launch_k_match<14>, launch_k_match<15>, launch_k_match<16>,
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

hipError_t match_device(hipStream_t stream, int n_cu, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2,
                        uint32_t dim, uint32_t* idx, uint32_t* dist, uint32_t* idx2, uint32_t* dist2,
                        double* ms_kernel) {
    // GCR_MATCH_SPLIT=k (1 .. 1024): pins the number of column splits (tests); read per call
    int pin = 0;
    if (const char* e = getenv("GCR_MATCH_SPLIT")) {
        const int v = atoi(e);
        if (v >= 1) pin = v < 1024 ? v : 1024;
    }
    uint32_t cols = 0;
    const uint32_t splits = match_plan(n1, n2, n_cu, pin, &cols);
    const size_t row_blocks = (n1 + kMatchRowsPerWg - 1) / kMatchRowsPerWg;

    const size_t b_d1 = up256(n1 * dim), b_d2 = up256(n2 * dim);
    const size_t b_n1 = up256(n1 * 4), b_n2 = up256(n2 * 4);
    const size_t b_out = up256(n1 * 4), b_part = splits > 1 ? up256((size_t)splits * n1 * 4) : 0;
    char* base = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), b_d1 + b_d2 + b_n1 + b_n2 + 4 * b_out + 4 * b_part);
    if (e != hipSuccess) return e;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    MatchArgs a{};
    char* p = base;
    a.d1 = reinterpret_cast<uint8_t*>(p), p += b_d1;
    a.d2 = reinterpret_cast<uint8_t*>(p), p += b_d2;
    uint32_t* norm1 = reinterpret_cast<uint32_t*>(p);
    p += b_n1;
    uint32_t* norm2 = reinterpret_cast<uint32_t*>(p);
    p += b_n2;
    a.norm1 = norm1;
    a.norm2 = norm2;
    a.idx = reinterpret_cast<uint32_t*>(p), p += b_out;
    a.dist = reinterpret_cast<uint32_t*>(p), p += b_out;
    a.idx2 = reinterpret_cast<uint32_t*>(p), p += b_out;
    a.dist2 = reinterpret_cast<uint32_t*>(p), p += b_out;
    if (splits > 1) {
        a.p_idx = reinterpret_cast<uint32_t*>(p), p += b_part;
        a.p_dist = reinterpret_cast<uint32_t*>(p), p += b_part;
        a.p_idx2 = reinterpret_cast<uint32_t*>(p), p += b_part;
        a.p_dist2 = reinterpret_cast<uint32_t*>(p), p += b_part;
    } else {
        a.p_idx = a.idx;
        a.p_dist = a.dist;
        a.p_idx2 = a.idx2;
        a.p_dist2 = a.dist2;
    }
    a.n1 = (uint32_t)n1;
    a.n2 = (uint32_t)n2;
    a.splits = splits;
    a.cols = cols;

    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipMemcpyAsync(const_cast<uint8_t*>(a.d1), d1, n1 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(const_cast<uint8_t*>(a.d2), d2, n2 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(ev0, stream);
    if (e == hipSuccess) {
        const uint32_t nb = (uint32_t)((n1 + n2 + kMatchThreads - 1) / kMatchThreads);
        hipLaunchKernelGGL(k_match_norms, dim3(nb), dim3(kMatchThreads), 0, stream, a.d1, a.n1, a.d2, a.n2, dim,
                           norm1, norm2);
        kLaunch[dim / 32 - 1](a, (uint32_t)(row_blocks * splits), stream);
        if (splits > 1)
            hipLaunchKernelGGL(k_match_merge, dim3((uint32_t)((n1 + kMatchThreads - 1) / kMatchThreads)),
                               dim3(kMatchThreads), 0, stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev1, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(idx, a.idx, n1 * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dist, a.dist, n1 * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(idx2, a.idx2, n1 * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dist2, a.dist2, n1 * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess && ms_kernel) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, ev0, ev1);
        *ms_kernel = (double)ms;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(stream);    // nothing in flight reads `base` past the free
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipFree(base);
    return e;
}

}  // namespace gcr
