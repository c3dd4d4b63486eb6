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
// The plan, the launches and the merge work on device pointers
// (match_plan_env, match_norms_enqueue, match_enqueue): the array entry is
// "allocate, upload, those, download, free", and the resident descriptor sets
// (match_sets.hip) call the same functions on their own buffers.
//
// Guided matching (match_geo.h is the definition; gcr_match_descriptors_guided
// the entry) adds two kernels and reuses k_match_norms and k_match_merge:
//   k_match_geo_terms  the factorised residual's per-point terms, four doubles
//                      per keypoint of either image, one thread per keypoint.
//   k_match_geo<NK>    k_match's tiling.  The kernel's ROWS are the result
//                      rows (image 1 forward, image 2 in reverse), its columns
//                      the other image.  A lane keeps its row's terms in
//                      registers; a step first stages its 64 columns' terms in
//                      the LDS and every lane evaluates the admissibility of
//                      its 2 x 16 pairs into two 16-bit masks.  Padded columns
//                      and padded rows are cleared from the masks by INDEX
//                      (their clamped positions are real keypoints').  A step
//                      in which no wave of the workgroup has an admissible pair
//                      stages no descriptors at all; a tile in which the wave
//                      has none runs no MFMA.  An inadmissible pair's e is
//                      INT_MAX before the minimum / __any / update sequence,
//                      which is k_match's.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>

#include "match.h"
#include "match_geo.h"

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

// ------------------------------------------------------------ guided matching --
struct MatchGeoArgs {
    MatchArgs m;                // d1 / norm1 / n1: the image of the result rows; d2 / norm2 / n2: the columns'
    const double* row_terms;    // [m.n1][kMatchGeoTerms]
    const double* col_terms;    // [m.n2][kMatchGeoTerms]
    double T;
    int kind, reverse;          // reverse: the rows are image 2
};

struct MatchGeoModel {
    double h[9];
};

// t1: the terms of image 1's keypoints, t2: of image 2's (whatever the direction)
__global__ __launch_bounds__(kMatchThreads) void k_match_geo_terms(const double* p1, uint32_t n1, const double* p2,
                                                                   uint32_t n2, MatchGeoModel mdl, int kind,
                                                                   double* t1, double* t2) {
    const uint32_t t = blockIdx.x * kMatchThreads + threadIdx.x;
    if (t >= n1 + n2) return;
    const bool first = t < n1;
    const uint32_t k = first ? t : t - n1;
    const double* p = (first ? p1 : p2) + 2 * (size_t)k;
    const double x = p[0], y = p[1];
    double v[kMatchGeoTerms];
    if (kind == kMatchGeoFundamental) {
        if (first) match_geo_terms1<kMatchGeoFundamental>(x, y, mdl.h, v);
        else match_geo_terms2<kMatchGeoFundamental>(x, y, mdl.h, v);
    } else {
        if (first) match_geo_terms1<kMatchGeoHomography>(x, y, mdl.h, v);
        else match_geo_terms2<kMatchGeoHomography>(x, y, mdl.h, v);
    }
    double* o = (first ? t1 : t2) + kMatchGeoTerms * (size_t)k;
#pragma unroll
    for (int q = 0; q < kMatchGeoTerms; ++q) o[q] = v[q];
}

// Bit reg of the result: the pair of the lane's row (terms rt) and the column
// (reg & 3) + 8 (reg >> 2) past ct's is admissible.  REV: the row is image 2's.
template <int KIND, bool REV>
__device__ __forceinline__ uint32_t geo_tile_mask(const double (&rt)[kMatchGeoTerms], const double* ct, double T) {
    uint32_t m = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const double* c = ct + ((reg & 3) + 8 * (reg >> 2)) * kMatchGeoTerms;
        double cv[kMatchGeoTerms] = {c[0], c[1], 0.0, 0.0};
        if constexpr (KIND == kMatchGeoFundamental) {
            cv[2] = c[2];
            cv[3] = c[3];
        }
        const bool adm = REV ? match_geo_adm<KIND>(cv, rt, T) : match_geo_adm<KIND>(rt, cv, T);
        m |= adm ? 1u << reg : 0u;
    }
    return m;
}

template <int NK>
__global__ __launch_bounds__(kMatchThreads) void k_match_geo(MatchGeoArgs g) {
    constexpr uint32_t DIM = NK * 32;
    constexpr uint32_t STRIDE = DIM + 16;                 // as k_match
    constexpr uint32_t CHUNKS = DIM / 16;
    static_assert(kMatchStepCols * kMatchGeoTerms == kMatchThreads, "one term per thread and step");
    __shared__ __attribute__((aligned(16))) uint8_t s_d2[kMatchStepCols * STRIDE];
    __shared__ __attribute__((aligned(16))) int s_nb[kMatchStepCols];
    // the steps alternate between two copies of the terms and of the flag: a
    // step's writes never meet the previous step's reads
    __shared__ __attribute__((aligned(16))) double s_ct[2][kMatchStepCols * kMatchGeoTerms];
    __shared__ int s_need[2];

    const MatchArgs& a = g.m;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t rb = blockIdx.x / a.splits, sp = blockIdx.x % a.splits;
    const uint32_t i = rb * kMatchRowsPerWg + wave * 32u + r;
    const bool row_ok = i < a.n1;
    const uint32_t ic = row_ok ? i : a.n1 - 1;            // rows past the end read the last row, never written

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
    double rt[kMatchGeoTerms];
#pragma unroll
    for (int q = 0; q < kMatchGeoTerms; ++q) rt[q] = g.row_terms[(size_t)ic * kMatchGeoTerms + q];
    const double T = g.T;
    const int mode = (g.kind == kMatchGeoFundamental ? 2 : 0) + (g.reverse ? 1 : 0);    // workgroup-uniform

    const uint32_t jbeg = sp * a.cols;
    const uint32_t jend = jbeg + a.cols < a.n2 ? jbeg + a.cols : a.n2;

    int e1 = INT_MAX, e2 = INT_MAX;
    uint32_t j1 = kMatchNone, j2 = kMatchNone;

    uint32_t par = 0;
    for (uint32_t j0 = jbeg; j0 < jend; j0 += kMatchStepCols, par ^= 1u) {
        double* ct = s_ct[par];
        {
            const uint32_t col = tid / kMatchGeoTerms;
            const uint32_t j = j0 + col < a.n2 ? j0 + col : a.n2 - 1;
            ct[tid] = g.col_terms[(size_t)j * kMatchGeoTerms + tid % kMatchGeoTerms];
        }
        if (tid == 0) s_need[par] = 0;
        __syncthreads();
        // admissibility of the lane's 16 columns of either tile
        uint32_t adm[kMatchStepCols / 32u];
#pragma unroll
        for (uint32_t q = 0; q < kMatchStepCols / 32u; ++q) {
            const uint32_t jt = j0 + q * 32u;             // wave-uniform
            adm[q] = 0;
            if (jt >= jend) continue;
            const double* c0 = ct + (q * 32u + 4u * h) * kMatchGeoTerms;
            uint32_t m;
            switch (mode) {
                case 0: m = geo_tile_mask<kMatchGeoHomography, false>(rt, c0, T); break;
                case 1: m = geo_tile_mask<kMatchGeoHomography, true>(rt, c0, T); break;
                case 2: m = geo_tile_mask<kMatchGeoFundamental, false>(rt, c0, T); break;
                default: m = geo_tile_mask<kMatchGeoFundamental, true>(rt, c0, T); break;
            }
            // padded columns and padded rows leave by index: their terms are a real keypoint's
            if (jt + 32u > jend) {
                const uint32_t jl = jt + 4u * h;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if (jl + (reg & 3) + 8 * (reg >> 2) >= jend) m &= ~(1u << reg);
            }
            adm[q] = row_ok ? m : 0u;
        }
        bool wany[kMatchStepCols / 32u];
        bool any = false;
#pragma unroll
        for (uint32_t q = 0; q < kMatchStepCols / 32u; ++q) {
            wany[q] = __any(adm[q] != 0u);                // wave-uniform
            any |= wany[q];
        }
        if (any && lane == 0) s_need[par] = 1;
        __syncthreads();
        if (!s_need[par]) continue;                       // no admissible pair in the whole step: nothing staged

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
            if (!wany[q]) continue;                       // the wave has no admissible pair in the tile: no MFMA
            const uint32_t jt = j0 + q * 32u;
            v16i acc = {};
            const uint8_t* arow = &s_d2[(q * 32u + r) * STRIDE + h * 16u];
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                const v4i av = *reinterpret_cast<const v4i*>(arow + ks * 32);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, breg[ks], acc, 0, 0, 0);
            }
            int e[16];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const v4i nb = *reinterpret_cast<const v4i*>(&s_nb[q * 32u + 8u * gq + 4u * h]);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    e[4 * gq + k] = (adm[q] >> (4 * gq + k)) & 1u ? nb[k] - 2 * acc[4 * gq + k] : INT_MAX;
            }
            const uint32_t jl = jt + 4u * h;              // the lane's first column of the tile
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
    if (h == 0 && row_ok) {
        const size_t o = (size_t)sp * a.n1 + i;
        a.p_idx[o] = (uint32_t)k1;
        a.p_dist[o] = (uint32_t)(k1 >> 32);
        a.p_idx2[o] = (uint32_t)k2;
        a.p_dist2[o] = (uint32_t)(k2 >> 32);
    }
}

template <int NK>
void launch_k_match_geo(const MatchGeoArgs& g, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(k_match_geo<NK>, dim3(blocks), dim3(kMatchThreads), 0, stream, g);
}

using LaunchGeoFn = void (*)(const MatchGeoArgs&, uint32_t, hipStream_t);
constexpr LaunchGeoFn kLaunchGeo[16] = {
    launch_k_match_geo<1>,  launch_k_match_geo<2>,  launch_k_match_geo<3>,  launch_k_match_geo<4>,
    launch_k_match_geo<5>,  launch_k_match_geo<6>,  launch_k_match_geo<7>,  launch_k_match_geo<8>,
    launch_k_match_geo<9>,  launch_k_match_geo<10>, launch_k_match_geo<11>, launch_k_match_geo<12>,
    launch_k_match_geo<13>, launch_k_match_geo<14>, launch_k_match_geo<15>, launch_k_match_geo<16>,
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

MatchArgs match_args(const MatchDev& m) {
    MatchArgs a{};
    a.d1 = m.d1;
    a.d2 = m.d2;
    a.norm1 = m.norm1;
    a.norm2 = m.norm2;
    a.n1 = (uint32_t)m.n1;
    a.n2 = (uint32_t)m.n2;
    a.splits = m.splits;
    a.cols = m.cols;
    a.idx = m.out[0];
    a.dist = m.out[1];
    a.idx2 = m.out[2];
    a.dist2 = m.out[3];
    const bool split = m.splits > 1;
    a.p_idx = split ? m.part[0] : a.idx;
    a.p_dist = split ? m.part[1] : a.dist;
    a.p_idx2 = split ? m.part[2] : a.idx2;
    a.p_dist2 = split ? m.part[3] : a.dist2;
    return a;
}

// the array entries' one allocation: descriptors, norms, results and partials of one search
struct MatchArrayBufs {
    char* base = nullptr;
    uint8_t *d1 = nullptr, *d2 = nullptr;
    uint32_t *norm1 = nullptr, *norm2 = nullptr;
    double* dbl[4] = {};        // guided: positions of image 1 and 2, terms of image 1 and 2
};

// `lead` doubles-first bytes (lead_b[4], 0 for the plain matcher), then MatchDev's buffers
hipError_t match_array_alloc(MatchDev& m, const size_t lead_b[4], MatchArrayBufs& b) {
    const size_t b_d1 = up256(m.n1 * m.dim), b_d2 = up256(m.n2 * m.dim);
    const size_t b_n1 = up256(m.n1 * 4), b_n2 = up256(m.n2 * 4);
    const size_t b_out = up256(m.n1 * 4), b_part = m.splits > 1 ? up256((size_t)m.splits * m.n1 * 4) : 0;
    size_t lead = 0;
    for (int k = 0; k < 4; ++k) lead += lead_b[k];
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&b.base),
                                   lead + b_d1 + b_d2 + b_n1 + b_n2 + 4 * b_out + 4 * b_part);
    if (e != hipSuccess) return e;
    char* p = b.base;                                     // the doubles first: 256-byte aligned either way
    for (int k = 0; k < 4; ++k) {
        b.dbl[k] = reinterpret_cast<double*>(p);
        p += lead_b[k];
    }
    b.d1 = reinterpret_cast<uint8_t*>(p), p += b_d1;
    b.d2 = reinterpret_cast<uint8_t*>(p), p += b_d2;
    b.norm1 = reinterpret_cast<uint32_t*>(p), p += b_n1;
    b.norm2 = reinterpret_cast<uint32_t*>(p), p += b_n2;
    for (int k = 0; k < 4; ++k) m.out[k] = reinterpret_cast<uint32_t*>(p), p += b_out;
    for (int k = 0; k < 4; ++k) m.part[k] = reinterpret_cast<uint32_t*>(p), p += b_part;
    m.d1 = b.d1;
    m.d2 = b.d2;
    m.norm1 = b.norm1;
    m.norm2 = b.norm2;
    return hipSuccess;
}

// the four results to the host, the synchronisation, the event time, the free
hipError_t match_array_finish(hipError_t e, hipStream_t stream, const MatchDev& m, MatchArrayBufs& b, hipEvent_t ev0,
                              hipEvent_t ev1, uint32_t* const host_out[4], double* ms_kernel) {
    if (e == hipSuccess) e = hipEventRecord(ev1, stream);
    for (int k = 0; k < 4; ++k)
        if (e == hipSuccess) e = hipMemcpyAsync(host_out[k], m.out[k], m.n1 * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess && ms_kernel) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, ev0, ev1);
        *ms_kernel = (double)ms;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(stream);    // nothing in flight reads `base` past the free
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipFree(b.base);
    return e;
}

}  // namespace

uint32_t match_plan_env(size_t n1, size_t n2, int n_cu, uint32_t* cols_out) {
    // GCR_MATCH_SPLIT=k (1 .. 1024): pins the number of column splits (tests); read per call
    int pin = 0;
    if (const char* e = getenv("GCR_MATCH_SPLIT")) {
        const int v = atoi(e);
        if (v >= 1) pin = v < 1024 ? v : 1024;
    }
    return match_plan(n1, n2, n_cu, pin, cols_out);
}

void match_norms_enqueue(hipStream_t stream, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2, uint32_t dim,
                         uint32_t* norm1, uint32_t* norm2) {
    const uint32_t nb = (uint32_t)((n1 + n2 + kMatchThreads - 1) / kMatchThreads);
    hipLaunchKernelGGL(k_match_norms, dim3(nb), dim3(kMatchThreads), 0, stream, d1, (uint32_t)n1, d2, (uint32_t)n2,
                       dim, norm1, norm2);
}

void match_enqueue(hipStream_t stream, const MatchDev& m) {
    const MatchArgs a = match_args(m);
    const size_t row_blocks = (m.n1 + kMatchRowsPerWg - 1) / kMatchRowsPerWg;
    kLaunch[m.dim / 32 - 1](a, (uint32_t)(row_blocks * m.splits), stream);
    if (m.splits > 1)
        hipLaunchKernelGGL(k_match_merge, dim3((uint32_t)((m.n1 + kMatchThreads - 1) / kMatchThreads)),
                           dim3(kMatchThreads), 0, stream, a);
}

void match_geo_terms_enqueue(hipStream_t stream, const double* p1, size_t n1, const double* p2, size_t n2,
                             const double* model, int kind, double* t1, double* t2) {
    MatchGeoModel mdl;
    for (int k = 0; k < 9; ++k) mdl.h[k] = model[k];
    const uint32_t nb = (uint32_t)((n1 + n2 + kMatchThreads - 1) / kMatchThreads);
    hipLaunchKernelGGL(k_match_geo_terms, dim3(nb), dim3(kMatchThreads), 0, stream, p1, (uint32_t)n1, p2, (uint32_t)n2,
                       mdl, kind, t1, t2);
}

void match_geo_enqueue(hipStream_t stream, const MatchGeoDev& d) {
    MatchGeoArgs g{};
    g.m = match_args(d.m);
    g.row_terms = d.row_terms;
    g.col_terms = d.col_terms;
    g.T = d.T;
    g.kind = d.kind;
    g.reverse = d.reverse;
    const size_t row_blocks = (d.m.n1 + kMatchRowsPerWg - 1) / kMatchRowsPerWg;
    kLaunchGeo[d.m.dim / 32 - 1](g, (uint32_t)(row_blocks * d.m.splits), stream);
    if (d.m.splits > 1)
        hipLaunchKernelGGL(k_match_merge, dim3((uint32_t)((d.m.n1 + kMatchThreads - 1) / kMatchThreads)),
                           dim3(kMatchThreads), 0, stream, g.m);
}

// The array entry: allocate, upload, the device search, download, free.
hipError_t match_device(hipStream_t stream, int n_cu, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2,
                        uint32_t dim, uint32_t* idx, uint32_t* dist, uint32_t* idx2, uint32_t* dist2,
                        double* ms_kernel) {
    MatchDev m{};
    m.n1 = n1;
    m.n2 = n2;
    m.dim = dim;
    m.splits = match_plan_env(n1, n2, n_cu, &m.cols);
    MatchArrayBufs b;
    const size_t lead[4] = {0, 0, 0, 0};
    hipError_t e = match_array_alloc(m, lead, b);
    if (e != hipSuccess) return e;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d1, d1, n1 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d2, d2, n2 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(ev0, stream);
    if (e == hipSuccess) {
        match_norms_enqueue(stream, b.d1, n1, b.d2, n2, dim, b.norm1, b.norm2);
        match_enqueue(stream, m);
        e = hipGetLastError();
    }
    uint32_t* const host_out[4] = {idx, dist, idx2, dist2};
    return match_array_finish(e, stream, m, b, ev0, ev1, host_out, ms_kernel);
}

hipError_t match_geo_device(hipStream_t stream, int n_cu, const uint8_t* d1, size_t n1, const double* p1,
                            const uint8_t* d2, size_t n2, const double* p2, uint32_t dim, int kind, const double* model,
                            double sq_threshold, int reverse, uint32_t* idx, uint32_t* dist, uint32_t* idx2,
                            uint32_t* dist2, double* ms_kernel) {
    // the kernels' rows are the result rows, their columns the other image
    MatchGeoDev g{};
    MatchDev& m = g.m;
    m.n1 = reverse ? n2 : n1;
    m.n2 = reverse ? n1 : n2;
    m.dim = dim;
    m.splits = match_plan_env(m.n1, m.n2, n_cu, &m.cols);
    const uint8_t* dr = reverse ? d2 : d1;
    const uint8_t* dc = reverse ? d1 : d2;
    MatchArrayBufs b;
    const size_t lead[4] = {up256(n1 * 2 * sizeof(double)), up256(n2 * 2 * sizeof(double)),
                            up256(n1 * kMatchGeoTerms * sizeof(double)), up256(n2 * kMatchGeoTerms * sizeof(double))};
    hipError_t e = match_array_alloc(m, lead, b);
    if (e != hipSuccess) return e;
    double *dp1 = b.dbl[0], *dp2 = b.dbl[1], *t1 = b.dbl[2], *t2 = b.dbl[3];
    g.row_terms = reverse ? t2 : t1;
    g.col_terms = reverse ? t1 : t2;
    g.T = sq_threshold;
    g.kind = kind;
    g.reverse = reverse;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d1, dr, m.n1 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d2, dc, m.n2 * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dp1, p1, n1 * 2 * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dp2, p2, n2 * 2 * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(ev0, stream);
    if (e == hipSuccess) {
        match_norms_enqueue(stream, b.d1, m.n1, b.d2, m.n2, dim, b.norm1, b.norm2);
        match_geo_terms_enqueue(stream, dp1, n1, dp2, n2, model, kind, t1, t2);
        match_geo_enqueue(stream, g);
        e = hipGetLastError();
    }
    uint32_t* const host_out[4] = {idx, dist, idx2, dist2};
    return match_array_finish(e, stream, m, b, ev0, ev1, host_out, ms_kernel);
}

}  // namespace gcr
