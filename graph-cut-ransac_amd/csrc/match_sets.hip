// match_sets.hip -- matching two resident descriptor sets entirely on the
// device (match_sets.h; match_select.h is the rule's definition).
//
// The searches are match.hip's, on the sets' pointers (match_enqueue,
// match_geo_enqueue): the set's norms are computed once, at creation.  The
// rule and the compaction are three launches of kMatchSelectRows rows per
// workgroup, one row per thread:
//   k_match_select_count    match_select_row of every row; the workgroup's
//                           number of kept rows (wave ballots, popcounts).
//   k_match_select_scan     ONE workgroup: the exclusive scan of the workgroup
//                           counts, 256 per step with a carry, and their total M.
//   k_match_select_scatter  the rule again (cheaper than storing the flags and
//                           the ratios); a kept row's position is its
//                           workgroup's offset + the kept rows of the earlier
//                           waves + the popcount of the ballot below its lane.
// A row's position is a function of the rows before it alone -- no atomic
// decides it, so the output is sorted by row -- and no workgroup waits on
// another one's progress: the kernel boundaries are the only synchronisation
// between workgroups.
//
// Device buffers of a call, all in the context's MatchWorkspace:
//   scratch  the forward results and split partials, the reverse ones
//            (mutual), the guided terms, the workgroup counts and offsets;
//            reused by the pairs of a call in stream order.
//   output   M per pair | matches (2 x uint32 per row) | ratios (a double per
//            row), laid out by the caller's row offsets, downloaded in one
//            copy and handed out by M.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "match_sets.h"

namespace gcr {
namespace {

constexpr int kSelThreads = (int)kMatchSelectRows;
constexpr int kSelWaves = kSelThreads / 64;
static_assert(kSelThreads % 64 == 0, "whole waves");

struct SelectArgs {
    const uint32_t *idx, *dist, *idx2, *dist2;  // the forward search, n each
    const uint32_t* back;                       // the reverse search's idx (nb), or null
    uint32_t n, nb;
    MatchSelectRule rule;
    uint32_t* counts;           // [ceil(n / kMatchSelectRows)]
    uint32_t* offsets;          // the same, exclusive scan
    uint32_t* m;                // the total
    uint32_t* matches;          // 2 per kept row
    double* ratios;
};

__device__ __forceinline__ bool select_row(const SelectArgs& a, uint32_t i, double* ratio) {
    if (i >= a.n) return false;
    return match_select_row(a.rule, i, a.idx[i], a.dist[i], a.idx2[i], a.dist2[i], a.back, a.nb, ratio);
}

__global__ __launch_bounds__(kSelThreads) void k_match_select_count(SelectArgs a) {
    __shared__ uint32_t s_w[kSelWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    double ratio;
    const bool keep = select_row(a, blockIdx.x * kMatchSelectRows + tid, &ratio);
    const unsigned long long b = __ballot(keep);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
        for (int w = 0; w < kSelWaves; ++w) c += s_w[w];
        a.counts[blockIdx.x] = c;
    }
}

// one workgroup; nwg counts in, nwg exclusive offsets and the total out
__global__ __launch_bounds__(kSelThreads) void k_match_select_scan(const uint32_t* counts, uint32_t nwg,
                                                                   uint32_t* offsets, uint32_t* m) {
    __shared__ uint32_t s_w[kSelWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nwg; base += kSelThreads) {      // workgroup-uniform trip count
        const uint32_t k = base + tid;
        const uint32_t c = k < nwg ? counts[k] : 0u;
        uint32_t v = c;                                             // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)v, d);
            if ((int)lane >= d) v += t;
        }
        if (lane == 63) s_w[wave] = v;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < kSelWaves; ++w) {
            before += (uint32_t)w < wave ? s_w[w] : 0u;
            total += s_w[w];
        }
        if (k < nwg) offsets[k] = carry + before + v - c;
        carry += total;
        __syncthreads();                                            // s_w is rewritten by the next step
    }
    if (tid == 0) *m = carry;
}

__global__ __launch_bounds__(kSelThreads) void k_match_select_scatter(SelectArgs a) {
    __shared__ uint32_t s_w[kSelWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t i = blockIdx.x * kMatchSelectRows + tid;
    double ratio;
    const bool keep = select_row(a, i, &ratio);
    const unsigned long long b = __ballot(keep);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!keep) return;
    uint32_t pos = a.offsets[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) pos += s_w[w];
    pos += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    // pos < n: it counts kept rows before row i < n
    a.matches[2 * (size_t)pos] = i;
    a.matches[2 * (size_t)pos + 1] = a.idx[i];
    a.ratios[pos] = ratio;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// a bump allocator over the workspace: the first pass (base == nullptr) only measures
struct Carver {
    char* base;
    size_t used = 0;
    template <class T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += up256(count * sizeof(T));
        return p;
    }
};

struct PairPlan {
    uint32_t splits_f = 1, cols_f = 0, splits_b = 1, cols_b = 0;
};

struct PairBufs {
    uint32_t *f_out[4], *f_part[4], *b_out[4], *b_part[4];
    double *t1, *t2;
    uint32_t *counts, *offsets;
};

PairBufs carve_pair(Carver& c, const MatchSetsPair& p, const PairPlan& pl) {
    PairBufs b{};
    const size_t na = p.a->n, nb = p.b->n;
    for (int k = 0; k < 4; ++k) b.f_out[k] = c.take<uint32_t>(na);
    for (int k = 0; k < 4; ++k) b.f_part[k] = pl.splits_f > 1 ? c.take<uint32_t>((size_t)pl.splits_f * na) : nullptr;
    if (p.mutual) {
        for (int k = 0; k < 4; ++k) b.b_out[k] = c.take<uint32_t>(nb);
        for (int k = 0; k < 4; ++k)
            b.b_part[k] = pl.splits_b > 1 ? c.take<uint32_t>((size_t)pl.splits_b * nb) : nullptr;
    }
    if (p.rule.guided) {
        b.t1 = c.take<double>(na * kMatchGeoTerms);
        b.t2 = c.take<double>(nb * kMatchGeoTerms);
    }
    const size_t nwg = (na + kMatchSelectRows - 1) / kMatchSelectRows;
    b.counts = c.take<uint32_t>(nwg);
    b.offsets = c.take<uint32_t>(nwg);
    return b;
}

MatchDev search_dev(const gcr_descriptors* rows, const gcr_descriptors* cols, uint32_t splits, uint32_t ncols,
                    uint32_t* const out[4], uint32_t* const part[4]) {
    MatchDev m{};
    m.d1 = rows->d;
    m.norm1 = rows->norm;
    m.n1 = rows->n;
    m.d2 = cols->d;
    m.norm2 = cols->norm;
    m.n2 = cols->n;
    m.dim = rows->dim;
    m.splits = splits;
    m.cols = ncols;
    for (int k = 0; k < 4; ++k) {
        m.out[k] = out[k];
        m.part[k] = part[k];
    }
    return m;
}

void enqueue_search(hipStream_t stream, const MatchSetsPair& p, const PairBufs& b, const PairPlan& pl, bool reverse) {
    const gcr_descriptors* rows = reverse ? p.b : p.a;
    const gcr_descriptors* cols = reverse ? p.a : p.b;
    const MatchDev m = search_dev(rows, cols, reverse ? pl.splits_b : pl.splits_f, reverse ? pl.cols_b : pl.cols_f,
                                  reverse ? b.b_out : b.f_out, reverse ? b.b_part : b.f_part);
    if (!p.rule.guided) {
        match_enqueue(stream, m);
        return;
    }
    MatchGeoDev g{};
    g.m = m;
    g.row_terms = reverse ? b.t2 : b.t1;                  // t1 is image 1's (set a), whatever the direction
    g.col_terms = reverse ? b.t1 : b.t2;
    g.T = p.T;
    g.kind = p.kind;
    g.reverse = reverse ? 1 : 0;
    match_geo_enqueue(stream, g);
}

void enqueue_select(hipStream_t stream, const MatchSetsPair& p, const PairBufs& b, uint32_t* m, uint32_t* matches,
                    double* ratios) {
    SelectArgs a{};
    a.idx = b.f_out[0];
    a.dist = b.f_out[1];
    a.idx2 = b.f_out[2];
    a.dist2 = b.f_out[3];
    a.back = p.mutual ? b.b_out[0] : nullptr;
    a.n = (uint32_t)p.a->n;
    a.nb = (uint32_t)p.b->n;
    a.rule = p.rule;
    a.counts = b.counts;
    a.offsets = b.offsets;
    a.m = m;
    a.matches = matches;
    a.ratios = ratios;
    const uint32_t nwg = (a.n + kMatchSelectRows - 1) / kMatchSelectRows;
    hipLaunchKernelGGL(k_match_select_count, dim3(nwg), dim3(kSelThreads), 0, stream, a);
    hipLaunchKernelGGL(k_match_select_scan, dim3(1), dim3(kSelThreads), 0, stream, b.counts, nwg, b.offsets, m);
    hipLaunchKernelGGL(k_match_select_scatter, dim3(nwg), dim3(kSelThreads), 0, stream, a);
}

}  // namespace

hipError_t match_workspace_grow(hipStream_t stream, MatchWorkspace& ws, size_t dev_need, size_t host_need,
                                bool pageable) {
    if (dev_need > ws.dev_bytes) {
        hipError_t e = hipStreamSynchronize(stream);      // nothing of an earlier call reads the old block
        if (e != hipSuccess) return e;
        if (ws.dev) (void)hipFree(ws.dev);
        ws.dev = nullptr;
        ws.dev_bytes = 0;
        e = hipMalloc(reinterpret_cast<void**>(&ws.dev), dev_need);
        if (e != hipSuccess) return e;
        ws.dev_bytes = dev_need;
        ++ws.allocs;
    }
    if (pageable) {
        if (ws.pageable.size() < host_need) ws.pageable.resize(host_need);
    } else if (host_need > ws.pinned_bytes) {
        if (ws.pinned) (void)hipHostFree(ws.pinned);
        ws.pinned = nullptr;
        ws.pinned_bytes = 0;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ws.pinned), host_need, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        ws.pinned_bytes = host_need;
    }
    return hipSuccess;
}

hipError_t match_set_create(hipStream_t stream, const uint8_t* d, size_t n, uint32_t dim, const double* positions,
                            gcr_descriptors* out) {
    const size_t b_d = up256(n * dim), b_n = up256(n * 4), b_p = positions ? up256(n * 2 * sizeof(double)) : 0;
    char* base = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), b_p + b_d + b_n);
    if (e != hipSuccess) return e;
    char* p = base;                                       // the doubles first: 256-byte aligned either way
    double* pos = positions ? reinterpret_cast<double*>(p) : nullptr;
    p += b_p;
    uint8_t* dd = reinterpret_cast<uint8_t*>(p);
    p += b_d;
    uint32_t* norm = reinterpret_cast<uint32_t*>(p);
    e = hipMemcpyAsync(dd, d, n * dim, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && positions)
        e = hipMemcpyAsync(pos, positions, n * 2 * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        match_norms_enqueue(stream, dd, n, dd, 0, dim, norm, norm);
        e = hipGetLastError();
    }
    const hipError_t s = hipStreamSynchronize(stream);    // the host arrays are the caller's again
    if (e == hipSuccess) e = s;
    if (e != hipSuccess) {
        (void)hipFree(base);
        return e;
    }
    out->n = n;
    out->dim = dim;
    out->base = base;
    out->d = dd;
    out->norm = norm;
    out->pos = pos;
    return hipSuccess;
}

void match_set_destroy(gcr_descriptors* s) {
    if (s->base) (void)hipFree(s->base);
    s->base = nullptr;
}

void match_workspace_free(MatchWorkspace& ws) {
    if (ws.dev) (void)hipFree(ws.dev);
    if (ws.pinned) (void)hipHostFree(ws.pinned);
    for (hipEvent_t& e : ws.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    ws.dev = ws.pinned = nullptr;
    ws.dev_bytes = ws.pinned_bytes = 0;
}

hipError_t match_sets_run(hipStream_t stream, int n_cu, MatchWorkspace& ws, const MatchSetsPair* pairs, size_t npairs,
                          const size_t* offsets, uint32_t* matches_out, double* ratios_out, size_t* m_out, double* ms) {
    std::lock_guard<std::mutex> lk(ws.mu);
    // GCR_MATCH_SETS_PAGEABLE=1: the download lands in pageable memory (the measurement of the pinned staging)
    const char* pg = getenv("GCR_MATCH_SETS_PAGEABLE");
    const bool pageable = pg && atoi(pg) == 1;

    // the plans, then the scratch all pairs share (the largest) and the output all pairs split
    std::vector<PairPlan> plans(npairs);
    size_t scratch = 0;
    for (size_t k = 0; k < npairs; ++k) {
        const MatchSetsPair& p = pairs[k];
        PairPlan& pl = plans[k];
        pl.splits_f = match_plan_env(p.a->n, p.b->n, n_cu, &pl.cols_f);
        if (p.mutual) pl.splits_b = match_plan_env(p.b->n, p.a->n, n_cu, &pl.cols_b);
        Carver measure{nullptr};
        (void)carve_pair(measure, p, pl);
        if (measure.used > scratch) scratch = measure.used;
    }
    const size_t total = offsets[npairs];
    Carver out_measure{nullptr};
    (void)out_measure.take<uint32_t>(npairs);
    (void)out_measure.take<uint32_t>(2 * total);
    (void)out_measure.take<double>(total);
    const size_t out_bytes = out_measure.used;

    hipError_t e = match_workspace_grow(stream, ws, scratch + out_bytes, out_bytes, pageable);
    if (e != hipSuccess) return e;
    const bool timed = ms != nullptr;
    const bool phases = timed && npairs == 1;
    if (timed)
        for (hipEvent_t& ev : ws.ev)
            if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return e;

    char* out_base = ws.dev + scratch;
    Carver oc{out_base};
    uint32_t* d_m = oc.take<uint32_t>(npairs);
    uint32_t* d_matches = oc.take<uint32_t>(2 * total);
    double* d_ratios = oc.take<double>(total);

    if (timed) e = hipEventRecord(ws.ev[0], stream);
    for (size_t k = 0; k < npairs && e == hipSuccess; ++k) {
        const MatchSetsPair& p = pairs[k];
        Carver c{ws.dev};
        const PairBufs b = carve_pair(c, p, plans[k]);
        if (p.rule.guided)
            match_geo_terms_enqueue(stream, p.a->pos, p.a->n, p.b->pos, p.b->n, p.model, p.kind, b.t1, b.t2);
        enqueue_search(stream, p, b, plans[k], false);
        if (phases) e = hipEventRecord(ws.ev[1], stream);
        if (p.mutual) enqueue_search(stream, p, b, plans[k], true);
        if (phases && e == hipSuccess) e = hipEventRecord(ws.ev[2], stream);
        enqueue_select(stream, p, b, d_m + k, d_matches + 2 * offsets[k], d_ratios + offsets[k]);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (timed && e == hipSuccess) e = hipEventRecord(ws.ev[3], stream);
    char* stage = pageable ? ws.pageable.data() : ws.pinned;
    if (e == hipSuccess) e = hipMemcpyAsync(stage, out_base, out_bytes, hipMemcpyDeviceToHost, stream);
    const hipError_t s = hipStreamSynchronize(stream);    // the one synchronisation; also after an error
    if (e == hipSuccess) e = s;
    if (e != hipSuccess) return e;

    const uint32_t* h_m = reinterpret_cast<const uint32_t*>(stage);
    const uint32_t* h_matches = reinterpret_cast<const uint32_t*>(stage + (reinterpret_cast<char*>(d_matches) - out_base));
    const double* h_ratios = reinterpret_cast<const double*>(stage + (reinterpret_cast<char*>(d_ratios) - out_base));
    for (size_t k = 0; k < npairs; ++k) {
        const size_t m = h_m[k];
        if (m > pairs[k].a->n) return hipErrorUnknown;    // never: M counts rows of a
        m_out[k] = m;
        std::memcpy(matches_out + 2 * offsets[k], h_matches + 2 * offsets[k], m * 2 * sizeof(uint32_t));
        std::memcpy(ratios_out + offsets[k], h_ratios + offsets[k], m * sizeof(double));
    }
    if (timed) {
        float t = 0.f;
        e = hipEventElapsedTime(&t, ws.ev[0], ws.ev[3]);
        ms[kMsAll] = (double)t;
        if (phases && e == hipSuccess) {
            e = hipEventElapsedTime(&t, ws.ev[0], ws.ev[1]);
            ms[kMsForward] = (double)t;
            if (e == hipSuccess) e = hipEventElapsedTime(&t, ws.ev[1], ws.ev[2]);
            ms[kMsReverse] = (double)t;
            if (e == hipSuccess) e = hipEventElapsedTime(&t, ws.ev[2], ws.ev[3]);
            ms[kMsSelect] = (double)t;
        }
    }
    return e;
}

}  // namespace gcr
