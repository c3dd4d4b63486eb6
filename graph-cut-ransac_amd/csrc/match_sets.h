// match_sets.h -- resident descriptor sets and matching on them (match_sets.hip;
// gcr_descriptors_* and gcr_match_set* are the entries).
//
// A set is one image's descriptors on the device with their norms and,
// optionally, the keypoint positions: uploaded once.  A match of two sets runs
// the two searches through match.hip's kernels on the sets' pointers, applies
// match_select.h's rule and compacts the kept rows in order, all on the
// context's stream, with one synchronisation and one download at the end.
// Every buffer a call needs beyond the sets lives in the context's
// MatchWorkspace, which only ever grows.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "match_geo.h"
#include "match_select.h"

struct gcr_ctx;

struct gcr_descriptors {
    gcr_ctx* ctx = nullptr;
    size_t n = 0;
    uint32_t dim = 0;
    char* base = nullptr;       // the one allocation behind the three pointers
    uint8_t* d = nullptr;       // n x dim
    uint32_t* norm = nullptr;   // |row - 128|^2
    double* pos = nullptr;      // n x 2, or null
};

namespace gcr {

struct MatchWorkspace {
    std::mutex mu;              // one set call at a time per context
    char* dev = nullptr;
    size_t dev_bytes = 0;
    char* pinned = nullptr;     // the download's staging
    size_t pinned_bytes = 0;
    std::vector<char> pageable; // the staging under GCR_MATCH_SETS_PAGEABLE=1 (measurement)
    hipEvent_t ev[4] = {};      // created with the first call that asks for kernel times
    uint64_t allocs = 0;        // device allocations made for this workspace
};

// one pair of a call
struct MatchSetsPair {
    const gcr_descriptors *a, *b;
    int mutual;
    MatchSelectRule rule;
    // guided (rule.guided): the model and the squared bound
    int kind;
    double model[9];
    double T;
};

// kMsAll: every kernel of the call; forward and reverse: a search with its merge; select: its three launches
enum { kMsAll = 0, kMsForward = 1, kMsReverse = 2, kMsSelect = 3, kMsCount = 4 };

// Allocates the set's buffers, uploads, computes the norms; synchronises.
hipError_t match_set_create(hipStream_t stream, const uint8_t* d, size_t n, uint32_t dim, const double* positions,
                            gcr_descriptors* out);
void match_set_destroy(gcr_descriptors* s);

// Every pair queued on `stream`, one synchronisation, one download.  Pair p's
// rows go to matches_out + 2 * offsets[p] and ratios_out + offsets[p], its
// count to m_out[p]; offsets[p + 1] - offsets[p] >= pairs[p].a->n.  ms (may be
// null): kMsCount doubles for one pair, kMsAll alone for several.
hipError_t match_sets_run(hipStream_t stream, int n_cu, MatchWorkspace& ws, const MatchSetsPair* pairs, size_t npairs,
                          const size_t* offsets, uint32_t* matches_out, double* ratios_out, size_t* m_out, double* ms);

// The device block to at least dev_need bytes and the download's staging
// (pinned, or ws.pageable) to host_need; a device block that has to grow waits
// for the stream first.  The caller holds ws.mu.
hipError_t match_workspace_grow(hipStream_t stream, MatchWorkspace& ws, size_t dev_need, size_t host_need,
                                bool pageable);
void match_workspace_free(MatchWorkspace& ws);

}  // namespace gcr
