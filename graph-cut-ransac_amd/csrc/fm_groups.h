// Index arithmetic of the grouped feature-major fused scorer
// (k_score_fm<KIND, 16, true>, kernels.hip): one launch scores `groups`
// consecutive batches ("groups"), a workgroup keeps its 16 slots' position in
// every one of them and its waves hand over through LDS counters that only
// grow.  The kernel and the host model of the hand-over
// (tests/cpp/fm_groups_model.cpp) share these functions.
//
// Roles: 14 compute waves (band + exact pass, one survivor region each), the
// chain wave (folds the regions in order, writes a group's outputs), the
// look-ahead wave (generates the next group's slots and their constants).
//
// Counters (LDS, monotonic):
//   ready[w]     rounds wave w has published, as global round + 1
//   done[w]      rounds of wave w the chain wave has folded, global round + 1
//   cons_ready   groups whose constants are in LDS: group g readable at g + 1
//   groups_done  groups whose outputs the chain wave has written
// Constant sets (hypothesis constants, pre-band records, counters, generated
// models): two, group g uses set g & 1.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FMG_HD __host__ __device__ inline
#else
#define FMG_HD inline
#endif

namespace fmg {

constexpr uint32_t kMaxGroups = 8;

// the round number the flags run on: never reset inside a launch
FMG_HD uint32_t global_round(uint32_t g, uint32_t rounds, uint32_t r) { return g * rounds + r; }
// the run-length (wcnt) buffer of a round
FMG_HD uint32_t round_parity(uint32_t R) { return R & 1u; }
// the constant set of a group
FMG_HD uint32_t set_of(uint32_t g) { return g & 1u; }

// compute wave w publishes global round R as ready[w] = published(R); the
// chain wave marks it folded as done[w] = published(R)
FMG_HD uint32_t published(uint32_t R) { return R + 1u; }
// compute wave, before it overwrites its region in global round R > 0: the
// chain wave has folded its previous run, done[w] >= region_free(R)
FMG_HD uint32_t region_free(uint32_t R) { return R; }

// compute waves (and the chain wave) before group g's first use of its
// constant set: cons_ready >= cons_ready_for(g)
FMG_HD uint32_t cons_ready_for(uint32_t g) { return g + 1u; }
// look-ahead wave, before it fills set_of(gn) for group gn >= 1 (gn = groups:
// scratch for the next launch's slots): the chain wave has written the
// outputs of the set's previous user, group gn - 2, and with them every
// compute wave has left that group: groups_done >= set_free_for(gn)
FMG_HD uint32_t set_free_for(uint32_t gn) { return gn - 1u; }
// stage (a) only: compute waves enter group g once groups_done >= this
FMG_HD uint32_t boundary_wait(uint32_t g) { return g; }
// chain wave after group g's outputs: groups_done = outputs_written(g)
FMG_HD uint32_t outputs_written(uint32_t g) { return g + 1u; }

// slot index of hypothesis q of workgroup wg in group g of a launch whose
// first batch starts at slot0 (nh slots a batch, H slots a workgroup)
FMG_HD uint64_t slot_of(uint64_t slot0, uint32_t g, uint32_t nh, uint32_t wg, uint32_t H, uint32_t q) {
    return slot0 + (uint64_t)g * nh + (uint64_t)wg * H + q;
}

// host: batches of the launch that starts at batch b of nb, at most G, never
// across the end of a selection ring of R batches
FMG_HD uint32_t launch_batches(uint32_t b, uint32_t nb, uint32_t G, uint32_t R) {
    uint32_t c = G;
    if (c > R - b % R) c = R - b % R;
    if (c > nb - b) c = nb - b;
    return c;
}

}  // namespace fmg
