// Index arithmetic of the grouped feature-major fused scorer
// (k_score_fm<KIND, 16, true>, kernels.hip): one launch scores `groups`
// consecutive batches ("groups"), a workgroup keeps its 16 slots' position in
// every one of them and its waves hand over through LDS counters that only
// grow.  The kernel and the host models of the hand-over
// (tests/cpp/fm_groups_model.cpp, tests/cpp/fm_ring_model.cpp) share these
// functions.
//
// Roles: 14 compute waves (band + exact pass; each owns a value ring, in the
// correspondence scorers fixed survivor regions), the chain wave (folds the
// waves' runs in order, writes a group's outputs), the look-ahead wave
// (generates the next group's slots and their constants).  With the ring
// (below) a compute wave runs up to kRingDepth rounds ahead of the fold; the
// constant sets still keep it out of group g + 2 until group g's outputs are
// written.
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
// compute wave with fixed regions, before it overwrites its region in global
// round R > 0: the chain wave has folded its previous run, done[w] >=
// region_free(R) (with the ring: ring_wait below)
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

// ---- value ring (rectification scorers, KIND <= 2) -------------------------
// A compute wave's survivor values live in a ring of `cap` doubles (66 H: the
// bytes of H fixed regions of 66), one contiguous block a wave-round.  Run q
// of the block starts at base + sum_{q' < q} ring_pad(n_q') + ring_skew(q); a
// block never wraps (it starts at 0 when the tail is too short, and the tail
// is skipped); a round without survivors takes no block.  The worst block,
// H runs of 64 values, is exactly `cap`, so an empty ring takes any block.
// The run lengths and offsets of round R are in wcnt row ring_slot(R, D),
// packed by ring_pack.  D, the rows (a power of two, 2 .. kRingDepth), is how
// many rounds a wave may hold unfolded: kRingDepth in the fused scorer, 2 in
// the unfused one (15 compute waves: its LDS has no room for more rows).
constexpr uint32_t kRingDepth = 4;
constexpr uint32_t kRingRun = 16;                  // a run is padded to whole chain batches of 16 values

FMG_HD uint32_t ring_cap(uint32_t H) { return 66u * H; }
FMG_HD uint32_t ring_slot(uint32_t R, uint32_t D) { return R & (D - 1u); }
FMG_HD uint32_t ring_pad(uint32_t n) { return (n + kRingRun - 1u) & ~(kRingRun - 1u); }
// run q's first 16-byte slot falls on bank group q mod 8: of the chain's 16
// lanes only hypotheses h and h + 8 can meet on a bank
FMG_HD uint32_t ring_skew(uint32_t q) { return 2u * q; }
// doubles of the block whose padded runs sum to `padded`
FMG_HD uint32_t ring_block(uint32_t padded, uint32_t H) { return padded ? padded + ring_skew(H) : 0u; }
FMG_HD uint32_t ring_pack(uint32_t n, uint32_t off) { return n | off << 16; }
FMG_HD uint32_t ring_n(uint32_t v) { return v & 0xffffu; }
FMG_HD uint32_t ring_off(uint32_t v) { return v >> 16; }

// A compute wave's allocator (wave-uniform scalars): the end of its newest
// block and the extents of the blocks of its last D - 1 rounds, newest first
// (lo == hi: that round took no block).  Older rounds need no extent: the
// depth wait below covers them.
struct Ring {
    uint32_t head = 0;
    uint32_t lo[kRingDepth - 1] = {}, hi[kRingDepth - 1] = {};
};
// first double of the next block of `size` doubles
FMG_HD uint32_t ring_place(const Ring& s, uint32_t size, uint32_t cap) { return s.head + size > cap ? 0u : s.head; }
// before wave w writes global round R's block [base, base + size) and wcnt
// row ring_slot(R, D): done[w] >= ring_wait(...).  That is published(R') of
// the newest earlier round R' whose block overlaps the new one (the chain
// wave folds a wave's rounds in order, so every older one is folded too), and
// at least published(R - D), the previous user of the wcnt row.  The
// threshold never names a round the wave has not published: 0 is no wait.
FMG_HD uint32_t ring_wait(const Ring& s, uint32_t R, uint32_t base, uint32_t size, uint32_t D) {
    uint32_t need = R >= D ? published(R - D) : 0u;
    for (uint32_t d = kRingDepth - 1u; d >= 1u; --d)       // oldest first: the newest overlap wins
        if (size && d < D && d <= R && base < s.hi[d - 1u] && s.lo[d - 1u] < base + size) need = published(R - d);
    return need;
}
// the round's block is placed: it becomes the newest extent
FMG_HD void ring_commit(Ring& s, uint32_t base, uint32_t size) {
    for (uint32_t d = kRingDepth - 1u; d > 1u; --d) {
        s.lo[d - 1u] = s.lo[d - 2u];
        s.hi[d - 1u] = s.hi[d - 2u];
    }
    s.lo[0] = base;
    s.hi[0] = base + size;
    if (size) s.head = base + size;
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
