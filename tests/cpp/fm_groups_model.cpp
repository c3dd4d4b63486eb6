// Host model of the wave hand-over of the grouped feature-major fused scorer
// (k_score_fm<KIND, 16, true>, csrc/kernels.hip): 16 threads play the 14
// compute waves, the chain wave and the look-ahead wave of one workgroup with
// std::atomic counters in place of the LDS flags and the index arithmetic of
// csrc/fm_groups.h, yielding at random points.  Built with -fsanitize=thread:
// the survivor regions, the run-length buffers and the constant sets are plain
// memory, so a hand-over the counters do not order is a reported race, and the
// tags checked below catch a reuse that is ordered but too early.
//
// usage: fm_groups_model ROUNDS GROUPS STAGE(a|b) [SEED] [REPEATS]
// Checks: no region is rewritten before the chain wave has folded it; no
// constant set is rewritten while a wave of its group can still read it;
// every group completes.  A watchdog turns a stall into a failure with the
// counters printed.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "fm_groups.h"

namespace {

constexpr int kW = 14;

struct ConstSet {
    int64_t group = -1;               // whose constants these are (look-ahead wave / prologue)
    int64_t gen = -1;                 // whose generated slots (also the last pass's scratch)
    std::atomic<uint32_t> cnt{0};     // the compute waves' inlier-count atomics
};

struct Workgroup {
    uint32_t rounds, groups;
    bool stage_a;
    std::atomic<uint32_t> ready[kW], done[kW], cons_ready{0}, groups_done{0};
    // plain memory, ordered by the counters alone
    int64_t region[kW];               // global round whose runs the region holds
    bool folded[kW];                  // ... and whether the chain wave has folded them
    int64_t wcnt[2][kW];              // run lengths: the global round they belong to
    ConstSet set[2];
    std::vector<int> outputs;         // group g's outputs written
    std::atomic<bool> failed{false};
    std::atomic<uint64_t> progress{0};
};

struct Rng {
    std::minstd_rand r;
    explicit Rng(uint32_t s) : r(s) {}
    void maybe_yield() {
        const uint32_t v = (uint32_t)r();
        if ((v & 3u) == 0) std::this_thread::yield();
        if ((v & 255u) == 1) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
};

void fail(Workgroup& wg, const char* what, long a, long b) {
    if (!wg.failed.exchange(true)) std::fprintf(stderr, "FAIL: %s (%ld, %ld)\n", what, a, b);
}

// fm_wait_ge: poll a counter that only grows
bool wait_ge(Workgroup& wg, const std::atomic<uint32_t>& f, uint32_t v, Rng& rng) {
    while (f.load(std::memory_order_acquire) < v) {
        if (wg.failed.load(std::memory_order_relaxed)) return false;
        std::this_thread::yield();
        rng.maybe_yield();
    }
    return true;
}

void compute_wave(Workgroup& wg, int w, uint32_t seed) {
    Rng rng(seed);
    for (uint32_t g = 0; g < wg.groups; ++g) {
        if (g > 0) {
            if (wg.stage_a && !wait_ge(wg, wg.groups_done, fmg::boundary_wait(g), rng)) return;
            if (!wait_ge(wg, wg.cons_ready, fmg::cons_ready_for(g), rng)) return;
        }
        const ConstSet& cs = wg.set[fmg::set_of(g)];
        for (uint32_t r = 0; r < wg.rounds; ++r) {
            const uint32_t R = fmg::global_round(g, wg.rounds, r);
            rng.maybe_yield();
            // band: the pre-band records of the group's set, run lengths out
            if (cs.group != (int64_t)g) return fail(wg, "band read another group's constants", cs.group, g);
            wg.wcnt[fmg::round_parity(R)][w] = R;
            rng.maybe_yield();
            // exact pass: overwrite the region once its previous runs are folded
            if (R > 0 && !wait_ge(wg, wg.done[w], fmg::region_free(R), rng)) return;
            if (R > 0 && (!wg.folded[w] || wg.region[w] != (int64_t)R - 1))
                return fail(wg, "region rewritten before it was folded", wg.region[w], R);
            wg.region[w] = R;
            wg.folded[w] = false;
            rng.maybe_yield();
            if (cs.group != (int64_t)g) return fail(wg, "exact pass read another group's constants", cs.group, g);
            wg.set[fmg::set_of(g)].cnt.fetch_add(1, std::memory_order_relaxed);
            wg.ready[w].store(fmg::published(R), std::memory_order_release);
            wg.progress.fetch_add(1, std::memory_order_relaxed);
        }
    }
}

void chain_wave(Workgroup& wg, uint32_t seed) {
    Rng rng(seed);
    for (uint32_t g = 0; g < wg.groups; ++g) {
        for (uint32_t r = 0; r < wg.rounds; ++r) {
            const uint32_t R = fmg::global_round(g, wg.rounds, r);
            for (int w = 0; w < kW; ++w) {
                if (!wait_ge(wg, wg.ready[w], fmg::published(R), rng)) return;
                if (wg.wcnt[fmg::round_parity(R)][w] != (int64_t)R)
                    return fail(wg, "run lengths of another round", wg.wcnt[fmg::round_parity(R)][w], R);
                if (wg.region[w] != (int64_t)R || wg.folded[w])
                    return fail(wg, "region does not hold the round to fold", wg.region[w], R);
                rng.maybe_yield();
                wg.folded[w] = true;
                // (the kernel's store is relaxed: its fold only reads the region, and
                // the adds that consumed every read precede the store in program order)
                wg.done[w].store(fmg::published(R), std::memory_order_release);
            }
        }
        // the group's outputs: its set's counts, validity, generated models
        if (!wait_ge(wg, wg.cons_ready, fmg::cons_ready_for(g), rng)) return;
        ConstSet& cs = wg.set[fmg::set_of(g)];
        rng.maybe_yield();
        if (cs.group != (int64_t)g || cs.gen != (int64_t)g)
            return fail(wg, "outputs read another group's set", cs.group, g);
        if (cs.cnt.load(std::memory_order_relaxed) != (uint32_t)kW * wg.rounds)
            return fail(wg, "inlier counts of the group incomplete or mixed", cs.cnt.load(), g);
        wg.outputs[g] += 1;
        wg.groups_done.store(fmg::outputs_written(g), std::memory_order_release);
    }
}

void lookahead_wave(Workgroup& wg, uint32_t seed) {
    Rng rng(seed);
    for (uint32_t gn = 1; gn <= wg.groups; ++gn) {
        const bool inner = gn < wg.groups;
#ifdef FMG_MODEL_EARLY_SET
        // canary build (tests/test_fm_groups_model.py): one group too early
        const uint32_t free_at = fmg::set_free_for(gn) > 0 ? fmg::set_free_for(gn) - 1 : 0;
#else
        const uint32_t free_at = fmg::set_free_for(gn);
#endif
        if (!wait_ge(wg, wg.groups_done, free_at, rng)) return;
        ConstSet& ns = wg.set[fmg::set_of(gn)];
        rng.maybe_yield();
        ns.gen = gn;                   // generated models and attempts (the last pass: scratch)
        rng.maybe_yield();
        if (inner) {
            ns.group = gn;
            ns.cnt.store(0, std::memory_order_relaxed);
            wg.cons_ready.store(fmg::cons_ready_for(gn), std::memory_order_release);
        }
    }
}

bool run_once(uint32_t rounds, uint32_t groups, bool stage_a, uint32_t seed) {
    Workgroup wg;
    wg.rounds = rounds;
    wg.groups = groups;
    wg.stage_a = stage_a;
    wg.outputs.assign(groups, 0);
    for (int w = 0; w < kW; ++w) {
        wg.ready[w].store(0);
        wg.done[w].store(0);
        wg.region[w] = -1;
        wg.folded[w] = true;
        wg.wcnt[0][w] = wg.wcnt[1][w] = -1;
    }
    // the prologue: group 0 in set 0, then the start barrier
    wg.set[0].group = 0;
    wg.set[0].gen = 0;
    wg.cons_ready.store(fmg::cons_ready_for(0));
    std::vector<std::thread> th;
    std::atomic<int> running{kW + 2};
    auto wrap = [&](auto fn) { return [&, fn] { fn(); running.fetch_sub(1); }; };
    for (int w = 0; w < kW; ++w) th.emplace_back(wrap([&wg, w, seed] { compute_wave(wg, w, seed * 977u + (uint32_t)w); }));
    th.emplace_back(wrap([&wg, seed] { chain_wave(wg, seed * 977u + 100u); }));
    th.emplace_back(wrap([&wg, seed] { lookahead_wave(wg, seed * 977u + 101u); }));
    // watchdog: no progress for 10 s is a stall
    uint64_t last = 0;
    auto t_last = std::chrono::steady_clock::now();
    while (running.load() > 0) {
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        const uint64_t p = wg.progress.load();
        const auto now = std::chrono::steady_clock::now();
        if (p != last) {
            last = p;
            t_last = now;
        } else if (now - t_last > std::chrono::seconds(10) && !wg.failed.load()) {
            std::fprintf(stderr, "FAIL: stall (rounds %u groups %u stage %c): cons_ready %u groups_done %u\n", rounds,
                         groups, stage_a ? 'a' : 'b', wg.cons_ready.load(), wg.groups_done.load());
            for (int w = 0; w < kW; ++w)
                std::fprintf(stderr, "  wave %2d ready %u done %u\n", w, wg.ready[w].load(), wg.done[w].load());
            wg.failed.store(true);      // every wait returns
        }
    }
    for (auto& t : th) t.join();
    if (wg.failed.load()) return false;
    for (uint32_t g = 0; g < groups; ++g)
        if (wg.outputs[g] != 1) {
            std::fprintf(stderr, "FAIL: group %u wrote its outputs %d times\n", g, wg.outputs[g]);
            return false;
        }
    if (wg.groups_done.load() != groups) {
        std::fprintf(stderr, "FAIL: groups_done %u of %u\n", wg.groups_done.load(), groups);
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s ROUNDS GROUPS a|b [SEED] [REPEATS]\n", argv[0]);
        return 2;
    }
    const uint32_t rounds = (uint32_t)std::atoi(argv[1]), groups = (uint32_t)std::atoi(argv[2]);
    const bool stage_a = argv[3][0] == 'a';
    const uint32_t seed = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 1u;
    const int reps = argc > 5 ? std::atoi(argv[5]) : 1;
    if (rounds < 1 || groups < 1 || groups > fmg::kMaxGroups) return 2;
    for (int i = 0; i < reps; ++i)
        if (!run_once(rounds, groups, stage_a, seed + (uint32_t)i)) return 1;
    std::printf("OK rounds %u groups %u stage %c x %d\n", rounds, groups, stage_a ? 'a' : 'b', reps);
    return 0;
}
