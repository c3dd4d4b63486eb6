// Host model of the value ring of the feature-major rectification scorers
// (k_score_fm<KIND <= 2>, csrc/kernels.hip): the allocator and the two wait
// thresholds of csrc/fm_groups.h that the kernel itself uses.
//
// usage: fm_ring_model alloc [SEED]
//   One wave's allocator, single-threaded, under fixed and random sequences
//   of block sizes and random consumption orders.  Checks: a block lies in
//   [0, cap) and its runs inside it, on even doubles, run q's first 16-byte
//   slot on bank group q mod 8; it overlaps no published, unfolded block; the
//   wait threshold names a round this wave has already published (no
//   deadlock); with the ring empty no wait is needed for any size <= cap; a
//   wcnt row is not rewritten before its round is folded.  Run for both
//   depths (wcnt rows) the kernels use, 4 and 2.
// usage: fm_ring_model threads ROUNDS GROUPS MODE(typical|full|empty) [SEED] [REPEATS] [DEPTH]
//   14 compute waves, the chain wave and the look-ahead wave as threads with
//   std::atomic counters for the LDS flags.  The rings and the wcnt rows are
//   plain memory tagged with the round that wrote them, so ThreadSanitizer
//   reports a hand-over the counters do not order, and the tags catch one that
//   is ordered but too early.  A watchdog turns a stall into a failure.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "fm_groups.h"

namespace {

constexpr int kW = 14;
constexpr uint32_t kH = 16;
constexpr uint32_t kD = fmg::kRingDepth;
uint32_t g_depth = kD;             // wcnt rows: 4 (fused scorer) or 2 (unfused), argv
const uint32_t kCap = fmg::ring_cap(kH);

// block size of a wave-round whose runs have these lengths, as the kernel
// computes it; offs: each run's first double relative to the block's base
uint32_t block_of(const uint32_t n[kH], uint32_t offs[kH]) {
    uint32_t sum = 0;
    for (uint32_t q = 0; q < kH; ++q) {
        offs[q] = sum + fmg::ring_skew(q);
        sum += fmg::ring_pad(n[q]);
    }
    return fmg::ring_block(sum, kH);
}

// run lengths whose block has `size` doubles (size = 0 or 32 + 16 j)
void runs_for(uint32_t size, uint32_t n[kH], std::minstd_rand& rng) {
    std::memset(n, 0, sizeof(uint32_t) * kH);
    if (size == 0) return;
    uint32_t left = (size - fmg::ring_skew(kH)) / fmg::kRingRun;      // padded 16-value pieces
    while (left > 0) {
        const uint32_t q = (uint32_t)rng() % kH;
        if (n[q] >= 64) continue;
        n[q] = fmg::ring_pad(n[q]) + 1 + (uint32_t)rng() % 16;        // one more piece, partly filled
        --left;
    }
}

int g_fail = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (g_fail++ < 10) {                       \
                std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
                std::fprintf(stderr, "\n");            \
            }                                          \
        }                                              \
    } while (0)

// one wave, sizes from `next_size(R)`, the consumer folding a random number
// of published rounds whenever it may
void alloc_sequence(const char* name, uint32_t rounds, const std::vector<uint32_t>& sizes, uint32_t seed, int consume) {
    std::minstd_rand rng(seed);
    fmg::Ring ring;
    struct Blk { uint32_t lo, hi; };
    std::vector<Blk> blk;              // by round
    uint32_t done = 0;                 // done[w]: published(R) of the newest folded round
    int64_t row[kD];
    for (auto& r : row) r = -1;
    for (uint32_t R = 0; R < rounds; ++R) {
        const uint32_t want = sizes[R % sizes.size()];
        uint32_t n[kH], offs[kH];
        runs_for(want, n, rng);
        const uint32_t size = block_of(n, offs);
        CHECK(size == want, "%s: block of %u for runs of %u", name, size, want);
        CHECK(size <= kCap, "%s: block %u above the ring", name, size);
        const uint32_t base = fmg::ring_place(ring, size, kCap);
        const uint32_t need = fmg::ring_wait(ring, R, base, size, g_depth);
        fmg::ring_commit(ring, base, size);
        // the threshold is a round already published: published(R - 1) = R at most
        CHECK(need <= R, "%s: round %u waits for %u, not yet published", name, R, need);
        // ring empty (everything published is folded): nothing to wait for
        if (done == R) CHECK(need <= done, "%s: round %u waits (%u) on an empty ring", name, R, need);
        // the wait, then the consumer runs on by its own pace
        if (done < need) done = need;
        // block inside the ring, runs inside the block
        CHECK(base + size <= kCap && base % fmg::kRingRun == 0, "%s: round %u block [%u, +%u)", name, R, base, size);
        for (uint32_t q = 0; q < kH; ++q) {
            const uint32_t o = base + offs[q];
            CHECK(o % 2 == 0 && (o / 2) % 8 == q % 8, "%s: run %u at %u", name, q, o);
            CHECK(n[q] == 0 || o + fmg::ring_pad(n[q]) <= base + size, "%s: run %u leaves its block", name, q);
            CHECK(o < 65536 && n[q] < 65536 && fmg::ring_n(fmg::ring_pack(n[q], o)) == n[q] &&
                      fmg::ring_off(fmg::ring_pack(n[q], o)) == o, "%s: packed word", name);
        }
        // no overlap with a published, unfolded block: rounds r with published(r) > done
        for (uint32_t r = done; r < R; ++r)
            CHECK(!(size && base < blk[r].hi && blk[r].lo < base + size),
                  "%s: round %u block [%u, %u) overlaps unfolded round %u [%u, %u)", name, R, base, base + size, r,
                  blk[r].lo, blk[r].hi);
        // the wcnt row's previous round is folded
        const uint32_t s = fmg::ring_slot(R, g_depth);
        CHECK(row[s] < 0 || fmg::published((uint32_t)row[s]) <= done, "%s: wcnt row %u of round %ld rewritten in %u",
              name, s, (long)row[s], R);
        row[s] = R;
        blk.push_back({base, base + size});
        // round R is published: the consumer folds 0 .. all of what is there
        const uint32_t avail = fmg::published(R) - done;
        uint32_t k = consume == 0 ? 0 : consume == 1 ? avail : (uint32_t)rng() % (avail + 1);
        if (consume == 3 && (rng() & 7) != 0) k = 0;      // a slow consumer, in bursts
        done += k;
    }
}

int run_alloc(uint32_t seed) {
    CHECK(kCap == 1056 && fmg::ring_block(64 * kH, kH) == kCap, "ring capacity %u", kCap);
    const std::vector<std::pair<const char*, std::vector<uint32_t>>> fixed = {
        {"zeros", {0}},
        {"48", {48}},
        {"full", {1056}},
        {"full/48", {1056, 48}},
        {"48/full", {48, 1056, 48, 48, 1056}},
        {"zeros then full", {0, 0, 0, 0, 0, 0, 0, 0, 0, 1056, 0, 0, 0, 0, 0, 48}},
        {"half", {528}},
        {"just over half", {544}},
        {"thirds", {352, 368, 336}},
        {"typical", {368, 400, 480, 624, 304, 400, 416}},
    };
    for (const auto& f : fixed)
        for (int consume = 0; consume < 4; ++consume)
            alloc_sequence(f.first, 400, f.second, seed + (uint32_t)consume, consume);
    std::minstd_rand rng(seed * 7919u + 1u);
    for (int t = 0; t < 200; ++t) {
        std::vector<uint32_t> sz(64 + rng() % 64);
        const uint32_t kind = (uint32_t)rng() % 4;
        for (auto& s : sz) {
            const uint32_t v = (uint32_t)rng();
            const uint32_t pieces = kind == 0 ? v % 65 : kind == 1 ? 10 + v % 24 : kind == 2 ? (v & 1 ? 64 : v % 4) : 50 + v % 15;
            s = (kind != 3 && (v >> 8) % 5 == 0) ? 0u : fmg::ring_block(16 * std::max(1u, pieces), kH);
        }
        alloc_sequence("random", 600, sz, (uint32_t)rng(), 2 + t % 2);
    }
    if (g_fail) return 1;
    std::printf("OK alloc depth %u\n", g_depth);
    return 0;
}

// ------------------------------------------------------------ threaded model
struct Row { int64_t round = -1; uint32_t base = 0, size = 0; };

struct Workgroup {
    uint32_t rounds, groups;
    int mode;
    std::atomic<uint32_t> ready[kW], done[kW], cons_ready{0}, groups_done{0};
    // plain memory, ordered by the counters alone
    std::vector<int64_t> ring[kW];     // per double: the global round that wrote it
    Row wcnt[kD][kW];
    int64_t set_group[2] = {-1, -1};
    std::vector<int> outputs;
    std::atomic<bool> failed{false};
    std::atomic<uint64_t> progress{0};
    std::atomic<uint64_t> ahead_max{0};
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

bool wait_ge(Workgroup& wg, const std::atomic<uint32_t>& f, uint32_t v, Rng& rng) {
    while (f.load(std::memory_order_acquire) < v) {
        if (wg.failed.load(std::memory_order_relaxed)) return false;
        std::this_thread::yield();
        rng.maybe_yield();
    }
    return true;
}

uint32_t size_of_mode(int mode, Rng& rng) {
    const uint32_t v = (uint32_t)rng.r();
    uint32_t pieces;
    if (mode == 0) pieces = 10 + v % 28;                     // typical: 192 .. 624 doubles
    else if (mode == 1) pieces = (v & 1) ? 64 : 31 + v % 34; // full: half of the rounds need the whole ring
    else pieces = v % 4 == 0 ? 1 : 0;                        // near-empty: mostly no block at all
    return fmg::ring_block(16 * pieces, kH);
}

void compute_wave(Workgroup& wg, int w, uint32_t seed) {
    Rng rng(seed);
    fmg::Ring ring;
    for (uint32_t g = 0; g < wg.groups; ++g) {
        if (g > 0 && !wait_ge(wg, wg.cons_ready, fmg::cons_ready_for(g), rng)) return;
        // group g - 2's outputs are written before any wave enters group g
        if (g >= 2 && wg.groups_done.load(std::memory_order_acquire) < fmg::outputs_written(g - 2))
            return fail(wg, "entered a group two ahead of the outputs", g, wg.groups_done.load());
        if (wg.set_group[fmg::set_of(g)] != (int64_t)g)
            return fail(wg, "band read another group's constants", wg.set_group[fmg::set_of(g)], g);
        for (uint32_t r = 0; r < wg.rounds; ++r) {
            const uint32_t R = fmg::global_round(g, wg.rounds, r);
            rng.maybe_yield();
            const uint32_t size = size_of_mode(wg.mode, rng);
            const uint32_t base = fmg::ring_place(ring, size, kCap);
            const uint32_t need = fmg::ring_wait(ring, R, base, size, g_depth);
            fmg::ring_commit(ring, base, size);
            if (need > R) return fail(wg, "waits for a round not yet published", need, R);
            if (base + size > kCap) return fail(wg, "block leaves the ring", base, size);
            rng.maybe_yield();
            if (need > 0 && !wait_ge(wg, wg.done[w], need, rng)) return;
            {
                const uint64_t a = R + 1 - wg.done[w].load(std::memory_order_relaxed);   // rounds ahead of the fold
                uint64_t m = wg.ahead_max.load(std::memory_order_relaxed);
                while (a > m && !wg.ahead_max.compare_exchange_weak(m, a)) {}
            }
            // everything overwritten belongs to a round the wait covers
            Row& row = wg.wcnt[fmg::ring_slot(R, g_depth)][w];
            if (row.round >= 0 && fmg::published((uint32_t)row.round) > need)
                return fail(wg, "wcnt row rewritten before its round was folded", row.round, R);
            row.round = R;
            row.base = base;
            row.size = size;
            rng.maybe_yield();
            for (uint32_t i = base; i < base + size; ++i) {
                const int64_t old = wg.ring[w][i];
                if (old >= 0 && fmg::published((uint32_t)old) > need)
                    return fail(wg, "ring doubles rewritten before their round was folded", old, R);
                wg.ring[w][i] = R;
            }
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
                const Row row = wg.wcnt[fmg::ring_slot(R, g_depth)][w];
                if (row.round != (int64_t)R) return fail(wg, "run lengths of another round", row.round, R);
                for (uint32_t i = row.base; i < row.base + row.size; ++i)
                    if (wg.ring[w][i] != (int64_t)R) return fail(wg, "ring does not hold the round to fold", wg.ring[w][i], R);
                rng.maybe_yield();
                // (the kernel's store is relaxed: the fold only reads, and the adds that
                // consumed every read precede the store in program order)
                wg.done[w].store(fmg::published(R), std::memory_order_release);
            }
        }
        if (!wait_ge(wg, wg.cons_ready, fmg::cons_ready_for(g), rng)) return;
        if (wg.set_group[fmg::set_of(g)] != (int64_t)g)
            return fail(wg, "outputs read another group's set", wg.set_group[fmg::set_of(g)], g);
        wg.outputs[g] += 1;
        wg.groups_done.store(fmg::outputs_written(g), std::memory_order_release);
    }
}

void lookahead_wave(Workgroup& wg, uint32_t seed) {
    Rng rng(seed);
    for (uint32_t gn = 1; gn < wg.groups; ++gn) {
        if (!wait_ge(wg, wg.groups_done, fmg::set_free_for(gn), rng)) return;
        rng.maybe_yield();
        wg.set_group[fmg::set_of(gn)] = gn;
        wg.cons_ready.store(fmg::cons_ready_for(gn), std::memory_order_release);
    }
}

bool run_once(uint32_t rounds, uint32_t groups, int mode, uint32_t seed, uint64_t& ahead) {
    Workgroup wg;
    wg.rounds = rounds;
    wg.groups = groups;
    wg.mode = mode;
    wg.outputs.assign(groups, 0);
    for (int w = 0; w < kW; ++w) {
        wg.ready[w].store(0);
        wg.done[w].store(0);
        wg.ring[w].assign(kCap, -1);
    }
    wg.set_group[0] = 0;
    wg.cons_ready.store(fmg::cons_ready_for(0));
    std::vector<std::thread> th;
    std::atomic<int> running{kW + 2};
    auto wrap = [&](auto fn) { return [&, fn] { fn(); running.fetch_sub(1); }; };
    for (int w = 0; w < kW; ++w) th.emplace_back(wrap([&wg, w, seed] { compute_wave(wg, w, seed * 977u + (uint32_t)w); }));
    th.emplace_back(wrap([&wg, seed] { chain_wave(wg, seed * 977u + 100u); }));
    th.emplace_back(wrap([&wg, seed] { lookahead_wave(wg, seed * 977u + 101u); }));
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
            std::fprintf(stderr, "FAIL: stall (rounds %u groups %u): cons_ready %u groups_done %u\n", rounds, groups,
                         wg.cons_ready.load(), wg.groups_done.load());
            for (int w = 0; w < kW; ++w)
                std::fprintf(stderr, "  wave %2d ready %u done %u\n", w, wg.ready[w].load(), wg.done[w].load());
            wg.failed.store(true);
        }
    }
    for (auto& t : th) t.join();
    if (wg.failed.load()) return false;
    for (uint32_t g = 0; g < groups; ++g)
        if (wg.outputs[g] != 1) {
            std::fprintf(stderr, "FAIL: group %u wrote its outputs %d times\n", g, wg.outputs[g]);
            return false;
        }
    ahead = std::max<uint64_t>(ahead, wg.ahead_max.load());
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "alloc") {
        // both depths in use: the fused scorer's and the unfused one's
        for (uint32_t d : {fmg::kRingDepth, 2u}) {
            g_depth = d;
            if (run_alloc(argc > 2 ? (uint32_t)std::atoi(argv[2]) : 1u)) return 1;
        }
        return 0;
    }
    if (argc < 5 || std::string(argv[1]) != "threads") {
        std::fprintf(stderr, "usage: %s alloc [SEED] | threads ROUNDS GROUPS typical|full|empty [SEED] [REPEATS] [DEPTH]\n",
                     argv[0]);
        return 2;
    }
    const uint32_t rounds = (uint32_t)std::atoi(argv[2]), groups = (uint32_t)std::atoi(argv[3]);
    const std::string m = argv[4];
    const int mode = m == "typical" ? 0 : m == "full" ? 1 : 2;
    const uint32_t seed = argc > 5 ? (uint32_t)std::atoi(argv[5]) : 1u;
    const int reps = argc > 6 ? std::atoi(argv[6]) : 1;
    if (argc > 7) g_depth = (uint32_t)std::atoi(argv[7]);
    if (rounds < 1 || groups < 1 || groups > fmg::kMaxGroups || (g_depth != 2 && g_depth != fmg::kRingDepth)) return 2;
    uint64_t ahead = 0;
    for (int i = 0; i < reps; ++i)
        if (!run_once(rounds, groups, mode, seed + (uint32_t)i, ahead)) return 1;
    // a wave never holds more than the depth in unfolded rounds
    if (ahead > g_depth) {
        std::fprintf(stderr, "FAIL: a wave ran %lu rounds ahead of the fold\n", (unsigned long)ahead);
        return 1;
    }
    std::printf("OK rounds %u groups %u %s depth %u x %d (at most %lu rounds ahead)\n", rounds, groups, m.c_str(),
                g_depth, reps, (unsigned long)ahead);
    return 0;
}
