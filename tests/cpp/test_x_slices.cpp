// The host bookkeeping of CG / PCG's x updates paid in slices (kryst_amd/csrc/cg_logic.h: XSlices), driven on the CPU with a model of the ring
// of direction vectors: random sequences of advance / flush / advance for every batch length and tile count that matters.  Stand-alone: built with
// -fsanitize=address,undefined and run by tests/test_x_slices_cpu.py; needs no GPU and no HIP header.
#define KRYST_X_SLICES_HOST_ONLY
#include "../../kryst_amd/csrc/cg_logic.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using kr::XSliceLaunch;
using kr::XSlices;

static int failures = 0;
#define CHECK(cond, ...)                                                                                     \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            if (++failures <= 20) { std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                    \
    } while (0)

static uint64_t rng_state;
static uint64_t rnd() {                                     // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Model {
    int m; int64_t nt; bool sliced;
    XSlices xs;
    std::vector<long long> slot;                            // ring slot -> the iteration whose direction vector it holds (0: none yet)
    std::vector<long long> last;                            // tile -> the last iteration whose x update it has
    long long it = 0; long launches = 0;
    Model(int m_, int64_t nt_, bool sliced_) : m(m_), nt(nt_), sliced(sliced_), slot((size_t)m_ + 1, 0), last((size_t)nt_, 0) { xs.init(m, nt, sliced); }

    void launch(const XSliceLaunch& l) {
        ++launches;
        const long long cnt = l.hi - l.lo + 1;
        CHECK(cnt >= 1 && cnt <= m, "m %d nt %lld: a launch of %lld updates", m, (long long)nt, cnt);
        CHECK(l.hi <= it, "m %d: update %lld of an iteration not yet enqueued (%lld)", m, l.hi, it);
        CHECK(0 <= l.tile_lo && l.tile_lo < l.tile_hi && l.tile_hi <= nt, "m %d nt %lld: tiles [%lld, %lld)", m, (long long)nt, (long long)l.tile_lo, (long long)l.tile_hi);
        if (!(0 <= l.tile_lo && l.tile_hi <= nt) || cnt < 1 || cnt > 4 * (long long)m) return;
        for (long long i = l.lo; i <= l.hi; ++i)            // every direction vector it reads is still in its slot
            CHECK(slot[(size_t)(i % (m + 1))] == i, "m %d it %lld: p_%lld read from a slot that holds p_%lld", m, it, i, slot[(size_t)(i % (m + 1))]);
        for (int64_t q = l.tile_lo; q < l.tile_hi; ++q) {   // ascending, nothing skipped, nothing twice
            CHECK(last[(size_t)q] == l.lo - 1, "m %d nt %lld it %lld: tile %lld has %lld, launch starts at %lld", m, (long long)nt, it, (long long)q, last[(size_t)q], l.lo);
            last[(size_t)q] = l.hi;
        }
    }
    void iterate() {
        ++it;
        slot[(size_t)(it % (m + 1))] = it;                  // the SpMV (or ring pass) that forms p_it is enqueued first and overwrites p_{it-m-1}
        XSliceLaunch l;
        const long before = launches;
        if (xs.advance(it, &l)) launch(l);
        CHECK(launches - before <= 1, "more than one launch in an iteration");
        for (int64_t q = 0; q < nt; ++q)                    // what keeps the NEXT iteration's overwrite of p_{it-m} safe
            CHECK(last[(size_t)q] >= it - m + 1, "m %d nt %lld it %lld: tile %lld only has %lld", m, (long long)nt, it, (long long)q, last[(size_t)q]);
    }
    void flush() {
        std::vector<XSliceLaunch> owed;
        xs.flush(it, owed);
        CHECK((long long)owed.size() <= (sliced ? m : 1), "flush: %zu launches", owed.size());
        for (const XSliceLaunch& l : owed) launch(l);
        for (int64_t q = 0; q < nt; ++q) CHECK(last[(size_t)q] == it, "m %d nt %lld: after the flush at %lld tile %lld has %lld", m, (long long)nt, it, (long long)q, last[(size_t)q]);
        owed.assign(3, XSliceLaunch{0, 0, 0, 0});
        xs.flush(it, owed);                                 // a second flush owes nothing
        CHECK(owed.empty(), "a second flush launched %zu", owed.size());
    }
};

int main() {
    const int ms[] = {1, 2, 3, 7, 8, 31, 32};
    const int64_t nts[] = {0, 1, 5, 31, 32, 33, 64, 1000};
    long cases = 0;
    for (int sliced = 0; sliced < 2; ++sliced)
        for (int m : ms)
            for (int64_t nt : nts)
                for (int seed = 0; seed < 6; ++seed) {
                    rng_state = 0xC0FFEEull + 1000003ull * (uint64_t)seed + 131ull * (uint64_t)m + 7ull * (uint64_t)nt + (uint64_t)sliced;
                    Model mod(m, nt, sliced != 0);
                    if (seed == 0) mod.flush();             // a flush before any iteration launches nothing
                    if (seed == 0) CHECK(mod.launches == 0, "a flush at iteration 0 launched");
                    const int rounds = 4 + (int)(rnd() % 8);
                    for (int r = 0; r < rounds; ++r) {
                        // steps of 1, of a few, of exactly m, of more than two rounds of slices
                        const uint64_t pick = rnd() % 5;
                        const long long k = pick == 0 ? 1 : pick == 1 ? m : pick == 2 ? 1 + (long long)(rnd() % (uint64_t)m) : pick == 3 ? (long long)(rnd() % (uint64_t)(3 * m + 2)) : 2 * m + 1;
                        for (long long j = 0; j < k; ++j) mod.iterate();
                        if (rnd() % 3 != 0) mod.flush();
                    }
                    mod.flush();
                    if (nt == 0) CHECK(mod.launches == 0, "m %d: launches on an empty vector", m);
                    if (sliced && nt > 0 && nt < m) {       // most slices are empty: a flush launches at most one per tile
                        for (int j = 0; j < 2 * m + 1; ++j) mod.iterate();
                        const long before = mod.launches;
                        mod.flush();
                        CHECK(mod.launches - before <= nt, "m %d nt %lld: %ld launches for %lld tiles", m, (long long)nt, mod.launches - before, (long long)nt);
                    }
                    ++cases;
                }
    if (failures) { std::printf("%d check(s) failed in %ld cases\n", failures, cases); return 1; }
    std::printf("x slices ok: %ld cases\n", cases);
    return 0;
}
