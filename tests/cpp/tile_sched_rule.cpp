// tile_sched_rule.cpp — the launch rule, the kept state and the buffer layout of the tile schedule (csrc/tile_sched.hpp) on
// a machine without a GPU.  Every case is a sequence of launches driven the way launch_fused drives them (the rule, a build
// after a timed launch, the launch counted), and every expectation below is written out by hand from the rule's description,
// not computed by the header.  Built with -fsanitize=address,undefined by tests/test_tile_sched_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../realsense-pointcloud_amd/csrc/tile_sched.hpp"

namespace {

using namespace rsreg;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

// What launch_fused does around one launch.  A first-launch schedule of n tiles has FIRST(n) workgroups, a steady one
// STEADY(n): the figures of f4 = f2 = 0.25 (n4 = n2 = n / 4 rounded down to a multiple of 8) and of f4 = 0, f2 = 0.10, so that
// taking one schedule for the other shows.  400 tiles: 400 + 3 * 96 + 96 = 784 and 400 + 40 = 440.
uint32_t down8(uint32_t v) { return v - v % 8u; }
uint32_t FIRST(uint32_t n) { return n + 3u * down8(n / 4u) + down8(n / 4u); }
uint32_t STEADY(uint32_t n) { return n + down8(n / 10u); }

struct Sim {
    SchedCfg cfg;
    SchedKept kept;
    SchedRun run;
    bool stamps = false;
    void align() { run = SchedRun(); }   // (rsreg_icp_begin: a new IcpState)
    SchedLaunch launch(uint32_t n_tiles, bool restart_here)
    {
        const SchedLaunch l = sched_next(cfg, kept, run, n_tiles, restart_here, stamps);
        if (l.timed) {
            sched_built(kept, run, restart_here, restart_here ? FIRST(n_tiles) : STEADY(n_tiles), n_tiles);
            if (restart_here && cfg.at_launch == 0) sched_built(kept, run, false, STEADY(n_tiles), n_tiles);
        }
        ++run.fused_launches;
        return l;
    }
};

Sim fresh(int at = 1, uint32_t min_tiles = 1, uint32_t cap = 1000)
{
    Sim s;
    s.cfg.min_tiles = min_tiles;
    s.cfg.at_launch = at;
    sched_regrown(s.kept, cap);
    return s;
}

bool is(const SchedLaunch &l, bool eligible, SchedLaunch::From from, bool timed, uint32_t grid, uint32_t n_items, uint32_t first_extra)
{
    return l.eligible == eligible && l.from == from && l.timed == timed && l.grid == grid && l.n_items == n_items && l.first_extra == first_extra;
}
bool is(const KeptSched &k, uint32_t items, uint32_t tiles, int age) { return k.items == items && k.tiles == tiles && k.age == age; }
bool is(const SchedRun &r, int launches, bool ready, bool carried, uint32_t items)
{
    return r.fused_launches == launches && r.ready == ready && r.carried == carried && r.items == items;
}
bool same(const Sim &a, const Sim &b)
{
    return a.kept.cap_tiles == b.kept.cap_tiles && is(a.kept.steady, b.kept.steady.items, b.kept.steady.tiles, b.kept.steady.age) &&
           is(a.kept.first, b.kept.first.items, b.kept.first.tiles, b.kept.first.age) && is(a.run, b.run.fused_launches, b.run.ready, b.run.carried, b.run.items);
}

constexpr auto NONE = SchedLaunch::none, FROM_FIRST = SchedLaunch::first, FROM_STEADY = SchedLaunch::steady;

// an alignment that finds nothing to go by: the first launch timed, launch 1 timed, own schedule from launch 2
void check_builds_its_own(Sim &s)
{
    s.align();
    CHECK(is(s.launch(400, true), true, NONE, true, 400, 0, 0));
    CHECK(is(s.kept.first, 784, 400, 0) && is(s.run, 1, false, false, 0));
    CHECK(is(s.launch(400, false), true, NONE, true, 400, 0, 0));
    CHECK(is(s.kept.steady, 440, 400, 0) && is(s.kept.first, 784, 400, 0) && is(s.run, 2, true, false, 440));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400));
    CHECK(is(s.kept.steady, 440, 400, 0) && is(s.kept.first, 784, 400, 0) && is(s.run, 4, true, false, 440));
}

void test_fresh_then_kept_then_expired()
{
    Sim s = fresh();
    CHECK(s.kept.cap_tiles == 1000 && is(s.kept.steady, 0, 0, 0) && is(s.kept.first, 0, 0, 0));
    check_builds_its_own(s);   // alignment 0
    for (int k = 1; k <= 8; ++k) {   // alignments 1 to 8: served from the first launch on, nothing timed
        s.align();
        CHECK(is(s.launch(400, true), true, FROM_FIRST, false, 784, 784, 400));
        CHECK(is(s.kept.first, 784, 400, k) && is(s.kept.steady, 440, 400, k - 1) && is(s.run, 1, false, false, 0));
        for (int j = 1; j < 4; ++j) {
            CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400));
            CHECK(is(s.kept.first, 784, 400, k) && is(s.kept.steady, 440, 400, k) && is(s.run, j + 1, true, true, 440));
        }
    }
    check_builds_its_own(s);   // alignment 9: both have served kSchedKeepFor = 8 alignments
    s.align();                 // ... and the one after it is served again
    CHECK(is(s.launch(400, true), true, FROM_FIRST, false, 784, 784, 400));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400));
    CHECK(is(s.kept.first, 784, 400, 1) && is(s.kept.steady, 440, 400, 1));
}

// "about as many tiles" as the 400 a schedule was built for: n + n / 8 >= 400 holds from 356 (356 + 44 = 400; 355 + 44 = 399),
// 400 + 400 / 8 = 450 >= n up to 450
void test_fits_at_the_edges()
{
    CHECK(!sched_fits(355, 400) && sched_fits(356, 400) && sched_fits(357, 400));
    CHECK(sched_fits(449, 400) && sched_fits(450, 400) && !sched_fits(451, 400));
    CHECK(sched_fits(400, 400) && !sched_fits(0, 400) && !sched_fits(400, 0) && sched_fits(1, 1) && !sched_fits(7, 8) && sched_fits(8, 9) && sched_fits(9, 8));
    struct { uint32_t n; bool served; } const cases[] = {{355, false}, {356, true}, {357, true}, {449, true}, {450, true}, {451, false}};
    for (const auto &c : cases) {
        Sim s = fresh();
        check_builds_its_own(s);
        s.align();
        const SchedLaunch l0 = s.launch(c.n, true), l1 = s.launch(c.n, false);
        const uint32_t extra = c.n > 400 ? c.n - 400 : 0;
        if (c.served) {
            CHECK(is(l0, true, FROM_FIRST, false, 784 + extra, 784, 400) && is(l1, true, FROM_STEADY, false, 440 + extra, 440, 400));
            CHECK(is(s.kept.first, 784, 400, 1) && is(s.kept.steady, 440, 400, 1) && is(s.run, 2, true, true, 440 + extra));
        } else {   // timed afresh, and the schedules are this source's from here on
            CHECK(is(l0, true, NONE, true, c.n, 0, 0) && is(l1, true, NONE, true, c.n, 0, 0));
            CHECK(is(s.kept.first, FIRST(c.n), c.n, 0) && is(s.kept.steady, STEADY(c.n), c.n, 0) && is(s.run, 2, true, false, STEADY(c.n)));
            CHECK(is(s.launch(c.n, false), true, FROM_STEADY, false, STEADY(c.n), STEADY(c.n), c.n));
        }
    }
}

void test_fewer_and_more_tiles_than_kept()
{
    Sim s = fresh();
    check_builds_its_own(s);
    s.align();   // fewer: the kept items, no extras (the items of the tiles that are missing do nothing)
    CHECK(is(s.launch(380, true), true, FROM_FIRST, false, 784, 784, 400));
    CHECK(is(s.launch(380, false), true, FROM_STEADY, false, 440, 440, 400));
    CHECK(is(s.launch(380, false), true, FROM_STEADY, false, 440, 440, 400) && is(s.run, 3, true, true, 440));
    s.align();   // more: tiles 400 .. 429 behind the kept items
    CHECK(is(s.launch(430, true), true, FROM_FIRST, false, 814, 784, 400));
    CHECK(is(s.launch(430, false), true, FROM_STEADY, false, 470, 440, 400));
    CHECK(is(s.launch(430, false), true, FROM_STEADY, false, 470, 440, 400) && is(s.run, 3, true, true, 470));
    CHECK(is(s.kept.first, 784, 400, 2) && is(s.kept.steady, 440, 400, 2));
}

void test_ineligible_launches()
{
    for (int which = 0; which < 5; ++which) {
        for (int kept = 0; kept < 2; ++kept) {   // with nothing kept, and with both schedules kept and an alignment under way
            Sim s = fresh(1, 100, which == 1 ? (1u << 24) + 8u : 1000u);
            if (kept) {
                check_builds_its_own(s);
                s.align();
                (void)s.launch(400, true);
            }
            uint32_t n = 400;
            if (which == 0) n = 99;                 // fewer than min_tiles
            if (which == 1) n = 1u << 24;           // an item has 24 bits for its tile
            if (which == 2) n = 1001;               // more than the buffer was laid out for
            if (which == 3) s.stamps = true;        // per-wave stamps
            if (which == 4) s.cfg.on = false;
            const Sim before = s;
            for (int restart = 0; restart < 2; ++restart) {
                CHECK(is(sched_next(s.cfg, s.kept, s.run, n, restart != 0, s.stamps), false, NONE, false, n, 0, 0));
                CHECK(same(s, before));
            }
        }
    }
    Sim s = fresh(1, 100);   // the limits themselves are eligible
    CHECK(is(s.launch(100, true), true, NONE, true, 100, 0, 0));
    CHECK(is(s.launch(1000, true), true, NONE, true, 1000, 0, 0));
    s = fresh(1, 1, 1u << 24);
    CHECK(is(s.launch((1u << 24) - 1u, true), true, NONE, true, (1u << 24) - 1u, 0, 0));
}

void test_the_timed_launch()
{
    Sim s = fresh(0);   // at = 0: both schedules from the timed first launch
    s.align();
    CHECK(is(s.launch(400, true), true, NONE, true, 400, 0, 0));
    CHECK(is(s.kept.first, 784, 400, 0) && is(s.kept.steady, 440, 400, 0) && is(s.run, 1, true, false, 440));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400));
    s.align();
    CHECK(is(s.launch(400, true), true, FROM_FIRST, false, 784, 784, 400));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400) && is(s.run, 2, true, true, 440));

    s = fresh(2);   // at = 2: launch 2 is the timed one, launch 1 plain
    s.align();
    CHECK(is(s.launch(400, true), true, NONE, true, 400, 0, 0));
    CHECK(is(s.launch(400, false), true, NONE, false, 400, 0, 0) && is(s.kept.steady, 0, 0, 0) && is(s.run, 2, false, false, 0));
    CHECK(is(s.launch(400, false), true, NONE, true, 400, 0, 0) && is(s.kept.steady, 440, 400, 0) && is(s.run, 3, true, false, 440));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400));
    s.align();      // ... and a kept schedule is carried from launch 2 on
    CHECK(is(s.launch(400, true), true, FROM_FIRST, false, 784, 784, 400));
    CHECK(is(s.launch(400, false), true, NONE, false, 400, 0, 0) && is(s.kept.steady, 440, 400, 0) && is(s.run, 2, false, false, 0));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400) && is(s.kept.steady, 440, 400, 1) && is(s.run, 3, true, true, 440));
}

// a first launch that is not the unseeded one (the hash index, or a transform still pending): the first-launch schedule is
// neither consulted nor aged, and with at = 1 launch 0 is neither carried nor timed
void test_first_launch_that_is_no_restart()
{
    Sim s = fresh();
    check_builds_its_own(s);
    s.align();
    CHECK(is(s.launch(400, false), true, NONE, false, 400, 0, 0));
    CHECK(is(s.kept.first, 784, 400, 0) && is(s.kept.steady, 440, 400, 0) && is(s.run, 1, false, false, 0));
    CHECK(is(s.launch(400, false), true, FROM_STEADY, false, 440, 440, 400));
    CHECK(is(s.kept.first, 784, 400, 0) && is(s.kept.steady, 440, 400, 1) && is(s.run, 2, true, true, 440));
    Sim t = fresh();   // nothing kept: launch 0 plain, launch 1 timed, no first-launch schedule ever
    t.align();
    CHECK(is(t.launch(400, false), true, NONE, false, 400, 0, 0));
    CHECK(is(t.launch(400, false), true, NONE, true, 400, 0, 0));
    CHECK(is(t.launch(400, false), true, FROM_STEADY, false, 440, 440, 400) && is(t.kept.first, 0, 0, 0) && is(t.kept.steady, 440, 400, 0));
}

void test_regrown_buffer()
{
    Sim s = fresh();
    check_builds_its_own(s);
    s.align();
    (void)s.launch(400, true);
    (void)s.launch(400, false);
    sched_regrown(s.kept, 2000);
    CHECK(s.kept.cap_tiles == 2000 && is(s.kept.steady, 0, 0, 0) && is(s.kept.first, 0, 0, 0));
    check_builds_its_own(s);
}

void test_layout()
{
    const uint32_t caps[] = {1, 7, 2344, (1u << 24) - 1u};
    for (uint32_t cap : caps) {
        const SchedLayout l = sched_layout(cap);
        const size_t t = cap;
        // items and items_first: 4 words per tile, the most n + 3 n4 + n2 can reach with n4 + n2 <= n (f2 <= 1 - f4);
        // cost: one word per wave of a tile, two; done: one
        const size_t lo[4] = {l.items, l.cost, l.done, l.items_first}, len[4] = {4 * t, 2 * t, t, 4 * t};
        for (int a = 0; a < 4; ++a) {
            CHECK(lo[a] + len[a] <= l.words);
            for (int b = a + 1; b < 4; ++b) CHECK(lo[a] + len[a] <= lo[b] || lo[b] + len[b] <= lo[a]);
        }
        CHECK(l.words == 11 * t);
        CHECK(sched_capacity(l.words * 4) == cap && sched_capacity(l.words * 4 + 43) == cap && sched_capacity(l.words * 4 - 1) == cap - 1);
    }
    static_assert(kSchedCostWords == 2 && kSchedKeepFor == 8, "the figures the cases above are written for");
    CHECK(sched_capacity(0) == 0);
}

void test_random_walk()
{
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto rnd = [&x](uint32_t below) {   // (xorshift64*)
        x ^= x >> 12;
        x ^= x << 25;
        x ^= x >> 27;
        return (uint32_t)(((x * 0x2545f4914f6cdd1dull) >> 33) % below);
    };
    Sim s = fresh(1, 300, 600);
    uint32_t n = 400;
    int served = 0, timed = 0, plain = 0;
    for (int k = 0; k < 10000; ++k) {
        bool restart = false;
        if (rnd(5) == 0) {   // a new alignment, mostly of about as many tiles
            s.align();
            s.cfg.at_launch = (int)rnd(3);
            s.stamps = rnd(40) == 0;
            n = rnd(6) == 0 ? 250 + rnd(400) : (uint32_t)((int)n + (int)rnd(41) - 20);
            if (n < 250 || n > 650) n = 400;
            if (rnd(50) == 0) sched_regrown(s.kept, 500 + rnd(200));
            restart = rnd(4) != 0;
        }
        const SchedRun before = s.run;
        const SchedLaunch l = s.launch(n, restart);
        CHECK(!(l.timed && l.from != NONE));
        if (l.from != NONE) {
            CHECK(l.eligible && l.grid == l.n_items + (n > l.first_extra ? n - l.first_extra : 0u));
            CHECK(l.n_items == (l.from == FROM_FIRST ? s.kept.first.items : s.kept.steady.items));
        } else {
            CHECK(l.grid == n && l.n_items == 0 && l.first_extra == 0);
        }
        CHECK(l.n_items <= 4 * s.kept.cap_tiles && (l.eligible || !l.timed));
        CHECK(s.kept.first.age <= kSchedKeepFor && s.kept.steady.age <= kSchedKeepFor && s.kept.first.tiles <= s.kept.cap_tiles && s.kept.steady.tiles <= s.kept.cap_tiles);
        CHECK(s.run.fused_launches == before.fused_launches + 1 && (s.run.ready || !before.ready));
        served += l.from != NONE;
        timed += l.timed;
        plain += !l.timed && l.from == NONE;
    }
    CHECK(served > 1000 && timed > 100 && plain > 100);   // (the walk reaches every kind of launch)
}

}  // namespace

int main()
{
    test_fresh_then_kept_then_expired();
    test_fits_at_the_edges();
    test_fewer_and_more_tiles_than_kept();
    test_ineligible_launches();
    test_the_timed_launch();
    test_first_launch_that_is_no_restart();
    test_regrown_buffer();
    test_layout();
    test_random_walk();
    std::printf("tile schedule rule ok\n");
    return 0;
}
