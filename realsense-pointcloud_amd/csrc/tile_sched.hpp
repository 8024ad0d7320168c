// tile_sched.hpp — the host side of the fused dense search's tile schedule: the kernel argument, where the arrays lie in
// the context's schedule buffer, what a context and an alignment remember of it, and the rule that says what the next
// launch is.  No GPU call in here and nothing of the context: plain structs and functions of them, so that the rule can be
// read in one place and run without a GPU (tests/cpp/tile_sched_rule.cpp).  icp.hip builds the schedules (build_schedule,
// k_sched_build) and launches from them (launch_fused).
//
// A launch of ~14 k waves on 8 k wave slots ends with a long tail: a few waves run 3x longer than the mean, they all sit on
// the same (near, densely sampled) surfaces in every iteration, and nothing is left to fill the slots around them.  One
// launch of an alignment times every wave; from then on the tiles are launched longest first, and the longest few per cent
// are searched by 2 or 4 lanes per query.  What is summed, and in which order, does not change.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rsreg {

// How the workgroups of a fused launch map to tiles (icp.hip: build_schedule).  All null: workgroup b is tile b.
// With a schedule, the tiles that took longest in an earlier iteration come first, and the longest of
// them are split: 2 or 4 workgroups share the tile's 128 queries, 2 or 4 lanes search each query (DSplit),
// and whichever of those workgroups finishes last adds up the tile's 17 sums in the usual order.
struct TileSched {
    const uint32_t *items;   // per workgroup: tile | part << 24 | log2(lanes per query) << 28
    uint32_t *cost;          // per wave of an unsplit tile: how long it ran in this launch (100 MHz ticks), or null
    uint32_t *done;          // per tile: parts finished so far (split tiles; goes back to 0 by itself)
    int *pos;                // per query: where the parts of a split tile leave their matches
    float *d2;
    uint32_t n_tiles;        // slabs of `partials`
    // A schedule carried over from an earlier alignment of this context (sched_next below) was built for another source:
    // workgroups [0, n_items) take its items -- those of tiles this source does not have do nothing --, the workgroups
    // behind them the tiles it did not know, first_extra + 0, 1, ..., unsplit.  (A schedule of this alignment's own: n_items =
    // the grid, no extras.)
    uint32_t n_items, first_extra;
};

struct SchedCfg {
    bool on = true;
    double f4 = 0.0, f2 = 0.10;    // fractions of the tiles searched with 4 and with 2 lanes per query (swept on the bench pair)
    uint32_t min_tiles = 1024;     // below this a launch does not even fill the wave slots once
    int at_launch = 1;             // the launch that is timed (0 = the first, which runs without seeds)
};

constexpr int kSchedKeepFor = 8;         // alignments a tile schedule serves before a launch is timed again
constexpr uint32_t kSchedCostWords = 2;  // cost words per tile: one per wave of a tile (icp.hip ties it to kTileWaves)
constexpr uint32_t kSchedMaxTiles = 1u << 24;   // an item has 24 bits for its tile

// Where the arrays lie in the schedule buffer, in uint32 words, for a buffer laid out for cap_tiles tiles.  The offsets
// depend on the capacity only, never on the source at hand: the arrays stay put from one alignment to the next, which is
// what lets a schedule serve a later alignment.  items, items_first: the workgroups of the steady and of the first-launch
// schedule, 4 per tile (n + 3 n4 + n2 with n4 + n2 <= n); cost: the timed launch's stamps; done: the split tiles' counters.
struct SchedLayout {
    size_t items, cost, done, items_first, words;
};
constexpr SchedLayout sched_layout(uint32_t cap_tiles)
{
    const size_t t = cap_tiles;
    return SchedLayout{0, 4 * t, (4 + kSchedCostWords) * t, (5 + kSchedCostWords) * t, (9 + kSchedCostWords) * t};
}
constexpr uint32_t sched_capacity(size_t bytes) { return (uint32_t)(bytes / (sched_layout(1).words * 4)); }   // tiles a buffer of so many bytes holds

// A schedule that lies built in the buffer
struct KeptSched {
    uint32_t items = 0;   // its workgroups (0: none)
    uint32_t tiles = 0;   // tiles of the source it was built for
    int age = 0;          // alignments it has served since
};

// What a context remembers.  The FIRST launch of an alignment (unseeded, from the source itself under the guess: the only
// launch the reference's parameters ever run) has a cost profile of its own: it is timed once and scheduled from its own
// kind's costs in the alignments that follow, beside the steady schedule of the launches behind it.
struct SchedKept {
    uint32_t cap_tiles = 0;   // tiles the buffer was laid out for
    KeptSched steady, first;
};

// ... and an alignment
struct SchedRun {
    int fused_launches = 0;   // fused dense launches of this alignment so far
    bool ready = false;       // the buffer holds a steady schedule for this alignment
    bool carried = false;     // ... which an earlier alignment of the context built
    uint32_t items = 0;       // workgroups of a launch from it
};

struct SchedLaunch {
    enum From { none, first, steady };
    bool eligible;         // a schedule is possible at all: the launch gets the done / pos / d2 pointers
    From from;             // whose items it runs from
    bool timed;            // it gets the cost pointer, and a schedule is built from it
    uint32_t grid;         // workgroups
    uint32_t n_items, first_extra;   // TileSched's
};

// "about as many tiles": a schedule serves a source whose tile count is within an eighth of its own
constexpr bool sched_fits(uint32_t n_tiles, uint32_t kept_tiles) { return n_tiles + n_tiles / 8 >= kept_tiles && kept_tiles + kept_tiles / 8 >= n_tiles; }

// A new buffer: laid out for so many tiles, and without a schedule.
inline void sched_regrown(SchedKept &c, uint32_t cap_tiles) { c = SchedKept{cap_tiles, {}, {}}; }

// What the next fused launch over n_tiles tiles is.  restart_here: it is the alignment's first, unseeded launch;
// stamps_forbid: per-wave diagnostic stamps are on, whose layout knows no schedule.
// The schedule of an earlier alignment of this context serves this one too, from the launch that would otherwise be timed:
// the long tiles sit on the same surfaces from one frame to the next, a schedule is an order of work and never wrong, and
// the timed launch runs unscheduled (140 against 93 us at 10^6 points).  Kept for at most kSchedKeepFor alignments and only
// for a source of about as many tiles.
inline SchedLaunch sched_next(const SchedCfg &cfg, SchedKept &c, SchedRun &s, uint32_t n_tiles, bool restart_here, bool stamps_forbid)
{
    SchedLaunch l{false, SchedLaunch::none, false, n_tiles, 0, 0};
    l.eligible = cfg.on && !stamps_forbid && n_tiles >= cfg.min_tiles && n_tiles < kSchedMaxTiles && n_tiles <= c.cap_tiles;
    if (!l.eligible) return l;
    auto serves = [&](const KeptSched &k) { return k.items && k.age < kSchedKeepFor && sched_fits(n_tiles, k.tiles); };
    auto with_extras = [&](const KeptSched &k) { return k.items + (n_tiles > k.tiles ? n_tiles - k.tiles : 0u); };   // (the tiles it does not know run behind, unsplit)
    if (restart_here && serves(c.first)) {
        ++c.first.age;
        l.from = SchedLaunch::first;
        l.grid = with_extras(c.first);
        l.n_items = c.first.items;
        l.first_extra = c.first.tiles;
        return l;
    }
    if (!restart_here && !s.ready && s.fused_launches >= cfg.at_launch && serves(c.steady)) {
        s.ready = s.carried = true;
        s.items = with_extras(c.steady);
        ++c.steady.age;
    }
    if (s.ready) {
        l.from = SchedLaunch::steady;
        l.grid = s.items;
        l.n_items = s.carried ? c.steady.items : s.items;
        l.first_extra = c.steady.tiles;
    } else {
        l.timed = restart_here || s.fused_launches == cfg.at_launch;
    }
    return l;
}

// A schedule of `items` workgroups has just been built from a timed launch over n_tiles tiles (first: the first-launch one).
inline void sched_built(SchedKept &c, SchedRun &s, bool first, uint32_t items, uint32_t n_tiles)
{
    (first ? c.first : c.steady) = KeptSched{items, n_tiles, 0};
    if (first) return;
    s.ready = true;
    s.items = items;
}

}  // namespace rsreg
