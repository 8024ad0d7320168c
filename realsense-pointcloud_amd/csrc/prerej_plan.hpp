// prerej_plan.hpp — how the scoring of pose hypotheses against a whole target cloud is cut into workgroups (prerej.hip,
// prerej_kernels.hpp), and how many hypotheses a launch scores: the host-only rules.  Plain C++, no HIP: tests/cpp/
// prerej_plan_rule.cpp includes this header alone.
//
// A workgroup of kPrejBlock lanes owns ONE tile of kPrejTile source records (one a lane, in registers): one group of the sum tree
// of include/rsreg.h, its two waves the group's two waves.  It walks ONE slice of the hypothesis table in chunks of kPrejChunk rows.
// A slice is one chunk unless (tiles) x (chunks) would pass kPrejMaxGroups workgroups; then a slice takes as many chunks as keeps
// the grid under kPrejMaxGroups + tiles.  The counts are integers added by integer atomics and every d2 sum has one writer and a
// place of its own, so the rules decide speed only: the bytes do not depend on them.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSREG_PREJ_HD __host__ __device__
#else
#define RSREG_PREJ_HD
#endif

namespace rsreg {

constexpr uint32_t kPrejBlock = 128;                              // lanes of a workgroup: two waves
constexpr uint32_t kPrejTile = kPrejBlock;                        // source records of a workgroup: one group of the sum tree
constexpr uint32_t kPrejChunk = 16;                               // hypotheses between two flushes of a wave's counts: one a lane
constexpr uint32_t kPrejMaxGroups = 1u << 20;                     // workgroups of a launch before a slice grows
constexpr uint32_t kPrejMaxBatch = 256;                           // hypotheses of a launch at most
constexpr uint32_t kPrejRound = 16384;                            // hypotheses between two waits of the host at most (whole batches)
constexpr unsigned long long kPrejPartialBytes = 32ull << 20;     // the partials of a launch stay under this (one hypothesis: whatever it takes)
constexpr uint32_t kPrejPartialStride = 16;                       // bytes of a (hypothesis, group): two doubles, one a wave

struct PrejPlan {
    uint32_t tiles = 0;          // ceil(n / kPrejTile): the groups of the sum tree
    uint32_t chunks = 0;         // ceil(H / kPrejChunk)
    uint32_t slice_chunks = 0;   // chunks of a slice (>= 1)
    uint32_t slices = 0;         // ceil(chunks / slice_chunks)
};

// n >= 1 source records, H >= 1 hypotheses (both below 2^31).  Workgroup b of tiles * slices scores tile b % tiles against the
// hypotheses [slice * slice_chunks * kPrejChunk, min(H, (slice + 1) * slice_chunks * kPrejChunk)), slice = b / tiles: every
// (tile, hypothesis) once.  tiles * slices <= kPrejMaxGroups + tiles < 2^31: one launch dimension holds it.
inline PrejPlan prerej_plan(uint32_t n, uint32_t H)
{
    PrejPlan p;
    p.tiles = (uint32_t)(((unsigned long long)n + kPrejTile - 1) / kPrejTile);
    p.chunks = (uint32_t)(((unsigned long long)H + kPrejChunk - 1) / kPrejChunk);
    const unsigned long long cells = (unsigned long long)p.tiles * p.chunks;
    unsigned long long per = (cells + kPrejMaxGroups - 1) / kPrejMaxGroups;
    if (per < 1) per = 1;
    if (per > p.chunks) per = p.chunks;
    p.slice_chunks = (uint32_t)per;
    p.slices = p.slice_chunks ? (p.chunks + p.slice_chunks - 1) / p.slice_chunks : 0;
    return p;
}

// what workgroup b of the launch owns: its tile of the source ...
RSREG_PREJ_HD inline uint32_t prerej_group_tile(uint32_t b, uint32_t tiles) { return b % tiles; }
// ... and the hypotheses [*first, *past) of its slice
RSREG_PREJ_HD inline void prerej_group_slice(uint32_t b, uint32_t tiles, uint32_t slice_chunks, uint32_t H, uint32_t *first, uint32_t *past)
{
    const unsigned long long len = (unsigned long long)slice_chunks * kPrejChunk, a = (unsigned long long)(b / tiles) * len, e = a + len;
    *first = (uint32_t)(a < H ? a : H);
    *past = (uint32_t)(e < H ? e : H);
}

// the hypotheses a launch scores at most against n >= 1 source records: kPrejMaxBatch, fewer where their partials (one
// kPrejPartialStride per group of the source) would pass kPrejPartialBytes, one at the least
inline uint32_t prerej_batch_cap(uint32_t n)
{
    const unsigned long long groups = ((unsigned long long)n + kPrejTile - 1) / kPrejTile;
    unsigned long long b = kPrejPartialBytes / (groups * kPrejPartialStride);
    if (b > kPrejMaxBatch) b = kPrejMaxBatch;
    return (uint32_t)(b < 1 ? 1 : b);
}

// the hypotheses of the next launch when `done` of `total` have been queued.  Every hypothesis is a function of its number and
// every output has a place of its own, so the batches decide speed only.
inline uint32_t prerej_batch(uint32_t n, unsigned long long done, unsigned long long total)
{
    if (done >= total) return 0;
    const unsigned long long left = total - done, cap = prerej_batch_cap(n);
    return (uint32_t)(cap < left ? cap : left);
}

}  // namespace rsreg
