// sac_plan.hpp — how the scoring of RANSAC hypotheses against a correspondence list is cut into workgroups (sac.hip,
// sac_kernels.hpp), and how many hypotheses a launch scores: the host-only rules.  Plain C++, no HIP: tests/cpp/
// sac_plan_rule.cpp includes this header alone.
//
// A workgroup of kSacBlock lanes owns ONE tile of kSacTile pairs (kSacPairsPerLane a lane, in registers) and walks ONE slice of
// the hypothesis table in chunks of kSacChunk rows.  A slice is one chunk unless (tiles) x (chunks) would pass kSacMaxGroups
// workgroups; then a slice takes as many chunks as keeps the grid under kSacMaxGroups + tiles.  The counts are integers added
// by integer atomics, so the rules decide speed only: the bytes do not depend on them.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSREG_SAC_HD __host__ __device__
#else
#define RSREG_SAC_HD
#endif

namespace rsreg {

constexpr uint32_t kSacBlock = 256;                               // lanes of a workgroup: four waves
constexpr uint32_t kSacPairsPerLane = 2;
constexpr uint32_t kSacTile = kSacBlock * kSacPairsPerLane;       // pairs of a workgroup
constexpr uint32_t kSacChunk = 64;                                // hypotheses between two flushes of a wave's counts: one a lane
constexpr uint32_t kSacMaxGroups = 4096;                          // sixteen workgroups a CU before a slice grows
constexpr uint32_t kSacFirstBatch = 256, kSacMaxBatch = 4096;     // hypotheses of the rejector's first launch, of any launch at most
constexpr uint32_t kSacTries = 16;                                // draws of three pairs a hypothesis may make

struct SacPlan {
    uint32_t tiles = 0;          // ceil(n / kSacTile)
    uint32_t chunks = 0;         // ceil(H / kSacChunk)
    uint32_t slice_chunks = 0;   // chunks of a slice (>= 1)
    uint32_t slices = 0;         // ceil(chunks / slice_chunks)
};

// n >= 1 pairs, H >= 1 hypotheses (both below 2^31).  Workgroup b of tiles * slices scores tile b % tiles against the
// hypotheses [slice * slice_chunks * kSacChunk, min(H, (slice + 1) * slice_chunks * kSacChunk)), slice = b / tiles: every
// (tile, hypothesis) once.  tiles * slices <= kSacMaxGroups + tiles: one launch dimension holds it.
inline SacPlan sac_plan(uint32_t n, uint32_t H)
{
    SacPlan p;
    p.tiles = (uint32_t)(((unsigned long long)n + kSacTile - 1) / kSacTile);
    p.chunks = (uint32_t)(((unsigned long long)H + kSacChunk - 1) / kSacChunk);
    const unsigned long long cells = (unsigned long long)p.tiles * p.chunks;
    unsigned long long per = (cells + kSacMaxGroups - 1) / kSacMaxGroups;
    if (per < 1) per = 1;
    if (per > p.chunks) per = p.chunks;
    p.slice_chunks = (uint32_t)per;
    p.slices = p.slice_chunks ? (p.chunks + p.slice_chunks - 1) / p.slice_chunks : 0;
    return p;
}

// what workgroup b of the launch owns: its tile of the pairs ...
RSREG_SAC_HD inline uint32_t sac_group_tile(uint32_t b, uint32_t tiles) { return b % tiles; }
// ... and the hypotheses [*first, *past) of its slice
RSREG_SAC_HD inline void sac_group_slice(uint32_t b, uint32_t tiles, uint32_t slice_chunks, uint32_t H, uint32_t *first, uint32_t *past)
{
    const unsigned long long len = (unsigned long long)slice_chunks * kSacChunk, a = (unsigned long long)(b / tiles) * len, e = a + len;
    *first = (uint32_t)(a < H ? a : H);
    *past = (uint32_t)(e < H ? e : H);
}

// the hypotheses of the rejector's next launch when `done` have been scored and `max_iterations` is the most it may consume:
// kSacFirstBatch, then twice the last, at most kSacMaxBatch and never past max_iterations.  The stopping rule is replayed over
// the counts in hypothesis order, so the batches decide speed only.
inline uint32_t sac_batch(uint32_t done, uint32_t max_iterations)
{
    if (done >= max_iterations) return 0;
    unsigned long long b = kSacFirstBatch, start = 0;
    while (start + b <= done) {   // (the batches so far: 256, 512, 1024, 2048, 4096, 4096, ...)
        start += b;
        if (b < kSacMaxBatch) b *= 2;
    }
    const unsigned long long left = max_iterations - done;
    return (uint32_t)(b < left ? b : left);
}

}  // namespace rsreg
