// plane_seg_plan.hpp — the host-only rules of the RANSAC plane segmentation (segment.hip, plane_seg_kernels.hpp; contract:
// include/rsreg.h, "plane segmentation"): how the scoring of plane hypotheses against a cloud is cut into workgroups, how many
// hypotheses a launch scores, and PCL's stopping rule with its skip counter as a state machine that is fed one hypothesis at a
// time.  Plain C++, no HIP: tests/cpp/plane_seg_plan_rule.cpp includes this header alone.
//
// The cut is sac_plan.hpp's with constants of its own: a workgroup of kPlaneBlock lanes owns ONE tile of kPlaneTile records
// (kPlaneRecordsPerLane a lane, in registers) and walks ONE slice of the hypothesis table in chunks of kPlaneChunk rows; a slice is
// one chunk unless (tiles) x (chunks) would pass kPlaneMaxGroups workgroups.  The counts are integers added by integer atomics, so
// these rules decide speed only: the bytes do not depend on them.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sac_plan.hpp"

namespace rsreg {

constexpr uint32_t kPlaneBlock = 256;                                   // lanes of a workgroup: four waves
constexpr uint32_t kPlaneRecordsPerLane = 4;                            // three registers each
constexpr uint32_t kPlaneTile = kPlaneBlock * kPlaneRecordsPerLane;     // records of a workgroup
constexpr uint32_t kPlaneChunk = 64;                                    // hypotheses between two flushes of a wave's counts: one a lane
constexpr uint32_t kPlaneMaxGroups = 4096;                              // sixteen workgroups a CU before a slice grows
constexpr uint32_t kPlaneTries = kSacTries;                             // draws of three records a hypothesis may make
constexpr uint32_t kPlaneMaxBatch = kSacMaxBatch;                       // hypotheses of any launch at most (sac_batch)
constexpr uint32_t kPlaneMaxHypotheses = 0x7ffffff0u;                   // of a whole call at most

struct PlanePlan {
    uint32_t tiles = 0;          // ceil(n / kPlaneTile)
    uint32_t chunks = 0;         // ceil(H / kPlaneChunk)
    uint32_t slice_chunks = 0;   // chunks of a slice (>= 1)
    uint32_t slices = 0;         // ceil(chunks / slice_chunks)
};

// n >= 1 records, H >= 1 hypotheses (both below 2^31).  Workgroup b of tiles * slices scores tile b % tiles against the
// hypotheses [slice * slice_chunks * kPlaneChunk, min(H, (slice + 1) * slice_chunks * kPlaneChunk)), slice = b / tiles: every
// (tile, hypothesis) once.  tiles * slices <= kPlaneMaxGroups + tiles: one launch dimension holds it.
inline PlanePlan plane_plan(uint32_t n, uint32_t H)
{
    PlanePlan p;
    p.tiles = (uint32_t)(((unsigned long long)n + kPlaneTile - 1) / kPlaneTile);
    p.chunks = (uint32_t)(((unsigned long long)H + kPlaneChunk - 1) / kPlaneChunk);
    const unsigned long long cells = (unsigned long long)p.tiles * p.chunks;
    unsigned long long per = (cells + kPlaneMaxGroups - 1) / kPlaneMaxGroups;
    if (per < 1) per = 1;
    if (per > p.chunks) per = p.chunks;
    p.slice_chunks = (uint32_t)per;
    p.slices = p.slice_chunks ? (p.chunks + p.slice_chunks - 1) / p.slice_chunks : 0;
    return p;
}

// what workgroup b of the launch owns: its tile of the records ...
RSREG_SAC_HD inline uint32_t plane_group_tile(uint32_t b, uint32_t tiles) { return b % tiles; }
// ... and the hypotheses [*first, *past) of its slice
RSREG_SAC_HD inline void plane_group_slice(uint32_t b, uint32_t tiles, uint32_t slice_chunks, uint32_t H, uint32_t *first, uint32_t *past)
{
    const unsigned long long len = (unsigned long long)slice_chunks * kPlaneChunk, a = (unsigned long long)(b / tiles) * len, e = a + len;
    *first = (uint32_t)(a < H ? a : H);
    *past = (uint32_t)(e < H ? e : H);
}

// the most hypotheses a call may score: an invalid hypothesis spends no iteration, and the replay below ends before
// max_iterations valid and 10 * max_iterations invalid ones have been consumed
inline uint32_t plane_hypothesis_cap(uint32_t max_iterations)
{
    const unsigned long long cap = 11ull * max_iterations;
    return (uint32_t)(cap < kPlaneMaxHypotheses ? cap : kPlaneMaxHypotheses);
}

// the hypotheses of the next launch when `done` have been scored: sac_batch's doubling (256, 512, .., 4096, 4096, ..), never past
// the cap above.  The replay is fed in hypothesis order, so the batches decide speed only.
inline uint32_t plane_batch(uint32_t done, uint32_t max_iterations) { return sac_batch(done, plane_hypothesis_cap(max_iterations)); }

// PCL's stopping rule (ransac.hpp), its skip counter included, in double.  wants_more(): the loop condition before hypothesis
// `next`; feed(valid, count): what that hypothesis does.  An invalid hypothesis does ++skipped and nothing else.
struct PlaneReplay {
    double n = 0, log_probability = 0, k = 1.0;
    unsigned long long max_iterations = 0, it = 0, skipped = 0, next = 0;
    long long best = -1, winner = -1;   // (best: PCL's -INT_MAX -- the first valid hypothesis always sets k)

    PlaneReplay(unsigned long long n_records, double probability, unsigned long long max_it)
        : n((double)n_records), log_probability(std::log(1.0 - probability)), max_iterations(max_it) {}

    bool wants_more() const { return (double)it < k && it < max_iterations && skipped < 10ull * max_iterations; }

    void feed(bool valid, uint32_t count)
    {
        ++next;
        if (!valid) { ++skipped; return; }
        if ((long long)count > best) {
            best = count;
            winner = (long long)next - 1;
            const double w = (double)best / n;
            double q = 1.0 - w * w * w;
            q = q < DBL_EPSILON ? DBL_EPSILON : q;
            q = q > 1.0 - DBL_EPSILON ? 1.0 - DBL_EPSILON : q;
            k = log_probability / std::log(q);
        }
        ++it;
    }
};

}  // namespace rsreg
