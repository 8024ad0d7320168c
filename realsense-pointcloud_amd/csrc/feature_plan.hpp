// feature_plan.hpp — how a brute-force search in descriptor space is cut into workgroups (features.hip, feature_kernels.hpp):
// the host-only rule that turns (queries, target rows) into (query blocks) x (target slices).  Plain C++, no HIP: tests/cpp/
// feature_plan_rule.cpp includes this header alone.
//
// A workgroup is ONE wave whose lanes own kFmQueries query rows and walk one slice of the target in tiles of kFmTile rows.  With
// many queries one slice is enough; with few (a handful of key points against a whole frame) the target is cut so that the grid
// fills the 256 CUs kFmFill / 256 times over, and never finer than one tile a slice.  The slices' results merge by the minimum
// of unique (d2, index) keys, so the rule decides speed only: the bytes do not depend on it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSREG_FM_HD __host__ __device__
#else
#define RSREG_FM_HD
#endif

namespace rsreg {

constexpr uint32_t kFmQueries = 64;        // query rows of a workgroup: one a lane
constexpr uint32_t kFmTile = 64;           // target rows staged in LDS at a time
constexpr uint32_t kFmFill = 256 * 8;      // workgroups the grid aims for: eight a CU

struct FeaturePlan {
    uint32_t qblocks = 0;   // ceil(queries / kFmQueries)
    uint32_t slices = 0;    // the target is cut into so many pieces (>= 1)
};

// rows [feature_slice_begin(s), feature_slice_begin(s + 1)) are slice s of `slices` over nt rows: they tile [0, nt) without a gap
// or an overlap, and each holds at least floor(nt / slices) rows
RSREG_FM_HD inline uint32_t feature_slice_begin(uint32_t s, uint32_t slices, uint32_t nt)
{
    return (uint32_t)((unsigned long long)s * nt / slices);
}

// nq >= 1 queries against nt target rows (both below 2^31).  slices <= max(1, nt / kFmTile): a slice is never shorter than one
// tile unless the whole target is.  qblocks * slices stays below 2^26 + kFmFill: one launch dimension holds it, uncapped.
inline FeaturePlan feature_plan(uint32_t nq, uint32_t nt)
{
    FeaturePlan p;
    p.qblocks = (nq + kFmQueries - 1) / kFmQueries;
    const uint32_t want = p.qblocks ? (kFmFill + p.qblocks - 1) / p.qblocks : 1u;
    const uint32_t most = nt / kFmTile > 1u ? nt / kFmTile : 1u;
    p.slices = want < most ? want : most;
    if (p.slices < 1u) p.slices = 1u;
    return p;
}

}  // namespace rsreg
