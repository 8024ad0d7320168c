// feature_plan_rule — the host-only rule of csrc/feature_plan.hpp, which cuts a brute-force descriptor search into (query blocks) x
// (target slices), tabulated for tests/test_feature_match_cpu.py.  Includes that header alone: plain C++, no HIP, no GPU.
//   feature_plan_rule < pairs.txt        one "nq nt" a line
// prints, a line a pair: nq nt qblocks slices begin(0) begin(1) ... begin(slices)
// and "constants <queries> <tile> <fill>" first.
#include <cinttypes>
#include <cstdio>

#include "../../realsense-pointcloud_amd/csrc/feature_plan.hpp"

int main()
{
    std::printf("constants %u %u %u\n", rsreg::kFmQueries, rsreg::kFmTile, rsreg::kFmFill);
    unsigned long long nq = 0, nt = 0;
    while (std::scanf("%llu %llu", &nq, &nt) == 2) {
        const rsreg::FeaturePlan p = rsreg::feature_plan((uint32_t)nq, (uint32_t)nt);
        std::printf("%llu %llu %u %u", nq, nt, p.qblocks, p.slices);
        for (uint32_t s = 0; s <= p.slices; ++s) std::printf(" %u", rsreg::feature_slice_begin(s, p.slices, (uint32_t)nt));
        std::printf("\n");
    }
    return 0;
}
