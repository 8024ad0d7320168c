// sac_plan_rule — the host-only rules of csrc/sac_plan.hpp, which cut the scoring of RANSAC hypotheses into (pair tiles) x
// (hypothesis slices) and the rejector's hypotheses into batches, tabulated for tests/test_sac_cpu.py.  Includes that header
// alone: plain C++, no HIP, no GPU.
//   sac_plan_rule < lines.txt      "plan n H", "cover n H" or "batches max_iterations" a line
// prints "constants <block> <pairs per lane> <tile> <chunk> <max groups> <first batch> <max batch> <tries>" first, then a line a line:
//   plan n H tiles chunks slice_chunks slices
//   cover n H groups bad     walks every workgroup of the launch and marks the (tile, chunk) cells it owns; bad = cells not
//                            marked exactly once + workgroups with an empty or a ragged-inside slice
//   batches max_iterations b0 b1 ...
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../realsense-pointcloud_amd/csrc/sac_plan.hpp"

int main()
{
    using namespace rsreg;
    std::printf("constants %u %u %u %u %u %u %u %u\n", kSacBlock, kSacPairsPerLane, kSacTile, kSacChunk, kSacMaxGroups, kSacFirstBatch, kSacMaxBatch, kSacTries);
    char what[32];
    unsigned long long a = 0, b = 0;
    while (std::scanf("%31s", what) == 1) {
        if (!std::strcmp(what, "batches")) {
            if (std::scanf("%llu", &a) != 1) return 2;
            std::printf("batches %llu", a);
            uint32_t done = 0;
            for (uint32_t B; (B = sac_batch(done, (uint32_t)a)) != 0; done += B) std::printf(" %u", B);
            std::printf("\n");
            continue;
        }
        if (std::scanf("%llu %llu", &a, &b) != 2) return 2;
        const SacPlan p = sac_plan((uint32_t)a, (uint32_t)b);
        if (!std::strcmp(what, "plan")) {
            std::printf("plan %llu %llu %u %u %u %u\n", a, b, p.tiles, p.chunks, p.slice_chunks, p.slices);
            continue;
        }
        std::vector<uint8_t> seen((size_t)p.tiles * p.chunks, 0);
        unsigned long long bad = 0;
        const uint32_t groups = p.tiles * p.slices;
        for (uint32_t g = 0; g < groups; ++g) {
            uint32_t first, past;
            sac_group_slice(g, p.tiles, p.slice_chunks, (uint32_t)b, &first, &past);
            const uint32_t tile = sac_group_tile(g, p.tiles);
            if (first >= past || first % kSacChunk || tile >= p.tiles) ++bad;
            for (uint32_t h = first; h < past; h += kSacChunk) {
                uint8_t &cell = seen[(size_t)tile * p.chunks + h / kSacChunk];
                if (cell < 2) ++cell;
            }
        }
        for (uint8_t c : seen) bad += c != 1;
        std::printf("cover %llu %llu %u %llu\n", a, b, groups, bad);
    }
    return 0;
}
