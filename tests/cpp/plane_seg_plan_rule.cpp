// plane_seg_plan_rule — the host-only rules of csrc/plane_seg_plan.hpp, which cut the scoring of plane hypotheses into (record
// tiles) x (hypothesis slices), the hypotheses of a segmentation into batches, and replay PCL's stopping rule with its skip
// counter; tabulated for tests/test_plane_seg_cpu.py.  Includes that header alone: plain C++, no HIP, no GPU.
//   plane_seg_plan_rule < lines.txt      "plan n H", "cover n H", "batches max_iterations" or "replay ..." a line
// prints "constants <block> <records per lane> <tile> <chunk> <max groups> <first batch> <max batch> <tries>" first, then a line a line:
//   plan n H tiles chunks slice_chunks slices
//   cover n H groups bad     walks every workgroup of the launch and marks the (tile, chunk) cells it owns; bad = cells not
//                            marked exactly once + workgroups with an empty or a ragged-inside slice
//   batches max_iterations b0 b1 ...      (at most 64 are printed, then "..." and their number and sum)
//   replay n probability max_iterations L v0 c0 v1 c1 ..   ->   replay best winner iterations skipped consumed ran_out
//                            feeds PlaneReplay the L (valid, count) pairs while it wants more; ran_out = it still wanted more
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../realsense-pointcloud_amd/csrc/plane_seg_plan.hpp"

int main()
{
    using namespace rsreg;
    std::printf("constants %u %u %u %u %u %u %u %u\n", kPlaneBlock, kPlaneRecordsPerLane, kPlaneTile, kPlaneChunk, kPlaneMaxGroups, kSacFirstBatch, kPlaneMaxBatch,
                kPlaneTries);
    char what[32];
    unsigned long long a = 0, b = 0;
    while (std::scanf("%31s", what) == 1) {
        if (!std::strcmp(what, "batches")) {
            if (std::scanf("%llu", &a) != 1) return 2;
            std::printf("batches %llu", a);
            uint32_t done = 0, count = 0;
            for (uint32_t B; (B = plane_batch(done, (uint32_t)a)) != 0; done += B)
                if (count++ < 64) std::printf(" %u", B);
            std::printf(" ... %u %u\n", count, done);
            continue;
        }
        if (!std::strcmp(what, "replay")) {
            unsigned long long n = 0, max_it = 0, L = 0;
            double probability = 0;
            if (std::scanf("%llu %lf %llu %llu", &n, &probability, &max_it, &L) != 4) return 2;
            PlaneReplay rp(n, probability, max_it);
            for (unsigned long long i = 0; i < L; ++i) {
                unsigned v = 0, c = 0;
                if (std::scanf("%u %u", &v, &c) != 2) return 2;
                if (rp.wants_more()) rp.feed(v != 0, c);
            }
            std::printf("replay %lld %lld %llu %llu %llu %d\n", rp.best, rp.winner, rp.it, rp.skipped, rp.next, rp.wants_more() ? 1 : 0);
            continue;
        }
        if (std::scanf("%llu %llu", &a, &b) != 2) return 2;
        const PlanePlan p = plane_plan((uint32_t)a, (uint32_t)b);
        if (!std::strcmp(what, "plan")) {
            std::printf("plan %llu %llu %u %u %u %u\n", a, b, p.tiles, p.chunks, p.slice_chunks, p.slices);
            continue;
        }
        std::vector<uint8_t> seen((size_t)p.tiles * p.chunks, 0);
        unsigned long long bad = 0;
        const uint32_t groups = p.tiles * p.slices;
        for (uint32_t g = 0; g < groups; ++g) {
            uint32_t first, past;
            plane_group_slice(g, p.tiles, p.slice_chunks, (uint32_t)b, &first, &past);
            const uint32_t tile = plane_group_tile(g, p.tiles);
            if (first >= past || first % kPlaneChunk || tile >= p.tiles) ++bad;
            for (uint32_t h = first; h < past; h += kPlaneChunk) {
                uint8_t &cell = seen[(size_t)tile * p.chunks + h / kPlaneChunk];
                if (cell < 2) ++cell;
            }
        }
        for (uint8_t c : seen) bad += c != 1;
        std::printf("cover %llu %llu %u %llu\n", a, b, groups, bad);
    }
    return 0;
}
