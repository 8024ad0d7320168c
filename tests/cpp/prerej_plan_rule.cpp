// prerej_plan_rule — the host-only rules of csrc/prerej_plan.hpp, which cut the scoring of pose hypotheses against a whole target
// cloud into (source tiles) x (hypothesis slices) and the hypotheses into batches, tabulated for tests/test_prerej_cpu.py.  Includes
// that header alone: plain C++, no HIP, no GPU.
//   prerej_plan_rule < lines.txt      "plan n H", "cover n H" or "batches n total" a line
// prints "constants <block> <tile> <chunk> <max groups> <max batch> <round> <partial bytes> <partial stride>" first, then a line a line:
//   plan n H tiles chunks slice_chunks slices
//   cover n H groups bad     walks every workgroup of the launch and marks the (tile, hypothesis) pairs it owns; bad = pairs not
//                            marked exactly once + workgroups with an empty slice, one that starts inside a chunk or a tile outside the source
//   batches n total cap b0 b1 ...   (the batches are printed run-length coded: "b x times")
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../realsense-pointcloud_amd/csrc/prerej_plan.hpp"

int main()
{
    using namespace rsreg;
    std::printf("constants %u %u %u %u %u %u %llu %u\n", kPrejBlock, kPrejTile, kPrejChunk, kPrejMaxGroups, kPrejMaxBatch, kPrejRound, kPrejPartialBytes,
                kPrejPartialStride);
    char what[32];
    unsigned long long a = 0, b = 0;
    while (std::scanf("%31s %llu %llu", what, &a, &b) == 3) {
        if (!std::strcmp(what, "batches")) {
            std::printf("batches %llu %llu %u", a, b, prerej_batch_cap((uint32_t)a));
            unsigned long long done = 0;
            uint32_t last = 0, times = 0;
            for (uint32_t B; (B = prerej_batch((uint32_t)a, done, b)) != 0; done += B) {
                if (B == last) { ++times; continue; }
                if (times) std::printf(" %ux%u", last, times);
                last = B;
                times = 1;
            }
            if (times) std::printf(" %ux%u", last, times);
            std::printf("\n");
            continue;
        }
        const PrejPlan p = prerej_plan((uint32_t)a, (uint32_t)b);
        if (!std::strcmp(what, "plan")) {
            std::printf("plan %llu %llu %u %u %u %u\n", a, b, p.tiles, p.chunks, p.slice_chunks, p.slices);
            continue;
        }
        std::vector<uint8_t> seen((size_t)p.tiles * b, 0);   // one cell per (tile, hypothesis)
        unsigned long long bad = 0;
        const uint32_t groups = p.tiles * p.slices;
        for (uint32_t g = 0; g < groups; ++g) {
            uint32_t first, past;
            prerej_group_slice(g, p.tiles, p.slice_chunks, (uint32_t)b, &first, &past);
            const uint32_t tile = prerej_group_tile(g, p.tiles);
            if (first >= past || first % kPrejChunk || tile >= p.tiles || (unsigned long long)tile * kPrejTile >= a) ++bad;
            for (uint32_t h = first; h < past; ++h) {
                uint8_t &cell = seen[(size_t)tile * b + h];
                if (cell < 2) ++cell;
            }
        }
        for (uint8_t c : seen) bad += c != 1;
        std::printf("cover %llu %llu %u %llu\n", a, b, groups, bad);
    }
    return 0;
}
