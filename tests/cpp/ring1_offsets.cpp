// ring1_offsets.cpp — csrc/ring1_offsets.hpp on the host: the decode of neighbour j = dz * 9 + dy * 3 + dx into the six
// compares a search step selects with, and the table offset put together from +-sxy, +-sx, +-1, against the plain formula
// (dz - 1) * sxy + (dy - 1) * sx + (dx - 1) in 64-bit arithmetic -- all 27 j over the edge dimensions of a grid: 1, 2 and
// 4 000 cells, and strides up to sx * sy = 2^28, far beyond what a 24-bit multiply holds.  The same function fills the
// table the GPU search reads (icp_dense.hpp: dense_ring1_setup).  Built with -fsanitize=address,undefined by
// tests/test_ring1_offsets_cpu.py.  Prints "ring1_offsets ok: <checks> checks" or the first mismatches.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ring1_offsets.hpp"

int main()
{
    const int dims[] = {1, 2, 3, 4000, 4094, 16382};   // cells along an axis; the padded stride is two more (16382 + 2 = 2^14)
    int bad = 0;
    long long checks = 0;
    for (int nx : dims)
        for (int ny : dims) {
            const int64_t sx64 = nx + 2, sxy64 = sx64 * (ny + 2);
            if (sxy64 > (int64_t)1 << 28) continue;
            const int sx = (int)sx64, sxy = (int)sxy64;
            std::vector<int64_t> seen;
            for (int j = 0; j < 27; ++j) {
                const int dz = j / 9, dy = (j / 3) % 3, dx = j % 3;
                const rsreg::Ring1Cell c = rsreg::ring1_cell(j);
                const bool sel_ok = c.z1 == (dz >= 1) && c.z2 == (dz >= 2) && c.y1 == (dy >= 1) && c.y2 == (dy >= 2) && c.x1 == (dx >= 1) && c.x2 == (dx >= 2);
                const int64_t want = (int64_t)(dz - 1) * sxy64 + (int64_t)(dy - 1) * sx64 + (dx - 1);
                const int64_t got = rsreg::ring1_offset(c, sx, sxy);
                // what a step picks with the selectors: the value of that axis offset
                const bool pick_ok = rsreg::ring1_pick(c.x1, c.x2, 10, 11, 12) == 10 + dx && rsreg::ring1_pick(c.y1, c.y2, 20, 21, 22) == 20 + dy &&
                                     rsreg::ring1_pick(c.z1, c.z2, 30.0f, 31.0f, 32.0f) == 30.0f + (float)dz;
                if ((!sel_ok || !pick_ok || got != want) && bad++ < 10)
                    std::printf("mismatch: nx %d ny %d j %d: offset %lld, want %lld; selectors %s, picks %s\n", nx, ny, j, (long long)got, (long long)want,
                                sel_ok ? "ok" : "WRONG", pick_ok ? "ok" : "WRONG");
                // the 27 offsets of a grid are distinct whenever its strides keep the neighbours apart (sx >= 3 always does)
                for (int64_t s : seen)
                    if (s == got && bad++ < 10) std::printf("offset %lld twice: nx %d ny %d j %d\n", (long long)got, nx, ny, j);
                seen.push_back(got);
                checks += 3;
            }
            if (rsreg::ring1_offset(rsreg::ring1_cell(13), sx, sxy) != 0 && bad++ < 10) std::printf("the own cell's offset is not 0: nx %d ny %d\n", nx, ny);
            ++checks;
        }
    if (bad) return 1;
    std::printf("ring1_offsets ok: %lld checks\n", checks);
    return 0;
}
