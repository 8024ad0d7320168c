// grid_layout.cpp — grid_layout of csrc/pointgrid.hpp on a machine without a GPU, for tests/test_pointgrid_layout_cpu.py to hold
// tests/pointgrid_layout.py against.  It calls no HIP function: the header's host template is all it runs.
//
//   grid_layout (mn_x mn_y mn_z mx_x mx_y mx_z nfin min_cell policy)...
//
// policy: knn, radius or fit; the floats in any form strtof reads (the test passes hex floats, so nothing is rounded on the way).
// One line per group of nine arguments: cell inv_cell (both %a) dim_x dim_y dim_z.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rsreg_ctx.hpp"
#include "pointgrid.hpp"

int main(int argc, char **argv)
{
    using namespace rsreg;
    if (argc < 10 || (argc - 1) % 9 != 0) {
        std::fprintf(stderr, "usage: %s (mn_x mn_y mn_z mx_x mx_y mx_z nfin min_cell knn|radius|fit)...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 9 <= argc; a += 9) {
        float mn[3], mx[3];
        for (int k = 0; k < 3; ++k) {
            mn[k] = std::strtof(argv[a + k], nullptr);
            mx[k] = std::strtof(argv[a + 3 + k], nullptr);
        }
        const uint32_t nfin = (uint32_t)std::strtoul(argv[a + 6], nullptr, 10);
        const double min_cell = std::strtod(argv[a + 7], nullptr);
        const char *policy = argv[a + 8];
        PointGrid gx;
        if (!std::strcmp(policy, "knn")) grid_layout<KnnGridPolicy>(mn, mx, nfin, gx, min_cell);
        else if (!std::strcmp(policy, "radius")) grid_layout<RadiusGridPolicy>(mn, mx, nfin, gx, min_cell);
        else if (!std::strcmp(policy, "fit")) grid_layout<FitGridPolicy>(mn, mx, nfin, gx, min_cell);
        else {
            std::fprintf(stderr, "unknown policy %s\n", policy);
            return 2;
        }
        std::printf("%a %a %d %d %d\n", (double)gx.cell, (double)gx.inv_cell, gx.dims[0], gx.dims[1], gx.dims[2]);
    }
    return 0;
}
