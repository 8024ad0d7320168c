// icp_grid_plan.cpp — icp_grid_plan and icp_refine_factor of csrc/icp_grid_plan.hpp on a machine without a GPU, for
// tests/test_icp_scale_cpu.py to hold tests/icp_grid_layout.py against.  Includes that header alone: plain C++ (g++), no HIP.
//
//   icp_grid_plan (mn_x mn_y mn_z mx_x mx_y mx_z nfin max_dist refine cell_cap wide_cells dense_max_cells n_unique n_cells)...
//
// The floats in any form strtof / strtod read (the test passes hex floats, so nothing is rounded on the way; "inf" is read too).
// One line per group of fourteen arguments:
//   cell inv_cell origin_x origin_y origin_z (all %a) dim_x dim_y dim_z max_ring index_kind bounded served refine_factor(n_unique, n_cells) (%a)
#include <cstdio>
#include <cstdlib>

#include "../../realsense-pointcloud_amd/csrc/icp_grid_plan.hpp"

int main(int argc, char **argv)
{
    using namespace rsreg;
    constexpr int kArgs = 14;
    if (argc < 1 + kArgs || (argc - 1) % kArgs != 0) {
        std::fprintf(stderr, "usage: %s (mn_x mn_y mn_z mx_x mx_y mx_z nfin max_dist refine cell_cap wide_cells dense_max_cells n_unique n_cells)...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + kArgs <= argc; a += kArgs) {
        IcpGridInput in;
        for (int k = 0; k < 3; ++k) {
            in.mn[k] = std::strtof(argv[a + k], nullptr);
            in.mx[k] = std::strtof(argv[a + 3 + k], nullptr);
        }
        in.nfin = (uint32_t)std::strtoul(argv[a + 6], nullptr, 10);
        in.max_dist = std::strtod(argv[a + 7], nullptr);
        in.refine = std::strtod(argv[a + 8], nullptr);
        in.cell_cap = std::strtod(argv[a + 9], nullptr);
        in.wide_cells = std::atoi(argv[a + 10]) != 0;
        in.dense_max_cells = std::atoll(argv[a + 11]);
        const unsigned long long n_unique = std::strtoull(argv[a + 12], nullptr, 10), n_cells = std::strtoull(argv[a + 13], nullptr, 10);
        const IcpGridPlan p = icp_grid_plan(in);
        std::printf("%a %a %a %a %a %d %d %d %d %d %d %d %a\n", (double)p.cell, (double)p.inv_cell, (double)p.origin[0], (double)p.origin[1],
                    (double)p.origin[2], p.dims[0], p.dims[1], p.dims[2], p.max_ring, p.index_kind, p.bounded ? 1 : 0, p.served ? 1 : 0,
                    icp_refine_factor(n_unique, n_cells));
    }
    return 0;
}
