// icp_grid_plan.hpp — the grid of the ICP correspondence search, decided on the host from what a target build knows before it
// places a point: the box of the finite records, their number, the correspondence gate, the refinement factor of a second
// pass and three switches.  Plain C++, no HIP and nothing of the context: tests/cpp/icp_grid_plan.cpp includes this header
// alone, and tests/icp_grid_layout.py restates it in Python (tests/test_icp_scale_cpu.py holds the two against each other).
// icp.hip (build_grid) calls icp_grid_plan and builds what it says.
//
// The rule:
//   * a gate that is "bounded" (positive, finite, below a quarter of the extent + 1 mm) is cut into 1 .. 8 equal parts no larger
//     than the cap, and a part (of the gate padded by 4 %) is the cell; a gate below the cap takes the cap itself (wide_cells);
//   * every other gate (unbounded, or wider than the cloud) takes the cap;
//   * the cap is cell_cap (tuned on 10^6-point frames), up to three times that for sparser clouds, times `refine`;
//   * never fewer than extent / 60 000 metres a cell (the cell key's bits per axis), never less than 1e-6 m;
//   * origin = the box's minimum; dims = cell of the box's maximum + 2, by the float32 operations of the device's cell_coord;
//   * max_ring: the rings (in cells) that cover the gate, or one more than the longest axis;
//   * the dense cell-start table when its padded cells fit dense_max_cells, else the brick hash.
// The constants are absolute (metres): the same cloud at another scale gets another grid.  What that costs a search, and up to which
// cost a search is served, is stated at rsreg_icp_set_target (include/rsreg.h).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace rsreg {

constexpr float kIcpPlanMargin = 0.03f;        // = kCellMargin (records.hpp; icp.hip asserts it)
constexpr float kIcpCoordMax = 70000.0f;       // cell_coord's clamp (icp_kernels.hpp)
constexpr double kIcpAxisCells = 60000.0;      // cells along the longest axis at most
constexpr float kIcpCellMax = 0x1p60f;         // the largest cell a search is served with (IcpGridPlan::served)

struct IcpGridInput {
    float mn[3], mx[3];                    // box of the finite records
    uint32_t nfin = 0;                     // their number (> 0)
    double max_dist = 0;                   // the correspondence gate
    double refine = 1.0;                   // second pass of the brick-hash build: icp_refine_factor
    double cell_cap = 0.014;               // tunables: cell_cap, wide_cells, dense_max_cells
    bool wide_cells = true;
    long long dense_max_cells = 1ll << 28;
};

struct IcpGridPlan {
    float cell = 1.0f, inv_cell = 1.0f;
    float origin[3] = {0, 0, 0};
    int dims[3] = {0, 0, 0};
    int max_ring = 0;
    int index_kind = 0;                    // rsreg_grid_info::index_kind: 0 brick hash, 1 dense table
    bool bounded = false;                  // which branch fixed the cell (diagnostic: the mirror reports the same)
    // Whether the searches' float32 arithmetic holds on this grid: a target whose plan says no is built and never searched -- every
    // search over it is refused (icp.hip: refuse_unserved; rsreg.h).
    //   * cell <= 2^60: the bounds are taken in cell units and scaled by cell * cell or 1 / (cell * cell), which are then normal
    //     floats (2^-120 .. 2^120; the cell is never below 1e-6); above 1.8e19 the square is +inf, its inverse 0, and every row or
    //     brick but the query's own is skipped;
    //   * (max - min) is a finite float along every axis: (p - origin) of a target record never overflows;
    //   * the cell of the box's maximum is below cell_coord's clamp: every record lies in its own cell, and a brick's coordinate
    //     fits the 14 bits the brick key gives it.
    bool served = false;
};

// host mirror of cell_coord (same IEEE operations, no contraction)
inline int host_cell_coord(float p, float origin, float inv_cell)
{
    volatile float d = p - origin;
    volatile float v = d * inv_cell;
    float f = std::floor(v);
    f = std::min(std::max(f, -4.0f), kIcpCoordMax);
    return (int)f;
}

inline IcpGridPlan icp_grid_plan(const IcpGridInput &in)
{
    IcpGridPlan gp;
    const double max_dist = in.max_dist, refine = in.refine;
    // the cap is tuned on 10^6-point D435i-like frames; sparser clouds (lower resolution of the same
    // scene: sample spacing ~ n^-1/2) do best with somewhat larger cells (swept at 50 k and 300 k points)
    const double cap = in.cell_cap * std::min(3.0, std::max(1.0, std::pow(1.0e6 / std::max<double>(in.nfin, 1.0e4), 0.28)));
    double extent = 0;
    for (int k = 0; k < 3; ++k) extent = std::max(extent, (double)in.mx[k] - (double)in.mn[k]);
    double cell;
    const bool bounded = std::isfinite(max_dist) && max_dist > 0 && max_dist < 0.25 * extent + 1e-3;
    if (bounded) {
        const double padded = max_dist * 1.04;
        // the far phase walks (2*parts/4+3)^3 bricks for an unmatched query: 8 parts at most.  (Clamped as a double: the ratio of a
        // gate of 10^11 m to the cap does not fit an int, and the conversion of such a double is undefined -- on x86-64 it came
        // out as INT_MIN, one part, where every smaller gate of the same shape got eight.)
        const int parts = (int)std::min(8.0, std::max(1.0, std::ceil(padded / (cap * refine))));
        cell = padded / parts;
        // a gate below the cap (the reference's 1 cm on sparse edge clouds): cells as large as the cap still need one
        // ring only, and the table (cleared and scanned on every build) shrinks with the cube of the cell
        if (in.wide_cells && parts == 1 && cap * refine > padded) cell = cap * refine;
    } else {
        cell = cap * refine;
    }
    cell = std::max(cell, extent / kIcpAxisCells);  // 16 bits per axis in the cell key
    cell = std::max(cell, 1e-6);
    gp.bounded = bounded;
    gp.cell = (float)cell;
    gp.inv_cell = 1.0f / gp.cell;
    gp.served = gp.cell <= kIcpCellMax;
    for (int k = 0; k < 3; ++k) {
        gp.origin[k] = in.mn[k];
        gp.dims[k] = host_cell_coord(in.mx[k], gp.origin[k], gp.inv_cell) + 2;
        volatile float span = in.mx[k] - in.mn[k];
        if (!std::isfinite(span) || gp.dims[k] - 2 >= (int)kIcpCoordMax) gp.served = false;
    }
    const int max_dim = std::max(gp.dims[0], std::max(gp.dims[1], gp.dims[2]));
    int max_ring = max_dim + 1;
    if (std::isfinite(max_dist) && max_dist >= 0) {
        const double rings = std::ceil(max_dist / (double)gp.cell + kIcpPlanMargin);   // smallest R with (R - margin) * cell >= gate
        if (rings < (double)(max_dim + 1)) max_ring = std::max(1, (int)rings);
    }
    gp.max_ring = max_ring;
    const long long padded_cells = (long long)(gp.dims[0] + 2) * (gp.dims[1] + 2) * (gp.dims[2] + 2);
    // (the dense search addresses points by 32-bit byte offsets: 16 B x 2^28)
    gp.index_kind = (padded_cells <= in.dense_max_cells && (unsigned long long)in.nfin + 4ull < (1ull << 28)) ? 1 : 0;
    return gp;
}

// The brick-hash build looks at what it has built: more than 14 distinct points an occupied cell, and it builds once more with
// the cap times this factor (towards ~8 points a cell, never below a fifth).  1: the first build stays.
inline double icp_refine_factor(uint64_t n_unique, uint64_t n_cells)
{
    if (n_cells == 0) return 1.0;
    const double per_cell = (double)n_unique / (double)n_cells;
    if (!(per_cell > 14.0)) return 1.0;
    return std::max(0.2, std::sqrt(8.0 / per_cell));
}

}  // namespace rsreg
