// ring1_offsets.hpp — neighbour j of a cell's 27-cell neighbourhood, for host and device (icp_dense.hpp: dense_ring1_lane;
// tests/cpp/ring1_offsets.cpp checks it on the host against the plain formula).
//
// j = dz * 9 + dy * 3 + dx with dx, dy, dz in 0..2 (the cell at (dx - 1, dy - 1, dz - 1)), the bit numbering of the
// occupancy words.  A search step needs, of j: which of three values to pick per axis (the gap to the slab on that side),
// and where the neighbour's entry lies in the padded table, (dz - 1) * sxy + (dy - 1) * sx + (dx - 1) entries from the cell's
// own.  Both come from the same six compares, and the offset is put together from +-sxy, +-sx, +-1 by selects and adds:
// no division of j, no multiply (sxy may exceed 2^24, where a 24-bit multiply would be wrong, and a full 32-bit one is a
// quarter-rate instruction on the GPU).
#pragma once

#if defined(__HIPCC__)
#define RSREG_R1_HD __host__ __device__ __forceinline__
#else
#define RSREG_R1_HD inline
#endif

namespace rsreg {

struct Ring1Cell {
    bool z1, z2;   // dz >= 1, dz >= 2
    bool y1, y2;   // dy >= 1, dy >= 2
    bool x1, x2;   // dx >= 1, dx >= 2
};

RSREG_R1_HD Ring1Cell ring1_cell(int j)
{
    Ring1Cell c;
    c.z1 = j >= 9;
    c.z2 = j >= 18;
    const int r = j - (c.z2 ? 18 : (c.z1 ? 9 : 0));     // dy * 3 + dx
    c.y1 = r >= 3;
    c.y2 = r >= 6;
    const int dx = r - (c.y2 ? 6 : (c.y1 ? 3 : 0));
    c.x1 = dx >= 1;
    c.x2 = dx >= 2;
    return c;
}

// a0, a1 or a2 for an axis offset of 0, 1 or 2
template <typename T> RSREG_R1_HD T ring1_pick(bool ge1, bool ge2, T a0, T a1, T a2) { return ge2 ? a2 : (ge1 ? a1 : a0); }

// table entries from the own cell's to the neighbour's; sx, sxy: the padded table's strides (DenseDev)
RSREG_R1_HD int ring1_offset(const Ring1Cell &c, int sx, int sxy)
{
    return ring1_pick(c.z1, c.z2, -sxy, 0, sxy) + ring1_pick(c.y1, c.y2, -sx, 0, sx) + ring1_pick(c.x1, c.x2, -1, 0, 1);
}

}  // namespace rsreg
