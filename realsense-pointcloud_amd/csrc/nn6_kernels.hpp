// nn6_kernels.hpp — the exact nearest neighbour in (x, y, z, w L', w a', w b'): the correspondence search of
// pcl::GeneralizedIterativeClosestPoint6D (include/rsreg.h, "GICP6D", holds the contract).  Included by icp.hip only, behind
// fitness_kernels.hpp: the index is a PointGrid of its own (pointgrid.hpp, block-major) over every finite target record that can
// win (below: exact 6-D copies), and the walk is fit_nearest's with another candidate rule.
//
// Why a grid over x, y, z alone serves six dimensions: d6 = ((((dx^2 + dy^2) + dz^2) + dL^2) + da^2) + db^2 is never below its
// 3-D part, in float as well (adding a non-negative term with round-to-nearest is monotone).  grid_lb2 bounds the 3-D part of
// every point of a cell, a block or a slab from below, so a bound above the best d6 so far -- or above the gate -- rules out
// everything behind it in six dimensions too.  Ties: a bound EQUAL to the limit is opened, and the key's low word decides.
//
// Why not the alignment's own index: it keeps one point per distinct x, y, z (the record of lowest index), and target records
// that are exact copies in space but differ in colour are different candidates here.
#pragma once

#include "fitness_kernels.hpp"

namespace rsreg {

// float4 {x, y, z, 0} records in HBM (what rsreg_gicp_set_target_lab keeps of the target); an indexed point carries its record's number
struct Xyz4Records {
    const float4 *rec;
    __device__ __forceinline__ float3 xyz(uint32_t i) const
    {
        const float4 t = rec[i];
        return make_float3(t.x, t.y, t.z);
    }
    __device__ __forceinline__ float tag(uint32_t i) const { return __uint_as_float(i); }
    __device__ __forceinline__ void not_finite(uint32_t) const {}
};

// the first three floats of records of any stride (a multiple of 4) -> float4 {a, b, c, 0}: a target's x, y, z; a cloud's L', a', b'
__global__ __launch_bounds__(kBlock) void k_nn6_pack3(const char *rec, size_t stride, uint32_t n, float4 *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    out[i] = make_float4(p[0], p[1], p[2], 0.0f);
}

// ---- exact 6-D copies among the target records.  A record whose x, y, z, L', a', b' equal (bit for bit) those of a record of lower
// index can never be a pair's target: the same d6 for every query, and the tie goes to the lower index.  Such records stay out of
// the index: a RealSense frame holds 10^4 .. 10^5 black records at (0, 0, 0), which would otherwise share one cell, to be scanned
// whole by every source record of that kind.  An insert-only hash set of record numbers, open addressing, at most half full: the
// slot of a class of equal records ends up holding the class's lowest index.
constexpr uint32_t kNn6Empty = 0xffffffffu;

__device__ __forceinline__ uint32_t nn6_hash(const float4 &p, const float4 &c)
{
    const uint32_t w[6] = {__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), __float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z)};
    uint32_t h = 0x9e3779b1u;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        h = (h ^ w[k]) * 0x85ebca77u;
        h ^= h >> 15;
    }
    return h;
}

__device__ __forceinline__ bool nn6_same(const float4 &p, const float4 &c, const float4 &q, const float4 &d)
{
    return __float_as_uint(p.x) == __float_as_uint(q.x) && __float_as_uint(p.y) == __float_as_uint(q.y) && __float_as_uint(p.z) == __float_as_uint(q.z) &&
           __float_as_uint(c.x) == __float_as_uint(d.x) && __float_as_uint(c.y) == __float_as_uint(d.y) && __float_as_uint(c.z) == __float_as_uint(d.z);
}

// table (mask + 1 slots, all kNn6Empty on entry): every finite record finds or claims the slot of its class
__global__ __launch_bounds__(kBlock) void k_nn6_copies_insert(const float4 *xyz, const float4 *lab, uint32_t n, uint32_t *table, uint32_t mask)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = xyz[i], c = lab[i];
    if (!finite3(p.x, p.y, p.z)) return;
    for (uint32_t s = nn6_hash(p, c) & mask;; s = (s + 1) & mask) {
        const uint32_t cur = atomicCAS(&table[s], kNn6Empty, i);
        if (cur == kNn6Empty) return;
        if (nn6_same(p, c, xyz[cur], lab[cur])) {   // (whichever member of the class holds the slot right now)
            atomicMin(&table[s], i);
            return;
        }
    }
}

// ... and a record that is not its class's lowest index gets x = NaN: the index build passes it over.  (Only slot holders are
// read here, only other records are written.)
__global__ __launch_bounds__(kBlock) void k_nn6_copies_drop(float4 *xyz, const float4 *lab, uint32_t n, const uint32_t *table, uint32_t mask)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = xyz[i], c = lab[i];
    if (!finite3(p.x, p.y, p.z)) return;
    for (uint32_t s = nn6_hash(p, c) & mask;; s = (s + 1) & mask) {
        const uint32_t cur = table[s];
        if (cur == i) return;
        if (cur == kNn6Empty) return;   // (not reached: every finite record was inserted)
        if (nn6_same(p, c, xyz[cur], lab[cur])) {
            xyz[i].x = __int_as_float(0x7fc00000);
            return;
        }
    }
}

// k_grid_scatter that leaves records of the sorted target's layout (records.hpp: tgt_rec -- x, y, record number, z), so that the
// kernels behind the search read a pair's target as they read it from the alignment's own index
__global__ __launch_bounds__(kBlock) void k_nn6_scatter(Xyz4Records rd, uint32_t n, PointGridDev g, const uint32_t *start, uint32_t *count, float4 *sorted)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float3 p = rd.xyz(i);
    uint32_t c;
    if (!grid_point_cell<true>(g, p, c)) return;
    const uint32_t k = atomicSub(&count[c], 1u) - 1u;
    sorted[start[c] + k] = tgt_rec(p.x, p.y, p.z, i);
}

__device__ __forceinline__ float4 nn6_scaled(const float4 &lab, float w)
{
    return make_float4(__fmul_rn(w, lab.x), __fmul_rn(w, lab.y), __fmul_rn(w, lab.z), 0.0f);
}

// the colours of the indexed points in the index's order, scaled once per begin: col[p] = w * lab[record of point p]
__global__ __launch_bounds__(kBlock) void k_nn6_target_colours(const float4 *pts, uint32_t n_pts, const float4 *lab, float w, float4 *col)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pts) return;
    col[p] = nn6_scaled(lab[tgt_idx(pts[p])], w);
}

// the colour of every working point: that of its record (6-D mode works on unmerged sources: first[u] is the point's one record)
__global__ __launch_bounds__(kBlock) void k_nn6_source_colours(const uint32_t *perm, const uint32_t *first, uint32_t n, const float4 *lab, float w, float4 *col)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    col[u] = nn6_scaled(lab[perm[first[u]]], w);
}

// A source that was merged into weighted distinct points by x, y, z (icp_kernels.hpp: k_source_unique) taken apart again, in its
// spatial order: every record a working point of its own with weight 1 -- exact copies that differ in colour are different queries
__global__ __launch_bounds__(kBlock) void k_source_unmerge(const float4 *src_all, uint32_t n, float4 *src, uint32_t *uniq_of, uint32_t *first)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    src[j] = src_all[j];
    uniq_of[j] = j;
    first[j] = j;
    if (j == n - 1) first[n] = n;
}

// the points of one block's occupied cells, each cell on its bound (pointgrid.hpp: fit_visit_block with the 6-D candidate rule).
// The colour line of a candidate is read only when its 3-D part is not already above the best distance.
__device__ __forceinline__ void nn6_visit_block(const PointGridDev &g, const float4 *col, int bx, int by, int bz, float ux, float uy, float uz,
                                                float qx, float qy, float qz, const float4 &qc, Best &b, float &limit2)
{
    const uint32_t blk = grid_block_id(g, bx, by, bz);
    unsigned long long m = g.mask[blk];
    while (m) {
        const int bit = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int x = (bx << 2) | (bit & 3), y = (by << 2) | ((bit >> 2) & 3), z = (bz << 2) | (bit >> 4);
        if (grid_lb2(axis_gap(ux, x, x), axis_gap(uy, y, y), axis_gap(uz, z, z), g.cell) > limit2) continue;
        const uint32_t c = blk * 64u + (uint32_t)bit;
        const uint32_t e = g.start[c + 1];
        for (uint32_t p = g.start[c]; p < e; ++p) {
            const float4 t = g.pts[p];
            const float d3 = l2_simple(qx, qy, qz, t.x, t.y, tgt_z(t));
            if (!(d3 <= b.d2)) continue;   // (d6 >= d3: it cannot win; a NaN 3-D part makes a NaN d6)
            const float4 tc = col[p];
            const float dL = __fsub_rn(qc.x, tc.x), da = __fsub_rn(qc.y, tc.y), db = __fsub_rn(qc.z, tc.z);
            const float d6 = __fadd_rn(__fadd_rn(__fadd_rn(d3, __fmul_rn(dL, dL)), __fmul_rn(da, da)), __fmul_rn(db, db));
            if (d6 == d6) consider(b, d6, tgt_idx(t), p);
        }
        limit2 = fminf(limit2, b.d2);
    }
}

// fit_nearest's walk (shells of blocks, nearest first; the six slabs beyond a shell end it) with the limit at the best d6
__device__ __forceinline__ Best nn6_query(const PointGridDev &g, const float4 *col, float qx, float qy, float qz, const float4 &qc, float limit2)
{
    Best b{~0ull, -1, __int_as_float(0x7f800000)};
    if (g.dx <= 0) return b;
    const float ux = bound_pos(cell_pos(qx, g.ox, g.inv_cell)), uy = bound_pos(cell_pos(qy, g.oy, g.inv_cell)),
                uz = bound_pos(cell_pos(qz, g.oz, g.inv_cell));
    const int qbx = axis_cell(qx, g.ox, g.inv_cell, g.dx) >> 2, qby = axis_cell(qy, g.oy, g.inv_cell, g.dy) >> 2,
              qbz = axis_cell(qz, g.oz, g.inv_cell, g.dz) >> 2;
    const float hx = axis_gap(ux, 0, g.dx - 1), hy = axis_gap(uy, 0, g.dy - 1), hz = axis_gap(uz, 0, g.dz - 1);
    const int rb_max = max(max(max(qbx, g.bx - 1 - qbx), max(qby, g.by - 1 - qby)), max(qbz, g.bz - 1 - qbz));
    for (int rb = 0; rb <= rb_max; ++rb) {
        const int z0 = max(qbz - rb, 0), z1 = min(qbz + rb, g.bz - 1);
        const int y0 = max(qby - rb, 0), y1 = min(qby + rb, g.by - 1);
        for (int bz = z0; bz <= z1; ++bz) {
            const float gz = axis_gap(uz, bz << 2, (bz << 2) + 3);
            if (grid_lb2(0.0f, 0.0f, gz, g.cell) > limit2) continue;
            for (int by = y0; by <= y1; ++by) {
                const float gy = axis_gap(uy, by << 2, (by << 2) + 3);
                if (grid_lb2(0.0f, gy, gz, g.cell) > limit2) continue;
                const bool face = abs(bz - qbz) == rb || abs(by - qby) == rb;   // a face row: every block of it; else its two ends
                const int xa = qbx - rb, xb = qbx + rb;
                for (int bx = face ? max(xa, 0) : xa; bx <= (face ? min(xb, g.bx - 1) : xb); bx += face ? 1 : max(2 * rb, 1)) {
                    if (bx < 0 || bx >= g.bx) continue;
                    const float gx = axis_gap(ux, bx << 2, (bx << 2) + 3);
                    if (grid_lb2(gx, gy, gz, g.cell) > limit2) continue;
                    nn6_visit_block(g, col, bx, by, bz, ux, uy, uz, qx, qy, qz, qc, b, limit2);
                }
            }
        }
        float lb = __int_as_float(0x7f800000);
        if (qbx + rb + 1 < g.bx) lb = fminf(lb, grid_lb2(axis_gap(ux, (qbx + rb + 1) << 2, g.dx - 1), hy, hz, g.cell));
        if (qbx - rb - 1 >= 0) lb = fminf(lb, grid_lb2(axis_gap(ux, 0, ((qbx - rb - 1) << 2) + 3), hy, hz, g.cell));
        if (qby + rb + 1 < g.by) lb = fminf(lb, grid_lb2(hx, axis_gap(uy, (qby + rb + 1) << 2, g.dy - 1), hz, g.cell));
        if (qby - rb - 1 >= 0) lb = fminf(lb, grid_lb2(hx, axis_gap(uy, 0, ((qby - rb - 1) << 2) + 3), hz, g.cell));
        if (qbz + rb + 1 < g.bz) lb = fminf(lb, grid_lb2(hx, hy, axis_gap(uz, (qbz + rb + 1) << 2, g.dz - 1), g.cell));
        if (qbz - rb - 1 >= 0) lb = fminf(lb, grid_lb2(hx, hy, axis_gap(uz, 0, ((qbz - rb - 1) << 2) + 3), g.cell));
        if (lb > limit2) break;
    }
    return b;
}

// k_nn_search in six dimensions: corr_pos[i] = the winner's place in the 6-D index's point array (-1: none), corr_d2[i] = its d6.
// prune2: the gate's square as a float, rounded up (+inf: unbounded); the pair is kept iff !((double)d6 > gate2).
__global__ __launch_bounds__(kBlock) void k_nn_search6(const float4 *cur, const float4 *cur_col, uint32_t n, PointGridDev g, const float4 *col, float prune2,
                                                       double gate2, int *corr_pos, float *corr_d2)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 q = cur[i];
    int pos = -1;
    float d2 = 0.0f;
    if (q.w != 0.0f && finite3(q.x, q.y, q.z)) {
        const float4 qc = cur_col[i];
        if (finite3(qc.x, qc.y, qc.z)) {
            const Best b = nn6_query(g, col, q.x, q.y, q.z, qc, prune2);
            if (b.pos >= 0 && !((double)b.d2 > gate2)) {
                pos = b.pos;
                d2 = b.d2;
            }
        }
    }
    corr_pos[i] = pos;
    corr_d2[i] = d2;
}

}  // namespace rsreg
