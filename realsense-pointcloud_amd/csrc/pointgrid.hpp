// pointgrid.hpp — the dense point grid of the exact searches (rsreg_ctx.hpp: PointGrid): its layout, its
// build, its device view, and the bounds both searches prune with.  Included by icp.hip (through fitness_kernels.hpp),
// filters.hip (through knn_kernels.hpp), ndt.hip (the box kernel) and prerej.hip.  Everything here is a template or inline: the header is
// shared by several translation units.
//
// A build is: the box and number of the finite points (one kernel, one round trip), the cell size from them (grid_layout),
// points per cell, the exclusive prefix sum of the counts (oscan.hpp), the scatter of the points to their cells.  What differs
// between the consumers is a policy (how fine, which cell numbering) and a record reader (where x, y, z come from, what
// goes into the fourth word of an indexed point, what a non-finite record leaves behind).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "records.hpp"
#include "oscan.hpp"

namespace rsreg {

// ------------------------------------------------------------------------------ layout
// A policy: about kCellsPerPoint cells over the box for every finite point, kMinCells at the least, kMaxCells at the most;
// kBlocks: cells numbered block-major, 4x4x4 cells a block, one 64-bit occupancy word per block, cells per axis rounded up to
// whole blocks; else cells numbered x fastest.
struct FitGridPolicy {   // getFitnessScore: a thread walks blocks around its query
    static constexpr double kCellsPerPoint = 4.0, kMinCells = 64.0, kMaxCells = 16777216.0;
    static constexpr bool kBlocks = true;
};
struct KnnGridPolicy {   // k-NN of the cloud filters: a depth frame is a surface, so 64 cells per point are a few points per OCCUPIED cell
    static constexpr double kCellsPerPoint = 64.0, kMinCells = 4096.0, kMaxCells = 33554432.0;
    static constexpr bool kBlocks = false;
};
struct RadiusGridPolicy {   // radius search (radius_kernels.hpp): the cell is the radius (grid_layout's min_cell), so a ball's box is a few
                            // cells a side; these numbers only cap the cells where the radius is tiny against the box -- the cell then
                            // stays larger than the radius, as fine as the k-NN grid of the same cloud
    static constexpr double kCellsPerPoint = 64.0, kMinCells = 4096.0, kMaxCells = 33554432.0;
    static constexpr bool kBlocks = false;
};
constexpr int kGridMaxAxis = 4096;   // cells along an axis at most: what kCellMargin is argued for (grid_lb2)

// The cell: about kCellsPerPoint cells per finite point over the box, never more than 4 000 along an axis, never so small that
// the float rounding of a coordinate is a sizeable part of it, never smaller than min_cell (a radius search: its radius).  Cells per
// axis: floor(extent / cell) + 2 (rounded up to whole blocks).
template <typename Policy>
void grid_layout(const float mn[3], const float mx[3], uint32_t nfin, PointGrid &gx, double min_cell = 0.0)
{
    double e[3], emax = 0, big = 0;
    for (int k = 0; k < 3; ++k) {
        e[k] = (double)mx[k] - (double)mn[k];
        emax = std::max(emax, e[k]);
        big = std::max(big, std::max(std::fabs((double)mn[k]), std::fabs((double)mx[k])));
    }
    const double target = std::min(std::max(Policy::kCellsPerPoint * nfin, Policy::kMinCells), Policy::kMaxCells);
    auto cells_along = [&](int k, double c) {
        const int64_t d = (int64_t)std::floor(e[k] / c) + 2;
        return Policy::kBlocks ? (d + 3) & ~(int64_t)3 : d;
    };
    auto cells_for = [&](double c) { return (double)cells_along(0, c) * (double)cells_along(1, c) * (double)cells_along(2, c); };
    double lo = std::max(std::max(emax / 4000.0, big * 1e-5), 1e-30);
    if (emax == 0) lo = std::max(big * 1e-5, 1.0);
    lo = std::max(lo, std::min(min_cell, std::max(emax, lo) * 2.0));   // (two cells per axis hold any ball: no cell needs to be larger)
    double cell = lo;
    if (cells_for(lo) > target) {
        double hi = std::max(emax, lo) * 2.0;   // (two cells per axis)
        for (int it = 0; it < 100; ++it) {
            const double mid = std::sqrt(lo * hi);
            if (cells_for(mid) > target) lo = mid; else hi = mid;
        }
        cell = hi;
    }
    gx.cell = (float)cell;
    gx.inv_cell = (float)(1.0 / (double)gx.cell);
    for (int k = 0; k < 3; ++k) {
        gx.origin[k] = mn[k];
        gx.dims[k] = (int)cells_along(k, (double)gx.cell);
    }
}

// ------------------------------------------------------------------------------ device view
struct PointGridDev {
    float ox, oy, oz, inv_cell, cell;
    int dx, dy, dz;                   // cells per axis (4 096 at most; dx == 0: no point)
    int bx, by, bz;                   // block-major: blocks per axis
    uint32_t n;                       // points indexed
    const unsigned long long *mask;   // block-major: per block, its occupied cells, bit = lz*16 + ly*4 + lx
    const uint32_t *start;            // per cell + 1: first point of the cell
    const float4 *pts;                // {x, y, z, tag}, cell by cell
};

inline PointGridDev grid_dev(const PointGrid &gx)
{
    PointGridDev g{};
    g.ox = gx.origin[0]; g.oy = gx.origin[1]; g.oz = gx.origin[2];
    g.inv_cell = gx.inv_cell;
    g.cell = gx.cell;
    g.dx = gx.n_points ? gx.dims[0] : 0; g.dy = gx.dims[1]; g.dz = gx.dims[2];
    g.bx = gx.dims[0] >> 2; g.by = gx.dims[1] >> 2; g.bz = gx.dims[2] >> 2;
    g.n = gx.n_points;
    g.mask = gx.d_mask.as<unsigned long long>();
    g.start = gx.d_start.as<uint32_t>();
    g.pts = gx.d_pts.as<float4>();
    return g;
}

// the cell of p along one axis, clamped into the grid (cell_pos: the SAME expression places the points and the queries)
__device__ __forceinline__ int axis_cell(float p, float origin, float inv_cell, int d)
{
    const float v = fminf(fmaxf(floorf(cell_pos(p, origin, inv_cell)), 0.0f), (float)(d - 1));
    return (int)v;
}

__device__ __forceinline__ uint32_t grid_block_id(const PointGridDev &g, int bx, int by, int bz)
{
    return ((uint32_t)bz * (uint32_t)g.by + (uint32_t)by) * (uint32_t)g.bx + (uint32_t)bx;
}

// The position the bounds below measure from: cell_pos, or NaN where the position says nothing that float arithmetic can use --
// (q - origin) has overflowed (a query at the far end of a box that spans most of the float range), or the query lies more than
// kPosMax cells from the origin (a source record far outside a tiny target box: its gaps would square to +inf while its distances
// are finite floats).  axis_gap of a NaN is 0 for every cell (fmaxf drops the NaN), the one bound that is always true: such a
// query visits everything.  Below kPosMax the sum of three squared gaps stays under 3.1e36.  (axis_cell clamps the same
// positions to the first or the last cell, for the points and the queries alike.)
constexpr float kPosMax = 1e18f;
__device__ __forceinline__ float bound_pos(float u)
{
    return fabsf(u) <= kPosMax ? u : __int_as_float(0x7fc00000);
}

// A lower bound on the squared FLOAT distance (l2_simple) to anything beyond the per-axis gaps (cells, from axis_gap): what
// lets a search skip a cell, a block or everything outside a shell and still return the exact nearest float distance.
// axis_gap's kCellMargin covers the rounding of the cell assignment inside the grid (kGridMaxAxis cells at most along an axis:
// 1e-3 cells); the relative factor covers what grows with the distance -- the rounding of (q - origin) * inv_cell for a query far
// outside the grid (3 ulp), that of this sum and its three products (6 ulp) and of the cell against 1 / inv_cell (2 ulp), and
// l2_simple's own (5 ulp): 16 ulp of 2^-24, 1e-6 < 4e-6.
// The range is every finite float32 cloud and every finite query.  The sum (finite: bound_pos) is multiplied by the cell TWICE,
// not by cell * cell: that float product is +inf for a cell above 1.8e19 and 0 or a denormal of a few bits for one below 1e-19,
// while distances of a few cells are still finite floats, or still tell records apart.  Taken one after the other, a product
// overflows only where the bound, and with it every float distance it stands for, is above FLT_MAX (the first one only for a cell
// above 1e2: the sum is below 3.1e36); gaps of 0 give 0, never 0 * inf.  Where the result is a float denormal, so is d2: each of
// l2_simple's three products is then rounded to a multiple of 2^-149 (their sums are exact) and d2 can lie 1.5 * 2^-149 below the
// real value, the last two roundings here move the bound by 2^-149 at most (a denormal first product is multiplied by a cell
// below 1e-19 once more), and 4 * 2^-149 comes off -- nothing against a normal float.
__device__ __forceinline__ float grid_lb2(float gx, float gy, float gz, float cell)
{
    return __fsub_rn(__fmul_rn(__fmul_rn(__fmul_rn(gx * gx + gy * gy + gz * gz, 0.999996f), cell), cell), 0x1p-147f);
}

// ------------------------------------------------------------------------------ the nearest point (block-major grids)
// A search walks shells of BLOCKS around the query's block (clamped into the grid), skips empty blocks on their word and cells on a
// lower bound, and stops when the six slabs beyond the last shell are all farther than the best distance found (or the range):
// fitness_kernels.hpp (getFitnessScore) and prerej_kernels.hpp (the score of a pose hypothesis) both call it.
__device__ __forceinline__ void fit_visit_block(const PointGridDev &g, int bx, int by, int bz, float ux, float uy, float uz, float cell,
                                                float qx, float qy, float qz, float &best, float &limit2)
{
    const uint32_t b = grid_block_id(g, bx, by, bz);
    unsigned long long m = g.mask[b];
    while (m) {
        const int bit = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int x = (bx << 2) | (bit & 3), y = (by << 2) | ((bit >> 2) & 3), z = (bz << 2) | (bit >> 4);
        if (grid_lb2(axis_gap(ux, x, x), axis_gap(uy, y, y), axis_gap(uz, z, z), cell) > limit2) continue;
        const uint32_t c = b * 64u + (uint32_t)bit;
        const uint32_t e = g.start[c + 1];
        for (uint32_t p = g.start[c]; p < e; ++p) {
            const float4 t = g.pts[p];
            best = fminf(best, l2_simple(qx, qy, qz, t.x, t.y, t.z));
        }
        limit2 = fminf(limit2, best);
    }
}

// The nearest squared float distance from q to the indexed points (+inf: none within limit2).  limit2: nothing farther is wanted
// (+inf: unbounded).  Every cell that could hold a point at least as close as the best so far is opened.
__device__ __forceinline__ float fit_nearest(const PointGridDev &g, float qx, float qy, float qz, float limit2)
{
    float best = __int_as_float(0x7f800000);
    if (g.dx <= 0) return best;
    const float ux = bound_pos(cell_pos(qx, g.ox, g.inv_cell)), uy = bound_pos(cell_pos(qy, g.oy, g.inv_cell)),
                uz = bound_pos(cell_pos(qz, g.oz, g.inv_cell));
    const int qbx = axis_cell(qx, g.ox, g.inv_cell, g.dx) >> 2, qby = axis_cell(qy, g.oy, g.inv_cell, g.dy) >> 2,
              qbz = axis_cell(qz, g.oz, g.inv_cell, g.dz) >> 2;
    // gaps to the whole grid along each axis: what a slab beyond a shell is at least away along the other two
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
                    fit_visit_block(g, bx, by, bz, ux, uy, uz, g.cell, qx, qy, qz, best, limit2);
                }
            }
        }
        // every block not visited yet lies in one of the six slabs beyond this shell
        float lb = __int_as_float(0x7f800000);
        if (qbx + rb + 1 < g.bx) lb = fminf(lb, grid_lb2(axis_gap(ux, (qbx + rb + 1) << 2, g.dx - 1), hy, hz, g.cell));
        if (qbx - rb - 1 >= 0) lb = fminf(lb, grid_lb2(axis_gap(ux, 0, ((qbx - rb - 1) << 2) + 3), hy, hz, g.cell));
        if (qby + rb + 1 < g.by) lb = fminf(lb, grid_lb2(hx, axis_gap(uy, (qby + rb + 1) << 2, g.dy - 1), hz, g.cell));
        if (qby - rb - 1 >= 0) lb = fminf(lb, grid_lb2(hx, axis_gap(uy, 0, ((qby - rb - 1) << 2) + 3), hz, g.cell));
        if (qbz + rb + 1 < g.bz) lb = fminf(lb, grid_lb2(hx, hy, axis_gap(uz, (qbz + rb + 1) << 2, g.dz - 1), g.cell));
        if (qbz - rb - 1 >= 0) lb = fminf(lb, grid_lb2(hx, hy, axis_gap(uz, 0, ((qbz - rb - 1) << 2) + 3), g.cell));
        if (lb > limit2) break;
    }
    return best;
}

// ------------------------------------------------------------------------------ record readers
// the cell-sorted target of an alignment (float4 {x, y, idx, z}: records.hpp, tgt_rec); an indexed point carries no tag
struct TargetRecords {
    const float4 *pts;
    __device__ __forceinline__ float3 xyz(uint32_t i) const
    {
        const float4 t = pts[i];
        return make_float3(t.x, t.y, tgt_z(t));
    }
    __device__ __forceinline__ float tag(uint32_t) const { return 0.0f; }
    __device__ __forceinline__ void not_finite(uint32_t) const {}
};

// records of any stride that begin with x, y, z; an indexed point carries its record's number; the count pass gives a
// non-finite record PCL's distance 0 (dist: null when nothing is counted)
struct StridedRecords {
    const char *rec;
    size_t stride;
    float *dist;
    __device__ __forceinline__ float3 xyz(uint32_t i) const
    {
        const float *p = rec_xyz(rec, stride, i);
        return make_float3(p[0], p[1], p[2]);
    }
    __device__ __forceinline__ float tag(uint32_t i) const { return __uint_as_float(i); }
    __device__ __forceinline__ void not_finite(uint32_t i) const { dist[i] = 0.0f; }
};

// ------------------------------------------------------------------------------ build kernels
// box[0..2] = min, [3..5] = max (ordered uints), [6] = number of finite points; box = {~0 x 3, 0 x 5} on entry.  One set of
// atomics per workgroup, not per wave: they all hit the same seven words.
// (static: k_grid_box<StridedRecords> is instantiated by filters.hip and by ndt.hip.  With external linkage their host stubs merge at
// link, and a launch from one unit runs -- and first has to load -- the other unit's code object.)
template <typename Reader>
static __global__ __launch_bounds__(kBlock) void k_grid_box(Reader rd, uint32_t n, uint32_t *box)
{
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    uint32_t cnt = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float3 p = rd.xyz(i);
        if (finite3(p.x, p.y, p.z)) {
            mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
            mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
            ++cnt;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], __shfl_down(mn[k], off));
            mx[k] = fmaxf(mx[k], __shfl_down(mx[k], off));
        }
        cnt += __shfl_down(cnt, off);
    }
    constexpr int kWaves = kBlock / 64;
    __shared__ float smn[kWaves][3], smx[kWaves][3];
    __shared__ uint32_t scnt[kWaves];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 3; ++k) { smn[wave][k] = mn[k]; smx[wave][k] = mx[k]; }
        scnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) {
            for (int k = 0; k < 3; ++k) { mn[k] = fminf(mn[k], smn[w][k]); mx[k] = fmaxf(mx[k], smx[w][k]); }
            cnt += scnt[w];
        }
        if (cnt) {
            for (int k = 0; k < 3; ++k) {
                atomicMin(&box[k], float_ordered(mn[k]));
                atomicMax(&box[3 + k], float_ordered(mx[k]));
            }
            atomicAdd(&box[6], cnt);
        }
    }
}

// the cell of a finite point: x fastest, or block * 64 + bit with bit = lz*16 + ly*4 + lx
template <bool kBlocks>
__device__ __forceinline__ bool grid_point_cell(const PointGridDev &g, const float3 &p, uint32_t &cell)
{
    if (!finite3(p.x, p.y, p.z)) return false;
    const int cx = axis_cell(p.x, g.ox, g.inv_cell, g.dx), cy = axis_cell(p.y, g.oy, g.inv_cell, g.dy), cz = axis_cell(p.z, g.oz, g.inv_cell, g.dz);
    if (kBlocks) cell = grid_block_id(g, cx >> 2, cy >> 2, cz >> 2) * 64u + (uint32_t)((cz & 3) << 4 | (cy & 3) << 2 | (cx & 3));
    else cell = ((uint32_t)cz * (uint32_t)g.dy + (uint32_t)cy) * (uint32_t)g.dx + (uint32_t)cx;
    return true;
}

// points per cell and, block-major, the blocks' occupancy words (count and mask zero on entry)
template <bool kBlocks, typename Reader>
__global__ __launch_bounds__(kBlock) void k_grid_count(Reader rd, uint32_t n, PointGridDev g, uint32_t *count, unsigned long long *mask)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c;
    if (!grid_point_cell<kBlocks>(g, rd.xyz(i), c)) {
        rd.not_finite(i);
        return;
    }
    atomicAdd(&count[c], 1u);
    if (kBlocks) atomicOr(&mask[c >> 6], 1ull << (c & 63u));
}

// each finite point to a free place of its cell (start = exclusive prefix of the counts; the counts go back to zero).  The order
// inside a cell is whatever the atomics make it: only distance values are read from the index.
template <bool kBlocks, typename Reader>
__global__ __launch_bounds__(kBlock) void k_grid_scatter(Reader rd, uint32_t n, PointGridDev g, const uint32_t *start, uint32_t *count, float4 *sorted)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float3 p = rd.xyz(i);
    uint32_t c;
    if (!grid_point_cell<kBlocks>(g, p, c)) return;
    const uint32_t k = atomicSub(&count[c], 1u) - 1u;
    sorted[start[c] + k] = make_float4(p.x, p.y, p.z, rd.tag(i));
}

// ------------------------------------------------------------------------------ host build
// Indexes the n records of rd in gx's own buffers, on ctx->stream: box (one round trip through h, 8 pinned words), layout,
// counts, prefix sum, placement.  gx.n_points = the finite records; fewer than min_points (>= 1) of them: nothing is indexed and
// gx.dims stay 0.  place(g, start, count, cells) queues what puts the points into gx.d_pts cell by cell and leaves the counts zero;
// the order inside a cell is the placement's (grid_build: whatever the atomics make it).
template <typename Policy, typename Reader, typename Place>
int grid_build_placed(rsreg_ctx *ctx, PointGrid &gx, const Reader &rd, uint32_t n, uint32_t min_points, uint32_t *h, double min_cell, Place place)
{
    constexpr bool kBlocks = Policy::kBlocks;
    hipStream_t st = ctx->stream;
    const uint32_t nb = (n + kBlock - 1) / kBlock;
    gx.built = false;
    gx.n_points = 0;
    gx.dims[0] = gx.dims[1] = gx.dims[2] = 0;
    RSREG_HIP(ctx, gx.d_box.reserve(64));
    h[6] = 0;
    if (n) {
        RSREG_HIP(ctx, hipMemsetAsync(gx.d_box.ptr, 0xff, 12, st));
        RSREG_HIP(ctx, hipMemsetAsync(gx.d_box.as<char>() + 12, 0, 20, st));
        k_grid_box<<<std::min<uint32_t>(nb, 1024), kBlock, 0, st>>>(rd, n, gx.d_box.as<uint32_t>());
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipMemcpyAsync(h, gx.d_box.ptr, 32, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
    }
    const uint32_t nfin = h[6];
    gx.n_points = nfin;
    if (nfin < min_points) {
        gx.built = true;
        return RSREG_OK;
    }
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) {
        mn[k] = ordered_float(h[k]);
        mx[k] = ordered_float(h[3 + k]);
    }
    grid_layout<Policy>(mn, mx, nfin, gx, min_cell);
    const size_t cells = (size_t)gx.dims[0] * (size_t)gx.dims[1] * (size_t)gx.dims[2];
    if (gx.dims[0] > kGridMaxAxis || gx.dims[1] > kGridMaxAxis || gx.dims[2] > kGridMaxAxis || cells > 0x7ffffff0ull)
        return fail(ctx, RSREG_ERR_STATE, "point grid layout out of range");
    const size_t count_cap_before = gx.d_count.cap;
    RSREG_HIP(ctx, gx.d_pts.reserve((size_t)nfin * sizeof(float4) + 16));
    RSREG_HIP(ctx, gx.d_start.reserve((cells + 1) * 4));
    RSREG_HIP(ctx, gx.d_count.reserve((cells + 1) * 4));
    RSREG_HIP(ctx, gx.d_scan.reserve(oscan_scratch_bytes<uint32_t>(cells + 1)));
    if (gx.d_count.cap != count_cap_before || count_cap_before == 0)   // (a new buffer; an old one is zero after every scatter)
        RSREG_HIP(ctx, hipMemsetAsync(gx.d_count.ptr, 0, gx.d_count.cap, st));
    if (kBlocks) {
        RSREG_HIP(ctx, gx.d_mask.reserve(cells / 64 * 8));
        RSREG_HIP(ctx, hipMemsetAsync(gx.d_mask.ptr, 0, cells / 64 * 8, st));
    }
    const PointGridDev g = grid_dev(gx);
    uint32_t *count = gx.d_count.as<uint32_t>(), *start = gx.d_start.as<uint32_t>();
    k_grid_count<kBlocks><<<nb, kBlock, 0, st>>>(rd, n, g, count, gx.d_mask.as<unsigned long long>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, oscan<uint32_t>(count, start, cells + 1, 0u, gx.d_scan.ptr, st));
    const int rc = place(g, start, count, cells);
    if (rc) return rc;
    gx.built = true;
    return RSREG_OK;
}

template <typename Policy, typename Reader>
int grid_build(rsreg_ctx *ctx, PointGrid &gx, const Reader &rd, uint32_t n, uint32_t min_points, uint32_t *h)
{
    return grid_build_placed<Policy>(ctx, gx, rd, n, min_points, h, 0.0, [&](const PointGridDev &g, uint32_t *start, uint32_t *count, size_t) {
        k_grid_scatter<Policy::kBlocks><<<(n + kBlock - 1) / kBlock, kBlock, 0, ctx->stream>>>(rd, n, g, start, count, gx.d_pts.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
        return (int)RSREG_OK;
    });
}

}  // namespace rsreg
