// radius_kernels.hpp — the exact radius search of every point of a cloud within the same cloud, and its two consumers:
// the neighbour counts under pcl::RadiusOutlierRemoval and pcl::NormalEstimation with setRadiusSearch (include/rsreg.h:
// rsreg_cloud_radius_count, rsreg_cloud_radius_outlier_removal, rsreg_cloud_normals_radius).  Included by filters.hip only; the
// index, its layout and the bounds the walk prunes with are pointgrid.hpp's, the tail of the normal is normals_kernels.hpp's.
//
// PCL 1.9.1 / FLANN, recalled (neither is available to check against; include/rsreg.h is the contract):
//   KdTreeFLANN::radiusSearch(point, radius, ...):  flann_index_->radiusSearch(..., static_cast<float>(radius * radius), ...)
//   RadiusResultSet::addPoint(dist, index):         if (dist < radius) ...        // `radius` is the squared one here: STRICT
// so record j is a neighbour of record i when l2_simple(i, j) < r2 in float32, r2 = (float)((double)radius * (double)radius).  The
// record itself and exact copies are neighbours like any other.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "normals_kernels.hpp"
#include "osort.hpp"

namespace rsreg {

// ------------------------------------------------------------------------------ index
// The grid is pointgrid.hpp's x-fastest form under RadiusGridPolicy with the radius as the smallest cell.  What differs from the
// k-NN build is the placement: the points of a cell lie in ASCENDING ORIGINAL RECORD INDEX, by a stable sort (osort.hpp) of
// (cell, record) pairs written in record order -- a function of the cloud and the radius alone, where k_grid_scatter leaves the order
// its atomics make.  The counts do not care; the f64 sums of the normals do (their last bits depend on the order of the addends).
struct RadiusRecords {
    const char *rec;
    size_t stride;
    uint32_t *count;   // nullable: a non-finite record has no neighbour
    __device__ __forceinline__ float3 xyz(uint32_t i) const
    {
        const float *p = rec_xyz(rec, stride, i);
        return make_float3(p[0], p[1], p[2]);
    }
    __device__ __forceinline__ float tag(uint32_t i) const { return __uint_as_float(i); }
    __device__ __forceinline__ void not_finite(uint32_t i) const { if (count) count[i] = 0u; }
};

// keys[i] = the cell of record i (no_cell, above every cell, for a non-finite record: they end up behind the indexed points),
// vals[i] = i
__global__ __launch_bounds__(kBlock) void k_radius_cell_keys(RadiusRecords rd, uint32_t n, PointGridDev g, uint32_t no_cell, uint32_t *keys, uint32_t *vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c;
    keys[i] = grid_point_cell<false>(g, rd.xyz(i), c) ? c : no_cell;
    vals[i] = i;
}

// the sorted pair j is the point j of the index: start[] is the exclusive prefix sum of the same cells' counts.  The counts go
// back to zero (every writer of a word writes the same 0).
__global__ __launch_bounds__(kBlock) void k_radius_place(RadiusRecords rd, uint32_t nfin, const uint32_t *keys, const uint32_t *vals, uint32_t *count,
                                                         float4 *sorted)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nfin) return;
    const uint32_t i = vals[j];
    const float3 p = rd.xyz(i);
    sorted[j] = make_float4(p.x, p.y, p.z, rd.tag(i));
    count[keys[j]] = 0u;
}

// ------------------------------------------------------------------------------ search
// What a walk needs beside the index: r2, and how far (in cells) a ball reaches along an axis -- from the ACTUAL cell, which is the
// radius or larger (grid_layout), with the slack of every geometric bound here (kCellMargin: the float rounding of the point -> cell
// assignment) and that of the float compare (d2 < r2 leaves |dx| <= radius * (1 + 2^-22)).
struct RadiusQuery {
    float r2, reach;
};

inline RadiusQuery radius_query(double radius, const PointGrid &gx)
{
    RadiusQuery rq;
    rq.r2 = (float)(radius * radius);
    rq.reach = (float)(radius / (double)gx.cell * 1.00001 + 2.0 * (double)kCellMargin);   // (may be +inf: the box is clamped in float)
    return rq;
}

// the cells lo .. hi along one axis that a ball around in-grid position u can touch.  A point's cell is floor(its position) clamped into
// the grid, the query's too (axis_cell); clamping is monotone, so clamping both ends of [u - reach, u + reach] covers a ball that
// reaches past a face as well as a query that lies outside the grid.  A NaN (bound_pos: the position says nothing)
// leaves lo = 0 and hi = d - 1, the whole axis: fmaxf and fminf drop it, and each end meets first the clamp it then falls to.
__device__ __forceinline__ void radius_axis_cells(float u, float reach, int d, int &lo, int &hi)
{
    const float top = (float)(d - 1);
    lo = (int)fminf(fmaxf(floorf(u - reach), 0.0f), top);
    hi = (int)fmaxf(fminf(floorf(u + reach), top), 0.0f);
}

// One wave hands every point of the index with l2_simple(q, point) < r2 to f, each to ONE lane (f(point), under divergence).  It visits
// the rows of cells (runs along x: one run of the cell-sorted array each) of the box of cells the ball can touch: the lanes fetch the
// starts of 64 rows side by side, a row beyond the bound (grid_lb2 > r2) is skipped, the others are read 64 points at a time, 16
// bytes a lane.  The bound is fixed, so nothing is selected, nothing is kept in LDS, and the walk ends when the box is done.  The
// order in which a lane meets its candidates -- rows ascending, a row's points ascending -- is a function of the index alone.
template <typename F>
__device__ __forceinline__ void radius_walk(const PointGridDev &g, const float4 q, const RadiusQuery rq, int lane, F &f)
{
    const float ux = bound_pos(cell_pos(q.x, g.ox, g.inv_cell)), uy = bound_pos(cell_pos(q.y, g.oy, g.inv_cell)),
                uz = bound_pos(cell_pos(q.z, g.oz, g.inv_cell));
    int x0, x1, y0, y1, z0, z1;
    radius_axis_cells(ux, rq.reach, g.dx, x0, x1);
    radius_axis_cells(uy, rq.reach, g.dy, y0, y1);
    radius_axis_cells(uz, rq.reach, g.dz, z0, z1);
    const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
    const float gx = axis_gap(ux, x0, x1);
    for (int base = 0; base < rows; base += kKnnWave) {
        const int row = base + lane;
        uint32_t s = 0, e = 0;
        if (row < rows) {
            const int y = y0 + row % ny, z = z0 + row / ny;
            if (!(grid_lb2(gx, axis_gap(uy, y, y), axis_gap(uz, z, z), g.cell) > rq.r2)) {
                const size_t c0 = ((size_t)z * (size_t)g.dy + (size_t)y) * (size_t)g.dx;
                s = g.start[c0 + (size_t)x0];
                e = g.start[c0 + (size_t)x1 + 1];
            }
        }
        unsigned long long todo = __ballot(e > s);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t ss = __shfl(s, l), ee = __shfl(e, l);
            for (uint32_t p = ss; p < ee; p += kKnnWave) {
                const uint32_t i = p + (uint32_t)lane;
                if (i < ee) {
                    const float4 t = g.pts[i];
                    if (l2_simple(q.x, q.y, q.z, t.x, t.y, t.z) < rq.r2) f(t);
                }
            }
        }
    }
}

// The same walk for a consumer that works as a WAVE: f(point, hit) runs in uniform control flow after every 64-point read, every
// lane with the point it read (unspecified where there was none) and whether it is a neighbour, so f may ballot, shuffle and meet
// a barrier.  The rows, the reads and a read's lanes are those of radius_walk: the ascending (row, point) order of the hits is a
// function of the index alone.
template <typename F>
__device__ __forceinline__ void radius_walk_wave(const PointGridDev &g, const float4 q, const RadiusQuery rq, int lane, F &f)
{
    const float ux = bound_pos(cell_pos(q.x, g.ox, g.inv_cell)), uy = bound_pos(cell_pos(q.y, g.oy, g.inv_cell)),
                uz = bound_pos(cell_pos(q.z, g.oz, g.inv_cell));
    int x0, x1, y0, y1, z0, z1;
    radius_axis_cells(ux, rq.reach, g.dx, x0, x1);
    radius_axis_cells(uy, rq.reach, g.dy, y0, y1);
    radius_axis_cells(uz, rq.reach, g.dz, z0, z1);
    const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
    const float gx = axis_gap(ux, x0, x1);
    for (int base = 0; base < rows; base += kKnnWave) {
        const int row = base + lane;
        uint32_t s = 0, e = 0;
        if (row < rows) {
            const int y = y0 + row % ny, z = z0 + row / ny;
            if (!(grid_lb2(gx, axis_gap(uy, y, y), axis_gap(uz, z, z), g.cell) > rq.r2)) {
                const size_t c0 = ((size_t)z * (size_t)g.dy + (size_t)y) * (size_t)g.dx;
                s = g.start[c0 + (size_t)x0];
                e = g.start[c0 + (size_t)x1 + 1];
            }
        }
        unsigned long long todo = __ballot(e > s);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t ss = __shfl(s, l), ee = __shfl(e, l);
            for (uint32_t p = ss; p < ee; p += kKnnWave) {
                const uint32_t i = p + (uint32_t)lane;
                float4 t = q;
                bool hit = false;
                if (i < ee) {
                    t = g.pts[i];
                    hit = l2_simple(q.x, q.y, q.z, t.x, t.y, t.z) < rq.r2;
                }
                f(t, hit);
            }
        }
    }
}

// ------------------------------------------------------------------------------ counts
struct RadiusCount {
    uint32_t n = 0;
    __device__ __forceinline__ void operator()(const float4 &) { ++n; }
};

// One workgroup of ONE wave per query, queries in cell order (the grid-stride loop of k_knn_mean_distance).  count[record] = its
// neighbours within the radius, itself among them; the words of non-finite records have been zeroed by the build.
__global__ __launch_bounds__(kKnnWave) void k_radius_count(PointGridDev g, RadiusQuery rq, uint32_t *count)
{
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        RadiusCount c;
        radius_walk(g, q, rq, lane, c);
        uint32_t m = c.n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
        if (lane == 0) count[__float_as_uint(q.w)] = m;
    }
}

// pcl::RadiusOutlierRemoval: removed when count <= min_neighbors (negative: when count > min_neighbors); a non-finite record's
// count is 0 and the same rule holds for it
__global__ __launch_bounds__(kBlock) void k_ror_flags(const uint32_t *count, uint32_t n, uint32_t min_neighbors, int negative, uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool above = count[i] > min_neighbors;
    flags[i] = (negative ? !above : above) ? 1u : 0u;
}

// ------------------------------------------------------------------------------ normals
// a lane's nine running f64 sums over its candidates, in walk order, d = neighbour - query
struct RadiusMoments {
    double qx, qy, qz;
    double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    uint32_t n = 0;
    __device__ __forceinline__ void operator()(const float4 &t)
    {
#pragma clang fp contract(off)
        const double dx = (double)t.x - qx, dy = (double)t.y - qy, dz = (double)t.z - qz;
        sx += dx; sy += dy; sz += dz;
        sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
        syy += dy * dy; syz += dy * dz; szz += dz * dz;
        ++n;
    }
};

// One workgroup of ONE wave per query, queries in cell order: the walk, the lanes' sums through wave_sum_fixed, then k_normals' tail
// over the m neighbours.  m < 3 (PCL's computePointNormal returns false below three points): four quiet NaNs, and *any_nan = 1.
// out: record `record` = {normal_x, normal_y, normal_z, 0, curvature, 0, 0, 0}.
__global__ __launch_bounds__(kKnnWave) void k_normals_radius(PointGridDev g, RadiusQuery rq, float vpx, float vpy, float vpz, float *out, uint32_t *any_nan)
{
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        RadiusMoments a;
        a.qx = (double)q.x; a.qy = (double)q.y; a.qz = (double)q.z;
        radius_walk(g, q, rq, lane, a);
        uint32_t m = a.n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
        if (m < 3u) {
            if (lane < 8) out[(size_t)__float_as_uint(q.w) * 8 + (size_t)lane] = (lane < 3 || lane == 4) ? __uint_as_float(0x7fc00000u) : 0.0f;
            if (lane == 0) *any_nan = 1u;
            continue;
        }
        const double sx = wave_sum_fixed(a.sx), sy = wave_sum_fixed(a.sy), sz = wave_sum_fixed(a.sz);
        const double sxx = wave_sum_fixed(a.sxx), sxy = wave_sum_fixed(a.sxy), sxz = wave_sum_fixed(a.sxz);
        const double syy = wave_sum_fixed(a.syy), syz = wave_sum_fixed(a.syz), szz = wave_sum_fixed(a.szz);
        normal_from_sums(q, (double)m, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, vpx, vpy, vpz, lane, out);
    }
}

}  // namespace rsreg
