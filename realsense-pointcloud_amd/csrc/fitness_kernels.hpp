// fitness_kernels.hpp — device code of Registration::getFitnessScore (include/rsreg.h: rsreg_icp_fitness_score,
// rsreg_ndt_fitness_score): the search and the sums.  Included by icp.hip only (icp_kernels.hpp: wave_sum); the index itself,
// its build and the bounds the search prunes with are pointgrid.hpp's.
//
// PCL 1.9 (registration.hpp):
//   transformPointCloud(*input_, input_transformed, final_transformation_);
//   for each point: tree_->nearestKSearch(point, 1, ...); if (nn_dists[0] <= max_range) { fitness_score += nn_dists[0]; ++nr; }
//   return nr > 0 ? fitness_score / nr : DBL_MAX;
//
// The index (rsreg_ctx.hpp: PointGrid, built with FitGridPolicy) is a dense grid of 4x4x4-cell blocks over the target's box:
// one 64-bit occupancy word per block, the cells' starts numbered block-major.  A search walks shells of BLOCKS around the query's block
// (clamped into the grid), skips empty blocks on their word and cells on a lower bound, and stops when the six slabs beyond
// the last shell are all farther than the best distance found (or the range).  Nothing bounds the walk but that test: the
// result is the exact nearest float distance at any range, for queries inside the box or far outside it.
#pragma once

#include "icp_kernels.hpp"
#include "pointgrid.hpp"

namespace rsreg {

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

// ------------------------------------------------------------------------------ score
// Record j of the source (float4 {x, y, z, valid}) moved by T with k_apply_final's arithmetic, its nearest target distance;
// out[perm[j]] = that distance if (double)d2 <= max_range, else -1 (not counted: outside the range, or a non-finite point)
__global__ __launch_bounds__(kBlock) void k_fit_search(const float4 *src, uint32_t n, Mat34 T, const uint32_t *perm, PointGridDev g, float limit2,
                                                       double max_range, float *out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const float4 s = src[j];
    float r = -1.0f;
    if (s.w != 0.0f) {
        const float3 t = xform(T, s.x, s.y, s.z);
        if (finite3(t.x, t.y, t.z)) {
            const float d = fit_nearest(g, t.x, t.y, t.z, limit2);
            if ((double)d <= max_range) r = d;
        }
    }
    out[perm ? perm[j] : j] = r;
}

// Workgroup b adds the records [b * kBlock, (b + 1) * kBlock) of the caller's order: partials[b] = count, partials[nblocks + b] = sum
// of d2, in f64, in a fixed tree (k_final_reduce adds the slabs next)
__global__ __launch_bounds__(kBlock) void k_fit_tiles(const float *d2, uint32_t n, double *partials)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0.0, s = 0.0;
    if (i < n) {
        const float d = d2[i];
        if (d >= 0.0f) {
            c = 1.0;
            s = (double)d;
        }
    }
    c = wave_sum(c);
    s = wave_sum(s);
    __shared__ double sh[2][kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh[0][wave] = c;
        sh[1][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double v = sh[threadIdx.x][0];
        for (int w = 1; w < kBlock / 64; ++w) v += sh[threadIdx.x][w];
        partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = v;
    }
}

}  // namespace rsreg
