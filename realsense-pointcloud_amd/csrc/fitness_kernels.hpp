// fitness_kernels.hpp — device code of Registration::getFitnessScore (include/rsreg.h: rsreg_icp_fitness_score,
// rsreg_ndt_fitness_score): the kernels of the search and the sums.  Included by icp.hip only (icp_kernels.hpp: wave_sum); the
// index itself, its build, the bounds the search prunes with and the walk of one query (fit_nearest: prerej.hip scores
// pose hypotheses with it too) are pointgrid.hpp's.
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
