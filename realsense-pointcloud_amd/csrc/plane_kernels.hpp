// plane_kernels.hpp — device code of point-to-plane ICP (pcl::IterativeClosestPointWithNormals with its default
// TransformationEstimationPointToPlaneLLS): the 32 sums of include/rsreg.h (RSREG_NUM_PLANE_SUMS) over the pairs the
// search kept, and the target's normals packed by original target index.  Included by icp.hip behind icp_kernels.hpp.
#pragma once

#include "icp_kernels.hpp"

namespace rsreg {

// three floats at `in + i * stride` -> float4 {nx, ny, nz, 0}: pcl::Normal records (stride 32), PointXYZRGBNormal records
// with the pointer at normal_x (stride 48), packed xyz staged from the host (stride 12)
__global__ __launch_bounds__(kBlock) void k_pack_normals(const char *in, size_t stride, uint32_t n, float4 *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = rec_xyz(in, stride, i);
    out[i] = make_float4(r[0], r[1], r[2], 0.0f);
}

// tile_reduce_store (icp_kernels.hpp) for 32 sums: recursive halving over the 64 lanes -- 16 + 8 + 4 + 2 + 1 + 1 doubles
// move in the six steps, after which every second lane owns one sum -- then the tile's two waves in order.  Every sum goes
// through the same tree of additions as a sum of the 17 does (a step adds lane l's and lane l ^ mask's value of a sum,
// whichever index the sum has), so sums [0] and [1] here are bit-equal to sums [0] and [16] there.
__device__ __forceinline__ void plane_tile_reduce_store(double (&a)[RSREG_NUM_PLANE_SUMS], double *partials, uint32_t nblocks, uint32_t slot)
{
    __shared__ double shr[kTileWaves][RSREG_NUM_PLANE_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0, cnt = RSREG_NUM_PLANE_SUMS;
    double v16[16], v8[8], v4[4], v2[2], v1[1], v0[1];
    halve_sums<RSREG_NUM_PLANE_SUMS>(a, v16, lane, 32, base, cnt);
    halve_sums<16>(v16, v8, lane, 16, base, cnt);
    halve_sums<8>(v8, v4, lane, 8, base, cnt);
    halve_sums<4>(v4, v2, lane, 4, base, cnt);
    halve_sums<2>(v2, v1, lane, 2, base, cnt);
    halve_sums<1>(v1, v0, lane, 1, base, cnt);
    if (cnt >= 1) shr[wave][base] = v0[0];   // exactly one lane of a wave ends up owning each of the 32 sums
    __syncthreads();
    if (threadIdx.x < RSREG_NUM_PLANE_SUMS) {
        double v = shr[0][threadIdx.x];
        for (int w = 1; w < kTileWaves; ++w) v += shr[w][threadIdx.x];
        partials[(size_t)threadIdx.x * nblocks + slot] = v;
    }
}

// The mapping of k_cov_reduce: one distinct source point per thread, block b covers points [b*128, b*128+128).  The pair's
// weight is the multiplicity cur[i].w of merged source copies, or cw[i] (the copies a correspondence filter left in play)
// when cw is given.  Every product below is one IEEE double operation on the float inputs (the library is compiled without
// contraction): a pair's 32 terms are the ones include/rsreg.h spells out, whatever the launch.
__global__ __launch_bounds__(kTile) void k_plane_reduce(const float4 *cur, const int *corr_pos, const float *corr_d2, const uint32_t *cw,
                                                        const float4 *tgt, const float4 *normals, uint32_t n, double *partials)
{
    double a[RSREG_NUM_PLANE_SUMS];
#pragma unroll
    for (int k = 0; k < RSREG_NUM_PLANE_SUMS; ++k) a[k] = 0.0;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int pos = corr_pos[i];
        const uint32_t w = cw ? cw[i] : 1u;
        if (pos >= 0 && w) {
            const float4 p = cur[i];
            const float4 q = tgt[pos];
            const float4 nr = normals[tgt_idx(q)];
            const double W = cw ? (double)w : (double)p.w;
            a[0] = W;
            a[1] = W * (double)corr_d2[i];
            if (finite3(nr.x, nr.y, nr.z)) {
                const double px = p.x, py = p.y, pz = p.z, qx = q.x, qy = q.y, qz = tgt_z(q), nx = nr.x, ny = nr.y, nz = nr.z;
                const double J[6] = {nz * py - ny * pz, nx * pz - nz * px, ny * px - nx * py, nx, ny, nz};
                const double r = ((nx * qx + ny * qy) + nz * qz) - ((nx * px + ny * py) + nz * pz);
                a[2] = W;
                a[3] = W * (r * r);
                int k = 4;
#pragma unroll
                for (int rr = 0; rr < 6; ++rr)
#pragma unroll
                    for (int cc = rr; cc < 6; ++cc) a[k++] = W * (J[rr] * J[cc]);
#pragma unroll
                for (int rr = 0; rr < 6; ++rr) a[25 + rr] = W * (J[rr] * r);
            }
        }
    }
    plane_tile_reduce_store(a, partials, gridDim.x, blockIdx.x);
}

}  // namespace rsreg
