// iss_kernels.hpp — pcl::ISSKeypoint3D (Intrinsic Shape Signatures, Zhong 2009) over the exact radius search of radius_kernels.hpp:
// device code of rsreg_cloud_iss_saliency, rsreg_cloud_iss_non_max and rsreg_cloud_iss_keypoints (include/rsreg.h holds the
// contract).  Included by filters.hip only.
//
// PCL 1.9.1 keypoints/impl/iss_3d.hpp, recalled (PCL is not available to check against):
//   getScatterMatrix(i):   cov = sum over the radiusSearch(i, salient_radius) of (neighbour - point)(neighbour - point)^T, not
//                          divided, not centred;
//   detectKeypoints:       nb_neighbors >= min_neighbors_: e1 >= e2 >= e3 of the scatter; a value that is not finite, or e3 < 0:
//                          the record is passed over; else (e2 / e1 < gamma_21_) && (e3 / e2 < gamma_32_): third_eigen_value_[i] = e3,
//                          otherwise 0; then, over radiusSearch(i, non_max_radius): third_eigen_value_[i] > 0, n_neighbors >=
//                          min_neighbors_ and no neighbour j with third_eigen_value_[i] < third_eigen_value_[j]: a keypoint.
//
// ONE INDEX for both walks.  The index is built once, at the salient radius; the walk of the non-max radius runs over the same
// grid with a RadiusQuery of its own.  Nothing in radius_walk ties the radius to the cell: `reach` is computed from the ACTUAL
// cell (radius_query), the rows are pruned with grid_lb2 over that cell, and the compare is the float32 d2 < r2 of every walk -- a
// radius above the cell only makes the box of cells wider (reach 2.5 at non_max = 2.5 salient: 7 x 7 rows), one below it makes
// the walk read more candidates than a grid of its own would (reach 0.1: still the 3 x 3 rows around the record).  Both stay
// exact; the order of the hits is the order of the index, a function of the cloud and the SALIENT radius alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "radius_kernels.hpp"

namespace rsreg {

// a lane's six running f64 second moments about the query over its candidates, in walk order, d = neighbour - query
struct IssScatter {
    double qx, qy, qz;
    double sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    uint32_t n = 0;
    __device__ __forceinline__ void operator()(const float4 &t)
    {
#pragma clang fp contract(off)
        const double dx = (double)t.x - qx, dy = (double)t.y - qy, dz = (double)t.z - qz;
        sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
        syy += dy * dy; syz += dy * dz; szz += dz * dz;
        ++n;
    }
};

// PCL's third_eigen_value_ from the ascending eigenvalues: l3 = ev[0] unless a value is not finite, l3 < 0, or a ratio (IEEE f64
// division; a NaN ratio fails its compare) is not below its gamma
__device__ __forceinline__ double iss_saliency(const double (&ev)[3], double gamma_21, double gamma_32)
{
    const double l1 = ev[2], l2 = ev[1], l3 = ev[0];
    const bool finite = isfinite(l1) && isfinite(l2) && isfinite(l3);
    return (finite && l3 >= 0.0 && l2 / l1 < gamma_21 && l3 / l2 < gamma_32) ? l3 : 0.0;
}

// One workgroup of ONE wave per finite record, records in index order (the frame of k_normals_radius): the walk at the salient radius,
// the lanes' six sums through wave_sum_fixed, the Jacobi of eig_sym3_smallest (its eigenvector is not used), the thresholds.
// Record `record`: eig[3 * record ..] = the eigenvalues ascending, saliency[record], count[record] = m_s.  m_s < min_neighbors:
// zeros (the scatter is never formed).  The words of non-finite records have been zeroed before the launch.
__global__ __launch_bounds__(kKnnWave) void k_iss_saliency(PointGridDev g, RadiusQuery rq, uint32_t min_neighbors, double gamma_21, double gamma_32,
                                                           double *eig, double *saliency, uint32_t *count)
{
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        IssScatter a;
        a.qx = (double)q.x; a.qy = (double)q.y; a.qz = (double)q.z;
        radius_walk(g, q, rq, lane, a);
        uint32_t m = a.n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
        double ev[3] = {0.0, 0.0, 0.0}, sal = 0.0;
        if (m >= min_neighbors) {   // (uniform: m is the wave's)
            const double c[6] = {wave_sum_fixed(a.sxx), wave_sum_fixed(a.sxy), wave_sum_fixed(a.sxz),
                                 wave_sum_fixed(a.syy), wave_sum_fixed(a.syz), wave_sum_fixed(a.szz)};
            double vec[3];
            eig_sym3_smallest(c, ev, vec);
            sal = iss_saliency(ev, gamma_21, gamma_32);
        }
        const size_t id = (size_t)__float_as_uint(q.w);
        if (lane < 3) eig[id * 3 + (size_t)lane] = pick3(ev[0], ev[1], ev[2], lane);
        if (lane == 3) saliency[id] = sal;
        if (lane == 4) count[id] = m;
    }
}

// a lane's hits at the non-max radius and whether one of them has a saliency above the query's (the compare as written: a NaN on
// either side is not above)
struct IssNonMax {
    const double *saliency;
    double mine;
    uint32_t n = 0;
    bool below = false;
    __device__ __forceinline__ void operator()(const float4 &t)
    {
        ++n;
        below |= mine < saliency[__float_as_uint(t.w)];
    }
};

// One workgroup of ONE wave per finite record, records in index order.  flags[record] = 1 when saliency[record] > 0, m_n >=
// min_neighbors and no neighbour within the non-max radius has a larger saliency; a record whose saliency is not above 0 leaves
// before the walk (one record is one wave: uniform).  flags[] has been zeroed before the launch.
__global__ __launch_bounds__(kKnnWave) void k_iss_non_max(PointGridDev g, RadiusQuery rq, const double *saliency, uint32_t min_neighbors, uint32_t *flags)
{
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        const uint32_t id = __float_as_uint(q.w);
        IssNonMax f;
        f.saliency = saliency;
        f.mine = saliency[id];
        if (!(f.mine > 0.0)) continue;
        radius_walk(g, q, rq, lane, f);
        uint32_t m = f.n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
        const bool below = __ballot(f.below) != 0ull;
        if (lane == 0) flags[id] = (m >= min_neighbors && !below) ? 1u : 0u;
    }
}

// the kept records' indices in their order: index[pos[i]] = i where flags[i]; thread 0 leaves their number in *n_kept
__global__ __launch_bounds__(kBlock) void k_iss_indices(const uint32_t *flags, const uint32_t *pos, uint32_t n, int32_t *index, uint32_t *n_kept)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *n_kept = pos[n - 1] + flags[n - 1];
    if (i >= n || !flags[i]) return;
    index[pos[i]] = (int32_t)i;
}

}  // namespace rsreg
