// gicp_cov_kernels.hpp — the per-record regularised covariance of pcl::GeneralizedIterativeClosestPoint (computeCovariances):
// device code of rsreg_cloud_gicp_covariances (include/rsreg.h holds the contract).  Included by filters.hip only, behind
// normals_kernels.hpp: the search (knn_walk<KnnKeys>), the moment sums (knn_moment_sums), the covariance (cov_about_query) and the
// Jacobi (eig_sym3_smallest) are the normals' own; what is new is the tail, C' = I - (1 - epsilon) n n^T in f64.
#pragma once

#include "normals_kernels.hpp"

namespace rsreg {

constexpr size_t kGicpCovBytes = 48;   // six doubles: xx, xy, xz, yy, yz, zz

// the records of the non-finite input records: six quiet NaNs
__global__ __launch_bounds__(kBlock) void k_gicp_cov_not_finite(const char *rec, size_t stride, uint32_t n, double *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    if (finite3(p[0], p[1], p[2])) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int k = 0; k < 6; ++k) out[(size_t)i * 6 + k] = qnan;
}

// One workgroup of ONE wave per finite record, queries in cell order (the frame of k_normals): the search, the nine sums, the
// covariance and its smallest eigenvector n ((0, 0, 1) when the trace is 0), then lanes 0 .. 5 write
//   C'_ab = delta_ab - s * (n_a * n_b),  s = 1 - epsilon      (three roundings an entry: the product, the scaling, the difference)
// into record `q.w` of out.
__global__ __launch_bounds__(kKnnWave) void k_gicp_cov(PointGridDev g, int k, const char *rec, size_t stride, double epsilon, double *out)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long buf[kKnnBuf];
    const int lane = (int)threadIdx.x;
    const double s1 = 1.0 - epsilon;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        knn_walk<KnnKeys>(g, q, k, buf, lane);
        double s[9], c[6];
        knn_moment_sums(buf, k, rec, stride, q, lane, s);
        cov_about_query((double)k, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], c);
        const double trace = (c[0] + c[3]) + c[5];
        double ev[3], nv[3] = {0.0, 0.0, 1.0};
        if (trace != 0.0) eig_sym3_smallest(c, ev, nv);
        if (lane < 6) {
            const double a = lane < 3 ? nv[0] : (lane < 5 ? nv[1] : nv[2]);
            const double b = (lane == 0) ? nv[0] : ((lane == 1 || lane == 3) ? nv[1] : nv[2]);
            const double v = s1 * (a * b);
            const bool diag = lane == 0 || lane == 3 || lane == 5;
            out[(size_t)__float_as_uint(q.w) * 6 + (size_t)lane] = diag ? 1.0 - v : 0.0 - v;
        }
    }
}

}  // namespace rsreg
