// normals_kernels.hpp — the identity-carrying output of the exact k-nearest-neighbour search (knn_kernels.hpp: knn_walk<KnnKeys>)
// and pcl::NormalEstimation (setKSearch) on top of it: device code of rsreg_cloud_knn and rsreg_cloud_normals (include/rsreg.h).
// Included by filters.hip only.
//
// The search leaves a query's k smallest keys (float bits of d2 << 32 | original record index), ascending, in LDS.  The record
// itself and exact copies are neighbours like any other (PCL's nearestKSearch).  A neighbour's coordinates are read from the
// cloud's own records through the original index in the key: no position in the cell-sorted array is kept and nothing is
// searched twice.
//
// The normal (PCL 1.9.1 features/normal_3d.h, recalled: computePointNormal, solvePlaneParameters, flipNormalTowardsViewpoint),
// by the wave that searched, while the k keys are in LDS -- no n x k index array goes through HBM:
//   d_i = neighbour_i - query in f64 (lanes 0 .. k-1); 3 first and 6 second moments summed over the wave by a fixed butterfly;
//   C = (sum d d^T) / k - (sum d / k)(sum d / k)^T;  the eigenpairs of C by cyclic Jacobi in f64;
//   normal = the unit eigenvector of the smallest eigenvalue l0, curvature = (float)|l0 / (l0 + l1 + l2)|, 0 when the trace is 0;
//   flipped when, with v = viewpoint - p in float, (v.x * nx + v.y * ny) + v.z * nz < 0 (float, no contraction).
//   A neighbourhood whose points all coincide (trace 0): (0, 0, 1) before the flip, curvature 0.
//
// STATED DEVIATION FROM PCL.  PCL's computeMeanAndCovarianceMatrix accumulates nine raw moments about the ORIGIN in float,
// in FLANN's neighbour order: at 2 m range with centimetre neighbourhoods that loses percent-level accuracy in C, and under
// ties it is not reproducible.  Here the covariance is the one the formula defines, in f64, about the query point, and the
// result depends on nothing but the cloud: not on the grid, the launch or the run.  A PCL build agrees with it to PCL's own
// rounding.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "knn_kernels.hpp"

namespace rsreg {

// ------------------------------------------------------------------------------ search
// rsreg_cloud_knn: row `record` of index_out (k int32, nullable) and of d2_out (k floats, nullable), queries in cell order.  The
// rows of non-finite records have been filled before the launch.
__global__ __launch_bounds__(kKnnWave) void k_knn_indices(PointGridDev g, int k, int32_t *index_out, float *d2_out)
{
    __shared__ unsigned long long buf[kKnnBuf];
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        knn_walk<KnnKeys>(g, q, k, buf, lane);
        if (lane < k) {
            const unsigned long long key = buf[lane];
            const size_t at = (size_t)__float_as_uint(q.w) * (size_t)k + (size_t)lane;
            if (index_out) index_out[at] = (int32_t)(uint32_t)key;
            if (d2_out) d2_out[at] = __uint_as_float((uint32_t)(key >> 32));
        }
        __syncthreads();   // (the next query appends to the same buffer)
    }
}

// ------------------------------------------------------------------------------ normals
// the sum of v over the 64 lanes, the same bits in every lane: a butterfly, so every lane adds the same pairs in the same order
__device__ __forceinline__ double wave_sum_fixed(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Eigenvalues (ascending in ev) of the symmetric 3 x 3 matrix {a00, a01, a02, a11, a12, a22} and the unit eigenvector of the
// smallest, by cyclic Jacobi in f64 (the rotations of host_linalg.hpp's eig_sym3; every index a compile-time constant).
__device__ inline void eig_sym3_smallest(const double (&c)[6], double (&ev)[3], double (&vec)[3])
{
#pragma clang fp contract(off)
    double A[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]}, V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
        const double dia = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
        if (off <= 1e-36 * dia || off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p * 3 + q];
                if (apq == 0.0) continue;
                const double th = (A[q * 3 + q] - A[p * 3 + p]) / (2.0 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double a = A[i * 3 + p], b = A[i * 3 + q];
                    A[i * 3 + p] = cs * a - sn * b;
                    A[i * 3 + q] = sn * a + cs * b;
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double a = A[p * 3 + i], b = A[q * 3 + i];
                    A[p * 3 + i] = cs * a - sn * b;
                    A[q * 3 + i] = sn * a + cs * b;
                }
                A[p * 3 + q] = A[q * 3 + p] = 0.0;   // (what the rotation was chosen for)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double a = V[i * 3 + p], b = V[i * 3 + q];
                    V[i * 3 + p] = cs * a - sn * b;
                    V[i * 3 + q] = sn * a + cs * b;
                }
            }
    }
    const double d0 = A[0], d1 = A[4], d2 = A[8];
    int o0 = 0, o1 = 1, o2 = 2;   // ascending; equal values keep their order
    if (pick3(d0, d1, d2, o1) < pick3(d0, d1, d2, o0)) { const int t = o0; o0 = o1; o1 = t; }
    if (pick3(d0, d1, d2, o2) < pick3(d0, d1, d2, o0)) { const int t = o0; o0 = o2; o2 = t; }
    if (pick3(d0, d1, d2, o2) < pick3(d0, d1, d2, o1)) { const int t = o1; o1 = o2; o2 = t; }
    ev[0] = pick3(d0, d1, d2, o0);
    ev[1] = pick3(d0, d1, d2, o1);
    ev[2] = pick3(d0, d1, d2, o2);
    const double x = pick3(V[0], V[1], V[2], o0), y = pick3(V[3], V[4], V[5], o0), z = pick3(V[6], V[7], V[8], o0);
    const double inv = 1.0 / sqrt((x * x + y * y) + z * z);   // (orthogonal up to rounding: the norm is 1 within a few ulp)
    vec[0] = x * inv;
    vec[1] = y * inv;
    vec[2] = z * inv;
}

// the 32-byte pcl::Normal records of the non-finite input records: four quiet NaNs (normal and curvature), pads 0
__global__ __launch_bounds__(kBlock) void k_normals_not_finite(const char *rec, size_t stride, uint32_t n, float *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    if (finite3(p[0], p[1], p[2])) return;
    const float qnan = __uint_as_float(0x7fc00000u);
    float4 *o = reinterpret_cast<float4 *>(out + (size_t)i * 8);
    o[0] = make_float4(qnan, qnan, qnan, 0.0f);
    o[1] = make_float4(qnan, 0.0f, 0.0f, 0.0f);
}

// The covariance {xx, xy, xz, yy, yz, zz} of kk neighbours about the query from their nine moment sums: S / kk - m m^T.  One place
// for the normals (k neighbours, a radius) and the GICP covariances (gicp_cov_kernels.hpp): the same operations in the same order.
__device__ __forceinline__ void cov_about_query(double kk, double sx, double sy, double sz, double sxx, double sxy, double sxz, double syy, double syz,
                                                double szz, double (&c)[6])
{
#pragma clang fp contract(off)
    const double mx = sx / kk, my = sy / kk, mz = sz / kk;
    c[0] = sxx / kk - mx * mx;
    c[1] = sxy / kk - mx * my;
    c[2] = sxz / kk - mx * mz;
    c[3] = syy / kk - my * my;
    c[4] = syz / kk - my * mz;
    c[5] = szz / kk - mz * mz;
}

// The nine moment sums {x, y, z, xx, xy, xz, yy, yz, zz} of (neighbour - query) in f64 over the k neighbours whose keys knn_walk left
// in buf, the same bits in every lane.  A barrier stands between the lanes' reads of the keys and the return: the caller may search
// the next query at once.
__device__ __forceinline__ void knn_moment_sums(const unsigned long long *buf, int k, const char *rec, size_t stride, const float4 &q, int lane, double (&s)[9])
{
#pragma clang fp contract(off)
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (lane < k) {
        const float *t = rec_xyz(rec, stride, (size_t)(uint32_t)buf[lane]);
        dx = (double)t[0] - (double)q.x;
        dy = (double)t[1] - (double)q.y;
        dz = (double)t[2] - (double)q.z;
    }
    __syncthreads();   // (the keys have been read: the next query may append)
    s[0] = wave_sum_fixed(dx);
    s[1] = wave_sum_fixed(dy);
    s[2] = wave_sum_fixed(dz);
    s[3] = wave_sum_fixed(dx * dx);
    s[4] = wave_sum_fixed(dx * dy);
    s[5] = wave_sum_fixed(dx * dz);
    s[6] = wave_sum_fixed(dy * dy);
    s[7] = wave_sum_fixed(dy * dz);
    s[8] = wave_sum_fixed(dz * dz);
}

// The tail of both estimators (k neighbours here, the neighbours within a radius in radius_kernels.hpp), by every lane of the wave that
// holds the sums over the kk neighbours of the query q (the same bits in every lane): the covariance, its smallest eigenpair, the
// curvature, the flip towards the viewpoint; lanes 0 .. 7 write the record `q.w` of out.
__device__ __forceinline__ void normal_from_sums(const float4 &q, double kk, double sx, double sy, double sz, double sxx, double sxy, double sxz, double syy,
                                                 double syz, double szz, float vpx, float vpy, float vpz, int lane, float *out)
{
#pragma clang fp contract(off)
    double c[6];
    cov_about_query(kk, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, c);
    const double trace = (c[0] + c[3]) + c[5];
    float nx = 0.0f, ny = 0.0f, nz = 1.0f, curv = 0.0f;
    if (trace != 0.0) {
        double ev[3], vec[3];
        eig_sym3_smallest(c, ev, vec);
        nx = (float)vec[0];
        ny = (float)vec[1];
        nz = (float)vec[2];
        const double sum = (ev[0] + ev[1]) + ev[2];
        curv = sum != 0.0 ? (float)fabs(ev[0] / sum) : 0.0f;
    }
    const float vx = __fsub_rn(vpx, q.x), vy = __fsub_rn(vpy, q.y), vz = __fsub_rn(vpz, q.z);
    const float cos_view = __fadd_rn(__fadd_rn(__fmul_rn(vx, nx), __fmul_rn(vy, ny)), __fmul_rn(vz, nz));
    if (cos_view < 0.0f) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    if (lane < 8) {
        const float v = lane == 0 ? nx : (lane == 1 ? ny : (lane == 2 ? nz : (lane == 4 ? curv : 0.0f)));
        out[(size_t)__float_as_uint(q.w) * 8 + (size_t)lane] = v;
    }
}

// One workgroup of ONE wave per query, queries in cell order: the search, then the normal of the k neighbours while their keys
// are in LDS.  out: record `record` = {normal_x, normal_y, normal_z, 0, curvature, 0, 0, 0}.
__global__ __launch_bounds__(kKnnWave) void k_normals(PointGridDev g, int k, const char *rec, size_t stride, float vpx, float vpy, float vpz, float *out)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long buf[kKnnBuf];
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        knn_walk<KnnKeys>(g, q, k, buf, lane);
        double s[9];
        knn_moment_sums(buf, k, rec, stride, q, lane, s);
        normal_from_sums(q, (double)k, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], vpx, vpy, vpz, lane, out);
    }
}

}  // namespace rsreg
