// gicp_kernels.hpp — device code of the GICP alignment (pcl::GeneralizedIterativeClosestPoint, plane-to-plane ICP): the per-pair
// Mahalanobis matrix and the 32 sums of include/rsreg.h (RSREG_NUM_GICP_SUMS) at an increment X, over the pairs the staged search
// kept.  Included by icp.hip behind plane_kernels.hpp: the tile reduction is plane_tile_reduce_store, so a sum here goes through
// the addition tree a plane sum and a point-to-point sum go through.  (The covariances themselves: gicp_cov_kernels.hpp.)
#pragma once

#include "plane_kernels.hpp"

namespace rsreg {

// rows of the 3 x 4 part of a double 4 x 4, by value in the kernel arguments: the increment X, or (columns 0 .. 2) the rotation R
struct Mat34d {
    double r0[4], r1[4], r2[4];
};

// six doubles at `in + i * stride` -> record i of out (the covariances of a device cloud: stride 48 or any multiple of 8 above)
__global__ __launch_bounds__(kBlock) void k_gicp_pack_cov(const char *in, size_t stride, uint32_t n, double *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = reinterpret_cast<const double *>(in + (size_t)i * stride);
#pragma unroll
    for (int k = 0; k < 6; ++k) out[(size_t)i * 6 + k] = r[k];
}

__device__ __forceinline__ bool finite6(const double (&c)[6])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && fabs(c[k]) <= 1.7976931348623157e308;   // (false for NaN and +-inf)
    return ok;
}

// M = (C_t[j] + R C_s[i] R^T)^-1 of every kept pair, six doubles {xx, xy, xz, yy, yz, zz} per distinct source point u; a pair with
// a non-finite covariance on either side, or whose inverse is not finite, gets six quiet NaNs (the marker k_gicp_reduce reads in
// M.xx); an entry without a pair is not written.  src_rec[u] = perm[first[u]]: the caller's index of the first copy of u (exact
// copies share their covariance).  The operation order is the header's:
//   B = R C_s:  B_rc = (R_r0 C_0c + R_r1 C_1c) + R_r2 C_2c;   D = B R^T (c >= r):  D_rc = (B_r0 R_c0 + B_r1 R_c1) + B_r2 R_c2
//   A = C_t + D;  adjugate: a00 = A11 A22 - A12 A12, a01 = A02 A12 - A01 A22, a02 = A01 A12 - A02 A11, a11 = A00 A22 - A02 A02,
//   a12 = A01 A02 - A00 A12, a22 = A00 A11 - A01 A01;  det = (A00 a00 + A01 a01) + A02 a02;  M_ab = a_ab * (1 / det)
__global__ __launch_bounds__(kBlock) void k_gicp_mahalanobis(const int *corr_pos, const float4 *tgt, const uint32_t *perm, const uint32_t *first,
                                                             const double *cov_s, const double *cov_t, Mat34d R, uint32_t n, double *m_out)
{
#pragma clang fp contract(off)
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const int pos = corr_pos[u];
    if (pos < 0) return;
    const size_t is = perm[first[u]], it = tgt_idx(tgt[pos]);
    double cs[6], ct[6], m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        cs[k] = cov_s[is * 6 + k];
        ct[k] = cov_t[it * 6 + k];
    }
    bool ok = finite6(cs) && finite6(ct);
    if (ok) {
        const double C[3][3] = {{cs[0], cs[1], cs[2]}, {cs[1], cs[3], cs[4]}, {cs[2], cs[4], cs[5]}};
        const double Rm[3][3] = {{R.r0[0], R.r0[1], R.r0[2]}, {R.r1[0], R.r1[1], R.r1[2]}, {R.r2[0], R.r2[1], R.r2[2]}};
        double B[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) B[r][c] = (Rm[r][0] * C[0][c] + Rm[r][1] * C[1][c]) + Rm[r][2] * C[2][c];
        double A[6];
        int k = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) {
                A[k] = ct[k] + ((B[r][0] * Rm[c][0] + B[r][1] * Rm[c][1]) + B[r][2] * Rm[c][2]);
                ++k;
            }
        const double a00 = A[3] * A[5] - A[4] * A[4], a01 = A[2] * A[4] - A[1] * A[5], a02 = A[1] * A[4] - A[2] * A[3];
        const double a11 = A[0] * A[5] - A[2] * A[2], a12 = A[1] * A[2] - A[0] * A[4], a22 = A[0] * A[3] - A[1] * A[1];
        const double det = (A[0] * a00 + A[1] * a01) + A[2] * a02;
        const double inv = 1.0 / det;
        m[0] = a00 * inv;
        m[1] = a01 * inv;
        m[2] = a02 * inv;
        m[3] = a11 * inv;
        m[4] = a12 * inv;
        m[5] = a22 * inv;
        ok = finite6(m);
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int k = 0; k < 6; ++k) m_out[(size_t)u * 6 + k] = ok ? m[k] : qnan;
}

// The mapping of k_plane_reduce: one distinct source point per thread, block b covers points [b*128, b*128+128), the pair's weight
// W is the multiplicity cur[i].w of merged source copies.  With p' = X p (p float -> double), e = q - p', J = [-[p']x | I3]:
//   p'_r = ((X_r0 p.x + X_r1 p.y) + X_r2 p.z) + X_r3;   g = M e:  g_r = (M_r0 e_0 + M_r1 e_1) + M_r2 e_2;   cost = (e_0 g_0 + e_1 g_1) + e_2 g_2
//   G = [p']x M (column c: p' x M_.c):  G_0c = p'y M_2c - p'z M_1c,  G_1c = p'z M_0c - p'x M_2c,  G_2c = p'x M_1c - p'y M_0c
//   H rot-rot (r <= c) = G [p']x^T:  H_r0 = G_r2 p'y - G_r1 p'z,  H_r1 = G_r0 p'z - G_r2 p'x,  H_r2 = G_r1 p'x - G_r0 p'y
//   H rot-trans = G,  H trans-trans = M;   b rot = p' x g,  b trans = g
// every operation rounded once; a pair's 32 terms are W times these, whatever the launch.
__global__ __launch_bounds__(kTile) void k_gicp_reduce(const float4 *cur, const int *corr_pos, const float *corr_d2, const float4 *tgt, const double *mah,
                                                       Mat34d X, uint32_t n, double *partials)
{
#pragma clang fp contract(off)
    double a[RSREG_NUM_GICP_SUMS];
#pragma unroll
    for (int k = 0; k < RSREG_NUM_GICP_SUMS; ++k) a[k] = 0.0;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int pos = corr_pos[i];
        if (pos >= 0) {
            const float4 p = cur[i];
            const float4 q = tgt[pos];
            const double W = (double)p.w;
            a[0] = W;
            a[1] = W * (double)corr_d2[i];
            const double m00 = mah[(size_t)i * 6];
            if (m00 == m00) {
                const double m01 = mah[(size_t)i * 6 + 1], m02 = mah[(size_t)i * 6 + 2], m11 = mah[(size_t)i * 6 + 3], m12 = mah[(size_t)i * 6 + 4],
                             m22 = mah[(size_t)i * 6 + 5];
                const double px = p.x, py = p.y, pz = p.z;
                const double x = ((X.r0[0] * px + X.r0[1] * py) + X.r0[2] * pz) + X.r0[3];
                const double y = ((X.r1[0] * px + X.r1[1] * py) + X.r1[2] * pz) + X.r1[3];
                const double z = ((X.r2[0] * px + X.r2[1] * py) + X.r2[2] * pz) + X.r2[3];
                const double e0 = (double)q.x - x, e1 = (double)q.y - y, e2 = (double)tgt_z(q) - z;
                const double g0 = (m00 * e0 + m01 * e1) + m02 * e2, g1 = (m01 * e0 + m11 * e1) + m12 * e2, g2 = (m02 * e0 + m12 * e1) + m22 * e2;
                const double M[3][3] = {{m00, m01, m02}, {m01, m11, m12}, {m02, m12, m22}};
                double G[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    G[0][c] = y * M[2][c] - z * M[1][c];
                    G[1][c] = z * M[0][c] - x * M[2][c];
                    G[2][c] = x * M[1][c] - y * M[0][c];
                }
                double H[6][6];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    H[r][0] = G[r][2] * y - G[r][1] * z;
                    H[r][1] = G[r][0] * z - G[r][2] * x;
                    H[r][2] = G[r][1] * x - G[r][0] * y;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        H[r][3 + c] = G[r][c];
                        H[3 + r][3 + c] = M[r][c];
                    }
                }
                a[2] = W;
                a[3] = W * ((e0 * g0 + e1 * g1) + e2 * g2);
                int k = 4;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = r; c < 6; ++c) a[k++] = W * H[r][c];
                a[25] = W * (y * g2 - z * g1);
                a[26] = W * (z * g0 - x * g2);
                a[27] = W * (x * g1 - y * g0);
                a[28] = W * g0;
                a[29] = W * g1;
                a[30] = W * g2;
            }
        }
    }
    plane_tile_reduce_store(a, partials, gridDim.x, blockIdx.x);
}

}  // namespace rsreg
