// iinormals_kernels.hpp — pcl::IntegralImageNormalEstimation (AVERAGE_3D_GRADIENT, border policy IGNORE, no depth-dependent
// smoothing) on an organized frame: device code of rsreg_cloud_integral_normals (include/rsreg.h states the contract, recalled
// from PCL 1.9.1 features/impl/integral_image_normal.hpp).  Included by iinormals.hip only.
//
//   k_iin_prepare   the depth-change map as the distance map's start (0 at a depth change, w + h elsewhere) and the two
//                   difference images, one thread per pixel;
//   k_iin_chamfer   one of the two chamfer passes of the distance map, one workgroup per band of rows;
//   k_iin_normals   the window size, the window's two sums and the normal, one thread per pixel.
//
// The passes.  As PCL writes them they are 2 x w x h dependent steps.  What they compute is
//   D[r][c] = min(D0[r][c], D[r-1][c-1] + 1.4f, D[r-1][c] + 1.0f, D[r-1][c+1] + 1.4f, D[r][c-1] + 1.0f)
// (min of floats does not depend on its order), and the backward pass is the forward pass on the array read back to front:
// flat index n - 1 - i.  PCL's flat indexing makes "up-right" of the last column the FIRST column of the same row, which the
// pass never writes: a value that is there before the pass starts.  Only values below min(D, s) + 1 can reach the output, and
// x -> fl(x + 1.0f), x -> fl(x + 1.4f) are monotone and add at least 1 - 1e-5 below 128.  So a value v comes from a chain of
// strictly smaller values that climbs at most v / (1 - 1e-5) rows and, inside a row, runs back at most as many columns:
//   * a band of rows that starts `halo` rows early from the values as they were before the pass gives, in its own rows, the
//     sequential pass's bits wherever those are below halo * (1 - 1e-5), and something not smaller elsewhere;
//   * inside a row, D[c] = min(a[c], fl(D[c-1] + 1.0f)) is evaluated from a[c - look] on, adding the 1.0f `look` times in
//     sequence -- fl(fl(a + 1) + 1), never a + 2.
// The host passes halo = look = (int)s + 3: exact below s + 2, which is all min(D, s) and (int) of it can see.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "records.hpp"

namespace rsreg {

constexpr int kIinBand = 8;          // rows of the distance map a workgroup of a pass owns
constexpr int kIinMaxWidth = 8192;   // two rows of floats in LDS
constexpr int kIinTile = 16;         // k_iin_normals: 16 x 16 pixels a workgroup, so that its windows share the L1

struct IinGrad {   // the differences of one pixel: {x, y, z, 1 if (x + y) + z is finite else 0}
    float4 dx, dy;
};

__device__ __forceinline__ bool iin_depth_change(float zc, float zn, float factor)
{
    const float t = __fmul_rn(__fmul_rn(factor, __fadd_rn(fabsf(zc), 1.0f)), 2.0f);
    return fabsf(__fsub_rn(zc, zn)) > t || !isfinite(zc) || !isfinite(zn);
}

__device__ __forceinline__ float4 iin_diff(const float *a, const float *b)
{
    const float x = __fsub_rn(a[0], b[0]), y = __fsub_rn(a[1], b[1]), z = __fsub_rn(a[2], b[2]);
    return make_float4(x, y, z, isfinite(__fadd_rn(__fadd_rn(x, y), z)) ? 1.0f : 0.0f);
}

// dist0[i] = 0 where pixel i takes part in a depth change (as the centre of PCL's loop over [0, h-1) x [0, w-1), or as its
// right or lower neighbour), (float)(w + h) elsewhere; grad[i] = the central differences, zero on the frame's outer ring.
__global__ __launch_bounds__(kBlock) void k_iin_prepare(const char *rec, size_t stride, int w, int h, float factor, float *dist0, IinGrad *grad)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)w * (size_t)h) return;
    const int r = (int)(i / (size_t)w), c = (int)(i % (size_t)w);
    const float *p = rec_xyz(rec, stride, i);
    const float z = p[2];
    bool edge = false;
    if (r < h - 1 && c < w - 1)
        edge = iin_depth_change(z, rec_xyz(rec, stride, i + 1)[2], factor) || iin_depth_change(z, rec_xyz(rec, stride, i + (size_t)w)[2], factor);
    if (!edge && c >= 1 && r < h - 1) edge = iin_depth_change(rec_xyz(rec, stride, i - 1)[2], z, factor);
    if (!edge && r >= 1 && c < w - 1) edge = iin_depth_change(rec_xyz(rec, stride, i - (size_t)w)[2], z, factor);
    dist0[i] = edge ? 0.0f : (float)(w + h);
    IinGrad g;
    g.dx = g.dy = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if (r >= 1 && r < h - 1 && c >= 1 && c < w - 1) {
        g.dx = iin_diff(rec_xyz(rec, stride, i + 1), rec_xyz(rec, stride, i - 1));
        g.dy = iin_diff(rec_xyz(rec, stride, i + (size_t)w), rec_xyz(rec, stride, i - (size_t)w));
    }
    grad[i] = g;
}

// One chamfer pass over src into dst (two different arrays: a band's halo rows read what another band owns).  Workgroup b owns
// the rows [b * kIinBand, (b + 1) * kIinBand) of the pass's own numbering -- rev: row and column counted from the far corner --
// and starts `halo` rows before them.  LDS: 2 * w floats.
__global__ __launch_bounds__(kBlock) void k_iin_chamfer(const float *src, float *dst, int w, int h, int halo, int look, int rev)
{
    extern __shared__ float iin_rows[];
    float *prev = iin_rows, *cur = iin_rows + w;
    const size_t last = (size_t)w * (size_t)h - 1;
    const int tid = (int)threadIdx.x;
    const int r0 = (int)blockIdx.x * kIinBand, r1 = min(r0 + kIinBand, h), ra = max(r0 - halo, 0);
    {
        const size_t row = (size_t)ra * (size_t)w;
        for (int c = tid; c < w; c += kBlock) {
            const size_t i = rev ? last - (row + (size_t)c) : row + (size_t)c;
            const float v = src[i];
            prev[c] = v;
            if (ra == r0) dst[i] = v;   // (row 0: no pass writes it)
        }
    }
    __syncthreads();
    for (int r = ra + 1; r < r1; ++r) {
        const size_t row = (size_t)r * (size_t)w;
        const float first = src[rev ? last - row : row];   // column 0 of this row, which the pass leaves as it is
        for (int c = tid; c < w; c += kBlock) {
            float a = src[rev ? last - (row + (size_t)c) : row + (size_t)c];
            if (c > 0) {
                const float ul = __fadd_rn(prev[c - 1], 1.4f), up = __fadd_rn(prev[c], 1.0f);
                const float ur = __fadd_rn(c + 1 < w ? prev[c + 1] : first, 1.4f);
                a = fminf(fminf(a, ul), fminf(up, ur));
            }
            cur[c] = a;
        }
        __syncthreads();   // (everyone has read prev: it may take the new row)
        for (int c = tid; c < w; c += kBlock) {
            int j = max(c - look, 0);
            float t = cur[j];
            for (++j; j <= c; ++j) t = fminf(cur[j], __fadd_rn(t, 1.0f));
            prev[c] = t;
            if (r >= r0) dst[rev ? last - (row + (size_t)c) : row + (size_t)c] = t;
        }
        __syncthreads();
    }
}

// Pixel (r, c): the window size R = (int)min(D, s) inside the border of `border` pixels where z is finite and min(D, s) > 2,
// the f64 sums of the finite differences over columns [c - R/2, c - R/2 + R) and rows [r - R/2, r - R/2 + R), row by row, and
// the normal gy x gx.  R <= border, so the window lies inside the frame: c - R/2 >= border - border/2 >= 0 and
// c - R/2 + R <= w - border - 1 + (R + 1) / 2 < w.  out: {normal_x, normal_y, normal_z, 0, curvature = NaN, 0, 0, 0}.
__global__ __launch_bounds__(kIinTile * kIinTile) void k_iin_normals(const char *rec, size_t stride, int w, int h, const float *dist, const IinGrad *grad,
                                                                     float smoothing, int border, float vpx, float vpy, float vpz, float *out,
                                                                     uint8_t *rect)
{
#pragma clang fp contract(off)
    const int c = (int)blockIdx.x * kIinTile + (int)(threadIdx.x % kIinTile), r = (int)blockIdx.y * kIinTile + (int)(threadIdx.x / kIinTile);
    if (c >= w || r >= h) return;
    const size_t i = (size_t)r * (size_t)w + (size_t)c;
    const float qnan = __uint_as_float(0x7fc00000u);
    const float *p = rec_xyz(rec, stride, i);
    int R = 0;
    if (r >= border && r < h - border && c >= border && c < w - border && isfinite(p[2])) {
        const float sm = fminf(dist[i], smoothing);
        if (sm > 2.0f) R = (int)sm;
    }
    float nx = qnan, ny = qnan, nz = qnan;
    if (R > 0) {
        double gx0 = 0.0, gx1 = 0.0, gx2 = 0.0, gy0 = 0.0, gy1 = 0.0, gy2 = 0.0;
        uint32_t cnt_x = 0, cnt_y = 0;
        const int c0 = c - R / 2, rr0 = r - R / 2;
        for (int rr = rr0; rr < rr0 + R; ++rr) {
            const IinGrad *g = grad + (size_t)rr * (size_t)w + (size_t)c0;
            for (int k = 0; k < R; ++k) {
                const float4 dx = g[k].dx, dy = g[k].dy;
                if (dx.w != 0.0f) {
                    gx0 += (double)dx.x;
                    gx1 += (double)dx.y;
                    gx2 += (double)dx.z;
                    ++cnt_x;
                }
                if (dy.w != 0.0f) {
                    gy0 += (double)dy.x;
                    gy1 += (double)dy.y;
                    gy2 += (double)dy.z;
                    ++cnt_y;
                }
            }
        }
        if (cnt_x != 0 && cnt_y != 0) {
            const double n0 = __dsub_rn(__dmul_rn(gy1, gx2), __dmul_rn(gy2, gx1));
            const double n1 = __dsub_rn(__dmul_rn(gy2, gx0), __dmul_rn(gy0, gx2));
            const double n2 = __dsub_rn(__dmul_rn(gy0, gx1), __dmul_rn(gy1, gx0));
            const double l = __dadd_rn(__dadd_rn(__dmul_rn(n0, n0), __dmul_rn(n1, n1)), __dmul_rn(n2, n2));
            if (l != 0.0) {
                const double len = __dsqrt_rn(l);
                nx = (float)__ddiv_rn(n0, len);
                ny = (float)__ddiv_rn(n1, len);
                nz = (float)__ddiv_rn(n2, len);
                const float vx = __fsub_rn(vpx, p[0]), vy = __fsub_rn(vpy, p[1]), vz = __fsub_rn(vpz, p[2]);
                const float cos_view = __fadd_rn(__fadd_rn(__fmul_rn(vx, nx), __fmul_rn(vy, ny)), __fmul_rn(vz, nz));
                if (cos_view < 0.0f) {
                    nx = -nx;
                    ny = -ny;
                    nz = -nz;
                }
            }
        }
    }
    float4 *o = reinterpret_cast<float4 *>(out + i * 8);
    o[0] = make_float4(nx, ny, nz, 0.0f);
    o[1] = make_float4(qnan, 0.0f, 0.0f, 0.0f);
    rect[i] = (uint8_t)R;
}

}  // namespace rsreg
