// depthcloud_kernels.hpp — the capture step on the device: a depth frame and a colour frame -> the 32-byte PointXYZRGB records
// of an organized cloud (include/rsreg.h, "capture", states the contract; recalled from librealsense 2.3x).  Included by
// depthcloud.hip only.
//
//   k_depth_to_cloud   one lane per record of the cloud.  Lanes of the window read their uint16 depth (neighbouring lanes,
//                      neighbouring pixels: coalesced), compute the vertex and the texture coordinate in registers, gather three
//                      colour bytes, and write the record as two 16-byte stores; lanes past the window write the default
//                      record.  No atomics, no LDS: the kernel is bound by its 32 bytes out per pixel against 5 in.
//
// Every float operation is spelled with the round-to-nearest intrinsics, one per operation of the contract, so that no two of
// them can be contracted whatever the build's flags are.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "depthcloud_plan.hpp"
#include "records.hpp"

namespace rsreg {

#define RSREG_DC_M(a, b) __fmul_rn((a), (b))
#define RSREG_DC_A(a, b) __fadd_rn((a), (b))

// f = 1 + k0*r2 + k1*r2*r2 + k4*r2*r2*r2, as C parses it
__device__ __forceinline__ float depth_radial(const float *k, float r2)
{
    const float a = RSREG_DC_A(1.0f, RSREG_DC_M(k[0], r2));
    const float b = RSREG_DC_A(a, RSREG_DC_M(RSREG_DC_M(k[1], r2), r2));
    return RSREG_DC_A(b, RSREG_DC_M(RSREG_DC_M(RSREG_DC_M(k[4], r2), r2), r2));
}

// s + 2*ka*x*y + kb*(r2 + 2*a*a): the tangential terms behind s (= x*f, or the scaled x)
__device__ __forceinline__ float depth_tangential(float s, float ka, float kb, float x, float y, float r2, float a)
{
    const float t1 = RSREG_DC_M(RSREG_DC_M(RSREG_DC_M(2.0f, ka), x), y);
    const float t2 = RSREG_DC_M(kb, RSREG_DC_A(r2, RSREG_DC_M(RSREG_DC_M(2.0f, a), a)));
    return RSREG_DC_A(RSREG_DC_A(s, t1), t2);
}

// (int)(uv * size + .5f) clamped to [0, size - 1]; a value C leaves undefined (NaN, outside [-2^31, 2^31)) is INT_MIN, as on
// x86, and so 0 -- written out: the conversion instruction here would saturate +inf to INT_MAX
__device__ __forceinline__ int depth_texel(float uv, float size_f, int size)
{
    const float t = RSREG_DC_A(RSREG_DC_M(uv, size_f), 0.5f);
    const int v = (t >= -2147483648.0f && t < 2147483648.0f) ? (int)t : (int)0x80000000;
    return min(max(v, 0), size - 1);
}

__global__ __launch_bounds__(kBlock) void k_depth_to_cloud(const unsigned char *__restrict__ depth, const unsigned char *__restrict__ color,
                                                           const DepthPlan p, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= p.n) return;
    uint4 lo = make_uint4(0u, 0u, 0u, __float_as_uint(1.0f)), hi = make_uint4(0xff000000u, 0u, 0u, 0u);   // a default PointXYZRGB
    if (i < p.count) {
        const uint32_t wr = i / p.win_cols, wc = i - wr * p.win_cols;
        const int r = p.r0 + (int)wr, c = p.c0 + (int)wc;
        const uint16_t d = *reinterpret_cast<const uint16_t *>(depth + (size_t)r * p.depth_stride + (size_t)c * 2);
        // (1) the vertex
        const float z = RSREG_DC_M(p.depth_scale, (float)d);
        float x = __fdiv_rn(__fsub_rn((float)c, p.d_ppx), p.d_fx);
        float y = __fdiv_rn(__fsub_rn((float)r, p.d_ppy), p.d_fy);
        if (p.d_inverse) {
            const float r2 = RSREG_DC_A(RSREG_DC_M(x, x), RSREG_DC_M(y, y));
            const float f = depth_radial(p.dk, r2);
            const float ux = depth_tangential(RSREG_DC_M(x, f), p.dk[2], p.dk[3], x, y, r2, x);
            const float uy = depth_tangential(RSREG_DC_M(y, f), p.dk[3], p.dk[2], x, y, r2, y);
            x = ux;
            y = uy;
        }
        const float px = RSREG_DC_M(z, x), py = RSREG_DC_M(z, y);
        // (2) the texture coordinate
        float u = 0.0f, v = 0.0f;
        if (!(z == 0.0f)) {
            float q[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                q[k] = RSREG_DC_A(RSREG_DC_A(RSREG_DC_A(RSREG_DC_M(p.R[0 + k], px), RSREG_DC_M(p.R[3 + k], py)), RSREG_DC_M(p.R[6 + k], z)), p.t[k]);
            float tx = __fdiv_rn(q[0], q[2]), ty = __fdiv_rn(q[1], q[2]);
            if (p.c_modified) {
                const float r2 = RSREG_DC_A(RSREG_DC_M(tx, tx), RSREG_DC_M(ty, ty));
                const float f = depth_radial(p.ck, r2);
                tx = RSREG_DC_M(tx, f);
                ty = RSREG_DC_M(ty, f);
                const float dx = depth_tangential(tx, p.ck[2], p.ck[3], tx, ty, r2, tx);
                const float dy = depth_tangential(ty, p.ck[3], p.ck[2], tx, ty, r2, ty);
                tx = dx;
                ty = dy;
            }
            u = __fdiv_rn(RSREG_DC_A(RSREG_DC_M(tx, p.c_fx), p.c_ppx), p.c_wf);
            v = __fdiv_rn(RSREG_DC_A(RSREG_DC_M(ty, p.c_fy), p.c_ppy), p.c_hf);
        }
        // (3) the colour: a byte gather
        const int xi = depth_texel(u, p.c_wf, p.c_w), yi = depth_texel(v, p.c_hf, p.c_h);
        const unsigned char *pix = color + (size_t)yi * p.color_stride + (size_t)xi * (size_t)p.bpp;
        const uint32_t cr = pix[p.r_off], cg = pix[1], cb = pix[p.b_off];
        lo.x = __float_as_uint(px), lo.y = __float_as_uint(py), lo.z = __float_as_uint(z);
        hi.x = 0xff000000u | (cr << 16) | (cg << 8) | cb;
    }
    // (4) the record: two 16-byte stores, 32 contiguous bytes a lane
    out[2 * (size_t)i] = lo;
    out[2 * (size_t)i + 1] = hi;
}

#undef RSREG_DC_M
#undef RSREG_DC_A

}  // namespace rsreg
