// depthcloud_plan.hpp — rsreg_depth_params checked and flattened: what both implementations of the capture step start from
// (depth_host.cpp, the sequential restatement; depthcloud.hip, whose kernel takes the plan by value).  include/rsreg.h,
// "capture", is the contract; nothing here is arithmetic on pixel values.  Plain C++, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rsreg.h"

namespace rsreg {

struct DepthPlan {
    float d_ppx, d_ppy, d_fx, d_fy, dk[5];   // depth intrinsics
    float c_ppx, c_ppy, c_fx, c_fy, ck[5];   // colour intrinsics
    float c_wf, c_hf;                        // (float)width, (float)height of the colour image
    float R[9], t[3], depth_scale;
    int d_inverse, c_modified;               // 1: the inverse / the modified Brown-Conrady form applies
    int c_w, c_h, bpp, r_off, b_off;         // colour image; where the r and the b byte of a pixel are (g is byte 1)
    int r0, c0;                              // the window's first row and column
    uint32_t win_rows, win_cols, count, n;   // rows and columns of the window, its pixels, records of the cloud
    uint32_t out_width, out_height;
    int is_dense;
    size_t depth_stride, color_stride;       // bytes
    size_t depth_bytes, color_bytes;         // what is read of either image, from its first byte
};

inline bool depth_coeffs_zero(const float k[5])
{
    for (int i = 0; i < 5; ++i)
        if (!(k[i] == 0.0f)) return false;
    return true;
}

// 0: no distortion applies; 1: `own` applies; -1: refused
inline int depth_model_use(const rsreg_intrinsics &in, int own)
{
    if (in.model < RSREG_DISTORTION_NONE || in.model > RSREG_DISTORTION_KANNALA_BRANDT4) return -1;
    if (in.model == RSREG_DISTORTION_NONE) return 0;
    if (in.model == own) return 1;
    return depth_coeffs_zero(in.coeffs) ? 0 : -1;
}

inline int depth_plan(const rsreg_depth_params *p, size_t depth_stride, size_t color_stride, DepthPlan *out, const char **why)
{
    auto bad = [&](const char *w) { if (why) *why = w; return (int)RSREG_ERR_INVALID_ARG; };
    if (!p || !out) return bad("no parameters");
    const rsreg_intrinsics &d = p->depth, &c = p->color;
    if (d.width <= 0 || d.height <= 0 || c.width <= 0 || c.height <= 0) return bad("an image has a zero size");
    if (p->out_width == 0 || p->out_height == 0) return bad("the cloud has a zero size");
    if (p->color_bytes_per_pixel != 3 && p->color_bytes_per_pixel != 4) return bad("3 or 4 bytes per colour pixel");
    if (depth_stride < 2 * (size_t)d.width || (depth_stride & 1)) return bad("the depth stride is smaller than a row, or odd");
    if (color_stride < (size_t)p->color_bytes_per_pixel * (size_t)c.width) return bad("the colour stride is smaller than a row");
    if (p->r0 < 0 || p->r0 > p->r1 || p->r1 > d.height || p->c0 < 0 || p->c0 > p->c1 || p->c1 > d.width)
        return bad("the window is outside the depth image");
    const uint64_t n = (uint64_t)p->out_width * p->out_height, count = (uint64_t)(p->r1 - p->r0) * (uint64_t)(p->c1 - p->c0);
    if (n > 0x7ffffff0ull) return bad("more than 2^31 - 16 records");
    if (count > n) return bad("the window holds more pixels than the cloud has records");
    const int du = depth_model_use(d, RSREG_DISTORTION_INVERSE_BROWN_CONRADY), cu = depth_model_use(c, RSREG_DISTORTION_MODIFIED_BROWN_CONRADY);
    if (du < 0 || cu < 0) return bad("a distortion model that is not built, with non-zero coefficients");
    DepthPlan &q = *out;
    q.d_ppx = d.ppx, q.d_ppy = d.ppy, q.d_fx = d.fx, q.d_fy = d.fy;
    q.c_ppx = c.ppx, q.c_ppy = c.ppy, q.c_fx = c.fx, q.c_fy = c.fy;
    for (int i = 0; i < 5; ++i) q.dk[i] = d.coeffs[i], q.ck[i] = c.coeffs[i];
    q.c_wf = (float)c.width, q.c_hf = (float)c.height;
    for (int i = 0; i < 9; ++i) q.R[i] = p->rotation[i];
    for (int i = 0; i < 3; ++i) q.t[i] = p->translation[i];
    q.depth_scale = p->depth_scale;
    q.d_inverse = du, q.c_modified = cu;
    q.c_w = c.width, q.c_h = c.height, q.bpp = p->color_bytes_per_pixel;
    q.r_off = p->color_bgr ? 2 : 0, q.b_off = p->color_bgr ? 0 : 2;
    q.r0 = p->r0, q.c0 = p->c0;
    q.win_rows = (uint32_t)(p->r1 - p->r0), q.win_cols = (uint32_t)(p->c1 - p->c0), q.count = (uint32_t)count, q.n = (uint32_t)n;
    q.out_width = p->out_width, q.out_height = p->out_height, q.is_dense = p->is_dense ? 1 : 0;
    q.depth_stride = depth_stride, q.color_stride = color_stride;
    q.depth_bytes = (size_t)(d.height - 1) * depth_stride + 2 * (size_t)d.width;
    q.color_bytes = (size_t)(c.height - 1) * color_stride + (size_t)q.bpp * (size_t)c.width;
    return RSREG_OK;
}

}  // namespace rsreg
