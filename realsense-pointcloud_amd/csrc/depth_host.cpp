// depth_host.cpp — the capture step on the host: a depth frame and a colour frame -> an organized PointXYZRGB cloud, the
// contract of include/rsreg.h ("capture") restated sequentially, pixel by pixel as the reference's convert_to_pcl walks them
// (src/capture.hpp:72-107, src/capture_opencv.hpp:128-160; rs2::pointcloud's vertices and texture coordinates recalled from
// librealsense 2.3x).  No context; the second implementation the kernel of depthcloud.hip is compared with.  The build
// passes -ffp-contract=off: every operator below is one rounded float operation.
#include <climits>
#include <cstdint>
#include <cstring>
#include <initializer_list>

#include "depthcloud_plan.hpp"

namespace {

using rsreg::DepthPlan;

// C's (int)t where it is defined; INT_MIN where it is not (NaN, or outside [-2^31, 2^31)): the x86 conversion's answer
inline int32_t to_int(float t)
{
    if (!(t >= -2147483648.0f && t < 2147483648.0f)) return INT32_MIN;
    return (int32_t)t;
}

inline int clamp_pixel(float uv, float size_f, int size)
{
    int v = to_int(uv * size_f + .5f);
    if (v < 0) v = 0;
    if (v > size - 1) v = size - 1;
    return v;
}

// one pixel of the window: the 32 bytes of its record
void record_of(const DepthPlan &p, const unsigned char *depth, const unsigned char *color, int r, int c, unsigned char *rec)
{
    uint16_t d;
    std::memcpy(&d, depth + (size_t)r * p.depth_stride + (size_t)c * 2, 2);
    // (1) the vertex
    const float z = p.depth_scale * (float)d;
    float x = ((float)c - p.d_ppx) / p.d_fx;
    float y = ((float)r - p.d_ppy) / p.d_fy;
    if (p.d_inverse) {
        const float *k = p.dk;
        const float r2 = x * x + y * y;
        const float f = 1 + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2;
        const float ux = x * f + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        const float uy = y * f + 2 * k[3] * x * y + k[2] * (r2 + 2 * y * y);
        x = ux;
        y = uy;
    }
    const float P[3] = {z * x, z * y, z};
    // (2) the texture coordinate
    float u = 0.0f, v = 0.0f;
    if (!(P[2] == 0.0f)) {
        float q[3];
        for (int k = 0; k < 3; ++k) q[k] = p.R[0 + k] * P[0] + p.R[3 + k] * P[1] + p.R[6 + k] * P[2] + p.t[k];
        float tx = q[0] / q[2], ty = q[1] / q[2];
        if (p.c_modified) {
            const float *k = p.ck;
            const float r2 = tx * tx + ty * ty;
            const float f = 1 + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2;
            tx = tx * f;
            ty = ty * f;
            const float dx = tx + 2 * k[2] * tx * ty + k[3] * (r2 + 2 * tx * tx);
            const float dy = ty + 2 * k[3] * tx * ty + k[2] * (r2 + 2 * ty * ty);
            tx = dx;
            ty = dy;
        }
        const float px = tx * p.c_fx + p.c_ppx, py = ty * p.c_fy + p.c_ppy;
        u = px / p.c_wf;
        v = py / p.c_hf;
    }
    // (3) the colour
    const int xi = clamp_pixel(u, p.c_wf, p.c_w), yi = clamp_pixel(v, p.c_hf, p.c_h);
    const unsigned char *px = color + (size_t)yi * p.color_stride + (size_t)xi * (size_t)p.bpp;
    const uint32_t rgba = 0xff000000u | ((uint32_t)px[p.r_off] << 16) | ((uint32_t)px[1] << 8) | (uint32_t)px[p.b_off];
    // (4) the record
    const float one = 1.0f;
    std::memset(rec, 0, 32);
    std::memcpy(rec, P, 12);
    std::memcpy(rec + 12, &one, 4);
    std::memcpy(rec + 16, &rgba, 4);
}

}  // namespace

extern "C" {

void rsreg_depth_params_default(uint32_t w, uint32_t h, rsreg_depth_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    for (rsreg_intrinsics *in : {&p->depth, &p->color}) {
        in->width = (int32_t)w, in->height = (int32_t)h;
        in->ppx = (float)w / 2.0f, in->ppy = (float)h / 2.0f;
        in->fx = in->fy = (float)w;
        in->model = RSREG_DISTORTION_NONE;
    }
    p->rotation[0] = p->rotation[4] = p->rotation[8] = 1.0f;
    p->depth_scale = 0.001f;
    p->color_bytes_per_pixel = 3;
    p->color_bgr = 1;
    p->r0 = 0, p->r1 = (int32_t)h, p->c0 = 0, p->c1 = (int32_t)w;
    p->out_width = w, p->out_height = h;
    p->is_dense = 0;
}

void rsreg_depth_params_reference(uint32_t w, uint32_t h, rsreg_depth_params *p)
{
    if (!p) return;
    rsreg_depth_params_default(w, h, p);
    const int iw = (int)w, ih = (int)h;   // (the reference's ints: sp.width(), sp.height())
    p->r0 = ih / 5, p->r1 = ih / 5 * 4;
    p->c0 = iw / 5, p->c1 = iw / 5 * 4;
    p->out_width = (uint32_t)(iw * 3 / 5), p->out_height = (uint32_t)(ih * 3 / 5);
    p->is_dense = 1;
}

int rsreg_depth_to_cloud(const void *depth, size_t depth_stride, const void *color, size_t color_stride, const rsreg_depth_params *prm,
                         void *out, size_t capacity_records, uint32_t *width, uint32_t *height, int *is_dense)
{
    DepthPlan p;
    const int rc = rsreg::depth_plan(prm, depth_stride, color_stride, &p, nullptr);
    if (rc) return rc;
    if (!depth || !color || !out || capacity_records < p.n) return RSREG_ERR_INVALID_ARG;
    unsigned char *rec = static_cast<unsigned char *>(out);
    const unsigned char *dimg = static_cast<const unsigned char *>(depth), *cimg = static_cast<const unsigned char *>(color);
    size_t i = 0;
    for (int r = p.r0; r < p.r0 + (int)p.win_rows; ++r)
        for (int c = p.c0; c < p.c0 + (int)p.win_cols; ++c) record_of(p, dimg, cimg, r, c, rec + 32 * i++);
    // the rest stays a default-constructed PointXYZRGB
    const float one = 1.0f;
    const uint32_t opaque_black = 0xff000000u;
    for (; i < p.n; ++i) {
        std::memset(rec + 32 * i, 0, 32);
        std::memcpy(rec + 32 * i + 12, &one, 4);
        std::memcpy(rec + 32 * i + 16, &opaque_black, 4);
    }
    if (width) *width = p.out_width;
    if (height) *height = p.out_height;
    if (is_dense) *is_dense = p.is_dense;
    return RSREG_OK;
}

}  // extern "C"
