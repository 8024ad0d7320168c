// depthcloud.hip — the capture step in HBM (C ABI: include/rsreg.h, "capture": rsreg_cloud_from_depth, _device): the
// reference's rs2::pointcloud + convert_to_pcl (src/capture.hpp:72-107, src/capture_opencv.hpp:128-160) from the depth and the
// colour image, 5 bytes a pixel over the link instead of the 32 of a finished record.
//
// One launch of k_depth_to_cloud (depthcloud_kernels.hpp) on the context's stream, straight into the output cloud's buffer.
// Host images are staged in a pinned buffer of this step's own (rsreg_ctx::depth), both in one piece, and go up in one copy
// on the same stream; the call returns when that copy has arrived (the staging buffer is free again, the caller's images have
// been read), not when the kernel has run.
#include <cstring>

#include "depthcloud_kernels.hpp"
#include "cloud_ops.hpp"

using namespace rsreg;

namespace {

int launch(rsreg_ctx *ctx, const unsigned char *d_depth, const unsigned char *d_color, const DepthPlan &p, rsreg_cloud *out)
{
    void *rec = nullptr;
    const int rc = rsreg_cloud_begin_write_(out, p.n, 32, &rec);
    if (rc) return rc;
    k_depth_to_cloud<<<(p.n + kBlock - 1) / kBlock, kBlock, 0, ctx->stream>>>(d_depth, d_color, p, static_cast<uint4 *>(rec));
    RSREG_HIP(ctx, hipGetLastError());
    return rsreg_cloud_end_write_(out, p.n, 32, p.out_width, p.out_height, p.is_dense);
}

int check_args(rsreg_ctx *ctx, const void *depth, const void *color, size_t depth_stride, size_t color_stride, const rsreg_depth_params *prm,
               rsreg_cloud *out, DepthPlan *p)
{
    if (!ctx || !out || rsreg_cloud_ctx_(out) != ctx) return RSREG_ERR_INVALID_ARG;
    const char *why = "";
    const int rc = depth_plan(prm, depth_stride, color_stride, p, &why);
    if (rc) return fail(ctx, rc, why);
    if (!depth || !color) return fail(ctx, RSREG_ERR_INVALID_ARG, "an image is missing");
    return RSREG_OK;
}

}  // namespace

extern "C" {

int rsreg_cloud_from_depth_device(rsreg_ctx *ctx, const void *d_depth, size_t depth_stride, const void *d_color, size_t color_stride,
                                  const rsreg_depth_params *prm, rsreg_cloud *out)
{
    DepthPlan p;
    const int rc = check_args(ctx, d_depth, d_color, depth_stride, color_stride, prm, out, &p);
    if (rc) return rc;
    if ((uintptr_t)d_depth & 1u) return fail(ctx, RSREG_ERR_INVALID_ARG, "the depth image must be 2-byte aligned");
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    return launch(ctx, static_cast<const unsigned char *>(d_depth), static_cast<const unsigned char *>(d_color), p, out);
}

int rsreg_cloud_from_depth(rsreg_ctx *ctx, const void *depth, size_t depth_stride, const void *color, size_t color_stride,
                           const rsreg_depth_params *prm, rsreg_cloud *out)
{
    DepthPlan p;
    const int rc = check_args(ctx, depth, color, depth_stride, color_stride, prm, out, &p);
    if (rc) return rc;
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    DepthScratch &sc = ctx->depth;
    const size_t color_at = (p.depth_bytes + 255) & ~(size_t)255, bytes = color_at + p.color_bytes;
    RSREG_HIP(ctx, sc.host.reserve(bytes));
    RSREG_HIP(ctx, sc.d_images.reserve(bytes));   // (stream-ordered behind the kernel that read the previous frame out of it)
    RSREG_HIP(ctx, sc.ev_up.ensure());
    char *stage = sc.host.as<char>();
    const char *ds = static_cast<const char *>(depth), *cs = static_cast<const char *>(color);
    constexpr size_t kUnit = 32;   // (host_parallel_for splits by records: 32-byte units here)
    host_parallel_for((p.depth_bytes + kUnit - 1) / kUnit, [=](size_t lo, size_t hi) {
        rsreg::stream_copy(stage + lo * kUnit, ds + lo * kUnit, std::min(hi * kUnit, p.depth_bytes) - lo * kUnit);
    });
    host_parallel_for((p.color_bytes + kUnit - 1) / kUnit, [=](size_t lo, size_t hi) {
        rsreg::stream_copy(stage + color_at + lo * kUnit, cs + lo * kUnit, std::min(hi * kUnit, p.color_bytes) - lo * kUnit);
    });
    RSREG_HIP(ctx, hipMemcpyAsync(sc.d_images.ptr, stage, bytes, hipMemcpyHostToDevice, ctx->stream));
    RSREG_HIP(ctx, hipEventRecord(sc.ev_up, ctx->stream));
    const unsigned char *dev = sc.d_images.as<unsigned char>();
    const int lrc = launch(ctx, dev, dev + color_at, p, out);
    RSREG_HIP(ctx, hipEventSynchronize(sc.ev_up));   // the staging buffer is reused by the next call
    return lrc;
}

}  // extern "C"
