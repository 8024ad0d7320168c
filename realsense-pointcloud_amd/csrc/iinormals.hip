// iinormals.hip — pcl::IntegralImageNormalEstimation on organized clouds resident in HBM (C ABI: include/rsreg.h,
// rsreg_cloud_integral_normals): the first step of the reference's edge extractor, src/edge_extractor.hpp:9-15
// (AVERAGE_3D_GRADIENT, setMaxDepthChangeFactor(0.02f), setNormalSmoothingSize(10.0f)).
//
// Four launches on the context's stream with the scratch rsreg_ctx::iin: k_iin_prepare, k_iin_chamfer forward and backward,
// k_iin_normals (iinormals_kernels.hpp).  Nothing here reads or writes a buffer of an index or of the cloud filters, and
// nothing depends on what the context ran before: the same cloud gives the same bytes.
#include <cmath>
#include <cstring>

#include "iinormals_kernels.hpp"
#include "cloud_ops.hpp"

using namespace rsreg;

extern "C" {

void rsreg_iin_params_default(rsreg_iin_params *p)
{
    if (!p) return;
    p->method = RSREG_IIN_AVERAGE_3D_GRADIENT;
    p->max_depth_change_factor = 0.02f;
    p->normal_smoothing_size = 10.0f;
    p->depth_dependent_smoothing = 0;
    p->border_policy = RSREG_IIN_BORDER_IGNORE;
    p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.0f;
}

int rsreg_cloud_integral_normals(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_iin_params *prm, rsreg_cloud *out, uint8_t *rect_out)
{
    if (!out || out == in) return RSREG_ERR_INVALID_ARG;
    rsreg_iin_params p;
    rsreg_iin_params_default(&p);
    if (prm) p = *prm;
    // (the frame's own limit, width and count at once, is below: the rule has none)
    constexpr CloudRule rule{kXyzRule.min_stride, kXyzRule.stride_mult4, kXyzRule.bad_stride, kAnyCount, nullptr};
    CloudView v;
    const int rc = cloud_view(ctx, in, out, rule, v);
    if (rc) return rc;
    const char *rec = v.rec;
    const size_t n = v.n, stride = v.stride;
    const uint32_t width = v.width, height = v.height;
    if (height <= 1 || width == 0 || (size_t)width * (size_t)height != n)
        return fail(ctx, RSREG_ERR_INVALID_ARG, "IntegralImageNormalEstimation needs an organized cloud (height > 1)");
    if (width > (uint32_t)kIinMaxWidth || n > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "frames wider than 8192 pixels are not supported");
    if (p.method != RSREG_IIN_AVERAGE_3D_GRADIENT) return fail(ctx, RSREG_ERR_INVALID_ARG, "only AVERAGE_3D_GRADIENT is implemented");
    if (p.depth_dependent_smoothing) return fail(ctx, RSREG_ERR_INVALID_ARG, "depth-dependent smoothing is not implemented");
    if (p.border_policy != RSREG_IIN_BORDER_IGNORE) return fail(ctx, RSREG_ERR_INVALID_ARG, "only the IGNORE border policy is implemented");
    if (!(p.normal_smoothing_size > 0.0f && p.normal_smoothing_size <= 64.0f))
        return fail(ctx, RSREG_ERR_INVALID_ARG, "normal_smoothing_size must be in (0, 64]");
    if (!(std::isfinite(p.max_depth_change_factor) && p.max_depth_change_factor >= 0.0f))
        return fail(ctx, RSREG_ERR_INVALID_ARG, "max_depth_change_factor must be finite and not negative");

    IinScratch &sc = ctx->iin;
    hipStream_t st = ctx->stream;
    const int w = (int)width, h = (int)height;
    const int border = (int)p.normal_smoothing_size, reach = border + 3;   // halo rows and look-back columns of the passes
    constexpr size_t kNormalBytes = 32;   // pcl::Normal
    RSREG_HIP(ctx, sc.d_dist0.reserve(n * 4 + 16));
    RSREG_HIP(ctx, sc.d_dist1.reserve(n * 4 + 16));
    RSREG_HIP(ctx, sc.d_dist2.reserve(n * 4 + 16));
    RSREG_HIP(ctx, sc.d_grad.reserve(n * sizeof(IinGrad) + 16));
    RSREG_HIP(ctx, sc.d_rect.reserve(n + 16));
    RSREG_HIP(ctx, sc.d_out.reserve(n * kNormalBytes + 16));
    if (rect_out) RSREG_HIP(ctx, sc.host.reserve(n + 16));

    k_iin_prepare<<<(uint32_t)((n + kBlock - 1) / kBlock), kBlock, 0, st>>>(rec, stride, w, h, p.max_depth_change_factor, sc.d_dist0.as<float>(),
                                                                           sc.d_grad.as<IinGrad>());
    RSREG_HIP(ctx, hipGetLastError());
    const uint32_t bands = (uint32_t)((h + kIinBand - 1) / kIinBand);
    const size_t lds = 2 * (size_t)w * sizeof(float);
    k_iin_chamfer<<<bands, kBlock, lds, st>>>(sc.d_dist0.as<float>(), sc.d_dist1.as<float>(), w, h, reach, reach, 0);
    RSREG_HIP(ctx, hipGetLastError());
    k_iin_chamfer<<<bands, kBlock, lds, st>>>(sc.d_dist1.as<float>(), sc.d_dist2.as<float>(), w, h, reach, reach, 1);
    RSREG_HIP(ctx, hipGetLastError());
    const dim3 tiles((uint32_t)((w + kIinTile - 1) / kIinTile), (uint32_t)((h + kIinTile - 1) / kIinTile));
    k_iin_normals<<<tiles, kIinTile * kIinTile, 0, st>>>(rec, stride, w, h, sc.d_dist2.as<float>(), sc.d_grad.as<IinGrad>(), p.normal_smoothing_size, border,
                                                        p.viewpoint[0], p.viewpoint[1], p.viewpoint[2], sc.d_out.as<float>(), sc.d_rect.as<uint8_t>());
    RSREG_HIP(ctx, hipGetLastError());
    if (rect_out) {
        RSREG_HIP(ctx, hipMemcpyAsync(sc.host.ptr, sc.d_rect.ptr, n, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        std::memcpy(rect_out, sc.host.ptr, n);
    }
    return rsreg_cloud_adopt_(out, &sc.d_out, n, kNormalBytes, width, height, 0);
}

}  // extern "C"
