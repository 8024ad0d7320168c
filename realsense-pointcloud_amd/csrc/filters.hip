// filters.hip — pcl::PassThrough and pcl::StatisticalOutlierRemoval on clouds resident in HBM (C ABI: include/rsreg.h,
// "cloud filters"): the reference's pre-filter, src/capture.hpp:112-132 (filter_pcl), which runs every captured frame through
// PassThrough (field z) and StatisticalOutlierRemoval (setMeanK(50), setStddevMulThresh(1.5)).
//
// PassThrough: one flag pass, a prefix sum of the flags (oscan.hpp), one ordered gather.  StatisticalOutlierRemoval: the exact
// k-NN index and search of knn_kernels.hpp, the threshold's two sums in PCL's own order, then the same flag / scan / gather.
// Everything runs on the context's stream with the index and scratch of rsreg_ctx::knn: nothing here reads or writes a
// buffer of the alignment's index or of the fitness indices.
#include <cmath>
#include <cstring>

#include "records.hpp"
#include "oscan.hpp"
#include "knn_kernels.hpp"

using namespace rsreg;

struct rsreg_cloud;
extern "C" {
int rsreg_cloud_adopt_(rsreg_cloud *c, DevBuf *buf, size_t n, size_t stride, uint32_t width, uint32_t height, int is_dense);   // cloud.hip
const rsreg_ctx *rsreg_cloud_ctx_(const rsreg_cloud *c);   // cloud.hip: the context a handle belongs to
}

namespace {

inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
inline uint32_t div_up64(unsigned long long a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

struct CloudView {
    const char *rec = nullptr;
    size_t n = 0, stride = 0;
    uint32_t width = 0, height = 0;
    int is_dense = 0;
};

// the input's records on the context's stream (an upload or a queued filter of it has been waited for)
int view_of(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *out, CloudView &v)
{
    if (!ctx || !in) return RSREG_ERR_INVALID_ARG;
    if (rsreg_cloud_ctx_(in) != ctx || (out && rsreg_cloud_ctx_(out) != ctx)) return RSREG_ERR_INVALID_ARG;
    int rc = rsreg_cloud_info(in, &v.n, &v.stride, &v.width, &v.height, &v.is_dense);
    if (rc) return rc;
    if (v.stride < 12 || v.stride % 4 != 0) return fail(ctx, RSREG_ERR_INVALID_ARG, "records need x, y, z floats and a stride that is a multiple of 4");
    if (v.n > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "cloud too large");
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    v.rec = static_cast<const char *>(rsreg_cloud_device_ptr(in));
    if (v.n && !v.rec) return fail(ctx, RSREG_ERR_STATE, "the cloud's records are not available");
    return RSREG_OK;
}

// The cells of the k-NN index: about 64 cells per finite point over the box -- a depth frame is a surface, so a few points per
// OCCUPIED cell -- 2^25 cells and 4 096 along an axis at most (the margin of knn_gap is argued for that many), never so small
// that the float rounding of a coordinate is a sizeable part of a cell.  Cells per axis: floor(extent / cell) + 2.
void knn_layout(const float mn[3], const float mx[3], uint32_t nfin, KnnIndex &kx)
{
    double e[3], emax = 0, big = 0;
    for (int k = 0; k < 3; ++k) {
        e[k] = (double)mx[k] - (double)mn[k];
        emax = std::max(emax, e[k]);
        big = std::max(big, std::max(std::fabs((double)mn[k]), std::fabs((double)mx[k])));
    }
    const double target = std::min(std::max(64.0 * nfin, 4096.0), 33554432.0);
    auto cells_along = [&](int k, double c) { return (int64_t)std::floor(e[k] / c) + 2; };
    auto cells_for = [&](double c) { return (double)cells_along(0, c) * (double)cells_along(1, c) * (double)cells_along(2, c); };
    double lo = std::max(std::max(emax / 4000.0, big * 1e-5), 1e-30);
    if (emax == 0) lo = std::max(big * 1e-5, 1.0);
    double cell = lo;
    if (cells_for(lo) > target) {
        double hi = std::max(emax, lo) * 2.0;   // (two cells per axis)
        for (int it = 0; it < 100; ++it) {
            const double mid = std::sqrt(lo * hi);
            if (cells_for(mid) > target) lo = mid; else hi = mid;
        }
        cell = hi;
    }
    kx.cell = (float)cell;
    kx.inv_cell = (float)(1.0 / (double)kx.cell);
    for (int k = 0; k < 3; ++k) {
        kx.origin[k] = mn[k];
        kx.dims[k] = (int)cells_along(k, (double)kx.cell);
    }
}

KnnDev knn_dev(const KnnIndex &kx)
{
    KnnDev g{};
    g.ox = kx.origin[0]; g.oy = kx.origin[1]; g.oz = kx.origin[2];
    g.inv_cell = kx.inv_cell;
    g.cell = kx.cell;
    g.dx = kx.dims[0]; g.dy = kx.dims[1]; g.dz = kx.dims[2];
    g.n = kx.n_points;
    g.start = kx.d_start.as<uint32_t>();
    g.pts = kx.d_pts.as<float4>();
    return g;
}

// d_dist[i] = record i's mean distance to its mean_k nearest neighbours (0 for a non-finite record), *nfin_out = finite records.
// The box (one round trip to the host), the counts, their prefix sum, the scatter, the search: on ctx->stream, not waited for.
int knn_mean_distance_device(rsreg_ctx *ctx, const CloudView &v, int mean_k, uint32_t *nfin_out)
{
    KnnIndex &kx = ctx->knn;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    if (mean_k < 1 || mean_k > kKnnMaxK) return fail(ctx, RSREG_ERR_INVALID_ARG, "mean_k must be between 1 and 64");
    RSREG_HIP(ctx, kx.d_box.reserve(64));
    RSREG_HIP(ctx, kx.host.reserve(256));
    uint32_t *h = kx.host.as<uint32_t>();
    h[6] = 0;
    if (n) {
        RSREG_HIP(ctx, hipMemsetAsync(kx.d_box.ptr, 0xff, 12, st));
        RSREG_HIP(ctx, hipMemsetAsync(kx.d_box.as<char>() + 12, 0, 20, st));
        k_knn_bbox<<<std::min<uint32_t>(div_up(n, kBlock), 1024), kBlock, 0, st>>>(v.rec, v.stride, n, kx.d_box.as<uint32_t>());
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipMemcpyAsync(h, kx.d_box.ptr, 32, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
    }
    const uint32_t nfin = h[6];
    *nfin_out = nfin;
    // PCL reads past nn_dists when the tree holds fewer than mean_k + 1 points
    if ((unsigned long long)nfin < (unsigned long long)mean_k + 1ull)
        return fail(ctx, RSREG_ERR_INVALID_ARG, "the cloud has fewer than mean_k + 1 finite records");
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) {
        mn[k] = ordered_float(h[k]);
        mx[k] = ordered_float(h[3 + k]);
    }
    knn_layout(mn, mx, nfin, kx);
    kx.n_points = nfin;
    const size_t cells = (size_t)kx.dims[0] * (size_t)kx.dims[1] * (size_t)kx.dims[2];
    if (kx.dims[0] > 4096 || kx.dims[1] > 4096 || kx.dims[2] > 4096 || cells > 0x7ffffff0ull)
        return fail(ctx, RSREG_ERR_STATE, "k-NN grid layout out of range");
    const size_t count_cap_before = kx.d_count.cap;
    RSREG_HIP(ctx, kx.d_pts.reserve((size_t)nfin * sizeof(float4) + 16));
    RSREG_HIP(ctx, kx.d_start.reserve((cells + 1) * 4));
    RSREG_HIP(ctx, kx.d_count.reserve((cells + 1) * 4));
    RSREG_HIP(ctx, kx.d_scan.reserve(std::max(oscan_scratch_bytes<uint32_t>(cells + 1), oscan_scratch_bytes<uint32_t>(v.n))));
    RSREG_HIP(ctx, kx.d_dist.reserve(v.n * 4 + 16));
    if (kx.d_count.cap != count_cap_before || count_cap_before == 0)   // (a new buffer; an old one is zero after every scatter)
        RSREG_HIP(ctx, hipMemsetAsync(kx.d_count.ptr, 0, kx.d_count.cap, st));
    const KnnDev g = knn_dev(kx);
    uint32_t *count = kx.d_count.as<uint32_t>(), *start = kx.d_start.as<uint32_t>();
    k_knn_count<<<div_up(n, kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, g, count, kx.d_dist.as<float>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, oscan<uint32_t>(count, start, cells + 1, 0u, kx.d_scan.ptr, st));
    k_knn_scatter<<<div_up(n, kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, g, start, count, kx.d_pts.as<float4>());
    RSREG_HIP(ctx, hipGetLastError());
    k_knn_mean_distance<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, st>>>(g, mean_k, kx.d_dist.as<float>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// flags -> positions -> the kept records in ctx->knn.d_out (waits for their number), handed to `out`
int compact_into(rsreg_ctx *ctx, const CloudView &v, rsreg_cloud *out, int is_dense, uint32_t *n_kept_out)
{
    KnnIndex &kx = ctx->knn;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    uint32_t kept = 0;
    if (n) {
        RSREG_HIP(ctx, kx.d_pos.reserve(v.n * 4 + 16));
        RSREG_HIP(ctx, kx.d_scan.reserve(oscan_scratch_bytes<uint32_t>(v.n)));
        RSREG_HIP(ctx, kx.d_out.reserve(v.n * v.stride + 16));
        RSREG_HIP(ctx, kx.d_box.reserve(64));
        RSREG_HIP(ctx, kx.host.reserve(256));
        RSREG_HIP(ctx, oscan<uint32_t>(kx.d_flags.as<uint32_t>(), kx.d_pos.as<uint32_t>(), v.n, 0u, kx.d_scan.ptr, st));
        uint32_t *d_kept = kx.d_box.as<uint32_t>() + 8;
        k_filter_gather<<<div_up64((unsigned long long)n * (v.stride / 4), kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, kx.d_flags.as<uint32_t>(),
                                                                                                   kx.d_pos.as<uint32_t>(), kx.d_out.as<char>(), d_kept);
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipMemcpyAsync(kx.host.as<uint32_t>() + 8, d_kept, 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        kept = kx.host.as<uint32_t>()[8];
    }
    *n_kept_out = kept;
    return rsreg_cloud_adopt_(out, &kx.d_out, kept, v.stride, kept, 1, is_dense);   // (in == out: the input has been consumed by now)
}

}  // namespace

extern "C" {

int rsreg_cloud_passthrough(rsreg_ctx *ctx, const rsreg_cloud *in, int field, float lo, float hi, int negative, int keep_organized,
                            rsreg_cloud *out)
{
    CloudView v;
    if (!out) return RSREG_ERR_INVALID_ARG;
    int rc = view_of(ctx, in, out, v);
    if (rc) return rc;
    // (PCL warns about a field it does not find and returns an empty cloud: here the call is refused)
    if (field < 0 || field > 2) return fail(ctx, RSREG_ERR_INVALID_ARG, "PassThrough filters on field 0 (x), 1 (y) or 2 (z)");
    KnnIndex &kx = ctx->knn;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    if (n) {
        RSREG_HIP(ctx, kx.d_flags.reserve(v.n * 4 + 16));
        k_pass_flags<<<div_up(n, kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, field, lo, hi, negative ? 1 : 0, kx.d_flags.as<uint32_t>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    uint32_t kept = 0;
    if (!keep_organized) return compact_into(ctx, v, out, 1, &kept);
    // every record stays; is_dense is false if anything was removed: the number of kept records decides
    uint32_t removed = 0;
    if (n) {
        RSREG_HIP(ctx, kx.d_pos.reserve(v.n * 4 + 16));
        RSREG_HIP(ctx, kx.d_scan.reserve(oscan_scratch_bytes<uint32_t>(v.n)));
        RSREG_HIP(ctx, kx.d_out.reserve(v.n * v.stride + 16));
        RSREG_HIP(ctx, kx.host.reserve(256));
        RSREG_HIP(ctx, (oscan<uint32_t, true>(kx.d_flags.as<uint32_t>(), kx.d_pos.as<uint32_t>(), v.n, 0u, kx.d_scan.ptr, st)));
        k_filter_organized<<<div_up64((unsigned long long)n * (v.stride / 4), kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, kx.d_flags.as<uint32_t>(),
                                                                                                      kx.d_out.as<char>());
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipMemcpyAsync(kx.host.as<uint32_t>() + 8, kx.d_pos.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        removed = n - kx.host.as<uint32_t>()[8];
    }
    return rsreg_cloud_adopt_(out, &kx.d_out, v.n, v.stride, v.width, v.height, removed ? 0 : v.is_dense);
}

int rsreg_cloud_knn_mean_distance(rsreg_ctx *ctx, const rsreg_cloud *in, int mean_k, float *host_out)
{
    CloudView v;
    if (!host_out) return RSREG_ERR_INVALID_ARG;
    int rc = view_of(ctx, in, nullptr, v);
    if (rc) return rc;
    uint32_t nfin = 0;
    rc = knn_mean_distance_device(ctx, v, mean_k, &nfin);
    if (rc) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(host_out, ctx->knn.d_dist.ptr, v.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSREG_OK;
}

int rsreg_cloud_sor(rsreg_ctx *ctx, const rsreg_cloud *in, int mean_k, double stddev_mult, int negative, rsreg_cloud *out, rsreg_sor_stats *stats)
{
    CloudView v;
    if (!out) return RSREG_ERR_INVALID_ARG;
    int rc = view_of(ctx, in, out, v);
    if (rc) return rc;
    uint32_t nfin = 0;
    rc = knn_mean_distance_device(ctx, v, mean_k, &nfin);
    if (rc) return rc;
    // PCL divides by n_valid - 1
    if (nfin < 2) return fail(ctx, RSREG_ERR_INVALID_ARG, "the cloud has fewer than two finite records");
    KnnIndex &kx = ctx->knn;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n, nb = div_up(n, kBlock);
    RSREG_HIP(ctx, kx.d_sums.reserve(64));
    RSREG_HIP(ctx, kx.d_flags.reserve(v.n * 4 + 16));
    k_sor_sums<<<2, kKnnWave, 0, st>>>(kx.d_dist.as<float>(), n, kx.d_sums.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    double *hs = kx.host.as<double>() + 8;
    RSREG_HIP(ctx, hipMemcpyAsync(hs, kx.d_sums.ptr, 16, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    // PCL: sum and sq_sum over ALL records (a non-finite record adds its 0), divided by the number of valid ones
    const double sum = hs[0], sq = hs[1], nv = (double)nfin;
    const double mean = sum / nv;
    const double variance = (sq - sum * sum / nv) / (nv - 1.0);
    const double stddev = std::sqrt(variance);
    const double threshold = mean + stddev_mult * stddev;
    k_sor_flags<<<nb, kBlock, 0, st>>>(v.rec, v.stride, kx.d_dist.as<float>(), n, threshold, negative ? 1 : 0, kx.d_flags.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    uint32_t kept = 0;
    rc = compact_into(ctx, v, out, v.is_dense, &kept);
    if (rc) return rc;
    if (stats) {
        stats->n_valid = nfin;
        stats->n_kept = kept;
        stats->mean = mean;
        stats->stddev = stddev;
        stats->threshold = threshold;
    }
    return RSREG_OK;
}

}  // extern "C"
