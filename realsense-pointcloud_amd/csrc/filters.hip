// filters.hip — pcl::PassThrough and pcl::StatisticalOutlierRemoval on clouds resident in HBM (C ABI: include/rsreg.h,
// "cloud filters"): the reference's pre-filter, src/capture.hpp:112-132 (filter_pcl), which runs every captured frame through
// PassThrough (field z) and StatisticalOutlierRemoval (setMeanK(50), setStddevMulThresh(1.5)).
//
// PassThrough: one flag pass, a prefix sum of the flags (oscan.hpp), one ordered gather.  StatisticalOutlierRemoval: the exact
// k-NN index and search of knn_kernels.hpp, the threshold's two sums in PCL's own order, then the same flag / scan / gather.
// pcl::RadiusOutlierRemoval and NormalEstimation by radius: the exact radius search of radius_kernels.hpp over an index of its own
// placement, then the same flag / scan / gather, or k_normals' tail.  pcl::FPFHEstimation (setKSearch): the k-NN search once, with
// the pair features of fpfh_kernels.hpp behind it, then the weighting pass over the neighbour rows the search left.  pcl::FPFHEstimationOMP
// (setRadiusSearch): fpfh_radius_kernels.hpp's two walks of the radius index, no neighbour list between them.  setSearchSurface
// (the *_surface calls): the same radius index over the surface, searched from the records of another cloud (surface_kernels.hpp).
// pcl::ISSKeypoint3D: iss_kernels.hpp's two walks over ONE radius index (the salient radius'), then the flag / scan / gather.
// pcl::EuclideanClusterExtraction: cluster_kernels.hpp's union-find inside the walk of the radius index, two sorts for the ranking,
// then (rsreg_cloud_cluster_filter) the same flag / scan / gather.
// Everything runs on the context's stream with the index rsreg_ctx::knn and the scratch rsreg_ctx::filt (the radius search:
// rsreg_ctx::rad too): nothing here reads or writes a buffer of the alignment's index or of the fitness indices.
#include <cmath>
#include <cstring>

#include "knn_kernels.hpp"
#include "normals_kernels.hpp"
#include "gicp_cov_kernels.hpp"
#include "radius_kernels.hpp"
#include "fpfh_kernels.hpp"
#include "fpfh_radius_kernels.hpp"
#include "surface_kernels.hpp"
#include "iss_kernels.hpp"
#include "cluster_kernels.hpp"
#include "cloud_ops.hpp"

using namespace rsreg;

namespace {

inline uint32_t div_up64(unsigned long long a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

// One launch leaves one word -- a count, or a flag it only ever sets (`clear`: zeroed first) -- and the word comes home with the
// stream: launch(d_word) queues the kernel.  The slot: kFiltWord of the index's box buffer and of the pinned scratch.
template <typename Launch> int word_home(rsreg_ctx *ctx, bool clear, Launch launch, uint32_t *word_out)
{
    hipStream_t st = ctx->stream;
    uint32_t *d_word = ctx->knn.d_box.as<uint32_t>() + kFiltWord, *h_word = ctx->filt.host.as<uint32_t>() + kFiltWord;
    if (clear) RSREG_HIP(ctx, hipMemsetAsync(d_word, 0, 4, st));
    launch(d_word);
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(h_word, d_word, 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    *word_out = *h_word;
    return RSREG_OK;
}

// The index of the cloud for a search that keeps `kept` neighbours (the record itself among them), on ctx->stream (pointgrid.hpp:
// one round trip to the host for the box); *nfin_out = finite records.  Refused with `too_few` when fewer than `kept` records are
// finite (PCL's nearestKSearch would return fewer: every caller here needs them all).
int knn_index_device(rsreg_ctx *ctx, const CloudView &v, int kept, const char *too_few, uint32_t *nfin_out)
{
    FilterScratch &fs = ctx->filt;
    RSREG_HIP(ctx, fs.host.reserve(256));
    RSREG_HIP(ctx, fs.d_dist.reserve(v.n * 4 + 16));   // (the count pass leaves a non-finite record's 0 there)
    int rc = grid_build<KnnGridPolicy>(ctx, ctx->knn, StridedRecords{v.rec, v.stride, fs.d_dist.as<float>()}, (uint32_t)v.n, (uint32_t)kept,
                                       fs.host.as<uint32_t>());
    if (rc) return rc;
    *nfin_out = ctx->knn.n_points;
    if (ctx->knn.n_points < (uint32_t)kept) return fail(ctx, RSREG_ERR_INVALID_ARG, too_few);
    return RSREG_OK;
}

// d_dist[i] = record i's mean distance to its mean_k nearest neighbours (0 for a non-finite record): the index and the search,
// not waited for.
int knn_mean_distance_device(rsreg_ctx *ctx, const CloudView &v, int mean_k, uint32_t *nfin_out)
{
    if (mean_k < 1 || mean_k > kKnnMaxK) return fail(ctx, RSREG_ERR_INVALID_ARG, "mean_k must be between 1 and 64");
    // PCL reads past nn_dists when the tree holds fewer than mean_k + 1 points
    int rc = knn_index_device(ctx, v, mean_k + 1, "the cloud has fewer than mean_k + 1 finite records", nfin_out);
    if (rc) return rc;
    k_knn_mean_distance<<<std::min<uint32_t>(*nfin_out, 1u << 16), kKnnWave, 0, ctx->stream>>>(grid_dev(ctx->knn), mean_k, ctx->filt.d_dist.as<float>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

}  // namespace

// (declared in cloud_ops.hpp: segment.hip ends its filters in these two as well)
namespace rsreg {

// flags -> positions -> the kept records in ctx->filt.d_out (waits for their number), handed to `out`
int compact_into(rsreg_ctx *ctx, const CloudView &v, rsreg_cloud *out, int is_dense, uint32_t *n_kept_out)
{
    PointGrid &kx = ctx->knn;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    uint32_t kept = 0;
    if (n) {
        RSREG_HIP(ctx, fs.d_pos.reserve(v.n * 4 + 16));
        RSREG_HIP(ctx, kx.d_scan.reserve(oscan_scratch_bytes<uint32_t>(v.n)));
        RSREG_HIP(ctx, fs.d_out.reserve(v.n * v.stride + 16));
        RSREG_HIP(ctx, kx.d_box.reserve(64));
        RSREG_HIP(ctx, fs.host.reserve(256));
        RSREG_HIP(ctx, oscan<uint32_t>(fs.d_flags.as<uint32_t>(), fs.d_pos.as<uint32_t>(), v.n, 0u, kx.d_scan.ptr, st));
        const int rc = word_home(ctx, false, [&](uint32_t *d_kept) {
            k_filter_gather<<<div_up64((unsigned long long)n * (v.stride / 4), kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, fs.d_flags.as<uint32_t>(),
                                                                                                       fs.d_pos.as<uint32_t>(), fs.d_out.as<char>(), d_kept);
        }, &kept);
        if (rc) return rc;
    }
    *n_kept_out = kept;
    return rsreg_cloud_adopt_(out, &fs.d_out, kept, v.stride, kept, 1, is_dense);   // (in == out: the input has been consumed by now)
}

// keep_organized: flags -> every record in ctx->filt.d_out, a removed one with x = y = z = quiet NaN (waits for the number of kept
// records: is_dense is false if anything was removed), handed to `out` with the input's width and height
int organized_into(rsreg_ctx *ctx, const CloudView &v, rsreg_cloud *out, uint32_t *n_kept_out)
{
    PointGrid &kx = ctx->knn;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    uint32_t removed = 0;
    if (n) {
        RSREG_HIP(ctx, fs.d_pos.reserve(v.n * 4 + 16));
        RSREG_HIP(ctx, kx.d_scan.reserve(oscan_scratch_bytes<uint32_t>(v.n)));
        RSREG_HIP(ctx, fs.d_out.reserve(v.n * v.stride + 16));
        RSREG_HIP(ctx, fs.host.reserve(256));
        RSREG_HIP(ctx, (oscan<uint32_t, true>(fs.d_flags.as<uint32_t>(), fs.d_pos.as<uint32_t>(), v.n, 0u, kx.d_scan.ptr, st)));
        k_filter_organized<<<div_up64((unsigned long long)n * (v.stride / 4), kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, fs.d_flags.as<uint32_t>(),
                                                                                                      fs.d_out.as<char>());
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipMemcpyAsync(fs.host.as<uint32_t>() + kFiltWord, fs.d_pos.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        removed = n - fs.host.as<uint32_t>()[kFiltWord];
    }
    *n_kept_out = n - removed;
    return rsreg_cloud_adopt_(out, &fs.d_out, v.n, v.stride, v.width, v.height, removed ? 0 : v.is_dense);
}

}  // namespace rsreg

namespace {

// The index of the cloud for a radius search and what a walk needs beside it (radius_kernels.hpp), on ctx->stream: pointgrid.hpp's
// build (one round trip to the host for the box) with the radius as the smallest cell and the ordered placement -- a stable sort of
// (cell, record) pairs.  count (nullable): the words of non-finite records are zeroed on the way.  No finite record: nothing is
// indexed, *nfin_out = 0.
int radius_index_device(rsreg_ctx *ctx, const CloudView &v, double radius, uint32_t *count, RadiusQuery *rq, uint32_t *nfin_out)
{
    FilterScratch &fs = ctx->filt;
    RadiusScratch &rs = ctx->rad;
    PointGrid &kx = ctx->knn;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    if (v.n >= (1ull << 30)) return fail(ctx, RSREG_ERR_INVALID_ARG, "cloud too large");
    RSREG_HIP(ctx, fs.host.reserve(256));
    const RadiusRecords rd{v.rec, v.stride, count};
    int rc = grid_build_placed<RadiusGridPolicy>(ctx, kx, rd, n, 1u, fs.host.as<uint32_t>(), radius,
                                                 [&](const PointGridDev &g, uint32_t *, uint32_t *cell_count, size_t cells) {
        for (int k = 0; k < 2; ++k) {
            RSREG_HIP(ctx, rs.d_keys[k].reserve(v.n * 4 + 16));
            RSREG_HIP(ctx, rs.d_vals[k].reserve(v.n * 4 + 16));
        }
        unsigned bits = 1;
        while ((cells >> bits) != 0) ++bits;   // the keys: every cell and `cells` itself, the non-finite records' key
        RSREG_HIP(ctx, rs.d_sort.reserve((size_t)osort_plan<uint32_t>(v.n, 0, bits).words * 4));
        uint32_t *keys[2] = {rs.d_keys[0].as<uint32_t>(), rs.d_keys[1].as<uint32_t>()}, *vals[2] = {rs.d_vals[0].as<uint32_t>(), rs.d_vals[1].as<uint32_t>()};
        k_radius_cell_keys<<<div_up(n, kBlock), kBlock, 0, st>>>(rd, n, g, (uint32_t)cells, keys[0], vals[0]);
        RSREG_HIP(ctx, hipGetLastError());
        bool in_first = true;
        RSREG_HIP(ctx, osort_pairs_cleared<uint32_t>(rs.d_sort.as<uint32_t>(), keys[0], keys[1], vals[0], vals[1], v.n, 0, bits, st, &in_first));
        const int at = in_first ? 0 : 1;
        k_radius_place<<<div_up(kx.n_points, kBlock), kBlock, 0, st>>>(rd, kx.n_points, keys[at], vals[at], cell_count, kx.d_pts.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
        return (int)RSREG_OK;
    });
    if (rc) return rc;
    *nfin_out = kx.n_points;
    *rq = radius_query(radius, kx);
    return RSREG_OK;
}

// d_count[i] = record i's neighbours within the radius, itself among them (0 for a non-finite record): the index and the search, not
// waited for
int radius_count_device(rsreg_ctx *ctx, const CloudView &v, double radius)
{
    if (!(radius > 0.0) || !std::isfinite(radius)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the radius must be finite and above 0");
    if (!v.n) return RSREG_OK;
    RadiusScratch &rs = ctx->rad;
    RSREG_HIP(ctx, rs.d_count.reserve(v.n * 4 + 16));
    RadiusQuery rq;
    uint32_t nfin = 0;
    int rc = radius_index_device(ctx, v, radius, rs.d_count.as<uint32_t>(), &rq, &nfin);
    if (rc) return rc;
    if (!nfin) {   // (the build stops at the box: nothing has written the counts)
        RSREG_HIP(ctx, hipMemsetAsync(rs.d_count.ptr, 0, v.n * 4, ctx->stream));
        return RSREG_OK;
    }
    k_radius_count<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, ctx->stream>>>(grid_dev(ctx->knn), rq, rs.d_count.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The first pass of FPFHEstimation, not waited for: the index, then every finite record's neighbour rows (fs.d_nn_idx, fs.d_nn_d2)
// and SPFH row (fs.d_spfh); the SPFH rows of non-finite records are zero.  v, nv: the views of the cloud and of its normals.
int fpfh_spfh_device(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, const rsreg_cloud *out, int k, CloudView &v, CloudView &nv,
                     uint32_t *nfin_out)
{
    if (!normals) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    rc = cloud_view(ctx, normals, nullptr, kXyzRule, nv);   // (a normal record: three floats first, the stride rule of every record here)
    if (rc) return rc;
    if (k < 2 || k > kKnnMaxK) return fail(ctx, RSREG_ERR_INVALID_ARG, "k must be between 2 and 64");
    if (nv.n != v.n) return fail(ctx, RSREG_ERR_INVALID_ARG, "the normals must hold one record per record of the cloud");
    if (v.n < (size_t)k) return fail(ctx, RSREG_ERR_INVALID_ARG, "the cloud has fewer than k finite records");
    rc = knn_index_device(ctx, v, k, "the cloud has fewer than k finite records", nfin_out);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const size_t cells = v.n * (size_t)k;
    RSREG_HIP(ctx, fs.d_nn_idx.reserve(cells * 4 + 16));
    RSREG_HIP(ctx, fs.d_nn_d2.reserve(cells * 4 + 16));
    RSREG_HIP(ctx, fs.d_spfh.reserve(v.n * kFpfhRow * 4 + 16));
    if (*nfin_out < v.n) RSREG_HIP(ctx, hipMemsetAsync(fs.d_spfh.ptr, 0, v.n * kFpfhRow * 4, st));
    const float hist_incr = 100.0f / (float)(k - 1);
    k_fpfh_spfh<<<std::min<uint32_t>(*nfin_out, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), k, hist_incr, v.rec, v.stride, nv.rec, nv.stride,
                                                                             fs.d_nn_idx.as<int32_t>(), fs.d_nn_d2.as<float>(), fs.d_spfh.as<float>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The first pass of FPFHEstimationOMP by radius, not waited for: the radius index, then every finite record's SPFH row
// (fs.d_spfh) and neighbour count (rs.d_count); the rows and counts of non-finite records are zero.  v, nv: the views of the cloud
// and of its normals.  An empty cloud: nothing is reserved or launched, *nfin_out = 0.
int fpfh_radius_spfh_device(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, const rsreg_cloud *out, double radius, CloudView &v,
                            CloudView &nv, RadiusQuery *rq, uint32_t *nfin_out)
{
    if (!normals) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    rc = cloud_view(ctx, normals, nullptr, kXyzRule, nv);
    if (rc) return rc;
    if (!(radius > 0.0) || !std::isfinite(radius)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the radius must be finite and above 0");
    if (nv.n != v.n) return fail(ctx, RSREG_ERR_INVALID_ARG, "the normals must hold one record per record of the cloud");
    *nfin_out = 0;
    if (!v.n) return RSREG_OK;
    FilterScratch &fs = ctx->filt;
    RadiusScratch &rs = ctx->rad;
    hipStream_t st = ctx->stream;
    RSREG_HIP(ctx, rs.d_count.reserve(v.n * 4 + 16));
    RSREG_HIP(ctx, fs.d_spfh.reserve(v.n * kFpfhRow * 4 + 16));
    rc = radius_index_device(ctx, v, radius, rs.d_count.as<uint32_t>(), rq, nfin_out);
    if (rc) return rc;
    if (*nfin_out < v.n) RSREG_HIP(ctx, hipMemsetAsync(fs.d_spfh.ptr, 0, v.n * kFpfhRow * 4, st));
    if (!*nfin_out) {   // (the build stops at the box: nothing has written the counts)
        RSREG_HIP(ctx, hipMemsetAsync(rs.d_count.ptr, 0, v.n * 4, st));
        return RSREG_OK;
    }
    k_fpfh_radius_spfh<<<std::min<uint32_t>(*nfin_out, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), *rq, nv.rec, nv.stride, fs.d_spfh.as<float>(),
                                                                                    rs.d_count.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The tail of a normals call, behind the index over `nfin` finite records: room for the pcl::Normal records, NaNs for the
// records that are not finite, the search -- launch(vp, d_normals, &any_nan) with PCL's default viewpoint if there is none,
// left out when nothing is finite -- and the records handed to `out`: a record that got NaNs makes the cloud not dense;
// otherwise it is what the input says.
constexpr size_t kNormalBytes = 32;   // pcl::Normal
template <typename Launch> int normals_into(rsreg_ctx *ctx, const CloudView &v, uint32_t nfin, const float viewpoint[3], rsreg_cloud *out, Launch launch)
{
    FilterScratch &fs = ctx->filt;
    const uint32_t n = (uint32_t)v.n;
    RSREG_HIP(ctx, fs.d_out.reserve(v.n * kNormalBytes + 16));
    if (nfin < n) {
        k_normals_not_finite<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(v.rec, v.stride, n, fs.d_out.as<float>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    const float vp[3] = {viewpoint ? viewpoint[0] : 0.0f, viewpoint ? viewpoint[1] : 0.0f, viewpoint ? viewpoint[2] : 0.0f};
    uint32_t any_nan = 0;
    if (nfin) {
        const int rc = launch(vp, fs.d_out.as<float>(), &any_nan);
        if (rc) return rc;
    }
    return rsreg_cloud_adopt_(out, &fs.d_out, v.n, kNormalBytes, v.width, v.height, (nfin < n || any_nan) ? 0 : v.is_dense);
}

// ---- a search surface (surface_kernels.hpp): the queries are one cloud, the index holds another
constexpr size_t kFpfhBytes = kFpfhRow * 4;   // pcl::FPFHSignature33
enum SurfacePass { kSurfaceOrder, kSurfaceCount, kSurfaceCountMark };   // how far surface_begin goes

struct SurfaceCall {
    CloudView qv, sv, nv;     // the queries, the surface, the surface's normals
    RadiusQuery rq;
    uint32_t nfin = 0;        // finite records of the surface: 0 = nothing is indexed and no query has a neighbour
    SurfaceQueries sq;        // the queries in the order of the surface cells they fall in (nfin and qv.n above 0)
    bool searched() const { return nfin && qv.n; }
};

// The way in of every call with a search surface, not waited for: the views (normals: null for a call without them), the refusals,
// the index over the surface, the queries' order, and -- pass above kSurfaceOrder -- every query's count in rs.d_count (zero for a
// non-finite one, and for all of them when the surface holds nothing finite); kSurfaceCountMark: rs.d_mark[j] = 1 for every
// surface record j that is a neighbour of a query, 0 for the others.
int surface_begin(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface, const rsreg_cloud *normals, const rsreg_cloud *out, double radius,
                  SurfacePass pass, SurfaceCall &sc)
{
    int rc = cloud_view(ctx, queries, out, kXyzRule, sc.qv);
    if (rc) return rc;
    rc = cloud_view(ctx, surface, nullptr, kXyzRule, sc.sv);
    if (rc) return rc;
    if (normals) {
        rc = cloud_view(ctx, normals, nullptr, kXyzRule, sc.nv);
        if (rc) return rc;
    }
    if (!(radius > 0.0) || !std::isfinite(radius)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the radius must be finite and above 0");
    if (normals && sc.nv.n != sc.sv.n) return fail(ctx, RSREG_ERR_INVALID_ARG, "the normals must hold one record per record of the search surface");
    if (sc.qv.n >= (1ull << 30)) return fail(ctx, RSREG_ERR_INVALID_ARG, "cloud too large");
    RadiusScratch &rs = ctx->rad;
    hipStream_t st = ctx->stream;
    const uint32_t nq = (uint32_t)sc.qv.n;
    if (pass != kSurfaceOrder) {
        RSREG_HIP(ctx, rs.d_count.reserve(sc.qv.n * 4 + 16));
        if (nq) RSREG_HIP(ctx, hipMemsetAsync(rs.d_count.ptr, 0, sc.qv.n * 4, st));
    }
    if (pass == kSurfaceCountMark) {
        RSREG_HIP(ctx, rs.d_mark.reserve(sc.sv.n * 4 + 16));
        if (sc.sv.n) RSREG_HIP(ctx, hipMemsetAsync(rs.d_mark.ptr, 0, sc.sv.n * 4, st));
    }
    if (!nq || !sc.sv.n) return RSREG_OK;
    rc = radius_index_device(ctx, sc.sv, radius, nullptr, &sc.rq, &sc.nfin);
    if (rc || !sc.nfin) return rc;
    // the queries by the surface cell they fall in, clamped like any point; a non-finite one behind them all
    const PointGridDev g = grid_dev(ctx->knn);
    const size_t cells = (size_t)ctx->knn.dims[0] * (size_t)ctx->knn.dims[1] * (size_t)ctx->knn.dims[2];
    unsigned bits = 1;
    while ((cells >> bits) != 0) ++bits;
    for (int k = 0; k < 2; ++k) {
        RSREG_HIP(ctx, rs.d_qkeys[k].reserve(sc.qv.n * 4 + 16));
        RSREG_HIP(ctx, rs.d_qvals[k].reserve(sc.qv.n * 4 + 16));
    }
    RSREG_HIP(ctx, rs.d_sort.reserve((size_t)osort_plan<uint32_t>(sc.qv.n, 0, bits).words * 4));
    uint32_t *keys[2] = {rs.d_qkeys[0].as<uint32_t>(), rs.d_qkeys[1].as<uint32_t>()}, *vals[2] = {rs.d_qvals[0].as<uint32_t>(), rs.d_qvals[1].as<uint32_t>()};
    k_radius_cell_keys<<<div_up(nq, kBlock), kBlock, 0, st>>>(RadiusRecords{sc.qv.rec, sc.qv.stride, nullptr}, nq, g, (uint32_t)cells, keys[0], vals[0]);
    RSREG_HIP(ctx, hipGetLastError());
    bool in_first = true;
    RSREG_HIP(ctx, osort_pairs_cleared<uint32_t>(rs.d_sort.as<uint32_t>(), keys[0], keys[1], vals[0], vals[1], sc.qv.n, 0, bits, st, &in_first));
    const int at = in_first ? 0 : 1;
    sc.sq = SurfaceQueries{sc.qv.rec, sc.qv.stride, keys[at], vals[at], nq, (uint32_t)cells};
    if (pass == kSurfaceOrder) return RSREG_OK;
    k_surface_count_mark<<<std::min<uint32_t>(nq, 1u << 16), kKnnWave, 0, st>>>(g, sc.rq, sc.sq, rs.d_count.as<uint32_t>(),
                                                                               pass == kSurfaceCountMark ? rs.d_mark.as<uint32_t>() : nullptr);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// Behind surface_begin(kSurfaceCountMark), with queries that were searched: the list of the needed points of the index (rs.d_list;
// waits for their number, *n_spfh_out) and their SPFH rows in fs.d_spfh, the other rows zero if `zero_rest` and unwritten otherwise.
int surface_spfh_device(rsreg_ctx *ctx, const SurfaceCall &sc, bool zero_rest, uint32_t *n_spfh_out)
{
    FilterScratch &fs = ctx->filt;
    RadiusScratch &rs = ctx->rad;
    PointGrid &kx = ctx->knn;
    hipStream_t st = ctx->stream;
    const PointGridDev g = grid_dev(kx);
    const uint32_t nfin = sc.nfin;
    RSREG_HIP(ctx, rs.d_need.reserve((size_t)nfin * 4 + 16));
    RSREG_HIP(ctx, rs.d_list.reserve((size_t)nfin * 4 + 16));
    RSREG_HIP(ctx, kx.d_scan.reserve(oscan_scratch_bytes<uint32_t>(nfin)));
    RSREG_HIP(ctx, fs.d_spfh.reserve(sc.sv.n * kFpfhRow * 4 + 16));
    uint32_t *need = rs.d_need.as<uint32_t>(), *h_n = fs.host.as<uint32_t>() + kFiltWord;
    k_surface_needed<<<div_up(nfin, kBlock), kBlock, 0, st>>>(g, rs.d_mark.as<uint32_t>(), need);
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, (oscan<uint32_t, true>(need, need, nfin, 0u, kx.d_scan.ptr, st)));
    RSREG_HIP(ctx, hipMemcpyAsync(h_n, need + (nfin - 1), 4, hipMemcpyDeviceToHost, st));
    if (zero_rest) RSREG_HIP(ctx, hipMemsetAsync(fs.d_spfh.ptr, 0, sc.sv.n * kFpfhRow * 4, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t n_spfh = *h_n;
    *n_spfh_out = n_spfh;
    if (!n_spfh) return RSREG_OK;
    k_surface_list<<<div_up(nfin, kBlock), kBlock, 0, st>>>(need, nfin, rs.d_list.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    k_surface_spfh<<<std::min<uint32_t>(n_spfh, 1u << 16), kKnnWave, 0, st>>>(g, sc.rq, sc.nv.rec, sc.nv.stride, rs.d_list.as<uint32_t>(), n_spfh,
                                                                             fs.d_spfh.as<float>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The tail of a call that leaves one row of `row_bytes` per query in fs.d_out (room for them has been reserved): the rows of
// non-finite queries have been queued by the caller; with nothing to search every row is `nan_mask`'s, otherwise launch(d_any)
// queues the kernel of the finite ones.  The rows go to `out` with the queries' shape; a NaN row makes it not dense.
template <typename Launch> int surface_rows_into(rsreg_ctx *ctx, const SurfaceCall &sc, size_t row_bytes, unsigned long long nan_mask, rsreg_cloud *out, Launch launch)
{
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const CloudView &qv = sc.qv;
    bool nan_rows = false;
    if (qv.n && !sc.nfin) {
        const size_t words = qv.n * (row_bytes / 4);
        k_surface_no_neighbours<<<div_up64(words, kBlock), kBlock, 0, st>>>(fs.d_out.as<float>(), words, (uint32_t)(row_bytes / 4), nan_mask);
        RSREG_HIP(ctx, hipGetLastError());
        nan_rows = true;
    } else if (qv.n) {
        // whether a query was not finite: the last key of the sorted pairs; it comes home with the kernel's word
        uint32_t *h_last = fs.host.as<uint32_t>() + kFiltWord + 1, any_nan = 0;
        RSREG_HIP(ctx, hipMemcpyAsync(h_last, sc.sq.keys + (sc.sq.n - 1), 4, hipMemcpyDeviceToHost, st));
        const int rc = word_home(ctx, true, launch, &any_nan);
        if (rc) return rc;
        nan_rows = any_nan || *h_last == sc.sq.no_cell;
    }
    return rsreg_cloud_adopt_(out, &fs.d_out, qv.n, row_bytes, qv.width, qv.height, nan_rows ? 0 : qv.is_dense);
}


// ---- pcl::ISSKeypoint3D (iss_kernels.hpp)
// what every ISS call refuses before anything is launched
int iss_check(rsreg_ctx *ctx, const double *radii, int n_radii, int min_neighbors, const double *gammas, int n_gammas)
{
    for (int k = 0; k < n_radii; ++k)
        if (!(radii[k] > 0.0) || !std::isfinite(radii[k])) return fail(ctx, RSREG_ERR_INVALID_ARG, "the salient and the non-max radius must be finite and above 0");
    if (min_neighbors < 0) return fail(ctx, RSREG_ERR_INVALID_ARG, "min_neighbors must not be negative");
    for (int k = 0; k < n_gammas; ++k)
        if (!std::isfinite(gammas[k])) return fail(ctx, RSREG_ERR_INVALID_ARG, "gamma_21 and gamma_32 must be finite");
    return RSREG_OK;
}

// The first pass, not waited for (v.n above 0): the index at the salient radius, then every record's eigenvalues (rs.d_iss_eig),
// saliency (rs.d_iss_sal) and m_s (rs.d_count), zeros for a non-finite record.  *rq: the query of the salient radius.
int iss_saliency_device(rsreg_ctx *ctx, const CloudView &v, const rsreg_iss_params &p, RadiusQuery *rq, uint32_t *nfin_out)
{
    RadiusScratch &rs = ctx->rad;
    hipStream_t st = ctx->stream;
    RSREG_HIP(ctx, rs.d_count.reserve(v.n * 4 + 16));
    RSREG_HIP(ctx, rs.d_iss_eig.reserve(v.n * 24 + 16));
    RSREG_HIP(ctx, rs.d_iss_sal.reserve(v.n * 8 + 16));
    int rc = radius_index_device(ctx, v, p.salient_radius, rs.d_count.as<uint32_t>(), rq, nfin_out);
    if (rc) return rc;
    if (*nfin_out < v.n) {
        RSREG_HIP(ctx, hipMemsetAsync(rs.d_iss_eig.ptr, 0, v.n * 24, st));
        RSREG_HIP(ctx, hipMemsetAsync(rs.d_iss_sal.ptr, 0, v.n * 8, st));
    }
    if (!*nfin_out) {   // (the build stops at the box: nothing has written the counts)
        RSREG_HIP(ctx, hipMemsetAsync(rs.d_count.ptr, 0, v.n * 4, st));
        return RSREG_OK;
    }
    k_iss_saliency<<<std::min<uint32_t>(*nfin_out, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), *rq, (uint32_t)p.min_neighbors, p.gamma_21, p.gamma_32,
                                                                                rs.d_iss_eig.as<double>(), rs.d_iss_sal.as<double>(), rs.d_count.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The second pass, not waited for (v.n above 0), over whatever index the context holds (nfin points): fs.d_flags[i] = 1 for the
// keypoints among the saliencies in rs.d_iss_sal
int iss_non_max_device(rsreg_ctx *ctx, const CloudView &v, double non_max_radius, int min_neighbors, uint32_t nfin)
{
    FilterScratch &fs = ctx->filt;
    RSREG_HIP(ctx, fs.d_flags.reserve(v.n * 4 + 16));
    RSREG_HIP(ctx, hipMemsetAsync(fs.d_flags.ptr, 0, v.n * 4, ctx->stream));
    if (!nfin) return RSREG_OK;
    k_iss_non_max<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, ctx->stream>>>(grid_dev(ctx->knn), radius_query(non_max_radius, ctx->knn),
                                                                                   ctx->rad.d_iss_sal.as<double>(), (uint32_t)min_neighbors, fs.d_flags.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}


int cluster_check(rsreg_ctx *ctx, const rsreg_cluster_params &p)
{
    if (!(p.tolerance > 0.0) || !std::isfinite(p.tolerance)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the cluster tolerance must be finite and above 0");
    if (p.min_cluster_size > p.max_cluster_size) return fail(ctx, RSREG_ERR_INVALID_ARG, "min_cluster_size must not exceed max_cluster_size");
    return RSREG_OK;
}

// EuclideanClusterExtraction on the device, not waited for (v.n above 0): the index at the tolerance, the hooks, the roots and sizes,
// the ranking.  Leaves every record's label (cs.d_label), the number of clusters (cs.d_n) and, with `lists`, the clusters' offsets
// (cs.d_offsets, n + 1 words) and their records cluster by cluster (*d_indices: n words, the records without a cluster at the end).
// No finite record (*nfin_out = 0): nothing but the index's box has run and nothing is left.
int cluster_labels_device(rsreg_ctx *ctx, const CloudView &v, const rsreg_cluster_params &p, bool lists, const uint32_t **d_indices, uint32_t *nfin_out)
{
    ClusterScratch &cs = ctx->clus;
    RadiusScratch &rs = ctx->rad;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n, nb = div_up(n, kBlock);
    RadiusQuery rq;
    int rc = radius_index_device(ctx, v, p.tolerance, nullptr, &rq, nfin_out);
    if (rc || !*nfin_out) return rc;
    for (DevBuf *b : {&cs.d_parent, &cs.d_root, &cs.d_size, &cs.d_rank, &cs.d_label}) RSREG_HIP(ctx, b->reserve(v.n * 4 + 16));
    RSREG_HIP(ctx, cs.d_offsets.reserve(v.n * 4 + 20));
    RSREG_HIP(ctx, cs.d_scan.reserve(oscan_scratch_bytes<uint32_t>(v.n + 1)));
    RSREG_HIP(ctx, cs.d_n.reserve(16));
    unsigned bits = 1;
    while (((size_t)n >> bits) != 0) ++bits;   // the keys of both sorts: a rank or n - size below n, and n itself
    RSREG_HIP(ctx, rs.d_sort.reserve((size_t)osort_plan<uint32_t>(v.n, 0, bits).words * 4));
    uint32_t *keys[2] = {rs.d_keys[0].as<uint32_t>(), rs.d_keys[1].as<uint32_t>()}, *vals[2] = {rs.d_vals[0].as<uint32_t>(), rs.d_vals[1].as<uint32_t>()};
    uint32_t *parent = cs.d_parent.as<uint32_t>(), *root = cs.d_root.as<uint32_t>(), *size = cs.d_size.as<uint32_t>(), *rank = cs.d_rank.as<uint32_t>();

    k_cluster_init<<<nb, kBlock, 0, st>>>(n, parent, size);
    k_cluster_hook<<<std::min<uint32_t>(*nfin_out, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), rq, parent);
    k_cluster_flatten<<<nb, kBlock, 0, st>>>(v.rec, v.stride, n, parent, root, size);
    k_cluster_keys<<<nb, kBlock, 0, st>>>(n, root, size, p.min_cluster_size, p.max_cluster_size, keys[0], vals[0]);
    RSREG_HIP(ctx, hipGetLastError());
    bool in_first = true;
    RSREG_HIP(ctx, osort_pairs_cleared<uint32_t>(rs.d_sort.as<uint32_t>(), keys[0], keys[1], vals[0], vals[1], v.n, 0, bits, st, &in_first));
    int at = in_first ? 0 : 1;
    k_cluster_rank<<<div_up(n + 1, kBlock), kBlock, 0, st>>>(n, keys[at], vals[at], rank, cs.d_offsets.as<uint32_t>(), cs.d_n.as<uint32_t>());
    k_cluster_labels<<<nb, kBlock, 0, st>>>(n, root, rank, cs.d_label.as<int32_t>(), lists ? keys[0] : nullptr, lists ? vals[0] : nullptr);
    RSREG_HIP(ctx, hipGetLastError());
    if (!lists) return RSREG_OK;
    RSREG_HIP(ctx, oscan<uint32_t>(cs.d_offsets.as<uint32_t>(), cs.d_offsets.as<uint32_t>(), v.n + 1, 0u, cs.d_scan.ptr, st));
    RSREG_HIP(ctx, osort_pairs_cleared<uint32_t>(rs.d_sort.as<uint32_t>(), keys[0], keys[1], vals[0], vals[1], v.n, 0, bits, st, &in_first));
    *d_indices = vals[in_first ? 0 : 1];
    return RSREG_OK;
}

}  // namespace

extern "C" {

void rsreg_iss_params_default(rsreg_iss_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->gamma_21 = 0.975;
    p->gamma_32 = 0.975;
    p->min_neighbors = 5;
}

int rsreg_cloud_iss_saliency(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_iss_params *params, double *eig_out, double *saliency_out,
                             uint32_t *count_out)
{
    CloudView v;
    if (!params) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    const double gammas[2] = {params->gamma_21, params->gamma_32};
    rc = iss_check(ctx, &params->salient_radius, 1, params->min_neighbors, gammas, 2);   // (the non-max radius is not used here)
    if (rc || !v.n) return rc;
    RadiusQuery rq;
    uint32_t nfin = 0;
    rc = iss_saliency_device(ctx, v, *params, &rq, &nfin);
    if (rc) return rc;
    RadiusScratch &rs = ctx->rad;
    hipStream_t st = ctx->stream;
    if (eig_out) RSREG_HIP(ctx, hipMemcpyAsync(eig_out, rs.d_iss_eig.ptr, v.n * 24, hipMemcpyDeviceToHost, st));
    if (saliency_out) RSREG_HIP(ctx, hipMemcpyAsync(saliency_out, rs.d_iss_sal.ptr, v.n * 8, hipMemcpyDeviceToHost, st));
    if (count_out) RSREG_HIP(ctx, hipMemcpyAsync(count_out, rs.d_count.ptr, v.n * 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    return RSREG_OK;
}

int rsreg_cloud_iss_non_max(rsreg_ctx *ctx, const rsreg_cloud *in, const double *saliency, double non_max_radius, int min_neighbors, uint8_t *is_keypoint_out)
{
    CloudView v;
    if (!saliency || !is_keypoint_out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    rc = iss_check(ctx, &non_max_radius, 1, min_neighbors, nullptr, 0);
    if (rc || !v.n) return rc;
    RadiusScratch &rs = ctx->rad;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    RSREG_HIP(ctx, rs.d_iss_sal.reserve(v.n * 8 + 16));
    RadiusQuery rq;
    uint32_t nfin = 0;
    rc = radius_index_device(ctx, v, non_max_radius, nullptr, &rq, &nfin);
    if (rc) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(rs.d_iss_sal.ptr, saliency, v.n * 8, hipMemcpyHostToDevice, st));
    rc = iss_non_max_device(ctx, v, non_max_radius, min_neighbors, nfin);
    if (rc) return rc;
    // the flags are words on the device and bytes at the caller's: they come home through the pinned scratch, a slice at a time
    constexpr size_t kSlice = 1u << 16;
    RSREG_HIP(ctx, fs.host.reserve(kSlice * 4));
    for (size_t at = 0; at < v.n; at += kSlice) {
        const size_t m = std::min(kSlice, v.n - at);
        RSREG_HIP(ctx, hipMemcpyAsync(fs.host.ptr, fs.d_flags.as<uint32_t>() + at, m * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        for (size_t i = 0; i < m; ++i) is_keypoint_out[at + i] = (uint8_t)fs.host.as<uint32_t>()[i];
    }
    return RSREG_OK;
}

int rsreg_cloud_iss_keypoints(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_iss_params *params, rsreg_cloud *out, int32_t *index_out, size_t capacity,
                              uint64_t *n_keypoints)
{
    CloudView v;
    if (!params || (out && out == in)) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    const double radii[2] = {params->salient_radius, params->non_max_radius}, gammas[2] = {params->gamma_21, params->gamma_32};
    rc = iss_check(ctx, radii, 2, params->min_neighbors, gammas, 2);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    RadiusScratch &rs = ctx->rad;
    PointGrid &kx = ctx->knn;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    uint32_t kept = 0;
    if (n) {
        RadiusQuery rq;
        uint32_t nfin = 0;
        rc = iss_saliency_device(ctx, v, *params, &rq, &nfin);
        if (rc) return rc;
        rc = iss_non_max_device(ctx, v, params->non_max_radius, params->min_neighbors, nfin);   // (over the same index)
        if (rc) return rc;
        // flags -> positions -> the keypoints' indices and, for `out`, their records (the path of RadiusOutlierRemoval); waits for their number
        RSREG_HIP(ctx, fs.d_pos.reserve(v.n * 4 + 16));
        RSREG_HIP(ctx, kx.d_scan.reserve(oscan_scratch_bytes<uint32_t>(v.n)));
        RSREG_HIP(ctx, rs.d_iss_index.reserve(v.n * 4 + 16));
        if (out) RSREG_HIP(ctx, fs.d_out.reserve(v.n * v.stride + 16));
        RSREG_HIP(ctx, kx.d_box.reserve(64));
        RSREG_HIP(ctx, fs.host.reserve(256));
        RSREG_HIP(ctx, oscan<uint32_t>(fs.d_flags.as<uint32_t>(), fs.d_pos.as<uint32_t>(), v.n, 0u, kx.d_scan.ptr, st));
        rc = word_home(ctx, false, [&](uint32_t *d_kept) {
            k_iss_indices<<<div_up(n, kBlock), kBlock, 0, st>>>(fs.d_flags.as<uint32_t>(), fs.d_pos.as<uint32_t>(), n, rs.d_iss_index.as<int32_t>(), d_kept);
            if (out)
                k_filter_gather<<<div_up64((unsigned long long)n * (v.stride / 4), kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, fs.d_flags.as<uint32_t>(),
                                                                                                           fs.d_pos.as<uint32_t>(), fs.d_out.as<char>(), d_kept);
        }, &kept);
        if (rc) return rc;
        const size_t home = std::min<size_t>(kept, capacity);
        if (index_out && home) {
            RSREG_HIP(ctx, hipMemcpyAsync(index_out, rs.d_iss_index.ptr, home * 4, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipStreamSynchronize(st));
        }
    }
    if (out) {
        rc = rsreg_cloud_adopt_(out, &fs.d_out, kept, v.stride, kept, 1, 1);
        if (rc) return rc;
    }
    if (n_keypoints) *n_keypoints = kept;
    return RSREG_OK;
}

int rsreg_cloud_radius_count_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface, double radius, uint32_t *host_out)
{
    if (!host_out) return RSREG_ERR_INVALID_ARG;
    SurfaceCall sc;
    int rc = surface_begin(ctx, queries, surface, nullptr, nullptr, radius, kSurfaceCount, sc);
    if (rc || !sc.qv.n) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(host_out, ctx->rad.d_count.ptr, sc.qv.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSREG_OK;
}

int rsreg_cloud_normals_radius_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface, double radius, const float viewpoint[3],
                                       rsreg_cloud *out)
{
    if (!out || out == queries || out == surface) return RSREG_ERR_INVALID_ARG;
    SurfaceCall sc;
    int rc = surface_begin(ctx, queries, surface, nullptr, out, radius, kSurfaceOrder, sc);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t nq = (uint32_t)sc.qv.n;
    RSREG_HIP(ctx, fs.d_out.reserve(sc.qv.n * kNormalBytes + 16));
    if (sc.searched()) {
        k_normals_not_finite<<<div_up(nq, kBlock), kBlock, 0, st>>>(sc.qv.rec, sc.qv.stride, nq, fs.d_out.as<float>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    const float vp[3] = {viewpoint ? viewpoint[0] : 0.0f, viewpoint ? viewpoint[1] : 0.0f, viewpoint ? viewpoint[2] : 0.0f};
    return surface_rows_into(ctx, sc, kNormalBytes, 0x17ull, out, [&](uint32_t *d_any) {
        k_surface_normals<<<std::min<uint32_t>(nq, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), sc.rq, sc.sq, vp[0], vp[1], vp[2], fs.d_out.as<float>(), d_any);
    });
}

int rsreg_cloud_spfh_radius_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface, const rsreg_cloud *surface_normals, double radius,
                                    float *host_out, uint32_t *needed_out, uint32_t *count_out)
{
    if (!host_out || !surface_normals) return RSREG_ERR_INVALID_ARG;
    SurfaceCall sc;
    int rc = surface_begin(ctx, queries, surface, surface_normals, nullptr, radius, kSurfaceCountMark, sc);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    if (!sc.searched()) {   // nothing is needed and nobody has a neighbour
        std::memset(host_out, 0, sc.sv.n * kFpfhRow * 4);
        if (needed_out) std::memset(needed_out, 0, sc.sv.n * 4);
        if (count_out) std::memset(count_out, 0, sc.qv.n * 4);
        return RSREG_OK;
    }
    uint32_t n_spfh = 0;
    rc = surface_spfh_device(ctx, sc, true, &n_spfh);
    if (rc) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(host_out, ctx->filt.d_spfh.ptr, sc.sv.n * kFpfhRow * 4, hipMemcpyDeviceToHost, st));
    if (needed_out) RSREG_HIP(ctx, hipMemcpyAsync(needed_out, ctx->rad.d_mark.ptr, sc.sv.n * 4, hipMemcpyDeviceToHost, st));
    if (count_out) RSREG_HIP(ctx, hipMemcpyAsync(count_out, ctx->rad.d_count.ptr, sc.qv.n * 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    return RSREG_OK;
}

int rsreg_cloud_fpfh_radius_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface, const rsreg_cloud *surface_normals, double radius,
                                    rsreg_cloud *out, uint64_t *n_spfh_out)
{
    if (!out || !surface_normals || out == queries || out == surface || out == surface_normals) return RSREG_ERR_INVALID_ARG;
    SurfaceCall sc;
    int rc = surface_begin(ctx, queries, surface, surface_normals, out, radius, kSurfaceCountMark, sc);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    RadiusScratch &rs = ctx->rad;
    hipStream_t st = ctx->stream;
    const uint32_t nq = (uint32_t)sc.qv.n;
    uint32_t n_spfh = 0;
    if (sc.searched()) {
        rc = surface_spfh_device(ctx, sc, false, &n_spfh);
        if (rc) return rc;
    }
    RSREG_HIP(ctx, fs.d_out.reserve(sc.qv.n * kFpfhBytes + 16));
    if (sc.searched()) {
        k_fpfh_radius_not_finite<<<div_up64((unsigned long long)nq * kFpfhRow, kBlock), kBlock, 0, st>>>(sc.qv.rec, sc.qv.stride, nq, fs.d_out.as<float>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    rc = surface_rows_into(ctx, sc, kFpfhBytes, 0x1ffffffffull, out, [&](uint32_t *d_any) {
        k_surface_fpfh_weight<<<std::min<uint32_t>(nq, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), sc.rq, sc.sq, rs.d_count.as<uint32_t>(), fs.d_spfh.as<float>(),
                                                                                    fs.d_out.as<float>(), d_any);
    });
    if (rc) return rc;
    if (n_spfh_out) *n_spfh_out = n_spfh;
    return RSREG_OK;
}

int rsreg_cloud_passthrough(rsreg_ctx *ctx, const rsreg_cloud *in, int field, float lo, float hi, int negative, int keep_organized,
                            rsreg_cloud *out)
{
    CloudView v;
    if (!out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    // (PCL warns about a field it does not find and returns an empty cloud: here the call is refused)
    if (field < 0 || field > 2) return fail(ctx, RSREG_ERR_INVALID_ARG, "PassThrough filters on field 0 (x), 1 (y) or 2 (z)");
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    if (n) {
        RSREG_HIP(ctx, fs.d_flags.reserve(v.n * 4 + 16));
        k_pass_flags<<<div_up(n, kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, field, lo, hi, negative ? 1 : 0, fs.d_flags.as<uint32_t>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    uint32_t kept = 0;
    if (!keep_organized) return compact_into(ctx, v, out, 1, &kept);
    return organized_into(ctx, v, out, &kept);
}

int rsreg_cloud_knn_mean_distance(rsreg_ctx *ctx, const rsreg_cloud *in, int mean_k, float *host_out)
{
    CloudView v;
    if (!host_out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    uint32_t nfin = 0;
    rc = knn_mean_distance_device(ctx, v, mean_k, &nfin);
    if (rc) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(host_out, ctx->filt.d_dist.ptr, v.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSREG_OK;
}

int rsreg_cloud_sor(rsreg_ctx *ctx, const rsreg_cloud *in, int mean_k, double stddev_mult, int negative, rsreg_cloud *out, rsreg_sor_stats *stats)
{
    CloudView v;
    if (!out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    uint32_t nfin = 0;
    rc = knn_mean_distance_device(ctx, v, mean_k, &nfin);
    if (rc) return rc;
    // PCL divides by n_valid - 1
    if (nfin < 2) return fail(ctx, RSREG_ERR_INVALID_ARG, "the cloud has fewer than two finite records");
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n, nb = div_up(n, kBlock);
    RSREG_HIP(ctx, fs.d_sums.reserve(64));
    RSREG_HIP(ctx, fs.d_flags.reserve(v.n * 4 + 16));
    k_sor_sums<<<2, kKnnWave, 0, st>>>(fs.d_dist.as<float>(), n, fs.d_sums.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    double *hs = fs.host.as<double>() + 8;
    RSREG_HIP(ctx, hipMemcpyAsync(hs, fs.d_sums.ptr, 16, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    // PCL: sum and sq_sum over ALL records (a non-finite record adds its 0), divided by the number of valid ones
    const double sum = hs[0], sq = hs[1], nv = (double)nfin;
    const double mean = sum / nv;
    const double variance = (sq - sum * sum / nv) / (nv - 1.0);
    const double stddev = std::sqrt(variance);
    const double threshold = mean + stddev_mult * stddev;
    k_sor_flags<<<nb, kBlock, 0, st>>>(v.rec, v.stride, fs.d_dist.as<float>(), n, threshold, negative ? 1 : 0, fs.d_flags.as<uint32_t>());
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

int rsreg_cloud_knn(rsreg_ctx *ctx, const rsreg_cloud *in, int k, int32_t *index_out, float *sqr_dist_out)
{
    CloudView v;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    if (k < 1 || k > kKnnMaxK) return fail(ctx, RSREG_ERR_INVALID_ARG, "k must be between 1 and 64");
    uint32_t nfin = 0;
    rc = knn_index_device(ctx, v, k, "the cloud has fewer than k finite records", &nfin);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const size_t cells = v.n * (size_t)k;
    int32_t *d_idx = nullptr;
    float *d_d2 = nullptr;
    if (index_out) {
        RSREG_HIP(ctx, fs.d_nn_idx.reserve(cells * 4 + 16));
        d_idx = fs.d_nn_idx.as<int32_t>();
        if (nfin < v.n) RSREG_HIP(ctx, hipMemsetAsync(d_idx, 0xff, cells * 4, st));   // a non-finite record's row: all -1
    }
    if (sqr_dist_out) {
        RSREG_HIP(ctx, fs.d_nn_d2.reserve(cells * 4 + 16));
        d_d2 = fs.d_nn_d2.as<float>();
        if (nfin < v.n) RSREG_HIP(ctx, hipMemsetAsync(d_d2, 0, cells * 4, st));      // ... all 0
    }
    if (!d_idx && !d_d2) return RSREG_OK;
    k_knn_indices<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), k, d_idx, d_d2);
    RSREG_HIP(ctx, hipGetLastError());
    if (d_idx) RSREG_HIP(ctx, hipMemcpyAsync(index_out, d_idx, cells * 4, hipMemcpyDeviceToHost, st));
    if (d_d2) RSREG_HIP(ctx, hipMemcpyAsync(sqr_dist_out, d_d2, cells * 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    return RSREG_OK;
}

int rsreg_cloud_normals(rsreg_ctx *ctx, const rsreg_cloud *in, int k, const float viewpoint[3], rsreg_cloud *out)
{
    CloudView v;
    if (!out || out == in) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    if (k < 3 || k > kKnnMaxK) return fail(ctx, RSREG_ERR_INVALID_ARG, "k must be between 3 and 64");
    uint32_t nfin = 0;
    rc = knn_index_device(ctx, v, k, "the cloud has fewer than k finite records", &nfin);
    if (rc) return rc;
    return normals_into(ctx, v, nfin, viewpoint, out, [&](const float vp[3], float *d_normals, uint32_t *) {
        k_normals<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, ctx->stream>>>(grid_dev(ctx->knn), k, v.rec, v.stride, vp[0], vp[1], vp[2], d_normals);
        RSREG_HIP(ctx, hipGetLastError());
        return (int)RSREG_OK;
    });
}

// GeneralizedIterativeClosestPoint::computeCovariances (include/rsreg.h: the contract): the index and the walk of rsreg_cloud_normals,
// k_gicp_cov in the place of k_normals, 48-byte records of six doubles
int rsreg_cloud_gicp_covariances(rsreg_ctx *ctx, const rsreg_cloud *in, int k, double epsilon, rsreg_cloud *out)
{
    CloudView v;
    if (!out || out == in) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    if (k < 4 || k > kKnnMaxK) return fail(ctx, RSREG_ERR_INVALID_ARG, "k must be between 4 and 64");
    if (!std::isfinite(epsilon)) return fail(ctx, RSREG_ERR_INVALID_ARG, "epsilon must be finite");
    uint32_t nfin = 0;
    rc = knn_index_device(ctx, v, k, "the cloud has fewer than k finite records", &nfin);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    const uint32_t n = (uint32_t)v.n;
    RSREG_HIP(ctx, fs.d_out.reserve(v.n * kGicpCovBytes + 16));
    if (nfin < n) {
        k_gicp_cov_not_finite<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(v.rec, v.stride, n, fs.d_out.as<double>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    if (nfin) {
        k_gicp_cov<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, ctx->stream>>>(grid_dev(ctx->knn), k, v.rec, v.stride, epsilon, fs.d_out.as<double>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    return rsreg_cloud_adopt_(out, &fs.d_out, v.n, kGicpCovBytes, v.width, v.height, nfin < n ? 0 : v.is_dense);
}

int rsreg_cloud_spfh(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, int k, float *host_out)
{
    CloudView v, nv;
    if (!host_out) return RSREG_ERR_INVALID_ARG;
    uint32_t nfin = 0;
    int rc = fpfh_spfh_device(ctx, in, normals, nullptr, k, v, nv, &nfin);
    if (rc) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(host_out, ctx->filt.d_spfh.ptr, v.n * kFpfhRow * 4, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSREG_OK;
}

int rsreg_cloud_fpfh(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, int k, rsreg_cloud *out)
{
    CloudView v, nv;
    if (!out || out == in || out == normals) return RSREG_ERR_INVALID_ARG;
    uint32_t nfin = 0;
    int rc = fpfh_spfh_device(ctx, in, normals, out, k, v, nv, &nfin);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    constexpr size_t kFpfhBytes = kFpfhRow * 4;   // pcl::FPFHSignature33
    RSREG_HIP(ctx, fs.d_out.reserve(v.n * kFpfhBytes + 16));
    // a record that is not finite, or whose own normal is not, gets NaNs: whether one did comes back with the stream
    uint32_t any_nan = 0;
    rc = word_home(ctx, true, [&](uint32_t *d_any) {
        k_fpfh_weight<<<std::min<uint32_t>(n, 1u << 16), kKnnWave, 0, st>>>(v.rec, v.stride, nv.rec, nv.stride, n, k, fs.d_nn_idx.as<int32_t>(),
                                                                           fs.d_nn_d2.as<float>(), fs.d_spfh.as<float>(), fs.d_out.as<float>(), d_any);
    }, &any_nan);
    if (rc) return rc;
    return rsreg_cloud_adopt_(out, &fs.d_out, v.n, kFpfhBytes, v.width, v.height, any_nan ? 0 : v.is_dense);
}

int rsreg_cloud_spfh_radius(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, double radius, float *host_out, uint32_t *count_out)
{
    CloudView v, nv;
    if (!host_out) return RSREG_ERR_INVALID_ARG;
    uint32_t nfin = 0;
    RadiusQuery rq;
    int rc = fpfh_radius_spfh_device(ctx, in, normals, nullptr, radius, v, nv, &rq, &nfin);
    if (rc || !v.n) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(host_out, ctx->filt.d_spfh.ptr, v.n * kFpfhRow * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (count_out) RSREG_HIP(ctx, hipMemcpyAsync(count_out, ctx->rad.d_count.ptr, v.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSREG_OK;
}

int rsreg_cloud_fpfh_radius(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, double radius, rsreg_cloud *out)
{
    CloudView v, nv;
    if (!out || out == in || out == normals) return RSREG_ERR_INVALID_ARG;
    uint32_t nfin = 0;
    RadiusQuery rq;
    int rc = fpfh_radius_spfh_device(ctx, in, normals, out, radius, v, nv, &rq, &nfin);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    constexpr size_t kFpfhBytes = kFpfhRow * 4;   // pcl::FPFHSignature33
    RSREG_HIP(ctx, fs.d_out.reserve(v.n * kFpfhBytes + 16));
    if (nfin < n) {
        k_fpfh_radius_not_finite<<<div_up64((unsigned long long)n * kFpfhRow, kBlock), kBlock, 0, st>>>(v.rec, v.stride, n, fs.d_out.as<float>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    // a record whose own normal is not finite gets NaNs too, and the arithmetic can make some: whether it did comes back with the stream
    uint32_t any_nan = 0;
    if (nfin) {
        rc = word_home(ctx, true, [&](uint32_t *d_any) {
            k_fpfh_radius_weight<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, st>>>(grid_dev(ctx->knn), rq, nv.rec, nv.stride, fs.d_spfh.as<float>(),
                                                                                         fs.d_out.as<float>(), d_any);
        }, &any_nan);
        if (rc) return rc;
    }
    return rsreg_cloud_adopt_(out, &fs.d_out, v.n, kFpfhBytes, v.width, v.height, (nfin < n || any_nan) ? 0 : v.is_dense);
}

int rsreg_cloud_radius_count(rsreg_ctx *ctx, const rsreg_cloud *in, double radius, uint32_t *host_out)
{
    CloudView v;
    if (!host_out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    rc = radius_count_device(ctx, v, radius);
    if (rc || !v.n) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(host_out, ctx->rad.d_count.ptr, v.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSREG_OK;
}

int rsreg_cloud_radius_outlier_removal(rsreg_ctx *ctx, const rsreg_cloud *in, double radius, int min_neighbors, int negative, int keep_organized,
                                       rsreg_cloud *out, uint64_t *n_kept)
{
    CloudView v;
    if (!out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    if (min_neighbors < 0) return fail(ctx, RSREG_ERR_INVALID_ARG, "min_neighbors must not be negative");
    rc = radius_count_device(ctx, v, radius);
    if (rc) return rc;
    FilterScratch &fs = ctx->filt;
    const uint32_t n = (uint32_t)v.n;
    if (n) {
        RSREG_HIP(ctx, fs.d_flags.reserve(v.n * 4 + 16));
        k_ror_flags<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(ctx->rad.d_count.as<uint32_t>(), n, (uint32_t)min_neighbors, negative ? 1 : 0,
                                                                  fs.d_flags.as<uint32_t>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    uint32_t kept = 0;
    rc = keep_organized ? organized_into(ctx, v, out, &kept) : compact_into(ctx, v, out, v.is_dense, &kept);
    if (rc) return rc;
    if (n_kept) *n_kept = kept;
    return RSREG_OK;
}

int rsreg_cloud_normals_radius(rsreg_ctx *ctx, const rsreg_cloud *in, double radius, const float viewpoint[3], rsreg_cloud *out)
{
    CloudView v;
    if (!out || out == in) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    if (!(radius > 0.0) || !std::isfinite(radius)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the radius must be finite and above 0");
    uint32_t nfin = 0;
    RadiusQuery rq;
    if (v.n) {
        rc = radius_index_device(ctx, v, radius, nullptr, &rq, &nfin);
        if (rc) return rc;
    }
    // a record with fewer than three neighbours gets NaNs too: whether one did comes back with the stream
    return normals_into(ctx, v, nfin, viewpoint, out, [&](const float vp[3], float *d_normals, uint32_t *any_nan) {
        return word_home(ctx, true, [&](uint32_t *d_any) {
            k_normals_radius<<<std::min<uint32_t>(nfin, 1u << 16), kKnnWave, 0, ctx->stream>>>(grid_dev(ctx->knn), rq, vp[0], vp[1], vp[2], d_normals, d_any);
        }, any_nan);
    });
}

void rsreg_cluster_params_default(rsreg_cluster_params *p)
{
    if (!p) return;
    p->tolerance = 0.0;
    p->min_cluster_size = 1u;
    p->max_cluster_size = 0x7fffffffu;
}

int rsreg_cloud_euclidean_clusters(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cluster_params *p, int32_t *labels_out, uint32_t *indices_out,
                                   uint32_t *offsets_out, uint32_t capacity, uint32_t *n_clusters_out)
{
    CloudView v;
    if (!p) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    rc = cluster_check(ctx, *p);
    if (rc) return rc;
    ClusterScratch &cs = ctx->clus;
    hipStream_t st = ctx->stream;
    uint32_t nfin = 0, count = 0;
    // at home (pinned): the count | n + 1 offsets | n indices -- what the caller gets of the last two depends on the count
    const uint32_t *h_offsets = nullptr, *h_indices = nullptr, *d_indices = nullptr;
    const bool lists = indices_out || offsets_out;
    if (v.n) {
        rc = cluster_labels_device(ctx, v, *p, lists, &d_indices, &nfin);
        if (rc) return rc;
    }
    if (nfin) {
        RSREG_HIP(ctx, cs.host.reserve((2 * v.n + 2) * 4));
        uint32_t *h = cs.host.as<uint32_t>();
        h_offsets = h + 1;
        h_indices = h + 2 + v.n;
        RSREG_HIP(ctx, hipMemcpyAsync(h, cs.d_n.ptr, 4, hipMemcpyDeviceToHost, st));
        if (lists) RSREG_HIP(ctx, hipMemcpyAsync(h + 1, cs.d_offsets.ptr, (v.n + 1) * 4, hipMemcpyDeviceToHost, st));
        if (indices_out) RSREG_HIP(ctx, hipMemcpyAsync(h + 2 + v.n, d_indices, v.n * 4, hipMemcpyDeviceToHost, st));
        if (labels_out) RSREG_HIP(ctx, hipMemcpyAsync(labels_out, cs.d_label.ptr, v.n * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        count = h[0];
    } else if (labels_out) {
        std::fill(labels_out, labels_out + v.n, -1);
    }
    const uint32_t reported = std::min(count, capacity);
    if (offsets_out) {
        if (nfin) std::memcpy(offsets_out, h_offsets, ((size_t)reported + 1) * 4);
        else offsets_out[0] = 0u;
    }
    if (indices_out && reported) std::memcpy(indices_out, h_indices, (size_t)h_offsets[reported] * 4);
    if (n_clusters_out) *n_clusters_out = count;
    return RSREG_OK;
}

int rsreg_cloud_cluster_filter(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cluster_params *p, uint32_t rank_lo, uint32_t rank_hi, int negative,
                               int keep_organized, rsreg_cloud *out, uint64_t *n_kept)
{
    CloudView v;
    if (!p || !out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    rc = cluster_check(ctx, *p);
    if (rc) return rc;
    if (rank_lo > rank_hi) return fail(ctx, RSREG_ERR_INVALID_ARG, "rank_lo must not exceed rank_hi");
    FilterScratch &fs = ctx->filt;
    ClusterScratch &cs = ctx->clus;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)v.n;
    if (n) {
        uint32_t nfin = 0;
        const uint32_t *d_indices = nullptr;
        rc = cluster_labels_device(ctx, v, *p, false, &d_indices, &nfin);
        if (rc) return rc;
        if (!nfin) {   // (the build stopped at the box: no record has a cluster)
            RSREG_HIP(ctx, cs.d_label.reserve(v.n * 4 + 16));
            RSREG_HIP(ctx, hipMemsetAsync(cs.d_label.ptr, 0xff, v.n * 4, st));
        }
        RSREG_HIP(ctx, fs.d_flags.reserve(v.n * 4 + 16));
        k_cluster_filter_flags<<<div_up(n, kBlock), kBlock, 0, st>>>(cs.d_label.as<int32_t>(), n, rank_lo, rank_hi, negative ? 1 : 0, fs.d_flags.as<uint32_t>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    uint32_t kept = 0;
    rc = keep_organized ? organized_into(ctx, v, out, &kept) : compact_into(ctx, v, out, v.is_dense, &kept);
    if (rc) return rc;
    if (n_kept) *n_kept = kept;
    return RSREG_OK;
}

}  // extern "C"
