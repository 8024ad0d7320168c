// features.hip — feature matching on clouds of descriptors resident in HBM (C ABI: include/rsreg.h, "feature matching"): the
// third stage of a feature-based pre-alignment, NormalEstimation -> FPFHEstimation -> matching.  rsreg_cloud_feature_knn is the
// exact k-nearest-neighbour search of every source row among the target's rows in the 33-dimensional space of
// pcl::FPFHSignature33; rsreg_cloud_feature_correspondences is pcl::registration::CorrespondenceEstimation over it
// (determineCorrespondences, determineReciprocalCorrespondences).
//
// Brute force (feature_kernels.hpp): the validity pass, the search cut into (query blocks) x (target slices) by the host-only
// rule of feature_plan.hpp, the merge of the slices.  The correspondences are the K = 1 search forwards and, if reciprocal, the
// same launch with the roles swapped, then one flag / scan (oscan.hpp) / gather over the source rows, ONE 8-byte count read back
// and one download.  Everything runs on the context's stream with the scratch rsreg_ctx::feat and touches no other buffer.
#include "records.hpp"
#include "cloud_ops.hpp"
#include "oscan.hpp"
#include "feature_kernels.hpp"

using namespace rsreg;

namespace {

constexpr CloudRule kDescRule{(size_t)kFmDim * 4, true, "a descriptor cloud's records start with 33 floats: a stride of at least 132 that is a multiple of 4",
                              0x7ffffff0ull, "cloud too large"};

// a descriptor cloud's records on the context's stream (an upload or a queued filter of it has been waited for)
int desc_view(rsreg_ctx *ctx, const rsreg_cloud *c, CloudView &v) { return cloud_view(ctx, c, nullptr, kDescRule, v); }

// fs.d_valid[which][i] = row i is valid; the count of valid rows into word `which` of fs.d_count (zeroed by the caller)
int valid_rows(rsreg_ctx *ctx, const CloudView &v, int which)
{
    FeatureScratch &fs = ctx->feat;
    RSREG_HIP(ctx, fs.d_valid[which].reserve(v.n * 4 + 16));
    if (!v.n) return RSREG_OK;
    k_fm_valid<<<div_up((uint32_t)v.n, kFmBlock), kFmBlock, 0, ctx->stream>>>(v.rec, v.stride, (uint32_t)v.n, fs.d_valid[which].as<uint32_t>(),
                                                                             fs.d_count.as<uint32_t>() + which);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

template <int K> int launch_search(rsreg_ctx *ctx, const CloudView &q, const uint32_t *qvalid, const CloudView &t, const uint32_t *tvalid, const FeaturePlan &p,
                                   unsigned long long *out)
{
    k_fm_search<K><<<p.qblocks * p.slices, kFmLanes, 0, ctx->stream>>>(q.rec, q.stride, qvalid, (uint32_t)q.n, t.rec, t.stride, tvalid, (uint32_t)t.n, p.slices, out);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

template <int K> int launch_merge(rsreg_ctx *ctx, const unsigned long long *keys, uint32_t lists, const uint32_t *qvalid, uint32_t nq, int k, int32_t *idx, float *d2)
{
    k_fm_merge<K><<<div_up(nq, kFmBlock), kFmBlock, 0, ctx->stream>>>(keys, lists, qvalid, nq, k, idx, d2);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// keys[i] = the nearest valid row of t to the valid row i of q (kFmNone: q's row is not valid, or t has no valid row): the K = 1
// search, not waited for.  q.n >= 1.
int nearest_keys(rsreg_ctx *ctx, const CloudView &q, const uint32_t *qvalid, const CloudView &t, const uint32_t *tvalid, DevBuf &keys)
{
    RSREG_HIP(ctx, keys.reserve(q.n * 8 + 16));
    RSREG_HIP(ctx, hipMemsetAsync(keys.ptr, 0xff, q.n * 8, ctx->stream));
    if (!t.n) return RSREG_OK;
    return launch_search<1>(ctx, q, qvalid, t, tvalid, feature_plan((uint32_t)q.n, (uint32_t)t.n), keys.as<unsigned long long>());
}

}  // namespace

extern "C" {

int rsreg_cloud_feature_knn(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, int k, int32_t *index_out, float *sqr_dist_out)
{
    CloudView sv, tv;
    int rc = desc_view(ctx, source, sv);
    if (rc) return rc;
    rc = desc_view(ctx, target, tv);
    if (rc) return rc;
    if (k < 1 || k > 16) return fail(ctx, RSREG_ERR_INVALID_ARG, "k must be between 1 and 16");
    if (!sv.n) return fail(ctx, RSREG_ERR_INVALID_ARG, "the source is empty");
    if (tv.n < (size_t)k) return fail(ctx, RSREG_ERR_INVALID_ARG, "the target has fewer than k valid rows");
    FeatureScratch &fs = ctx->feat;
    hipStream_t st = ctx->stream;
    RSREG_HIP(ctx, fs.d_count.reserve(64));
    RSREG_HIP(ctx, fs.host.reserve(64));
    RSREG_HIP(ctx, hipMemsetAsync(fs.d_count.ptr, 0, 16, st));
    const bool same = source == target;
    rc = valid_rows(ctx, tv, 1);
    if (rc) return rc;
    if (!same) rc = valid_rows(ctx, sv, 0);
    if (rc) return rc;
    // how many target rows are valid decides whether anything is searched: one word home
    RSREG_HIP(ctx, hipMemcpyAsync(fs.host.ptr, fs.d_count.as<uint32_t>() + 1, 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    if (fs.host.as<uint32_t>()[0] < (uint32_t)k) return fail(ctx, RSREG_ERR_INVALID_ARG, "the target has fewer than k valid rows");
    if (!index_out && !sqr_dist_out) return RSREG_OK;
    const uint32_t ns = (uint32_t)sv.n;
    const uint32_t *svalid = fs.d_valid[same ? 1 : 0].as<uint32_t>(), *tvalid = fs.d_valid[1].as<uint32_t>();
    const size_t cells = sv.n * (size_t)k;
    int32_t *d_idx = nullptr;
    float *d_d2 = nullptr;
    if (index_out) {
        RSREG_HIP(ctx, fs.d_idx.reserve(cells * 4 + 16));
        d_idx = fs.d_idx.as<int32_t>();
    }
    if (sqr_dist_out) {
        RSREG_HIP(ctx, fs.d_d2.reserve(cells * 4 + 16));
        d_d2 = fs.d_d2.as<float>();
    }
    if (k == 1) {
        rc = nearest_keys(ctx, sv, svalid, tv, tvalid, fs.d_keys[0]);
        if (!rc) rc = launch_merge<1>(ctx, fs.d_keys[0].as<unsigned long long>(), 1u, svalid, ns, k, d_idx, d_d2);
    } else {
        const int K = k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;   // the compile-time list that holds k
        const FeaturePlan p = feature_plan(ns, (uint32_t)tv.n);
        RSREG_HIP(ctx, fs.d_part.reserve((size_t)p.slices * K * sv.n * 8 + 16));
        unsigned long long *part = fs.d_part.as<unsigned long long>();
        const uint32_t lists = p.slices * (uint32_t)K;
        switch (K) {
        case 2:
            rc = launch_search<2>(ctx, sv, svalid, tv, tvalid, p, part);
            if (!rc) rc = launch_merge<2>(ctx, part, lists, svalid, ns, k, d_idx, d_d2);
            break;
        case 4:
            rc = launch_search<4>(ctx, sv, svalid, tv, tvalid, p, part);
            if (!rc) rc = launch_merge<4>(ctx, part, lists, svalid, ns, k, d_idx, d_d2);
            break;
        case 8:
            rc = launch_search<8>(ctx, sv, svalid, tv, tvalid, p, part);
            if (!rc) rc = launch_merge<8>(ctx, part, lists, svalid, ns, k, d_idx, d_d2);
            break;
        default:
            rc = launch_search<16>(ctx, sv, svalid, tv, tvalid, p, part);
            if (!rc) rc = launch_merge<16>(ctx, part, lists, svalid, ns, k, d_idx, d_d2);
            break;
        }
    }
    if (rc) return rc;
    if (d_idx) RSREG_HIP(ctx, hipMemcpyAsync(index_out, d_idx, cells * 4, hipMemcpyDeviceToHost, st));
    if (d_d2) RSREG_HIP(ctx, hipMemcpyAsync(sqr_dist_out, d_d2, cells * 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    return RSREG_OK;
}

int rsreg_cloud_feature_correspondences(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, double max_distance, int reciprocal,
                                        rsreg_correspondence *host_out, size_t capacity, size_t *n_out)
{
    CloudView sv, tv;
    int rc = desc_view(ctx, source, sv);
    if (rc) return rc;
    rc = desc_view(ctx, target, tv);
    if (rc) return rc;
    if (!n_out || (capacity && !host_out)) return RSREG_ERR_INVALID_ARG;
    if (!(max_distance >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_distance must not be negative or NaN");
    const double max_sqr = max_distance * max_distance;   // (DBL_MAX: +inf, which keeps every match)
    if (!sv.n || !tv.n) {
        *n_out = 0;
        return RSREG_OK;
    }
    FeatureScratch &fs = ctx->feat;
    hipStream_t st = ctx->stream;
    const uint32_t ns = (uint32_t)sv.n;
    RSREG_HIP(ctx, fs.d_count.reserve(64));
    RSREG_HIP(ctx, fs.host.reserve(64));
    RSREG_HIP(ctx, hipMemsetAsync(fs.d_count.ptr, 0, 16, st));
    const bool same = source == target;
    rc = valid_rows(ctx, tv, 1);
    if (rc) return rc;
    if (!same) rc = valid_rows(ctx, sv, 0);
    if (rc) return rc;
    const uint32_t *svalid = fs.d_valid[same ? 1 : 0].as<uint32_t>(), *tvalid = fs.d_valid[1].as<uint32_t>();
    rc = nearest_keys(ctx, sv, svalid, tv, tvalid, fs.d_keys[0]);
    if (rc) return rc;
    if (reciprocal) {   // every target row's nearest valid source row: the same launch, the roles swapped
        rc = nearest_keys(ctx, tv, tvalid, sv, svalid, fs.d_keys[1]);
        if (rc) return rc;
    }
    const size_t room = capacity < sv.n ? capacity : sv.n;
    RSREG_HIP(ctx, fs.d_flags.reserve(sv.n * 4 + 16));
    RSREG_HIP(ctx, fs.d_pos.reserve(sv.n * 4 + 16));
    RSREG_HIP(ctx, fs.d_scan.reserve(oscan_scratch_bytes<uint32_t>(sv.n)));
    RSREG_HIP(ctx, fs.d_out.reserve(room * sizeof(rsreg_correspondence) + 16));
    const unsigned long long *fwd = fs.d_keys[0].as<unsigned long long>();
    k_fm_corr_flags<<<div_up(ns, kFmBlock), kFmBlock, 0, st>>>(fwd, reciprocal ? fs.d_keys[1].as<unsigned long long>() : nullptr, ns, max_sqr,
                                                              fs.d_flags.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, oscan<uint32_t>(fs.d_flags.as<uint32_t>(), fs.d_pos.as<uint32_t>(), sv.n, 0u, fs.d_scan.ptr, st));
    unsigned long long *d_found = fs.d_count.as<unsigned long long>() + 1, *h_found = fs.host.as<unsigned long long>();
    k_fm_corr_gather<<<div_up(ns, kFmBlock), kFmBlock, 0, st>>>(fwd, fs.d_flags.as<uint32_t>(), fs.d_pos.as<uint32_t>(), ns, (unsigned long long)room,
                                                               fs.d_out.as<rsreg_correspondence>(), d_found);
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(h_found, d_found, 8, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    const size_t found = (size_t)*h_found, take = found < room ? found : room;
    if (take) {
        RSREG_HIP(ctx, hipMemcpyAsync(host_out, fs.d_out.ptr, take * sizeof(rsreg_correspondence), hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
    }
    *n_out = found;
    return RSREG_OK;
}

}  // extern "C"
