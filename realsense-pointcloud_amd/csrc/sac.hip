// sac.hip — a pose from a correspondence list, on clouds resident in HBM (C ABI: include/rsreg.h, "pose from correspondences"):
// the fourth stage of a feature-based pre-alignment, NormalEstimation -> FPFHEstimation -> matching -> this.
// rsreg_cloud_sac_correspondences is pcl::registration::CorrespondenceRejectorSampleConsensus (RANSAC over the pairs, the model
// SampleConsensusModelRegistration), rsreg_cloud_estimate_rigid_svd is TransformationEstimationSVD over a correspondence list,
// rsreg_cloud_count_inliers scores transforms the caller supplies.
//
// The list goes up once a call and becomes six coordinate planes (k_sac_gather).  The rejector launches batches of hypotheses
// (sac_plan.hpp: sac_batch) -- k_sac_hypotheses fills a table of transforms, k_sac_count scores all of them against all pairs --
// and replays PCL's stopping rule over the integer counts on the host, in hypothesis order.  Everything runs on the context's
// stream with the scratch rsreg_ctx::sac and touches no other buffer.
#include <cfloat>

#include "records.hpp"
#include "cloud_ops.hpp"
#include "oscan.hpp"
#include "sac_kernels.hpp"

using namespace rsreg;

namespace {

struct SacPairs {
    uint32_t n = 0, pitch = 0;
    const float *planes = nullptr;
};

// the least float >= t2 (t2 >= 0, not NaN): for a float d2, d2 < sac_thr_up(t2) is (double)d2 < t2
float sac_thr_up(double t2)
{
    float f = (float)t2;   // round to nearest: at most one step off
    if ((double)f < t2) f = std::nextafterf(f, INFINITY);
    return f;
}

// both clouds and the list checked, the list in HBM (sc.d_corr) and gathered into sc.d_planes; nothing is waited for
int sac_load(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const rsreg_correspondence *corr, size_t n, SacPairs &pr)
{
    CloudView sv, tv;
    int rc = cloud_view(ctx, source, nullptr, kXyzRule, sv);
    if (rc) return rc;
    rc = cloud_view(ctx, target, nullptr, kXyzRule, tv);
    if (rc) return rc;
    if (n && !corr) return fail(ctx, RSREG_ERR_INVALID_ARG, "a correspondence list is needed");
    if (n > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "correspondence list too large");
    for (size_t i = 0; i < n; ++i)
        if (corr[i].index_query < 0 || (size_t)corr[i].index_query >= sv.n || corr[i].index_match < 0 || (size_t)corr[i].index_match >= tv.n)
            return fail(ctx, RSREG_ERR_INVALID_ARG, "a correspondence names a record outside its cloud");
    pr.n = (uint32_t)n;
    if (!n) return RSREG_OK;
    SacScratch &sc = ctx->sac;
    hipStream_t st = ctx->stream;
    pr.pitch = div_up(pr.n, kSacTile) * kSacTile;
    const size_t bytes = n * sizeof(rsreg_correspondence);
    RSREG_HIP(ctx, hipStreamSynchronize(st));   // (a list of an earlier call may still be on its way out of the staging buffer)
    RSREG_HIP(ctx, sc.h_corr.reserve(bytes));
    RSREG_HIP(ctx, sc.d_corr.reserve(bytes + 16));
    RSREG_HIP(ctx, sc.d_planes.reserve((size_t)pr.pitch * 6 * 4 + 16));
    std::memcpy(sc.h_corr.ptr, corr, bytes);
    RSREG_HIP(ctx, hipMemcpyAsync(sc.d_corr.ptr, sc.h_corr.ptr, bytes, hipMemcpyHostToDevice, st));
    k_sac_gather<<<div_up(pr.pitch, kSacLanes), kSacLanes, 0, st>>>(sc.d_corr.as<rsreg_correspondence>(), pr.n, sv.rec, sv.stride, tv.rec, tv.stride,
                                                                   sc.d_planes.as<float>(), pr.pitch);
    RSREG_HIP(ctx, hipGetLastError());
    pr.planes = sc.d_planes.as<float>();
    return RSREG_OK;
}

// counts[0 .. H) = the inliers of the H rows of sc.d_table, queued
int sac_count(rsreg_ctx *ctx, const SacPairs &pr, uint32_t H, float thr_up)
{
    SacScratch &sc = ctx->sac;
    RSREG_HIP(ctx, hipMemsetAsync(sc.d_counts.ptr, 0, (size_t)H * 4, ctx->stream));
    const SacPlan p = sac_plan(pr.n, H);
    k_sac_count<<<p.tiles * p.slices, kSacBlock, 0, ctx->stream>>>(pr.planes, pr.pitch, sc.d_table.as<float>(), H, p.tiles, p.slice_chunks, thr_up,
                                                                  sc.d_counts.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// the 17 sums over the flagged finite pairs (flags nullptr: every finite pair), home and waited for
int sac_sums(rsreg_ctx *ctx, const SacPairs &pr, const uint32_t *flags, double sums[RSREG_NUM_SUMS])
{
    SacScratch &sc = ctx->sac;
    hipStream_t st = ctx->stream;
    const uint32_t nb = div_up(pr.n, (uint32_t)kSacSumTile);
    RSREG_HIP(ctx, sc.d_partials.reserve((size_t)nb * RSREG_NUM_SUMS * 8 + 16));
    RSREG_HIP(ctx, sc.d_sums.reserve(RSREG_NUM_SUMS * 8));
    RSREG_HIP(ctx, sc.host.reserve(4096));
    k_sac_sums<<<nb, kSacSumTile, 0, st>>>(pr.planes, pr.pitch, pr.n, flags, sc.d_partials.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    k_sac_final<<<RSREG_NUM_SUMS, kSacFinalBlock, 0, st>>>(sc.d_partials.as<double>(), nb, sc.d_sums.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(sc.host.ptr, sc.d_sums.ptr, RSREG_NUM_SUMS * 8, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    std::memcpy(sums, sc.host.ptr, RSREG_NUM_SUMS * 8);
    return RSREG_OK;
}

// flags = the pairs within the threshold under T; how many are set and how many differ from `old` (nullable), waited for
int sac_select(rsreg_ctx *ctx, const SacPairs &pr, const Mat4f &T, float thr_up, const uint32_t *old, uint32_t *flags, uint32_t &n_set, uint32_t &n_changed)
{
    SacScratch &sc = ctx->sac;
    hipStream_t st = ctx->stream;
    RSREG_HIP(ctx, hipMemsetAsync(sc.d_word.ptr, 0, 32, st));
    k_sac_flags<<<div_up(pr.n, kSacLanes), kSacLanes, 0, st>>>(pr.planes, pr.pitch, pr.n, to_mat34(T), thr_up, old, flags, sc.d_word.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(sc.host.ptr, sc.d_word.ptr, 8, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    n_set = sc.host.as<uint32_t>()[0];
    n_changed = sc.host.as<uint32_t>()[1];
    return RSREG_OK;
}

}  // namespace

extern "C" {

void rsreg_sac_params_default(rsreg_sac_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->inlier_threshold = 0.05;
    p->probability = 0.99;
    p->min_sample_distance = 0.0;
    p->max_iterations = 1000;
    p->refit_rounds = 0;
    p->seed = 0;
}

int rsreg_cloud_count_inliers(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const rsreg_correspondence *corr, size_t n,
                              const float *transforms, size_t H, double threshold, uint32_t *counts_out)
{
    SacPairs pr;
    int rc = sac_load(ctx, source, target, corr, n, pr);
    if (rc) return rc;
    if (!(threshold >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the threshold must not be negative or NaN");
    if (H > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "too many transforms");
    if (!H) return RSREG_OK;
    if (!transforms || !counts_out) return fail(ctx, RSREG_ERR_INVALID_ARG, "transforms and counts_out are needed");
    if (!n) {
        std::memset(counts_out, 0, H * 4);
        return RSREG_OK;
    }
    SacScratch &sc = ctx->sac;
    hipStream_t st = ctx->stream;
    RSREG_HIP(ctx, sc.host.reserve(H * 48 + 4096));
    RSREG_HIP(ctx, sc.d_table.reserve(H * 48 + 16));
    RSREG_HIP(ctx, sc.d_counts.reserve(H * 4 + 16));
    float *rows = sc.host.as<float>();
    for (size_t h = 0; h < H; ++h)   // column-major 4 x 4 -> the three rows the kernels read
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) rows[h * 12 + r * 4 + c] = transforms[h * 16 + c * 4 + r];
    RSREG_HIP(ctx, hipMemcpyAsync(sc.d_table.ptr, rows, H * 48, hipMemcpyHostToDevice, st));
    rc = sac_count(ctx, pr, (uint32_t)H, sac_thr_up(threshold * threshold));
    if (rc) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(counts_out, sc.d_counts.ptr, H * 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    return RSREG_OK;
}

int rsreg_cloud_estimate_rigid_svd(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const rsreg_correspondence *corr, size_t n,
                                   float t_out[16], double sums_out[RSREG_NUM_SUMS])
{
    SacPairs pr;
    int rc = sac_load(ctx, source, target, corr, n, pr);
    if (rc) return rc;
    if (n < 3) return fail(ctx, RSREG_ERR_INVALID_ARG, "fewer than three finite pairs");
    double sums[RSREG_NUM_SUMS];
    rc = sac_sums(ctx, pr, nullptr, sums);
    if (rc) return rc;
    if (!(sums[0] >= 3.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "fewer than three finite pairs");
    Mat4f T;
    if (!umeyama_from_sums(sums, T)) return fail(ctx, RSREG_ERR_INVALID_ARG, "fewer than three finite pairs");
    if (t_out) std::memcpy(t_out, T.m, sizeof T.m);
    if (sums_out) std::memcpy(sums_out, sums, sizeof sums);
    return RSREG_OK;
}

int rsreg_cloud_sac_correspondences(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const rsreg_correspondence *corr, size_t n,
                                    const rsreg_sac_params *params, rsreg_correspondence *host_out, size_t capacity, size_t *n_out, rsreg_sac_result *result)
{
    SacPairs pr;
    int rc = sac_load(ctx, source, target, corr, n, pr);
    if (rc) return rc;
    if (!n_out || (capacity && !host_out)) return fail(ctx, RSREG_ERR_INVALID_ARG, "n_out, and host_out with a capacity, are needed");
    rsreg_sac_params prm;
    if (params) prm = *params; else rsreg_sac_params_default(&prm);
    if (!(prm.inlier_threshold >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "inlier_threshold must not be negative or NaN");
    if (!(prm.probability > 0.0 && prm.probability < 1.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "probability must lie strictly between 0 and 1");
    if (!(prm.min_sample_distance >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "min_sample_distance must not be negative or NaN");
    if (prm.max_iterations < 0 || prm.refit_rounds < 0) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_iterations and refit_rounds must not be negative");
    const float thr_up = sac_thr_up(prm.inlier_threshold * prm.inlier_threshold);
    const double min_sample_sqr = prm.min_sample_distance * prm.min_sample_distance;

    rsreg_sac_result res;
    std::memset(&res, 0, sizeof res);
    const Mat4f eye = Mat4f::identity();
    std::memcpy(res.transform, eye.m, sizeof eye.m);
    res.best_hypothesis = -1;
    res.sample[0] = res.sample[1] = res.sample[2] = -1;

    SacScratch &sc = ctx->sac;
    hipStream_t st = ctx->stream;
    // ---- the hypotheses, a batch at a time, and PCL's stopping rule replayed over their counts in hypothesis order
    long long best = -1, best_h = -1;   // (best: PCL's -INT_MAX -- the first valid hypothesis always sets k)
    uint32_t consumed = 0;
    if (n >= 3) {
        const uint32_t max_it = (uint32_t)prm.max_iterations;
        const double log_probability = std::log(1.0 - prm.probability), eps = DBL_EPSILON;
        double k = 1.0;
        RSREG_HIP(ctx, sc.host.reserve((size_t)kSacMaxBatch * 20 + 4096));
        RSREG_HIP(ctx, sc.d_table.reserve((size_t)kSacMaxBatch * 48 + 16));
        RSREG_HIP(ctx, sc.d_sample.reserve((size_t)kSacMaxBatch * 16 + 16));
        RSREG_HIP(ctx, sc.d_counts.reserve((size_t)kSacMaxBatch * 4 + 16));
        uint32_t scored = 0;
        bool stop = false;
        while (!stop) {
            const uint32_t B = sac_batch(scored, max_it);
            if (!B) break;
            k_sac_hypotheses<<<div_up(B, 64u), 64, 0, st>>>(pr.planes, pr.pitch, pr.n, (unsigned long long)prm.seed, (unsigned long long)scored, B, min_sample_sqr,
                                                           sc.d_table.as<float>(), sc.d_sample.as<int32_t>());
            RSREG_HIP(ctx, hipGetLastError());
            rc = sac_count(ctx, pr, B, thr_up);
            if (rc) return rc;
            RSREG_HIP(ctx, hipMemcpyAsync(sc.host.ptr, sc.d_counts.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipMemcpyAsync(sc.host.as<uint32_t>() + kSacMaxBatch, sc.d_sample.ptr, (size_t)B * 16, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipStreamSynchronize(st));
            const uint32_t *counts = sc.host.as<uint32_t>();
            const int32_t *sample = sc.host.as<int32_t>() + kSacMaxBatch;   // ([4 j + 3]: the try that was good, -1 for an invalid hypothesis)
            for (uint32_t j = 0; j < B; ++j) {
                const uint32_t h = scored + j;
                if (!((double)h < k)) { stop = true; break; }
                if (sample[4 * j + 3] >= 0 && (long long)counts[j] > best) {
                    best = counts[j];
                    best_h = h;
                    const double w = (double)counts[j] / (double)n;
                    double q = 1.0 - w * w * w;
                    q = q < eps ? eps : q;
                    q = q > 1.0 - eps ? 1.0 - eps : q;
                    k = log_probability / std::log(q);
                }
                consumed = h + 1;
            }
            scored += B;
        }
    }
    res.iterations = (int32_t)consumed;
    const bool found = n >= 3 && best >= 3;
    if (!found) {   // PCL: computeModel failed -- every correspondence remains
        const size_t take = n < capacity ? n : capacity;
        if (take) std::memcpy(host_out, corr, take * sizeof(rsreg_correspondence));
        *n_out = n;
        if (result) *result = res;
        return RSREG_OK;
    }
    // ---- the winner again, alone: its transform and its sample (the generator is a function of the hypothesis number)
    k_sac_hypotheses<<<1, 64, 0, st>>>(pr.planes, pr.pitch, pr.n, (unsigned long long)prm.seed, (unsigned long long)best_h, 1u, min_sample_sqr,
                                      sc.d_table.as<float>(), sc.d_sample.as<int32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(sc.host.ptr, sc.d_table.ptr, 48, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipMemcpyAsync(sc.host.as<char>() + 64, sc.d_sample.ptr, 16, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    Mat4f T = Mat4f::identity();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) T(r, c) = sc.host.as<float>()[r * 4 + c];
    res.found = 1;
    res.best_hypothesis = (int32_t)best_h;
    for (int i = 0; i < 3; ++i) res.sample[i] = reinterpret_cast<const int32_t *>(sc.host.as<char>() + 64)[i];
    // ---- its inliers; the refit rounds
    RSREG_HIP(ctx, sc.d_flags[0].reserve(n * 4 + 16));
    RSREG_HIP(ctx, sc.d_flags[1].reserve(n * 4 + 16));
    RSREG_HIP(ctx, sc.d_word.reserve(64));
    int cur = 0;
    uint32_t n_in = 0, n_changed = 0;
    rc = sac_select(ctx, pr, T, thr_up, nullptr, sc.d_flags[cur].as<uint32_t>(), n_in, n_changed);
    if (rc) return rc;
    for (int r = 0; r < prm.refit_rounds && n_in >= 3; ++r) {
        double sums[RSREG_NUM_SUMS];
        rc = sac_sums(ctx, pr, sc.d_flags[cur].as<uint32_t>(), sums);
        if (rc) return rc;
        Mat4f Tr;
        if (!umeyama_from_sums(sums, Tr)) break;
        T = Tr;
        std::memcpy(res.sums, sums, sizeof sums);
        res.refit_rounds_run = r + 1;
        rc = sac_select(ctx, pr, T, thr_up, sc.d_flags[cur].as<uint32_t>(), sc.d_flags[cur ^ 1].as<uint32_t>(), n_in, n_changed);
        if (rc) return rc;
        cur ^= 1;
        if (!n_changed) break;
    }
    std::memcpy(res.transform, T.m, sizeof T.m);
    res.n_inliers = n_in;
    // ---- the kept correspondences, in input order
    const size_t room = capacity < n ? capacity : n;
    RSREG_HIP(ctx, sc.d_pos.reserve(n * 4 + 16));
    RSREG_HIP(ctx, sc.d_scan.reserve(oscan_scratch_bytes<uint32_t>(n)));
    RSREG_HIP(ctx, sc.d_out.reserve(room * sizeof(rsreg_correspondence) + 16));
    const uint32_t *flags = sc.d_flags[cur].as<uint32_t>();
    RSREG_HIP(ctx, oscan<uint32_t>(flags, sc.d_pos.as<uint32_t>(), n, 0u, sc.d_scan.ptr, st));
    unsigned long long *d_found = reinterpret_cast<unsigned long long *>(sc.d_word.as<char>() + 8);
    k_sac_emit<<<div_up(pr.n, kSacLanes), kSacLanes, 0, st>>>(sc.d_corr.as<rsreg_correspondence>(), flags, sc.d_pos.as<uint32_t>(), pr.n, (unsigned long long)room,
                                                             sc.d_out.as<rsreg_correspondence>(), d_found);
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(sc.host.ptr, d_found, 8, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    const size_t kept = (size_t)*sc.host.as<unsigned long long>(), take = kept < room ? kept : room;
    if (take) {
        RSREG_HIP(ctx, hipMemcpyAsync(host_out, sc.d_out.ptr, take * sizeof(rsreg_correspondence), hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
    }
    *n_out = kept;
    if (result) *result = res;
    return RSREG_OK;
}

}  // extern "C"
