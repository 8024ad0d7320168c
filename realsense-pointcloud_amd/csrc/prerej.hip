// prerej.hip — a pose from descriptor neighbours, scored against the whole target cloud, on clouds resident in HBM (C ABI:
// include/rsreg.h, "pose from descriptor neighbours"): pcl::SampleConsensusPrerejective, the alternative to the fourth stage of a
// feature-based pre-alignment (sac.hip), and its scoring stage on its own.
// rsreg_cloud_score_transforms scores transforms the caller supplies, rsreg_cloud_prerejective generates them from a table of
// descriptor neighbours (what rsreg_cloud_feature_knn wrote), scores the ones that pass the polygon test and replays the selection
// on the host in hypothesis order.
//
// The target is indexed once a call (pointgrid.hpp: grid_build, FitGridPolicy).  Hypotheses go out in batches (prerej_plan.hpp:
// prerej_batch) -- k_prerej_hypotheses fills a table, k_prerej_score searches every (valid hypothesis, source record),
// k_prerej_final adds the partial sums -- a round of batches is queued before the host waits once.  Everything runs on the context's
// stream with the index and the scratch of rsreg_ctx::prerej and touches no other buffer.
#include <cfloat>

#include "records.hpp"
#include "cloud_ops.hpp"
#include "oscan.hpp"
#include "prerej_kernels.hpp"

using namespace rsreg;

namespace {

// the least float >= t2 (t2 >= 0, not NaN): for a float d2, d2 < prerej_thr_up(t2) is (double)d2 < t2 (sac.hip: sac_thr_up)
float prerej_thr_up(double t2)
{
    float f = (float)t2;   // round to nearest: at most one step off
    if ((double)f < t2) f = std::nextafterf(f, INFINITY);
    return f;
}

}  // namespace

// ---- what scia.hip calls as well (declared in cloud_ops.hpp)
namespace rsreg {

// both clouds checked; nothing is launched
int prerej_views(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, PrejClouds &c)
{
    int rc = cloud_view(ctx, source, nullptr, kXyzRule, c.sv);
    if (rc) return rc;
    rc = cloud_view(ctx, target, nullptr, kXyzRule, c.tv);
    if (rc) return rc;
    c.ns = (uint32_t)c.sv.n;
    c.nt = (uint32_t)c.tv.n;
    return RSREG_OK;
}

// the target's index, queued and (for its box) waited for
int prerej_index(rsreg_ctx *ctx, const PrejClouds &c)
{
    PrerejScratch &sc = ctx->prerej;
    RSREG_HIP(ctx, sc.host.reserve(4096));
    return grid_build<FitGridPolicy>(ctx, sc.grid, PrejRecords{c.tv.rec, c.tv.stride}, c.nt, 1, sc.host.as<uint32_t>());
}

// the caller's table of descriptor neighbours, checked on the host: k, every entry, the rows of -1
int prerej_table_check(rsreg_ctx *ctx, const int32_t *neighbor_index, int k, uint32_t ns, uint32_t nt)
{
    if (k < 1 || k > 16) return fail(ctx, RSREG_ERR_INVALID_ARG, "k must lie in 1 .. 16");
    if (ns && !neighbor_index) return fail(ctx, RSREG_ERR_INVALID_ARG, "a neighbour table is needed");
    for (size_t i = 0; i < ns; ++i) {
        const int32_t *row = neighbor_index + i * (size_t)k;
        int minus = 0;
        for (int j = 0; j < k; ++j) {
            if (row[j] == -1) ++minus;
            else if (row[j] < 0 || (uint32_t)row[j] >= nt) return fail(ctx, RSREG_ERR_INVALID_ARG, "the neighbour table names a record outside the target");
        }
        if (minus && minus != k) return fail(ctx, RSREG_ERR_INVALID_ARG, "a row of the neighbour table is -1 in part");
    }
    return RSREG_OK;
}

// d_sums[h] = the partials of hypothesis h < B of the launch before (d_valid: which rows have any; null: every row), queued
int prerej_final(rsreg_ctx *ctx, const uint32_t *d_valid, uint32_t B, uint32_t tiles, double *d_sums)
{
    k_prerej_final<<<div_up(B, (uint32_t)kPrejLanes), kPrejLanes, 0, ctx->stream>>>(ctx->prerej.d_partials.as<double>(), d_valid, B, tiles, d_sums);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// the per-round buffers, for rounds of R hypotheses against ns source records
int prerej_reserve(rsreg_ctx *ctx, uint32_t ns, uint32_t R)
{
    PrerejScratch &sc = ctx->prerej;
    const size_t groups = ((size_t)ns + kPrejTile - 1) / kPrejTile;
    RSREG_HIP(ctx, sc.d_table.reserve((size_t)R * 48 + 16));
    RSREG_HIP(ctx, sc.d_valid.reserve((size_t)R * 4 + 16));
    RSREG_HIP(ctx, sc.d_sample.reserve((size_t)R * 32 + 16));
    RSREG_HIP(ctx, sc.d_counts.reserve((size_t)R * 4 + 16));
    RSREG_HIP(ctx, sc.d_sums.reserve((size_t)R * 8 + 16));
    RSREG_HIP(ctx, sc.d_partials.reserve((size_t)prerej_batch_cap(ns) * groups * kPrejPartialStride + 16));
    RSREG_HIP(ctx, sc.host.reserve((size_t)R * 96 + 4096));
    return RSREG_OK;
}

}  // namespace rsreg

namespace {

// the rows [0, B) of sc.d_table + 12 * at scored into sc.d_counts + at and sc.d_sums + at (valid: sc.d_valid + at, or every row), queued
int prerej_score(rsreg_ctx *ctx, const PrejClouds &c, uint32_t at, uint32_t B, bool use_valid, float limit2)
{
    PrerejScratch &sc = ctx->prerej;
    hipStream_t st = ctx->stream;
    const PrejPlan p = prerej_plan(c.ns, B);
    const uint32_t *valid = use_valid ? sc.d_valid.as<uint32_t>() + at : nullptr;
    RSREG_HIP(ctx, hipMemsetAsync(sc.d_counts.as<uint32_t>() + at, 0, (size_t)B * 4, st));
    k_prerej_score<<<p.tiles * p.slices, kPrejBlock, 0, st>>>(c.sv.rec, c.sv.stride, c.ns, sc.d_table.as<float>() + (size_t)at * 12, valid, B, p.tiles, p.slice_chunks,
                                                             grid_dev(sc.grid), limit2, sc.d_counts.as<uint32_t>() + at, sc.d_partials.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    return prerej_final(ctx, valid, B, p.tiles, sc.d_sums.as<double>() + at);
}

}  // namespace

extern "C" {

void rsreg_prerej_params_default(rsreg_prerej_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->max_correspondence_distance = std::sqrt(DBL_MAX);   // pcl::Registration's corr_dist_threshold_
    p->inlier_fraction = 0.0;
    p->similarity_threshold = 0.9f;
    p->max_iterations = 10;                                // pcl::Registration's max_iterations_
    p->select_by_inliers = 0;
    p->seed = 0;
}

int rsreg_cloud_score_transforms(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const float *transforms, size_t H, double max_range,
                                 uint32_t *counts_out, double *sums_out)
{
    PrejClouds c;
    int rc = prerej_views(ctx, source, target, c);
    if (rc) return rc;
    if (!(max_range >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_range must not be negative or NaN");
    if (H > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "too many transforms");
    if (!H) return RSREG_OK;
    if (!transforms) return fail(ctx, RSREG_ERR_INVALID_ARG, "transforms are needed");
    if (!c.ns) {
        if (counts_out) std::memset(counts_out, 0, H * 4);
        if (sums_out) std::memset(sums_out, 0, H * 8);
        return RSREG_OK;
    }
    rc = prerej_index(ctx, c);
    if (rc) return rc;
    PrerejScratch &sc = ctx->prerej;
    hipStream_t st = ctx->stream;
    const float limit2 = prerej_thr_up(max_range * max_range);
    const uint32_t R = (uint32_t)std::min<size_t>(H, kPrejRound);
    rc = prerej_reserve(ctx, c.ns, R);
    if (rc) return rc;
    for (size_t r0 = 0; r0 < H; r0 += R) {
        const uint32_t n = (uint32_t)std::min<size_t>(R, H - r0);
        float *rows = sc.host.as<float>();
        for (size_t h = 0; h < n; ++h)   // column-major 4 x 4 -> the three rows the kernels read
            for (int r = 0; r < 3; ++r)
                for (int col = 0; col < 4; ++col) rows[h * 12 + r * 4 + col] = transforms[(r0 + h) * 16 + col * 4 + r];
        RSREG_HIP(ctx, hipMemcpyAsync(sc.d_table.ptr, rows, (size_t)n * 48, hipMemcpyHostToDevice, st));
        for (uint32_t done = 0, B; (B = prerej_batch(c.ns, done, n)) != 0; done += B) {
            rc = prerej_score(ctx, c, done, B, false, limit2);
            if (rc) return rc;
        }
        if (counts_out) RSREG_HIP(ctx, hipMemcpyAsync(counts_out + r0, sc.d_counts.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (sums_out) RSREG_HIP(ctx, hipMemcpyAsync(sums_out + r0, sc.d_sums.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));   // (the staging rows are free again)
    }
    return RSREG_OK;
}

int rsreg_cloud_prerejective(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const int32_t *neighbor_index, int k,
                             const rsreg_prerej_params *params, int32_t *inliers_out, size_t capacity, size_t *n_out, rsreg_prerej_result *result)
{
    PrejClouds c;
    int rc = prerej_views(ctx, source, target, c);
    if (rc) return rc;
    if (!n_out || (capacity && !inliers_out)) return fail(ctx, RSREG_ERR_INVALID_ARG, "n_out, and inliers_out with a capacity, are needed");
    rsreg_prerej_params prm;
    if (params) prm = *params; else rsreg_prerej_params_default(&prm);
    if (prm.max_iterations < 0) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_iterations must not be negative");
    if (!(prm.similarity_threshold >= 0.0f && prm.similarity_threshold < 1.0f)) return fail(ctx, RSREG_ERR_INVALID_ARG, "similarity_threshold must lie in [0, 1)");
    if (!(prm.max_correspondence_distance >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_correspondence_distance must not be negative or NaN");
    if (!(prm.inlier_fraction >= 0.0 && prm.inlier_fraction <= 1.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "inlier_fraction must lie in [0, 1]");
    rc = prerej_table_check(ctx, neighbor_index, k, c.ns, c.nt);
    if (rc) return rc;

    rsreg_prerej_result res;
    std::memset(&res, 0, sizeof res);
    const Mat4f eye = Mat4f::identity();
    std::memcpy(res.transform, eye.m, sizeof eye.m);
    res.best_hypothesis = -1;
    for (int i = 0; i < 3; ++i) res.sample[i] = res.match[i] = -1;
    *n_out = 0;
    const uint32_t max_it = (uint32_t)prm.max_iterations;
    if (!c.ns || !c.nt || !max_it) {
        if (result) *result = res;
        return RSREG_OK;
    }

    PrerejScratch &sc = ctx->prerej;
    hipStream_t st = ctx->stream;
    rc = prerej_index(ctx, c);
    if (rc) return rc;
    const float limit2 = prerej_thr_up(prm.max_correspondence_distance * prm.max_correspondence_distance);
    const float sim2 = prm.similarity_threshold * prm.similarity_threshold;   // (float32; the build keeps products and sums apart)
    const size_t nbr_bytes = (size_t)c.ns * (size_t)k * 4;
    RSREG_HIP(ctx, sc.d_nbr.reserve(nbr_bytes + 16));
    RSREG_HIP(ctx, hipMemcpyAsync(sc.d_nbr.ptr, neighbor_index, nbr_bytes, hipMemcpyHostToDevice, st));   // (pageable: the copy has left the caller's array on return)
    const uint32_t R = std::min(max_it, kPrejRound);
    rc = prerej_reserve(ctx, c.ns, R);
    if (rc) return rc;

    // ---- the hypotheses, a round at a time, and the selection replayed over their counts and sums in hypothesis order
    long long best_h = -1;
    uint32_t best_count = 0;
    double best_err = 0.0;
    float best_row[12];
    int32_t best_sample[8];
    uint64_t n_valid = 0;
    for (uint32_t r0 = 0; r0 < max_it; r0 += R) {
        const uint32_t n = std::min(R, max_it - r0);
        for (uint32_t done = 0, B; (B = prerej_batch(c.ns, done, n)) != 0; done += B) {
            k_prerej_hypotheses<<<div_up(B, 64u), 64, 0, st>>>(c.sv.rec, c.sv.stride, c.ns, c.tv.rec, c.tv.stride, sc.d_nbr.as<int32_t>(), (uint32_t)k,
                                                              (unsigned long long)prm.seed, (unsigned long long)r0 + done, B, sim2,
                                                              sc.d_table.as<float>() + (size_t)done * 12, sc.d_valid.as<uint32_t>() + done,
                                                              sc.d_sample.as<int32_t>() + (size_t)done * 8);
            RSREG_HIP(ctx, hipGetLastError());
            rc = prerej_score(ctx, c, done, B, true, limit2);
            if (rc) return rc;
        }
        // home: counts | valid | sums | samples | rows, each at a multiple of 8 bytes
        char *h = sc.host.as<char>();
        const size_t o_valid = (size_t)R * 4, o_sums = (size_t)R * 8, o_sample = (size_t)R * 16, o_rows = (size_t)R * 48;
        RSREG_HIP(ctx, hipMemcpyAsync(h, sc.d_counts.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_valid, sc.d_valid.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_sums, sc.d_sums.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_sample, sc.d_sample.ptr, (size_t)n * 32, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_rows, sc.d_table.ptr, (size_t)n * 48, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        const uint32_t *counts = reinterpret_cast<const uint32_t *>(h), *valid = reinterpret_cast<const uint32_t *>(h + o_valid);
        const double *sums = reinterpret_cast<const double *>(h + o_sums);
        for (uint32_t j = 0; j < n; ++j) {
            if (!valid[j]) continue;
            ++n_valid;
            if (counts[j] < 1 || !((double)counts[j] / (double)c.ns >= prm.inlier_fraction)) continue;
            const double err = sums[j] / (double)counts[j];
            const bool better = best_h < 0 ? true
                              : prm.select_by_inliers ? (counts[j] > best_count || (counts[j] == best_count && err < best_err))
                                                      : err < best_err;
            if (!better) continue;
            best_h = (long long)r0 + j;
            best_count = counts[j];
            best_err = err;
            std::memcpy(best_row, h + o_rows + (size_t)j * 48, 48);
            std::memcpy(best_sample, h + o_sample + (size_t)j * 32, 32);
        }
    }
    res.n_valid = n_valid;
    if (best_h < 0) {
        if (result) *result = res;
        return RSREG_OK;
    }
    Mat4f T = Mat4f::identity();
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) T(r, col) = best_row[r * 4 + col];
    res.found = 1;
    res.best_hypothesis = (int32_t)best_h;
    for (int i = 0; i < 3; ++i) {
        res.sample[i] = best_sample[i];
        res.match[i] = best_sample[3 + i];
    }
    std::memcpy(res.transform, T.m, sizeof T.m);
    res.n_inliers = best_count;
    res.fitness = best_err;

    // ---- the winner's inliers, in ascending record order
    const size_t room = capacity < c.ns ? capacity : c.ns;
    RSREG_HIP(ctx, sc.d_flags.reserve((size_t)c.ns * 4 + 16));
    RSREG_HIP(ctx, sc.d_pos.reserve((size_t)c.ns * 4 + 16));
    RSREG_HIP(ctx, sc.d_scan.reserve(oscan_scratch_bytes<uint32_t>(c.ns)));
    RSREG_HIP(ctx, sc.d_out.reserve(room * 4 + 16));
    RSREG_HIP(ctx, sc.d_word.reserve(64));
    k_prerej_flags<<<div_up(c.ns, (uint32_t)kPrejLanes), kPrejLanes, 0, st>>>(c.sv.rec, c.sv.stride, c.ns, to_mat34(T), grid_dev(sc.grid), limit2, sc.d_flags.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, oscan<uint32_t>(sc.d_flags.as<uint32_t>(), sc.d_pos.as<uint32_t>(), c.ns, 0u, sc.d_scan.ptr, st));
    k_prerej_emit<<<div_up(c.ns, (uint32_t)kPrejLanes), kPrejLanes, 0, st>>>(sc.d_flags.as<uint32_t>(), sc.d_pos.as<uint32_t>(), c.ns, (unsigned long long)room,
                                                                            sc.d_out.as<int32_t>(), sc.d_word.as<unsigned long long>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(sc.host.ptr, sc.d_word.ptr, 8, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    const size_t kept = (size_t)*sc.host.as<unsigned long long>(), take = kept < room ? kept : room;
    if (kept != best_count) return fail(ctx, RSREG_ERR_STATE, "the winner's inlier list and its count disagree");
    if (take) {
        RSREG_HIP(ctx, hipMemcpyAsync(inliers_out, sc.d_out.ptr, take * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
    }
    *n_out = kept;
    if (result) *result = res;
    return RSREG_OK;
}

}  // extern "C"
