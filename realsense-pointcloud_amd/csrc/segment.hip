// segment.hip — the dominant plane of a cloud resident in HBM and the consumer of its indices (C ABI: include/rsreg.h, "plane
// segmentation"): pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE and SAC_RANSAC, and pcl::ExtractIndices.
// The step in front of EuclideanClusterExtraction: find the floor, take it out, cluster what is left.
//
// rsreg_cloud_plane_segment launches batches of hypotheses (plane_seg_plan.hpp: plane_batch) -- k_plane_hypotheses fills a table of
// models, k_plane_count scores all of them against all records -- and replays PCL's stopping rule, skip counter included, over the
// integer counts on the host, in hypothesis order (PlaneReplay).  The winner's inliers give ten double sums, the host turns them
// into the refined model (rsreg_plane_from_sums), and the inliers are selected again.  rsreg_cloud_plane_filter and
// rsreg_cloud_extract_indices end in the flag / scan / gather of the cloud filters (filters.hip: compact_into, organized_into).
// Everything runs on the context's stream with the scratch rsreg_ctx::pseg (the two filters: rsreg_ctx::filt too).
#include <cfloat>
#include <cmath>
#include <cstring>

#include "records.hpp"
#include "cloud_ops.hpp"
#include "oscan.hpp"
#include "plane_seg_kernels.hpp"

using namespace rsreg;

namespace {

// the least float >= t (t >= 0, not NaN): for a float f >= 0, f < plane_thr_up(t) is (double)f < t
float plane_thr_up(double t)
{
    float f = (float)t;   // round to nearest: at most one step off
    if ((double)f < t) f = std::nextafterf(f, INFINITY);
    return f;
}

int plane_params_check(rsreg_ctx *ctx, const rsreg_plane_params &p, PlaneAxis &axis)
{
    if (!(p.distance_threshold >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "distance_threshold must not be negative or NaN");
    if (!(p.probability > 0.0 && p.probability < 1.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "probability must lie strictly between 0 and 1");
    if (p.max_iterations < 0) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_iterations must not be negative");
    if (!(p.eps_angle >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "eps_angle must not be negative or NaN");
    if (!std::isfinite(p.axis[0]) || !std::isfinite(p.axis[1]) || !std::isfinite(p.axis[2])) return fail(ctx, RSREG_ERR_INVALID_ARG, "the axis must be finite");
    const bool on = p.eps_angle > 0.0 && (p.axis[0] != 0.0 || p.axis[1] != 0.0 || p.axis[2] != 0.0);
    axis = PlaneAxis{p.axis[0], p.axis[1], p.axis[2], on ? std::cos(p.eps_angle) : 0.0, on ? 1 : 0};
    return RSREG_OK;
}

// the models, samples and validity of the hypotheses h0 .. h0 + B - 1 into the scratch, queued
int plane_hypotheses(rsreg_ctx *ctx, const CloudView &v, const rsreg_plane_params &p, const PlaneAxis &axis, unsigned long long h0, uint32_t B)
{
    PlaneSegScratch &ps = ctx->pseg;
    RSREG_HIP(ctx, ps.d_table.reserve((size_t)B * 16 + 16));
    RSREG_HIP(ctx, ps.d_sample.reserve((size_t)B * 16 + 16));
    RSREG_HIP(ctx, ps.d_valid.reserve((size_t)B * 4 + 16));
    k_plane_hypotheses<<<div_up(B, 64u), 64, 0, ctx->stream>>>(v.rec, v.stride, (uint32_t)v.n, (unsigned long long)p.seed, h0, B, axis, ps.d_table.as<float4>(),
                                                              ps.d_sample.as<int32_t>(), ps.d_valid.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// d_counts[0 .. H) = the inliers of the H rows of d_table, queued (n >= 1, H >= 1)
int plane_count(rsreg_ctx *ctx, const CloudView &v, uint32_t H, float thr_up)
{
    PlaneSegScratch &ps = ctx->pseg;
    RSREG_HIP(ctx, ps.d_counts.reserve((size_t)H * 4 + 16));
    RSREG_HIP(ctx, hipMemsetAsync(ps.d_counts.ptr, 0, (size_t)H * 4, ctx->stream));
    const PlanePlan p = plane_plan((uint32_t)v.n, H);
    k_plane_count<<<p.tiles * p.slices, kPlaneBlock, 0, ctx->stream>>>(v.rec, v.stride, (uint32_t)v.n, ps.d_table.as<float4>(), H, p.tiles, p.slice_chunks, thr_up,
                                                                      ps.d_counts.as<uint32_t>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// flags = the inliers of the model (negative: the other records), queued
int plane_select(rsreg_ctx *ctx, const CloudView &v, const float m[4], float thr_up, int negative, uint32_t *flags)
{
    k_plane_flags<<<div_up((uint32_t)v.n, kPlaneLanes), kPlaneLanes, 0, ctx->stream>>>(v.rec, v.stride, (uint32_t)v.n, make_float4(m[0], m[1], m[2], m[3]), thr_up,
                                                                                      negative, flags);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// the ten sums over the flagged records relative to p0 = record i0, and p0 itself, home and waited for
int plane_sums(rsreg_ctx *ctx, const CloudView &v, const uint32_t *flags, uint32_t i0, double sums[RSREG_NUM_PLANE_SEG_SUMS], float p0[3])
{
    PlaneSegScratch &ps = ctx->pseg;
    hipStream_t st = ctx->stream;
    const uint32_t nb = div_up((uint32_t)v.n, (uint32_t)kPlaneSumTile);
    RSREG_HIP(ctx, ps.d_partials.reserve((size_t)nb * kPlaneSums * 8 + 16));
    RSREG_HIP(ctx, ps.d_sums.reserve(kPlaneSumsBytes));
    RSREG_HIP(ctx, ps.host.reserve(4096));
    k_plane_sums<<<nb, kPlaneSumTile, 0, st>>>(v.rec, v.stride, (uint32_t)v.n, flags, i0, ps.d_partials.as<double>(),
                                               reinterpret_cast<float *>(ps.d_sums.as<char>() + kPlaneSumsP0At));
    RSREG_HIP(ctx, hipGetLastError());
    k_plane_final<<<kPlaneSums, kPlaneFinalBlock, 0, st>>>(ps.d_partials.as<double>(), nb, ps.d_sums.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(ps.host.ptr, ps.d_sums.ptr, kPlaneSumsP0At + 12, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    std::memcpy(sums, ps.host.ptr, kPlaneSums * 8);
    std::memcpy(p0, ps.host.as<char>() + kPlaneSumsP0At, 12);
    return RSREG_OK;
}

// the host-only step of the refinement (include/rsreg.h): false, nothing written, when m < 3 or C is not finite
bool plane_from_sums(const double s[RSREG_NUM_PLANE_SEG_SUMS], const float p0[3], const float prior[4], float out[4])
{
    const double m = s[0];
    if (!(m >= 3.0)) return false;
    const double mean[3] = {s[1] / m, s[2] / m, s[3] / m};
    const double xx = s[4] / m - mean[0] * mean[0], xy = s[5] / m - mean[0] * mean[1], xz = s[6] / m - mean[0] * mean[2];
    const double yy = s[7] / m - mean[1] * mean[1], yz = s[8] / m - mean[1] * mean[2], zz = s[9] / m - mean[2] * mean[2];
    const double Cm[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
    for (double c : Cm)
        if (!std::isfinite(c)) return false;
    double ev[3], vec[9];
    eig_sym3(Cm, ev, vec);
    double nrm[3] = {vec[0], vec[3], vec[6]};   // the column of the smallest eigenvalue
    const double len = std::sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    for (double &c : nrm) c /= len;
    const double dot = (nrm[0] * (double)prior[0] + nrm[1] * (double)prior[1]) + nrm[2] * (double)prior[2];
    if (dot < 0.0)
        for (double &c : nrm) c = -c;
    const double q[3] = {(double)p0[0] + mean[0], (double)p0[1] + mean[1], (double)p0[2] + mean[2]};
    out[0] = (float)nrm[0];
    out[1] = (float)nrm[1];
    out[2] = (float)nrm[2];
    out[3] = (float)(-((nrm[0] * q[0] + nrm[1] * q[1]) + nrm[2] * q[2]));
    return true;
}

}  // namespace

extern "C" {

void rsreg_plane_params_default(rsreg_plane_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->distance_threshold = 0.0;
    p->probability = 0.99;
    p->max_iterations = 50;
    p->optimize_coefficients = 1;
}

int rsreg_plane_from_sums(const double sums[RSREG_NUM_PLANE_SEG_SUMS], const float p0[3], const float prior[4], float coeff_out[4])
{
    if (!sums || !p0 || !prior || !coeff_out) return RSREG_ERR_INVALID_ARG;
    float out[4];
    if (!plane_from_sums(sums, p0, prior, out)) return RSREG_ERR_INVALID_ARG;
    std::memcpy(coeff_out, out, sizeof out);
    return RSREG_OK;
}

int rsreg_cloud_plane_count(rsreg_ctx *ctx, const rsreg_cloud *in, const float *coeffs, size_t H, double threshold, uint32_t *counts_out)
{
    CloudView v;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    if (!(threshold >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the threshold must not be negative or NaN");
    if (H > kPlaneMaxHypotheses) return fail(ctx, RSREG_ERR_INVALID_ARG, "too many models");
    if (!H) return RSREG_OK;
    if (!coeffs || !counts_out) return fail(ctx, RSREG_ERR_INVALID_ARG, "coeffs and counts_out are needed");
    if (!v.n) {
        std::memset(counts_out, 0, H * 4);
        return RSREG_OK;
    }
    PlaneSegScratch &ps = ctx->pseg;
    hipStream_t st = ctx->stream;
    RSREG_HIP(ctx, hipStreamSynchronize(st));   // (the models of an earlier call may still be on their way out of the staging buffer)
    RSREG_HIP(ctx, ps.host.reserve(H * 16 + 4096));
    RSREG_HIP(ctx, ps.d_table.reserve(H * 16 + 16));
    std::memcpy(ps.host.ptr, coeffs, H * 16);
    RSREG_HIP(ctx, hipMemcpyAsync(ps.d_table.ptr, ps.host.ptr, H * 16, hipMemcpyHostToDevice, st));
    rc = plane_count(ctx, v, (uint32_t)H, plane_thr_up(threshold));
    if (rc) return rc;
    RSREG_HIP(ctx, hipMemcpyAsync(counts_out, ps.d_counts.ptr, H * 4, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    return RSREG_OK;
}

int rsreg_cloud_plane_hypotheses(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_plane_params *params, uint64_t h_first, size_t H, float *coeffs_out,
                                 int32_t *samples_out, int32_t *valid_out)
{
    CloudView v;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    rsreg_plane_params prm;
    if (params) prm = *params; else rsreg_plane_params_default(&prm);
    PlaneAxis axis;
    rc = plane_params_check(ctx, prm, axis);
    if (rc) return rc;
    if (H > kPlaneMaxHypotheses) return fail(ctx, RSREG_ERR_INVALID_ARG, "too many hypotheses");
    hipStream_t st = ctx->stream;
    PlaneSegScratch &ps = ctx->pseg;
    for (size_t done = 0; done < H;) {   // (a launch's worth at a time: the scratch stays the size of a batch)
        const uint32_t B = (uint32_t)std::min<size_t>(H - done, kPlaneMaxBatch);
        rc = plane_hypotheses(ctx, v, prm, axis, (unsigned long long)h_first + done, B);
        if (rc) return rc;
        if (coeffs_out) RSREG_HIP(ctx, hipMemcpyAsync(coeffs_out + 4 * done, ps.d_table.ptr, (size_t)B * 16, hipMemcpyDeviceToHost, st));
        if (samples_out) RSREG_HIP(ctx, hipMemcpyAsync(samples_out + 4 * done, ps.d_sample.ptr, (size_t)B * 16, hipMemcpyDeviceToHost, st));
        if (valid_out) RSREG_HIP(ctx, hipMemcpyAsync(valid_out + done, ps.d_valid.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        done += B;
    }
    return RSREG_OK;
}

int rsreg_cloud_plane_segment(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_plane_params *params, float coeff_out[4], int32_t *indices_out,
                              size_t capacity, size_t *n_inliers_out, rsreg_plane_result *result)
{
    CloudView v;
    int rc = cloud_view(ctx, in, nullptr, kXyzRule, v);
    if (rc) return rc;
    if (capacity && !indices_out) return fail(ctx, RSREG_ERR_INVALID_ARG, "indices_out is needed with a capacity");
    rsreg_plane_params prm;
    if (params) prm = *params; else rsreg_plane_params_default(&prm);
    PlaneAxis axis;
    rc = plane_params_check(ctx, prm, axis);
    if (rc) return rc;
    const float thr_up = plane_thr_up(prm.distance_threshold);
    const uint32_t n = (uint32_t)v.n;

    rsreg_plane_result res;
    std::memset(&res, 0, sizeof res);
    res.best_hypothesis = -1;
    res.sample[0] = res.sample[1] = res.sample[2] = -1;
    res.cos_eps = axis.cos_eps;
    float model[4] = {0.f, 0.f, 0.f, 0.f};   // (NO MODEL: zeros)

    PlaneSegScratch &ps = ctx->pseg;
    hipStream_t st = ctx->stream;
    // ---- the hypotheses, a batch at a time, and PCL's stopping rule replayed over their counts in hypothesis order
    PlaneReplay rp(v.n, prm.probability, (unsigned long long)prm.max_iterations);
    int32_t win_sample[3] = {-1, -1, -1};
    float win_model[4] = {0.f, 0.f, 0.f, 0.f};
    if (n >= 3) {
        RSREG_HIP(ctx, ps.host.reserve((size_t)kPlaneMaxBatch * kPlaneHostBatchWords * 4 + 4096));
        uint32_t scored = 0;
        while (rp.wants_more()) {
            const uint32_t B = plane_batch(scored, (uint32_t)prm.max_iterations);
            if (!B) break;
            rc = plane_hypotheses(ctx, v, prm, axis, scored, B);
            if (rc) return rc;
            rc = plane_count(ctx, v, B, thr_up);
            if (rc) return rc;
            uint32_t *h = ps.host.as<uint32_t>();
            RSREG_HIP(ctx, hipMemcpyAsync(h, ps.d_counts.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipMemcpyAsync(h + kPlaneHostValidAt * kPlaneMaxBatch, ps.d_valid.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipMemcpyAsync(h + kPlaneHostSampleAt * kPlaneMaxBatch, ps.d_sample.ptr, (size_t)B * 16, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipMemcpyAsync(h + kPlaneHostTableAt * kPlaneMaxBatch, ps.d_table.ptr, (size_t)B * 16, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipStreamSynchronize(st));
            const uint32_t *counts = h, *valid = h + kPlaneHostValidAt * kPlaneMaxBatch;
            const int32_t *sample = reinterpret_cast<const int32_t *>(h + kPlaneHostSampleAt * kPlaneMaxBatch);
            const float *rows = reinterpret_cast<const float *>(h + kPlaneHostTableAt * kPlaneMaxBatch);
            for (uint32_t j = 0; j < B && rp.wants_more(); ++j) {
                const long long before = rp.winner;
                rp.feed(valid[j] != 0u, counts[j]);
                if (rp.winner != before) {   // (the winner's model and sample are kept as they pass: no second launch for them)
                    std::memcpy(win_model, rows + 4 * j, sizeof win_model);
                    std::memcpy(win_sample, sample + 4 * j, sizeof win_sample);
                }
            }
            scored += B;
        }
    }
    res.iterations = (int32_t)rp.it;
    res.skipped = (int32_t)rp.skipped;
    size_t kept = 0;
    if (n >= 3 && rp.best >= 3) {
        res.found = 1;
        res.best_hypothesis = (int32_t)rp.winner;
        std::memcpy(model, win_model, sizeof model);
        std::memcpy(res.sample, win_sample, sizeof win_sample);
        std::memcpy(res.unrefined, model, sizeof model);
        // ---- its inliers (rp.best of them: the count that made it the winner); the refinement; the inliers again.  Nothing is
        // waited for but the sums: how many inliers the refined model has comes home with k_plane_emit's word
        RSREG_HIP(ctx, ps.d_flags.reserve(v.n * 4 + 16));
        uint32_t *flags = ps.d_flags.as<uint32_t>();
        rc = plane_select(ctx, v, model, thr_up, 0, flags);
        if (rc) return rc;
        if (prm.optimize_coefficients) {
            double sums[RSREG_NUM_PLANE_SEG_SUMS];
            float p0[3], refined[4];
            rc = plane_sums(ctx, v, flags, (uint32_t)res.sample[0], sums, p0);
            if (rc) return rc;
            std::memcpy(res.sums, sums, sizeof sums);
            if (plane_from_sums(sums, p0, model, refined)) {
                std::memcpy(model, refined, sizeof model);
                res.refined = 1;
                rc = plane_select(ctx, v, model, thr_up, 0, flags);
                if (rc) return rc;
            }
        }
        // ---- the inliers' indices, ascending
        const size_t room = capacity < v.n ? capacity : v.n;
        RSREG_HIP(ctx, ps.d_pos.reserve(v.n * 4 + 16));
        RSREG_HIP(ctx, ps.d_scan.reserve(oscan_scratch_bytes<uint32_t>(v.n)));
        RSREG_HIP(ctx, ps.d_out.reserve(room * 4 + 16));
        RSREG_HIP(ctx, oscan<uint32_t>(flags, ps.d_pos.as<uint32_t>(), v.n, 0u, ps.d_scan.ptr, st));
        RSREG_HIP(ctx, ps.d_word.reserve(8));
        unsigned long long *d_found = ps.d_word.as<unsigned long long>();
        k_plane_emit<<<div_up(n, kPlaneLanes), kPlaneLanes, 0, st>>>(flags, ps.d_pos.as<uint32_t>(), n, (unsigned long long)room, ps.d_out.as<int32_t>(), d_found);
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipMemcpyAsync(ps.host.ptr, d_found, 8, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        kept = (size_t)*ps.host.as<unsigned long long>();
        res.n_inliers = kept;
        const size_t take = kept < room ? kept : room;
        if (take) {
            RSREG_HIP(ctx, hipMemcpyAsync(indices_out, ps.d_out.ptr, take * 4, hipMemcpyDeviceToHost, st));
            RSREG_HIP(ctx, hipStreamSynchronize(st));
        }
    }
    if (coeff_out) std::memcpy(coeff_out, model, sizeof model);
    if (n_inliers_out) *n_inliers_out = kept;
    if (result) *result = res;
    return RSREG_OK;
}

int rsreg_cloud_plane_filter(rsreg_ctx *ctx, const rsreg_cloud *in, const float coeff[4], double threshold, int negative, int keep_organized, rsreg_cloud *out,
                             uint64_t *n_kept)
{
    CloudView v;
    if (!out || !coeff) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    if (!(threshold >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "the threshold must not be negative or NaN");
    FilterScratch &fs = ctx->filt;
    if (v.n) {
        RSREG_HIP(ctx, fs.d_flags.reserve(v.n * 4 + 16));
        rc = plane_select(ctx, v, coeff, plane_thr_up(threshold), negative ? 1 : 0, fs.d_flags.as<uint32_t>());
        if (rc) return rc;
    }
    uint32_t kept = 0;
    rc = keep_organized ? organized_into(ctx, v, out, &kept) : compact_into(ctx, v, out, v.is_dense, &kept);
    if (rc) return rc;
    if (n_kept) *n_kept = kept;
    return RSREG_OK;
}

int rsreg_cloud_extract_indices(rsreg_ctx *ctx, const rsreg_cloud *in, const int32_t *indices, size_t n_indices, int negative, rsreg_cloud *out,
                                uint64_t *n_kept)
{
    CloudView v;
    if (!out) return RSREG_ERR_INVALID_ARG;
    int rc = cloud_view(ctx, in, out, kXyzRule, v);
    if (rc) return rc;
    if (n_indices && !indices) return fail(ctx, RSREG_ERR_INVALID_ARG, "an index list is needed");
    if (n_indices > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "index list too large");
    for (size_t j = 0; j < n_indices; ++j)
        if (indices[j] < 0 || (size_t)indices[j] >= v.n) return fail(ctx, RSREG_ERR_INVALID_ARG, "an index names a record outside the cloud");
    PlaneSegScratch &ps = ctx->pseg;
    FilterScratch &fs = ctx->filt;
    hipStream_t st = ctx->stream;
    const uint32_t m = (uint32_t)n_indices;
    if (m) {
        RSREG_HIP(ctx, hipStreamSynchronize(st));   // (a list of an earlier call may still be on its way out of the staging buffer)
        RSREG_HIP(ctx, ps.host.reserve(n_indices * 4 + 4096));
        RSREG_HIP(ctx, ps.d_index.reserve(n_indices * 4 + 16));
        std::memcpy(ps.host.ptr, indices, n_indices * 4);
        RSREG_HIP(ctx, hipMemcpyAsync(ps.d_index.ptr, ps.host.ptr, n_indices * 4, hipMemcpyHostToDevice, st));
    }
    uint32_t kept = 0;
    if (negative) {
        if (v.n) {
            RSREG_HIP(ctx, fs.d_flags.reserve(v.n * 4 + 16));
            RSREG_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(fs.d_flags.ptr), 1, v.n, st));
            if (m) {
                k_extract_clear<<<div_up(m, kBlock), kBlock, 0, st>>>(ps.d_index.as<int32_t>(), m, fs.d_flags.as<uint32_t>());
                RSREG_HIP(ctx, hipGetLastError());
            }
        }
        rc = compact_into(ctx, v, out, v.is_dense, &kept);
        if (rc) return rc;
    } else {
        const unsigned long long words = (unsigned long long)m * (v.stride / 4);
        if (words > 0xffffff00ull * kBlock) return fail(ctx, RSREG_ERR_INVALID_ARG, "index list too large");
        if (m) {
            RSREG_HIP(ctx, fs.d_out.reserve(n_indices * v.stride + 16));
            k_extract_gather<<<(uint32_t)((words + kBlock - 1) / kBlock), kBlock, 0, st>>>(v.rec, v.stride, ps.d_index.as<int32_t>(), m, fs.d_out.as<char>());
            RSREG_HIP(ctx, hipGetLastError());
        }
        kept = m;
        rc = rsreg_cloud_adopt_(out, &fs.d_out, n_indices, v.stride, m, 1, v.is_dense);   // (in == out: the input has been consumed by now)
        if (rc) return rc;
        RSREG_HIP(ctx, hipStreamSynchronize(st));   // (every call of this section returns with the stream drained)
    }
    if (n_kept) *n_kept = kept;
    return RSREG_OK;
}

}  // extern "C"
