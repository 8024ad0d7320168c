// scia.hip — pcl::SampleConsensusInitialAlignment on clouds resident in HBM (C ABI: include/rsreg.h, "pose from descriptor
// neighbours, scored by a robust error"): the third estimator of the pose stage of a feature-based pre-alignment, beside sac.hip and
// prerej.hip.  rsreg_cloud_error_transforms scores transforms the caller supplies, rsreg_cloud_initial_alignment_hypotheses runs the
// sampler and the fit alone, rsreg_cloud_initial_alignment generates the hypotheses from a table of descriptor neighbours (what
// rsreg_cloud_feature_knn wrote), scores EVERY valid one and replays PCL's selection on the host in hypothesis order.
//
// The target's index, the scratch (rsreg_ctx::prerej), the plan of a launch (prerej_plan.hpp) and the kernel that adds a launch's
// partial sums are prerej.hip's (cloud_ops.hpp); the sampler and the scoring kernel are scia_kernels.hpp's.  Everything runs on the
// context's stream; every buffer is reserved before the first launch of a call that reads it.
#include <cfloat>
#include <cmath>
#include <limits>

#include "records.hpp"
#include "cloud_ops.hpp"
#include "scia_kernels.hpp"

using namespace rsreg;

namespace {

constexpr size_t kSciaHomeBytes = 8 + 4 + 64 + 48;   // of a hypothesis on its way home: error, valid word, 16 sample words, 12 floats

// params (or the defaults) checked; thr = the float the squared distances are compared with
int scia_params_check(rsreg_ctx *ctx, const rsreg_scia_params *params, rsreg_scia_params &prm, float &thr)
{
    if (params) prm = *params; else rsreg_scia_params_default(&prm);
    thr = (float)prm.max_correspondence_distance;
    if (!(thr > 0.0f)) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_correspondence_distance must be above 0 as a float and not NaN");
    if (!(prm.min_sample_distance >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "min_sample_distance must not be negative or NaN");
    if (prm.nr_samples < 3 || prm.nr_samples > kSciaMaxSamples) return fail(ctx, RSREG_ERR_INVALID_ARG, "nr_samples must lie in 3 .. 8");
    if (prm.error_function != RSREG_SCIA_TRUNCATED && prm.error_function != RSREG_SCIA_HUBER) return fail(ctx, RSREG_ERR_INVALID_ARG, "unknown error_function");
    if (prm.max_iterations < 0) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_iterations must not be negative");
    return RSREG_OK;
}

// prerej_reserve, and room for a hypothesis's 16 sample words and for what a round sends home
int scia_reserve(rsreg_ctx *ctx, uint32_t ns, uint32_t R)
{
    int rc = prerej_reserve(ctx, ns, R);
    if (rc) return rc;
    PrerejScratch &sc = ctx->prerej;
    RSREG_HIP(ctx, sc.d_sample.reserve((size_t)R * 64 + 16));
    RSREG_HIP(ctx, sc.host.reserve((size_t)R * kSciaHomeBytes + 4096));
    return RSREG_OK;
}

// the table of descriptor neighbours on the device, queued
int scia_table_up(rsreg_ctx *ctx, const int32_t *neighbor_index, uint32_t ns, int k)
{
    PrerejScratch &sc = ctx->prerej;
    const size_t bytes = (size_t)ns * (size_t)k * 4;
    RSREG_HIP(ctx, sc.d_nbr.reserve(bytes + 16));
    RSREG_HIP(ctx, hipMemcpyAsync(sc.d_nbr.ptr, neighbor_index, bytes, hipMemcpyHostToDevice, ctx->stream));   // (pageable: the copy has left the caller's array on return)
    return RSREG_OK;
}

// hypotheses h0 .. h0 + B - 1 into the rows [at, at + B) of the round's table, queued
int scia_hypotheses(rsreg_ctx *ctx, const PrejClouds &c, int k, const rsreg_scia_params &prm, unsigned long long h0, uint32_t at, uint32_t B)
{
    PrerejScratch &sc = ctx->prerej;
    k_scia_hypotheses<<<div_up(B, 64u), 64, 0, ctx->stream>>>(c.sv.rec, c.sv.stride, c.ns, c.tv.rec, c.tv.stride, sc.d_nbr.as<int32_t>(), (uint32_t)k,
                                                             (unsigned long long)prm.seed, h0, B, prm.nr_samples, prm.min_sample_distance * prm.min_sample_distance,
                                                             sc.d_table.as<float>() + (size_t)at * 12, sc.d_valid.as<uint32_t>() + at,
                                                             sc.d_sample.as<int32_t>() + (size_t)at * 16);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// the rows [at, at + B) of the round's table scored into sc.d_sums + at (valid: sc.d_valid + at, or every row), queued
int scia_score(rsreg_ctx *ctx, const PrejClouds &c, uint32_t at, uint32_t B, bool use_valid, int fn, float thr)
{
    PrerejScratch &sc = ctx->prerej;
    hipStream_t st = ctx->stream;
    const PrejPlan p = prerej_plan(c.ns, B);
    const uint32_t *valid = use_valid ? sc.d_valid.as<uint32_t>() + at : nullptr;
    const float *table = sc.d_table.as<float>() + (size_t)at * 12;
    if (fn == RSREG_SCIA_HUBER)
        k_scia_score<kSciaHuber><<<p.tiles * p.slices, kPrejBlock, 0, st>>>(c.sv.rec, c.sv.stride, c.ns, table, valid, B, p.tiles, p.slice_chunks, grid_dev(sc.grid), thr,
                                                                           sc.d_partials.as<double>());
    else
        k_scia_score<kSciaTruncated><<<p.tiles * p.slices, kPrejBlock, 0, st>>>(c.sv.rec, c.sv.stride, c.ns, table, valid, B, p.tiles, p.slice_chunks, grid_dev(sc.grid), thr,
                                                                               sc.d_partials.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    return prerej_final(ctx, valid, B, p.tiles, sc.d_sums.as<double>() + at);
}

// column-major 4 x 4 -> the three rows the kernels read
void scia_rows(const float *t16, float *rows)
{
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) rows[r * 4 + col] = t16[col * 4 + r];
}

}  // namespace

extern "C" {

void rsreg_scia_params_default(rsreg_scia_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->max_correspondence_distance = std::sqrt(DBL_MAX);   // pcl::Registration's corr_dist_threshold_
    p->min_sample_distance = 0.0;
    p->nr_samples = 3;
    p->error_function = RSREG_SCIA_TRUNCATED;
    p->max_iterations = 10;                                // pcl::Registration's max_iterations_
    p->seed = 0;
}

int rsreg_cloud_error_transforms(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const float *transforms, size_t H, int error_function,
                                 double max_correspondence_distance, double *errors_out)
{
    PrejClouds c;
    int rc = prerej_views(ctx, source, target, c);
    if (rc) return rc;
    const float thr = (float)max_correspondence_distance;
    if (!(thr > 0.0f)) return fail(ctx, RSREG_ERR_INVALID_ARG, "max_correspondence_distance must be above 0 as a float and not NaN");
    if (error_function != RSREG_SCIA_TRUNCATED && error_function != RSREG_SCIA_HUBER) return fail(ctx, RSREG_ERR_INVALID_ARG, "unknown error_function");
    if (H > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "too many transforms");
    if (!H) return RSREG_OK;
    if (!transforms || !errors_out) return fail(ctx, RSREG_ERR_INVALID_ARG, "transforms and errors_out are needed");
    if (!c.ns) {
        std::memset(errors_out, 0, H * 8);
        return RSREG_OK;
    }
    rc = prerej_index(ctx, c);
    if (rc) return rc;
    PrerejScratch &sc = ctx->prerej;
    hipStream_t st = ctx->stream;
    const uint32_t R = (uint32_t)std::min<size_t>(H, kPrejRound);
    rc = scia_reserve(ctx, c.ns, R);
    if (rc) return rc;
    for (size_t r0 = 0; r0 < H; r0 += R) {
        const uint32_t n = (uint32_t)std::min<size_t>(R, H - r0);
        float *rows = sc.host.as<float>();
        for (size_t h = 0; h < n; ++h) scia_rows(transforms + (r0 + h) * 16, rows + h * 12);
        RSREG_HIP(ctx, hipMemcpyAsync(sc.d_table.ptr, rows, (size_t)n * 48, hipMemcpyHostToDevice, st));
        for (uint32_t done = 0, B; (B = prerej_batch(c.ns, done, n)) != 0; done += B) {
            rc = scia_score(ctx, c, done, B, false, error_function, thr);
            if (rc) return rc;
        }
        RSREG_HIP(ctx, hipMemcpyAsync(errors_out + r0, sc.d_sums.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));   // (the staging rows are free again)
    }
    return RSREG_OK;
}

int rsreg_cloud_initial_alignment_hypotheses(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const int32_t *neighbor_index, int k,
                                             const rsreg_scia_params *params, uint64_t first, size_t count, float *transforms_out, int32_t *valid_out,
                                             int32_t *samples_out)
{
    PrejClouds c;
    int rc = prerej_views(ctx, source, target, c);
    if (rc) return rc;
    rsreg_scia_params prm;
    float thr;
    rc = scia_params_check(ctx, params, prm, thr);
    if (rc) return rc;
    rc = prerej_table_check(ctx, neighbor_index, k, c.ns, c.nt);
    if (rc) return rc;
    if (count > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "too many hypotheses");
    if (!count) return RSREG_OK;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (!c.ns) {   // no record to draw: nothing is valid
        for (size_t j = 0; j < count; ++j) {
            if (transforms_out) std::fill(transforms_out + j * 16, transforms_out + j * 16 + 16, nan);
            if (valid_out) valid_out[j] = 0;
            if (samples_out) std::fill(samples_out + j * 16, samples_out + j * 16 + 16, -1);
        }
        return RSREG_OK;
    }
    PrerejScratch &sc = ctx->prerej;
    hipStream_t st = ctx->stream;
    const uint32_t R = (uint32_t)std::min<size_t>(count, kPrejRound);
    rc = scia_reserve(ctx, c.ns, R);
    if (rc) return rc;
    rc = scia_table_up(ctx, neighbor_index, c.ns, k);
    if (rc) return rc;
    for (size_t r0 = 0; r0 < count; r0 += R) {
        const uint32_t n = (uint32_t)std::min<size_t>(R, count - r0);
        rc = scia_hypotheses(ctx, c, k, prm, (unsigned long long)first + r0, 0, n);
        if (rc) return rc;
        char *h = sc.host.as<char>();
        const size_t o_sample = (size_t)R * 4, o_rows = o_sample + (size_t)R * 64;
        RSREG_HIP(ctx, hipMemcpyAsync(h, sc.d_valid.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_sample, sc.d_sample.ptr, (size_t)n * 64, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_rows, sc.d_table.ptr, (size_t)n * 48, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        const uint32_t *valid = reinterpret_cast<const uint32_t *>(h);
        const float *rows = reinterpret_cast<const float *>(h + o_rows);
        for (size_t j = 0; j < n; ++j) {
            if (valid_out) valid_out[r0 + j] = valid[j] ? 1 : 0;
            if (samples_out) std::memcpy(samples_out + (r0 + j) * 16, h + o_sample + j * 64, 64);
            if (!transforms_out) continue;
            float *t = transforms_out + (r0 + j) * 16;
            if (!valid[j]) { std::fill(t, t + 16, nan); continue; }
            for (int r = 0; r < 3; ++r)
                for (int col = 0; col < 4; ++col) t[col * 4 + r] = rows[j * 12 + r * 4 + col];
            t[3] = t[7] = t[11] = 0.0f;
            t[15] = 1.0f;
        }
    }
    return RSREG_OK;
}

int rsreg_cloud_initial_alignment(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const int32_t *neighbor_index, int k,
                                  const rsreg_scia_params *params, const float *guess, double *errors_out, rsreg_scia_result *result)
{
    PrejClouds c;
    int rc = prerej_views(ctx, source, target, c);
    if (rc) return rc;
    rsreg_scia_params prm;
    float thr;
    rc = scia_params_check(ctx, params, prm, thr);
    if (rc) return rc;
    rc = prerej_table_check(ctx, neighbor_index, k, c.ns, c.nt);
    if (rc) return rc;

    const double inf = std::numeric_limits<double>::infinity(), qnan = std::numeric_limits<double>::quiet_NaN();
    rsreg_scia_result res;
    std::memset(&res, 0, sizeof res);
    const Mat4f eye = Mat4f::identity();
    std::memcpy(res.transform, eye.m, sizeof eye.m);
    res.best_hypothesis = -1;
    for (int i = 0; i < kSciaMaxSamples; ++i) res.sample[i] = res.match[i] = -1;
    res.error = inf;
    const uint32_t max_it = (uint32_t)prm.max_iterations;
    if (errors_out)
        for (uint32_t h = 0; h < max_it; ++h) errors_out[h] = qnan;
    const uint32_t H = guess ? (max_it ? max_it - 1 : 0) : max_it;   // the guess spends an iteration
    if (!c.ns || (!guess && !H)) {
        if (result) *result = res;
        return RSREG_OK;
    }

    PrerejScratch &sc = ctx->prerej;
    hipStream_t st = ctx->stream;
    rc = prerej_index(ctx, c);
    if (rc) return rc;
    const uint32_t R = std::max(std::min(H, kPrejRound), 1u);
    rc = scia_reserve(ctx, c.ns, R);
    if (rc) return rc;
    rc = scia_table_up(ctx, neighbor_index, c.ns, k);
    if (rc) return rc;

    // ---- the selection's state: PCL's lowest_error, and whether anything holds it yet (PCL's i_iter != 0)
    bool held = false;
    double lowest = inf;
    if (guess) {   // row 0 of a one-row table
        scia_rows(guess, sc.host.as<float>());
        RSREG_HIP(ctx, hipMemcpyAsync(sc.d_table.ptr, sc.host.ptr, 48, hipMemcpyHostToDevice, st));
        rc = scia_score(ctx, c, 0, 1, false, prm.error_function, thr);
        if (rc) return rc;
        RSREG_HIP(ctx, hipMemcpyAsync(sc.host.as<char>() + 64, sc.d_sums.ptr, 8, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        const double e = *reinterpret_cast<const double *>(sc.host.as<char>() + 64);
        res.error = e;
        if (!std::isnan(e)) { held = true; lowest = e; }
        if (std::isfinite(e)) std::memcpy(res.transform, guess, sizeof res.transform);
    }

    // ---- the hypotheses, a round at a time, and the selection replayed over their errors in hypothesis order
    long long best_h = -1;
    float best_row[12];
    int32_t best_sample[16];
    uint64_t n_valid = 0;
    for (uint32_t r0 = 0; r0 < H; r0 += R) {
        const uint32_t n = std::min(R, H - r0);
        for (uint32_t done = 0, B; (B = prerej_batch(c.ns, done, n)) != 0; done += B) {
            rc = scia_hypotheses(ctx, c, k, prm, (unsigned long long)r0 + done, done, B);
            if (rc) return rc;
            rc = scia_score(ctx, c, done, B, true, prm.error_function, thr);
            if (rc) return rc;
        }
        // home: errors | valid | samples | rows, each at a multiple of 8 bytes
        char *h = sc.host.as<char>();
        const size_t o_valid = (size_t)R * 8, o_sample = o_valid + (size_t)R * 4 + ((size_t)R * 4) % 8, o_rows = o_sample + (size_t)R * 64;
        RSREG_HIP(ctx, hipMemcpyAsync(h, sc.d_sums.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_valid, sc.d_valid.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_sample, sc.d_sample.ptr, (size_t)n * 64, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipMemcpyAsync(h + o_rows, sc.d_table.ptr, (size_t)n * 48, hipMemcpyDeviceToHost, st));
        RSREG_HIP(ctx, hipStreamSynchronize(st));
        const double *errs = reinterpret_cast<const double *>(h);
        const uint32_t *valid = reinterpret_cast<const uint32_t *>(h + o_valid);
        for (uint32_t j = 0; j < n; ++j) {
            if (!valid[j]) continue;
            ++n_valid;
            const double e = errs[j];
            if (errors_out) errors_out[r0 + j] = e;
            if (held ? !(e < lowest) : std::isnan(e)) continue;
            held = true;
            lowest = e;
            best_h = (long long)r0 + j;
            std::memcpy(best_row, h + o_rows + (size_t)j * 48, 48);
            std::memcpy(best_sample, h + o_sample + (size_t)j * 64, 64);
        }
    }
    res.n_valid = n_valid;
    if (best_h >= 0) {
        Mat4f T = Mat4f::identity();
        for (int r = 0; r < 3; ++r)
            for (int col = 0; col < 4; ++col) T(r, col) = best_row[r * 4 + col];
        std::memcpy(res.transform, T.m, sizeof T.m);
        res.found = 1;
        res.best_hypothesis = (int32_t)best_h;
        for (int i = 0; i < kSciaMaxSamples; ++i) {
            res.sample[i] = best_sample[i];
            res.match[i] = best_sample[8 + i];
        }
        res.error = lowest;
    }
    if (result) *result = res;
    return RSREG_OK;
}

}  // extern "C"
