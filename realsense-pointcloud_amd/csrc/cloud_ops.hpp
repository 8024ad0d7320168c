// cloud_ops.hpp — every function one translation unit defines for another, declared once: the users AND the definer include
// this header, so the compiler checks each definition against the declaration the callers see (most of these are extern "C":
// a prototype that drifted would still link).  Beside them the way in of an operation on device-resident clouds (CloudView,
// cloud_view).  The public ABI is include/rsreg.h; nothing here is exported to a caller of the library.
#pragma once

#include "rsreg_ctx.hpp"

struct rsreg_cloud;

extern "C" {

// cloud.hip: the context a handle belongs to (nullptr for a null handle)
const rsreg_ctx *rsreg_cloud_ctx_(const rsreg_cloud *c);
// cloud.hip: `c` takes a copy of the first n records of `buf`, queued on the context's stream (an upload or a download of `c`
// in flight is waited for first), and counts as rewritten; `buf` is the caller's again when the stream has run the copy
int rsreg_cloud_adopt_(rsreg_cloud *c, rsreg::DevBuf *buf, size_t n, size_t stride, uint32_t width, uint32_t height, int is_dense);
// cloud.hip: a kernel on the context's stream is about to write n records of `stride` bytes straight into `c`: what
// rsreg_cloud_upload does before its copy (*d_records: where they go) ...
int rsreg_cloud_begin_write_(rsreg_cloud *c, size_t n, size_t stride, void **d_records);
// ... and after it: `c` counts as rewritten and has this shape
int rsreg_cloud_end_write_(rsreg_cloud *c, size_t n, size_t stride, uint32_t width, uint32_t height, int is_dense);

// icp.hip: the ICP target without an index (GridParams::dense == 2), for at most kScanMaxSource source points: the records stay
// where they are and must stay unchanged until the next target is set
int rsreg_icp_set_target_scan_(rsreg_ctx *ctx, const void *d_points, size_t n, size_t stride, double max_correspondence_distance);
// icp.hip: the ICP target's normals from records in HBM whose first 12 bytes are the normal, one per target record, copied on
// the context's stream
int rsreg_icp_set_target_normals_device_(rsreg_ctx *ctx, const void *d_normals, size_t n, size_t stride);
int rsreg_icp_set_source_normals_device_(rsreg_ctx *ctx, const void *d_normals, size_t n, size_t stride);
// icp.hip: the GICP covariances of the ICP source (source != 0) or target from records in HBM whose first 48 bytes are six doubles
// (stride: a multiple of 8), one per record of that cloud, copied on the context's stream
int rsreg_gicp_set_covariances_device_(rsreg_ctx *ctx, int source, const void *d_cov, size_t n, size_t stride);
// icp.hip: the GICP6D colours of the ICP source (source != 0) or target from records in HBM whose first 12 bytes are L', a', b'
// (stride: a multiple of 4), one per record of that cloud, copied on the context's stream
int rsreg_gicp_set_lab_device_(rsreg_ctx *ctx, int source, const void *d_lab, size_t n, size_t stride);
// comm.cpp: the in-place sum over all ranks of `count` doubles in HBM, on the context's stream, not waited for; RSREG_ERR_STATE
// without a communicator
int rsreg_comm_allreduce_device_(rsreg_ctx *ctx, double *d_buf, int count);

}  // extern "C"

namespace rsreg {

// voxel.hip: ApproximateVoxelGrid on N records in HBM; the filtered records land in the scratch set's `out` (side_set >= 0: that
// set and its stream; -1: ctx->d_vox_out, the main stream), *n_out of them.  One host wait (the number of runs); the records
// themselves are only queued
int voxel_filter_device(rsreg_ctx *ctx, const char *d_in, uint32_t N, size_t stride, const float leaf[3], uint32_t *n_out, int side_set);
// edges.hip: the RGB-Canny edge points of an organized frame in HBM, into the same `out` of the same sets (their indices: the
// set's vals_alt), *n_out of them; waits for the stream
int edge_features_device(rsreg_ctx *ctx, const char *d_rec, size_t stride, uint32_t width, uint32_t height, uint32_t *n_out, int side_set);

// voxel.hip: the host-staged twins' way up -- n host records into ctx->d_vox_in through the pinned staging buffer, the copy
// queued on the context's stream (what reads d_vox_in there comes after it; `in` has been read when this returns) ...
int stage_up(rsreg_ctx *ctx, const void *in, size_t n, size_t stride);
// ... and their way down: the first n records of ctx->d_vox_out to `out`, waited for
int stage_down(rsreg_ctx *ctx, void *out, size_t n, size_t stride);

// ---- The way in of an operation on a device-resident cloud
struct CloudView {
    const char *rec = nullptr;   // the records in HBM, readable on the context's stream
    size_t n = 0, stride = 0;
    uint32_t width = 0, height = 0;
    int is_dense = 0;
};

// what an operation asks of its input's records
constexpr size_t kAnyCount = ~(size_t)0;
struct CloudRule {
    size_t min_stride;        // the bytes of a record the operation reads ...
    bool stride_mult4;        // ... and whether it reads them as words
    const char *bad_stride;   // the message when the stride breaks either
    size_t max_n;             // records at most (kAnyCount: the operation has a check of its own)
    const char *too_large;
};
// x, y, z floats, read word by word, counted in 31 bits: the cloud filters and the searches
constexpr CloudRule kXyzRule{12, true, "records need x, y, z floats and a stride that is a multiple of 4", 0x7ffffff0ull, "cloud too large"};

// cloud.hip: `in` (and `out`, if the operation has one) belong to `ctx`; a filter still queued INTO `in` has run
// (rsreg_cloud_info), its records keep the rule, the device is the context's, and an upload of `in` still in flight has arrived
// (rsreg_cloud_device_ptr) -- in this order.  RSREG_ERR_INVALID_ARG, with the rule's message where it has one; RSREG_ERR_STATE
// when the cloud holds records that cannot be reached (their upload failed).
int cloud_view(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *out_or_null, const CloudRule &rule, CloudView &view);

// ---- filters.hip, for segment.hip: the tail every cloud filter ends in.  ctx->filt.d_flags holds a keep flag (uint32, 0 or 1) per
// record of `v`, written on the context's stream.
// flags -> positions -> the kept records, handed to `out` (waits for their number); in == out is allowed
int compact_into(rsreg_ctx *ctx, const CloudView &v, rsreg_cloud *out, int is_dense, uint32_t *n_kept_out);
// keep_organized: every record, a removed one with x = y = z = quiet NaN, handed to `out` with the input's width and height
int organized_into(rsreg_ctx *ctx, const CloudView &v, rsreg_cloud *out, uint32_t *n_kept_out);

// ---- prerej.hip, for scia.hip: the two estimators that score poses against a whole target cloud share the context's PrerejScratch,
// the target's index and the kernel that adds a launch's partial sums
struct PrejClouds {
    CloudView sv, tv;
    uint32_t ns = 0, nt = 0;
};
// both clouds checked (kXyzRule); nothing is launched
int prerej_views(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, PrejClouds &c);
// the host table of descriptor neighbours: 1 <= k <= 16, a table where there are records, every entry -1 or a target record, no row -1 in part
int prerej_table_check(rsreg_ctx *ctx, const int32_t *neighbor_index, int k, uint32_t ns, uint32_t nt);
// the target's block-major point grid into ctx->prerej.grid, queued and (for its box) waited for
int prerej_index(rsreg_ctx *ctx, const PrejClouds &c);
// ctx->prerej's per-round buffers, for rounds of R hypotheses against ns source records
int prerej_reserve(rsreg_ctx *ctx, uint32_t ns, uint32_t R);
// k_prerej_final, queued: d_sums[h] = the partials a scoring launch left of its hypothesis h < B (d_valid null: of every one)
int prerej_final(rsreg_ctx *ctx, const uint32_t *d_valid, uint32_t B, uint32_t tiles, double *d_sums);

}  // namespace rsreg
