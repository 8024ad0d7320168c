// rsreg_ctx.hpp — the per-(device, stream) context behind the C ABI (include/rsreg.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <cmath>
#include <thread>
#include <vector>

#include "../../include/rsreg.h"
#include "host_linalg.hpp"
#include "tunables.hpp"
#include "owned.hpp"
#include "workers.hpp"
#include "tile_sched.hpp"

namespace rsreg {

// Buffers of dropped device clouds, kept for the clouds to come (cloud.hip).  `limit`: bytes kept at most
// (RSREG_CLOUD_POOL_MB, default 4096; 0 = every drop is a hipFree).
struct CloudPool {
    std::vector<DevBuf> slots;
    size_t held = 0;
    size_t limit = (size_t)tunables().cloud_pool_mb << 20;
};

// ---- The words of the small scratch buffers (uint32 words).  Kernels take plain pointers into them and index from there
// (stats[k], box[k]); the host spells every offset with these names.  A box is min xyz | max xyz (ordered uints) | finite
// count | a stamp or spare word.
constexpr uint32_t kBoxWords = 8;
constexpr uint32_t kBoxPartialGroups = 1024;   // k_bbox / k_source_plain leave one partial box per workgroup: so many at most
constexpr uint32_t kBoxPartialWords = kBoxPartialGroups * kBoxWords;
constexpr uint32_t kCounterWords = 16;         // the head of a device misc buffer: cleared by k_bbox_final, copied home by the brick / NDT builds
// d_misc (main stream, the caller's thread; voxel.hip uses the buffer for its own words between index builds)
constexpr uint32_t kMiscBoxMax = 3;                 // NDT's k_grid_box: maxima and count behind the three minima
constexpr uint32_t kMiscStats = 8;                  // [8, 12) an index build's counts: the kernels' stats[0 .. 3]
constexpr uint32_t kMiscMaxCell = kMiscStats + 2;   //   brick build: k_max_cell_count
constexpr uint32_t kMiscMaxCount = 20;              // RSREG_DIAG: k_dense_max_count
constexpr uint32_t kMiscWords = 64;
// d_smisc (the source load's: src.stream and the source worker, or the main stream for a plain load)
constexpr uint32_t kSmiscDistinct = 12;             // k_source_unique / k_source_plain: distinct points
constexpr uint32_t kSmiscPartials = 64;             // [64, 64 + 1024 * 8) the source's box partials
constexpr uint32_t kSmiscWords = kSmiscPartials + kBoxPartialWords;
// h_smisc (pinned).  Two threads write disjoint words: the source worker its box, the caller's thread the rest.
constexpr uint32_t kHsSrcBox = 0;                   // [0, 8)   k_bbox_final on src.stream: read by the source worker
constexpr uint32_t kHsDistinct = 32;                // [32]     k_source_unique / k_source_plain: read at the join (caller)
constexpr uint32_t kHsCounts = 40;                  // [40, 43) the target build's counts, k_cc_scan [0] [1], k_dense_compact / _scatter [0] [2] (caller)
constexpr uint32_t kHsCountWords = 3;
constexpr uint32_t kHsPlainBox = 48;                // [48, 56) k_source_plain's box and stamp: harvest_source_box (caller)
constexpr uint32_t kHsWords = 64;
// knn.d_box and filt.host (pinned), the cloud filters' (filters.hip): the word behind the box is where one launch leaves a
// flag or a count and where it lands at home
constexpr uint32_t kFiltWord = kBoxWords;
// d_sums and h_sums (pinned) hold so many doubles: room for an iteration's sums of every kind (k_final_reduce leaves them in one
// or the other: icp.hip, host_sums_target).
// the target's box borrows its scratch: the head of h_sums is where the box, or the head of d_misc, lands;
// d_comm holds the partials behind the 64 doubles of an allreduce
constexpr size_t kSumsDoubles = 64;
constexpr size_t kSumsBytes = kSumsDoubles * sizeof(double);
static_assert(RSREG_NUM_SUMS <= kSumsDoubles && RSREG_NUM_PLANE_SUMS <= kSumsDoubles && RSREG_NUM_GICP_SUMS <= kSumsDoubles,
              "d_sums / h_sums hold the sums of an ICP, a point-to-plane and a GICP iteration");
constexpr size_t kCommBytes = 64 * sizeof(double);
constexpr size_t kCommPartialsAt = kCommBytes;      // (bytes)
static_assert(kMiscBoxMax < kMiscStats && kMiscStats + 4 <= kCounterWords && kCounterWords <= kMiscMaxCount && kMiscMaxCount < kMiscWords, "d_misc");
static_assert(kSmiscDistinct < kCounterWords && kCounterWords <= kSmiscPartials, "d_smisc");
static_assert(kHsSrcBox + kBoxWords <= kHsDistinct && kHsDistinct < kHsCounts && kHsCounts + kHsCountWords <= kHsPlainBox &&
              kHsPlainBox + kBoxWords <= kHsWords, "h_smisc");
static_assert(kCounterWords * sizeof(uint32_t) <= kSumsBytes, "h_sums");

// Bounding box and number of the finite points of a cloud: what an index build or a source load starts from (one kernel
// pair and a round trip to the host).  A cloud handle keeps the box of its records as they are (cloud.hip: version), so a
// frame that was the source of one pair and is the target of the next is not measured twice.
// The order-preserving float <-> uint map the kernels keep float minima / maxima in (atomicMin / atomicMax on floats), both ways
RSREG_HD inline uint32_t float_ordered(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RSREG_HD inline float ordered_float(uint32_t u)
{
    const uint32_t v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    __builtin_memcpy(&f, &v, 4);
    return f;
}

struct CloudBox {
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    uint32_t nfin = 0;
    bool valid = false;
    // false: a box that CONTAINS the finite points without being measured on them (the transformed corners of a measured box,
    // a union with such a box).  Good enough for a target's index (the grid's origin and extent; the search is exact whatever
    // they are), not for a source's spatial order (its keys are quantised from the box: another box, another order of the sums)
    bool exact = true;
};

// a box around what `T` makes of everything inside `b` (eight corners, in double, widened by a margin far above the float
// rounding of the per-point transform): cloud.hip hands it to the output of a transform / an alignment
inline CloudBox transformed_box(const CloudBox &b, const float *T /* 4x4 column-major */)
{
    CloudBox o = b;
    if (!b.valid || b.nfin == 0) return o;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, big = 0;
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {(c & 1) ? b.mx[0] : b.mn[0], (c & 2) ? b.mx[1] : b.mn[1], (c & 4) ? b.mx[2] : b.mn[2]};
        for (int r = 0; r < 3; ++r) {
            const double v = (double)T[r] * p[0] + (double)T[4 + r] * p[1] + (double)T[8 + r] * p[2] + (double)T[12 + r];
            lo[r] = v < lo[r] ? v : lo[r];
            hi[r] = v > hi[r] ? v : hi[r];
            big = std::fabs(v) > big ? std::fabs(v) : big;
        }
    }
    const double margin = 1e-5 * big + 1e-6;   // (float rounding of R x + t is ~1e-7 of the coordinates' size)
    for (int r = 0; r < 3; ++r) {
        o.mn[r] = (float)(lo[r] - margin);
        o.mx[r] = (float)(hi[r] + margin);
        if (!(o.mn[r] == o.mn[r]) || !(o.mx[r] == o.mx[r]) || std::fabs(o.mn[r]) > 1e30f || std::fabs(o.mx[r]) > 1e30f) o.valid = false;   // (a transform that is not finite)
    }
    o.exact = false;
    return o;
}

inline CloudBox union_box(const CloudBox &a, const CloudBox &b)
{
    if (!a.valid || !b.valid) return CloudBox{};
    if (a.nfin == 0) return b;
    if (b.nfin == 0) return a;
    CloudBox o;
    for (int r = 0; r < 3; ++r) {
        o.mn[r] = a.mn[r] < b.mn[r] ? a.mn[r] : b.mn[r];
        o.mx[r] = a.mx[r] > b.mx[r] ? a.mx[r] : b.mx[r];
    }
    const unsigned long long nf = (unsigned long long)a.nfin + b.nfin;
    o.nfin = (uint32_t)nf;
    o.valid = nf < 0xfffffff0ull;
    o.exact = a.exact && b.exact;
    return o;
}

// Uniform-grid index over the target cloud, all device-resident (layout: DESIGN.md §3).
struct GridParams {
    float origin[3];
    float inv_cell;
    float cell;
    int dims[3];
    uint32_t table_mask;   // brick hash table has table_mask + 1 slots
    uint32_t n_points;     // unique finite target points in `sorted`
    uint32_t n_cells;      // occupied cells
    uint32_t n_bricks;     // occupied 4x4x4-cell bricks
    int max_ring;          // rings (cells) needed to cover the correspondence gate
    int dense;             // 1: dense cell-start table (d_dense), 0: brick hash (d_table + d_cellpos), 2: no index (scan_target)
    int xbits;             // dense: bits of the x position inside a cell in the sort key (16, or what a 32-bit key leaves)
    int table_sparse;      // dense: only the table entries of occupied cells (and the slot behind each) are valid
    int have_nbr;          // dense: the neighbourhood occupancy words are built (0: a counting build for a small source left them out, icp.hip)
    int unserved;          // 1: a grid the searches' float32 bounds do not hold on (icp_grid_plan.hpp: served) -- built, never searched
};
// dense == 2: so many source points at most -- one workgroup's lanes and LDS slots (icp_kernels.hpp: k_scan_*); cloud.hip
// picks that search by it
constexpr uint32_t kScanMaxSource = 64;

struct BrickEntry {          // 32 B, one hash-table slot
    unsigned long long key;  // packed brick coordinate, ~0 = empty
    unsigned long long mask; // occupancy of its 64 cells, bit = lz*16 + ly*4 + lx
    uint32_t base;           // id of its first occupied cell (cellpos index)
    uint32_t pad[3];
};

// Dense grid of cells over the finite points of a cloud: the index of the exact searches (pointgrid.hpp builds it).
// Cells are numbered either x fastest (a run of cells along x is ONE run of points: the k-NN walk of knn_kernels.hpp) or
// block-major, 4x4x4 cells a block with one occupancy word each (a block's 64 cell starts are contiguous: the nearest-point
// walk of fitness_kernels.hpp); which, and how fine the cells are, is the builder's policy.  An instance belongs to ONE
// consumer (the ICP target's fitness score, NDT's, the cloud filters) and shares no buffer with the alignment's index or
// with another instance.
struct PointGrid {
    bool built = false;
    float origin[3] = {0, 0, 0};
    float cell = 1, inv_cell = 1;
    int dims[3] = {0, 0, 0};       // cells per axis (0: nothing indexed)
    uint32_t n_points = 0;         // finite points of the cloud
    DevBuf d_pts;                  // float4 {x, y, z, the reader's tag}, cell by cell
    DevBuf d_start;                // uint32 per cell + 1: first point of each cell
    DevBuf d_count;                // uint32 per cell + 1: build scratch, all zero between builds
    DevBuf d_mask;                 // block-major only: uint64 per block, which of its 64 cells hold a point
    DevBuf d_scan;                 // the prefix sums' scratch
    DevBuf d_box;                  // the box / count of the finite points (ordered uints)
};

// Scratch of the cloud filters (filters.hip), per record of the cloud being filtered; not part of an index
struct FilterScratch {
    DevBuf d_dist;                 // float per record: its mean distance to its mean_k nearest neighbours
    DevBuf d_flags, d_pos;         // uint32 per record: keep flag, position among the kept
    DevBuf d_sums;                 // the threshold's two f64 sums
    DevBuf d_out;                  // the kept records (the normals), before the output cloud takes them
    DevBuf d_nn_idx, d_nn_d2;      // rsreg_cloud_knn, rsreg_cloud_fpfh: k original indices / k squared distances per record
    DevBuf d_spfh;                 // rsreg_cloud_spfh, rsreg_cloud_fpfh: 33 floats per record, the SPFH rows between the two passes
    PinnedBuf host;
};

// Scratch of the radius search (filters.hip, radius_kernels.hpp), per record of the cloud being searched; not part of an index
struct RadiusScratch {
    DevBuf d_keys[2], d_vals[2];   // uint32 per record, twice: (cell, record) pairs on their way through the stable sort that places the index
    DevBuf d_sort;                 // the sort's scratch block
    DevBuf d_count;                // uint32 per record: its neighbours within the radius (a search surface: per query)
    // a search surface (surface_kernels.hpp): the index holds the surface, the queries are another cloud
    DevBuf d_qkeys[2], d_qvals[2]; // uint32 per query, twice: (surface cell, query record) pairs on their way through the sort that orders the queries
    DevBuf d_mark;                 // uint32 per surface record: 1 if it is a neighbour of a query
    DevBuf d_need;                 // uint32 per indexed point: the marks in the order of the index, then their inclusive prefix sum
    DevBuf d_list;                 // uint32 per indexed point: the places in the index of the needed points
    // ISSKeypoint3D (iss_kernels.hpp), per record of the cloud
    DevBuf d_iss_eig, d_iss_sal;   // three f64 eigenvalues of the scatter, ascending; the f64 saliency (a caller's own: rsreg_cloud_iss_non_max)
    DevBuf d_iss_index;            // int32 per record: the keypoints' record indices, ascending
};

// Scratch of EuclideanClusterExtraction (filters.hip, cluster_kernels.hpp), per record of the cloud being clustered; the two sorts of the
// ranking go through RadiusScratch's pairs and sort block, free again once the index is placed
struct ClusterScratch {
    DevBuf d_parent;               // uint32 per record: the union-find's forest while the hooks run
    DevBuf d_root, d_size;         // uint32 per record: the smallest record of its component (kClusterNone: non-finite); at a root, the component's records
    DevBuf d_rank;                 // uint32 per record: at the root of a cluster, its rank; kClusterNone elsewhere
    DevBuf d_label;                // int32 per record: the rank of its cluster, -1 without one
    DevBuf d_offsets;              // uint32 per record + 1: the clusters' sizes by rank, then their exclusive prefix sum
    DevBuf d_scan;                 // the prefix sum's scratch
    DevBuf d_n;                    // one word: the number of clusters
    PinnedBuf host;                // where the count, the offsets and the indices land before the caller's share is copied out
};

// Scratch of feature matching (features.hip, feature_kernels.hpp), per row of the two descriptor clouds of a call; not part of an index
struct FeatureScratch {
    DevBuf d_valid[2];             // uint32 per row: all 33 floats finite; [0] the source's rows, [1] the target's (source == target: [1] alone)
    DevBuf d_keys[2];              // uint64 per row, (d2 bits << 32 | index): [0] every source row's nearest target row, [1] every target row's nearest source row
    DevBuf d_part;                 // k > 1: the K keys every (target slice, source row) leaves for the merge
    DevBuf d_idx, d_d2;            // rsreg_cloud_feature_knn: k indices / k squared distances per source row, before they go home
    DevBuf d_flags, d_pos, d_scan; // correspondences: keep flag per source row, its position among the kept, the prefix sum's scratch
    DevBuf d_out;                  // the 12-byte correspondences, before they go home
    DevBuf d_count;                // 16 bytes: valid rows of the source, of the target (uint32 each); correspondences found (uint64)
    PinnedBuf host;                // where the target's count, or the number found, lands
};

// Scratch of RANSAC over a correspondence list (sac.hip, sac_kernels.hpp), per pair of the list and per hypothesis of a launch; not part of an index
struct SacScratch {
    PinnedBuf h_corr;              // the caller's 12-byte correspondences, staged for the link ...
    DevBuf d_corr;                 // ... and in HBM
    DevBuf d_planes;               // float, six planes of (pairs rounded up to whole tiles): source x y z, target x y z; NaN where a pair is not finite
    DevBuf d_table;                // 12 floats per hypothesis of a launch: the rows of its transform
    DevBuf d_sample;               // 4 int32 per hypothesis of a launch: its three pairs and the try that gave them
    DevBuf d_counts;               // uint32 per hypothesis of a launch: its inliers
    DevBuf d_flags[2];             // uint32 per pair: inlier under the current transform; the two take turns over the refit rounds
    DevBuf d_pos, d_scan;          // the kept pairs' positions, the prefix sum's scratch
    DevBuf d_out;                  // the kept correspondences, before they go home
    DevBuf d_partials, d_sums;     // the 17 sums: a slab per workgroup, the totals
    DevBuf d_word;                 // 32 bytes: flags set, flags changed (uint32 each); correspondences kept (uint64 at byte 8)
    PinnedBuf host;                // counts, samples, rows, sums and words on their way home; a caller's transforms on their way out
};

// Scratch of the RANSAC plane segmentation and of ExtractIndices (segment.hip, plane_seg_kernels.hpp), per record of the cloud and per
// hypothesis of a launch; not part of an index.  rsreg_cloud_plane_filter and rsreg_cloud_extract_indices leave their keep flags in
// FilterScratch, where the filters' scan and gather read them.
struct PlaneSegScratch {
    DevBuf d_table;                // 4 floats per hypothesis of a launch: a, b, c, d (NaN: an invalid hypothesis)
    DevBuf d_sample;               // 4 int32 per hypothesis of a launch: its three records and the try that gave them
    DevBuf d_valid;                // uint32 per hypothesis of a launch: a good try that passed the axis test
    DevBuf d_counts;               // uint32 per hypothesis of a launch: its inliers
    DevBuf d_flags;                // uint32 per record: inlier under the current model
    DevBuf d_pos, d_scan;          // the inliers' positions, the prefix sum's scratch
    DevBuf d_out;                  // the inliers' record indices (int32), before they go home
    DevBuf d_partials, d_sums;     // the ten sums: a slab per workgroup; kPlaneSumsBytes: the totals, then p0's three floats
    DevBuf d_word;                 // the indices k_plane_emit found (uint64)
    DevBuf d_index;                // ExtractIndices: the caller's int32 indices in HBM
    PinnedBuf host;                // counts, samples, validity, rows, sums and words on their way home; a caller's models or indices on their way out
};
// d_sums of PlaneSegScratch: RSREG_NUM_PLANE_SEG_SUMS doubles, then (at byte kPlaneSumsP0At) the three floats of p0
constexpr size_t kPlaneSumsP0At = 10 * sizeof(double);
constexpr size_t kPlaneSumsBytes = kPlaneSumsP0At + 16;
// host of PlaneSegScratch while a batch comes home: counts at word 0, validity at word kPlaneMaxBatch (sac_plan.hpp's kSacMaxBatch),
// samples at word 2 * kPlaneMaxBatch (four a hypothesis), rows at word 6 * kPlaneMaxBatch (four a hypothesis)
constexpr uint32_t kPlaneHostValidAt = 1, kPlaneHostSampleAt = 2, kPlaneHostTableAt = 6, kPlaneHostBatchWords = 10;   // (in units of the largest batch)

// Index and scratch of SampleConsensusPrerejective (prerej.hip, prerej_kernels.hpp) and, a call at a time, of
// SampleConsensusInitialAlignment (scia.hip: 16 sample words a hypothesis, errors in d_sums): the target's point grid, rebuilt by every call,
// and what a round of hypotheses leaves; shares no buffer with another index or with the correspondence rejector
struct PrerejScratch {
    PointGrid grid;                // the target of the call, block-major (FitGridPolicy)
    DevBuf d_nbr;                  // int32, ns * k: the caller's table of descriptor neighbours
    DevBuf d_table;                // 12 floats per hypothesis of a round: the rows of its transform
    DevBuf d_valid;                // uint32 per hypothesis of a round: it has a transform
    DevBuf d_sample;               // 8 int32 per hypothesis of a round: its three source records, its three target records, two spare words
    DevBuf d_counts;               // uint32 per hypothesis of a round: its inliers
    DevBuf d_sums;                 // double per hypothesis of a round: the sum of its inliers' d2
    DevBuf d_partials;             // two doubles per (hypothesis of a launch, group of the source): the two waves' sums
    DevBuf d_flags, d_pos, d_scan; // the winner's inlier flag per source record, its position among the inliers, the prefix sum's scratch
    DevBuf d_out;                  // the winner's inliers (int32 record numbers), before they go home
    DevBuf d_word;                 // the number of inliers (uint64)
    PinnedBuf host;                // the box of the grid build; tables on their way out; counts, sums, flags, samples and rows on their way home
};

// Scratch of IntegralImageNormalEstimation (iinormals.hip), per pixel of the organized frame it is given
struct IinScratch {
    DevBuf d_dist0, d_dist1, d_dist2;   // float: the distance map as set up, after the forward pass, after the backward pass
    DevBuf d_grad;                      // 2 x float4: the horizontal and the vertical difference, .w = 1 where it is finite
    DevBuf d_rect;                      // uint8: the window size R, 0 = no window
    DevBuf d_out;                       // the pcl::Normal records, before the output cloud takes them
    PinnedBuf host;                     // the window sizes on their way to the caller
};

// Scratch of the capture step (depthcloud.hip): the depth and the colour image of one frame, in one piece
struct DepthScratch {
    PinnedBuf host;      // staged for the link ...
    DevBuf d_images;     // ... and in HBM, where the kernel reads them
    Event ev_up;         // behind the copy: the staging buffer is free again
};

// One normal per RECORD of the ICP target or source, in the caller's order (icp.hip: set_record_normals)
struct RecordNormals {
    bool have = false;
    DevBuf d;                  // float4 {nx, ny, nz, 0} per record
    DevBuf d_raw;              // packed normals of a host buffer as they came over the link (n x float3) ...
    PinnedBuf h;               // ... their staging buffer, on the upload stream like the clouds' own ...
    Event ev, ev_packed;       // ... the event behind its last copy, and: the main stream has read d_raw (made at first use)
};

// An ordered chain of correspondence rejectors (include/rsreg.h: rsreg_icp_set_rejectors); n == 0: none
struct RejectorChain {
    int n = 0;
    rsreg_rejector e[8];
    bool has(int kind) const
    {
        for (int i = 0; i < n; ++i)
            if (e[i].kind == kind) return true;
        return false;
    }
};

struct IcpState {
    rsreg_icp_params prm;
    RejectorChain chain;             // the context's chain as rsreg_icp_begin found it (GICP: none)
    bool chain_stats = false;        // d_rej_words holds the counts of this alignment's last search
    bool normals_restart_pending = false;   // d_src_nrm_cur = guess * src_nrm.d not done yet (a chain with the normal test)
    Mat4f final_t, t_inc;
    int iterations = 0, state = 0, converged = 0, similar = 0, active = 0;
    double prev_mse = 0, cur_mse = 0;
    uint64_t ncorr = 0;
    double sums_last[RSREG_NUM_SUMS] = {0};
    double plane_sums_last[RSREG_NUM_PLANE_SUMS] = {0};   // point-to-plane: the 32 sums of the last iteration
    double svd_v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // V of the previous Umeyama solve (warm start of the next)
    bool have_search = false;     // corr buffers hold the current iteration's search
    bool pending_transform = false;  // fused mode: t_inc not yet applied to d_cur
    bool restart_pending = false;    // d_cur = guess * d_src (and "no seeds") not done yet: ensure_restarted / launch_fused
    double ms_nn = 0, ms_reduce = 0, ms_transform = 0;
    int n_nn_launches = 0;
    int n_sched_launches = 0;      // ... of them launched from a tile schedule
    SchedRun sched;                // the tile schedule of the fused dense launches, as this alignment sees it (tile_sched.hpp)
    bool idle_after_sums = false;  // the caller's thread has waited for the main stream (the sums) and queued nothing since: rsreg_icp_end need not wait again
};

// A GICP alignment (rsreg_gicp_begin .. rsreg_gicp_end) on top of the ICP state above, which holds the transform, the search and
// the counters of the staged pipeline it runs on
struct GicpState {
    rsreg_gicp_params prm;
    int active = 0;
    bool have_search = false;      // d_gicp_m holds the Mahalanobis matrices of the current search
    int inner_evaluations = 0, rank_last = 0;
    double sums_last[RSREG_NUM_GICP_SUMS] = {0};
    int six = 0;                   // rsreg_gicp6d_begin: the search runs in (x, y, z, w L', w a', w b') over ctx->g6
    float lab_weight = 0;          // w
};

}  // namespace rsreg

// Every buffer, event and stream below releases itself (owned.hpp), and rsreg_ctx_destroy deletes the context only after
// the helper threads have stopped and every stream has been drained: the order of the members does not matter.  The main
// stream alone is a raw handle (it may be the caller's) and is destroyed last.
struct rsreg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool profiling = false;
    std::string last_error;
    std::mutex error_mutex;

    // ---- ICP target index
    bool have_target = false;
    rsreg::GridParams grid{};
    rsreg_grid_info grid_info{};
    double gate_built_for = 0;
    rsreg::DevBuf d_tgt_raw;      // packed xyz of the caller's target (n x float3)
    rsreg::DevBuf d_tgt_sorted;   // float4 {x,y,z,bits(orig index)}, cell-sorted, de-duplicated
    rsreg::DevBuf d_table;        // BrickEntry[table_mask+1]
    rsreg::DevBuf d_cellpos;      // uint32[n_cells+1]: first sorted point of each occupied cell
    rsreg::DevBuf d_dense;        // dense mode: uint32[(nx+2)(ny+2)(nz+2)+1] first sorted point of EVERY cell, followed by one uint32 per cell: occupancy of its 27-cell neighbourhood
    rsreg::DevBuf d_pos_of;       // dense mode: uint32 per target record, its position in d_tgt_sorted
    rsreg::DevBuf d_sched;        // tile schedule of the fused dense kernel, uint32 words: items (4 per tile) | wave costs (2) | done counters (1) | first-launch items (4): sched_layout
    rsreg::SchedKept sched;       // what the buffer was laid out for and the schedules kept in it (tile_sched.hpp)
    rsreg::DevBuf d_keys, d_keys_alt, d_vals, d_vals_alt, d_flags, d_scan, d_brick, d_tmp;
    rsreg::DevBuf d_misc;         // small: bbox, counters
    rsreg::DevBuf d_cnt;          // counting build (cellsort.hpp): points per table slot, all zero between builds
    rsreg::DevBuf d_arrived;      // ... and the records in arrival order, cell by cell
    void *cnt_zero_ptr = nullptr;
    size_t cnt_zero_cap = 0;
    bool cnt_flip = false;        // which of the two sets of per-span totals the next counting build fills
    bool cnt_dirty = false;       // a counting build is under way (or did not finish): the counts are not known to be zero
    // The two counts a counting build ends with (occupied cells, records in the sorted array) lie in pinned words; nothing the
    // searches do needs them on the host (they bound the record array by the number of finite points), so set_target does
    // not wait for the build: whoever wants the counts, or has just waited for the stream anyway, takes them over (icp.hip:
    // target_counts).
    bool counts_pending = false;
    size_t counts_total = 0, counts_n = 0;   // (table entries and input points of that build: for index_bytes)
    size_t n_target_raw = 0;
    rsreg::DevBuf d_scan_keys;           // no-index search (scan_target): one (distance, index) key per source point
    const char *scan_raw = nullptr;      // ... and the records the index is built from if an alignment needs it after all
    size_t scan_stride = 0;
    uint64_t tgt_cloud_id = 0, tgt_cloud_version = 0;   // the device cloud the ICP target index was built from (0: none)
    // point-to-plane ICP and the surface normal rejector: the target's normals per target RECORD in the caller's order (the
    // sorted target records carry that index); dropped by every rsreg_icp_set_target*
    rsreg::RecordNormals tgt_nrm;
    rsreg::DevBuf d_plane_partials;   // double[32][blocks] of k_plane_reduce (and of k_gicp_reduce)
    // GICP (rsreg_gicp_*): six doubles per source / target RECORD in the caller's order, dropped by the next rsreg_icp_set_source* /
    // rsreg_icp_set_target*; the Mahalanobis matrices of the last search, six doubles per distinct source point
    bool have_gicp_cs = false, have_gicp_ct = false;
    rsreg::DevBuf d_gicp_cs, d_gicp_ct, d_gicp_m;
    rsreg::GicpState gicp;
    // GICP6D (rsreg_gicp6d_*, nn6_kernels.hpp): one colour per source / target RECORD in the caller's order, float4 {L', a', b', 0},
    // dropped by the next rsreg_icp_set_source* / rsreg_icp_set_target*; the target's x, y, z per record as they were when its
    // colours were set (float4 {x, y, z, 0}; x = NaN for an exact 6-D copy of a record of lower index); the 6-D search's own index over them, built by the first rsreg_gicp6d_begin that
    // follows, with the indexed points' colours times w beside it; the working points' colours times w
    bool have_lab_s = false, have_lab_t = false, g6_built = false;
    rsreg::DevBuf d_lab_s, d_lab_t, d_t6_xyz, d_g6_col, d_src6_col;
    rsreg::PointGrid g6;
    rsreg::PinnedBuf h_g6;
    // the records the target's index was built from: the context's own copy of a host cloud (d_tgt_raw), else the caller's device
    // buffer -- read once more by rsreg_gicp_set_target_lab*, never after (nullptr: a cloud handle's buffer has changed hands since)
    const char *tgt_rec = nullptr;
    size_t tgt_rec_stride = 0;
    rsreg::DevBuf d_lab_tables;   // cloud.hip: the 256 + 4000 floats of the RGB -> L*a*b* tables (lab_kernels.hpp), uploaded at first use

    // ---- ICP source
    bool have_source = false;
    const struct rsreg_cloud *src_cloud = nullptr;   // set by rsreg_icp_set_source_cloud: where the aligned cloud's records come from
    uint64_t src_cloud_id = 0, src_cloud_version = 0;   // ... as it was then: a handle destroyed or rewritten since is refused (RSREG_ERR_STATE)
    size_t n_source = 0;          // source points handed in
    size_t n_work = 0;            // distinct source points the iteration works on (exact copies merged)
    // the source is loaded on a stream of its own (so that it runs beside the target's index build when the
    // caller sets the source first, as the reference does) and joined where the alignment begins
    struct SourceLane {
        rsreg::Stream stream;
        rsreg::Event ev_done, ev_main;   // the load is done; what the main stream held when the load was asked for
        hipError_t ensure() { return rsreg::ensure_lane(stream, {&ev_done, &ev_main}); }
    } src;
    bool src_pending = false;
    rsreg::DevBuf d_plain_ticket; // k_source_plain's ticket word (zero between launches)
    uint32_t plain_box_seq = 0, plain_box_counter = 0;   // the stamp the pending plain load leaves behind its box in h_smisc[48 .. 55] (0: none)
    bool src_plain = false;       // the pending load is k_source_plain on the MAIN stream (every record a query of its own): nothing to wait for at the join
    bool src_unmerged = false;    // a merged load taken apart again (rsreg_gicp_set_source_lab*): every record a working point of its own
    bool src_on_worker = false;   // ... and its launches are being queued by the context's worker thread right now
    std::unique_ptr<rsreg::SourceWorker> src_worker;   // (created with the first source load; RSREG_NO_WORKER=1: never, the load runs on the caller's thread)
    // everything of a pending source load has been queued on src.stream (so that src.ev_done is the event of THIS load)
    int source_enqueued() { return src_worker ? src_worker->wait() : 0; }
    rsreg::DevBuf d_skeys, d_skeys_alt, d_svals, d_sflags, d_sscan, d_stmp, d_smisc;   // its scratch (the target build has its own)
    rsreg::DevBuf d_shist;        // two sets of digit histograms of the source's sort, used in turn (k_source_keys_hist); the worker's
    bool shist_flip = false, shist_dirty = false;
    rsreg::PinnedBuf h_smisc;     // (the words of d_smisc / h_smisc: kSmisc*, kHs* above)
    rsreg::DevBuf d_src_all;      // float4 {x,y,z,valid} of every source point, spatially sorted
    rsreg::DevBuf d_uniq_of;      // uint32: sorted position -> distinct point id
    rsreg::DevBuf d_first;        // uint32[n_work+1]: first sorted position of each distinct point
    rsreg::DevBuf d_src_raw;      // packed xyz as handed in
    rsreg::DevBuf d_perm;         // uint32: spatially sorted position -> caller's index
    rsreg::DevBuf d_src;          // float4 {x,y,z,weight} of the distinct points, spatially sorted
    rsreg::DevBuf d_cur;          // float4 current (transformed) source
    rsreg::DevBuf d_corr_pos;     // int32: position in d_tgt_sorted, -1 = none
    rsreg::DevBuf d_corr_d2;      // float
    rsreg::DevBuf d_seed;         // int32: nearest target found in the previous iteration (-1 none)
    rsreg::DevBuf d_partials;     // double[blocks][17]
    rsreg::DevBuf d_sums;         // double[kSumsDoubles]: an iteration's 17, 32 plane or 32 GICP sums where a communicator exists (icp.hip: host_sums_target)
    rsreg::DevBuf d_icp_state;    // IcpDevState of the device-resident loop
    // optional correspondence filters (reciprocal correspondences, trimmed rejector)
    rsreg::DevBuf d_corr_w;       // uint32 per distinct source point: how many of its copies keep their match
    rsreg::DevBuf d_recip_pts;    // float4 per ORIGINAL source point: the current source in the caller's order
    rsreg_ctx *recip = nullptr;   // child context holding the index over the current source (reciprocal search)
    // the rejector chain (rsreg_icp_set_rejectors, rejector_kernels.hpp): it stays until replaced; an alignment works on the
    // copy rsreg_icp_begin took (icp.chain)
    rsreg::RejectorChain rejectors;
    rsreg::DevBuf d_rej_flags;    // uint32 per ORIGINAL source record (sorted position): in play behind the chain so far
    rsreg::DevBuf d_rej_words;    // kRejWords uint32: the counts in front of and behind every entry, the medians, the select's digit counts
    rsreg::DevBuf d_rej_table;    // one-to-one: one (d2, caller's index) key per position of the sorted target
    // the source's normals per source RECORD in the caller's order: as handed in, and as they stand now (turned by the guess
    // and every increment); dropped by every rsreg_icp_set_source*
    rsreg::RecordNormals src_nrm;
    rsreg::DevBuf d_src_nrm_cur;
    rsreg::PinnedBuf h_sums;      // pinned double[kSumsDoubles]
    // next_*: the box of the cloud about to be set, when its handle knows it (consumed by build_grid / load_source_queue);
    // last_*: what the last index build / source load started from (valid: computed or taken over)
    rsreg::CloudBox next_tgt_box, last_tgt_box, next_src_box, last_src_box;
    rsreg::CloudBox next_ndt_box, last_ndt_box;   // the same for the NDT target's grid (rsreg_ndt_set_target_cloud)

    rsreg::PinnedBuf h_stage;     // pinned staging for H2D / D2H of clouds
    // host clouds of rsreg_icp_set_source / _set_target: the upload stream, a staging buffer for each kind of cloud and the
    // event behind its last copy
    struct StageLane {
        rsreg::Stream stream;
        rsreg::Event ev_src, ev_tgt;
        rsreg::PinnedBuf h_src, h_tgt;
        hipError_t ensure() { return rsreg::ensure_lane(stream, {&ev_src, &ev_tgt}); }
    } h2d;
    rsreg_host_timing host_timing{};
    std::vector<rsreg::Event> ev_home;   // one per piece of an aligned cloud on its way to the host (rsreg_icp_end)
    rsreg::IcpState icp;

    // ---- ApproximateVoxelGrid on the device (voxel.hip)
    rsreg::DevBuf d_vox_in, d_vox_out, d_vox_cent;
    // rsreg_cloud_filter_async: scratch sets and streams of their own, so that the filters of the next frames (one wave
    // per long run, latency-bound: 0.4 ms for PCL's default 1 m leaf) run under the alignment of this one AND beside each
    // other; a set is used again in turn, behind the filter that used it last (same stream).  ev_side_gate lets a filter
    // start after what the main stream holds.  Round 6: TWO side workers (threads) -- a frame's extraction and filter are ~20
    // launches and two waits for counts, as long as the frame's two alignments on the caller's thread, and every other
    // frame waited for them; jobs that do not depend on each other alternate between the workers, a job whose input is the
    // output of a job still queued follows it on the same worker.  Worker w owns the sets w and w + 2 and uses them in turn.
    static constexpr int kSideWorkers = 2;
    static constexpr int kSideSets = 2 * kSideWorkers;
    struct SideSet {
        rsreg::Stream stream;
        rsreg::DevBuf out, keys, keys_alt, vals, vals_alt, flags, scan, cent, misc, tmp;
        rsreg::PinnedBuf host;
    } side_sets[kSideSets];
    int side_turn[kSideWorkers] = {0, 0};   // which of its two sets a worker's next job takes
    int side_rr = 0;                          // the worker of the next job that follows no other
    rsreg::Event ev_side_gate;
    std::unique_ptr<rsreg::TicketWorker> side_workers[kSideWorkers];   // (queue those jobs: rsreg_cloud_filter_async returns at once)

    // ---- NDT
    bool have_ndt_target = false;
    double ndt_resolution = 0;
    int ndt_centroid_mode = 0;              // 1: PCL's float running sum per voxel (rsreg_ndt_set_centroid_mode)
    int ndt_n_voxels = 0;
    uint64_t ndt_seq = 0;  // derivative passes launched; the final reduce stamps it into h_ndt
    rsreg::DevBuf d_ndt_vox;      // per voxel: 3 mean + 9 icov doubles + centroid float3 ...
    rsreg::DevBuf d_ndt_src, d_ndt_trans, d_ndt_partials, d_ndt_out;
    rsreg::DevBuf d_ndt_seg;      // first sorted point of every occupied leaf (NDT's own: d_cellpos belongs to the live ICP hash index)
    rsreg::Event ev_ndt[2];   // NDT's own event pair (the pool's indices belong to an ICP begin..end)
    std::vector<double> ndt_mean_cov_icov;   // 21 per voxel (host copy)
    std::vector<int> ndt_counts;
    std::vector<float> ndt_centroid;         // 3 per voxel
    rsreg::PinnedBuf h_ndt;
    rsreg::PinnedBuf h_ndt_build;   // the target build's transfers: the voxels' partial moments home, the finished table out (pageable copies cost a frame of the NDT-edge loop 0.1 ms)
    rsreg::DevBuf d_ndt_tgt;        // float4 (x, y, index, z) of every target record (fitness score: PCL scores NDT against its target POINTS)
    size_t ndt_tgt_n = 0;

    // ---- getFitnessScore (icp.hip: fitness_sums): valid after a completed alignment, until the next source / target change
    bool icp_fit_ok = false, ndt_fit_ok = false;
    rsreg::Mat4f icp_fit_t, ndt_fit_t;   // the final transforms of those alignments
    size_t ndt_fit_n = 0;                // records of the NDT source (d_ndt_src)
    rsreg::PointGrid fit_icp, fit_ndt;    // one index per target kind: neither touches the alignment's own index
    rsreg::DevBuf d_fit_d2, d_fit_partials, d_fit_sums;
    rsreg::PinnedBuf h_fit;

    // ---- device-resident clouds (cloud.hip)
    rsreg::CloudPool cloud_pool;
    std::vector<rsreg::Event> ev_copy;   // one per piece of a cloud download in flight
    // rsreg_cloud_upload_async: a copy stream, the event that lets it start only after what the main stream holds, two pinned
    // staging buffers used in turn and the event behind the last copy out of each
    struct UploadLane {
        rsreg::Stream stream;
        rsreg::Event ev_gate, ev[2];
        rsreg::PinnedBuf h[2];
        bool busy[2] = {false, false};   // (these two: the upload worker's, once it exists)
        int next = 0;
        std::unique_ptr<rsreg::TicketWorker> worker;
        hipError_t ensure() { return rsreg::ensure_lane(stream, {&ev_gate, &ev[0], &ev[1]}); }
    } up;
    // rsreg_cloud_download_async: a download stream, its gate, pinned staging buffers with an event each, the copy-out threads
    struct DownloadLane {
        static constexpr int kSlots = rsreg::DownloadWorker::kSlots;
        rsreg::Stream stream;
        rsreg::Event ev_gate, ev[kSlots];
        rsreg::PinnedBuf h[kSlots];
        int next = 0;
        std::unique_ptr<rsreg::DownloadWorker> worker;
        hipError_t ensure() { return rsreg::ensure_lane(stream, {&ev_gate, &ev[0], &ev[1], &ev[2], &ev[3]}); }
    } down;
    static_assert(DownloadLane::kSlots == 4, "DownloadLane::ensure names every slot's event");
    // rsreg_ctx_prepare: what a frame loop is about to need, made on a thread of its own while the caller goes on; whoever is
    // about to create one of these lazily joins that thread first (prep_join) and finds them there
    std::thread prep_thread;
    rsreg::DevBuf prep_model;     // a device buffer for the merged model, handed to the cloud pool at the join
    int prep_rc = 0;              // the first HIP error of that thread: reported (fail) by prep_join
    void prep_join();
    std::thread records_copy;     // rsreg_icp_align_records: the caller's source records on their way into aligned_out (joined by icp_end)

    // ---- RCCL
    void *comm = nullptr;         // ncclComm_t
    int rank = 0, nranks = 1;
    rsreg::DevBuf d_comm;

    // ---- profiling events
    std::vector<rsreg::Event> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<size_t, size_t>> ev_nn, ev_reduce, ev_transform, ev_allreduce;

    // ---- PassThrough / StatisticalOutlierRemoval (filters.hip): index and scratch of their own
    rsreg::PointGrid knn;            // rebuilt by every k-NN call from the cloud it is given
    rsreg::FilterScratch filt;
    rsreg::RadiusScratch rad;        // radius search: it indexes in `knn` too, with a placement of its own
    rsreg::ClusterScratch clus;      // EuclideanClusterExtraction: over the radius index

    // ---- feature matching (features.hip): scratch of its own
    rsreg::FeatureScratch feat;

    // ---- pose from correspondences (sac.hip): scratch of its own
    rsreg::SacScratch sac;

    // ---- RANSAC plane segmentation and ExtractIndices (segment.hip): scratch of its own
    rsreg::PlaneSegScratch pseg;

    // ---- pose from descriptor neighbours, scored against the whole target (prerej.hip): index and scratch of its own
    rsreg::PrerejScratch prerej;

    // ---- IntegralImageNormalEstimation (iinormals.hip)
    rsreg::IinScratch iin;

    // ---- capture: depth + colour images -> cloud (depthcloud.hip)
    rsreg::DepthScratch depth;
};

namespace rsreg {

void cloud_pool_clear(rsreg_ctx *ctx);   // cloud.hip: frees the buffers kept in ctx->cloud_pool

// icp.hip: getFitnessScore's two numbers, sums[0] = records with a nearest target point at squared distance <= max_range,
// sums[1] = the sum of those squared distances, over the records src[0 .. n) (float4 {x, y, z, valid}) moved by T.  perm
// (nullable): record j is the caller's record perm[j] -- the sums run in the caller's order.  `fx` is built from the target
// records tgt[0 .. n_tgt) (x, y, index, z) if it is not built yet.  On ctx->stream; waits for it.
int fitness_sums(rsreg_ctx *ctx, PointGrid &fx, const float4 *tgt, size_t n_tgt, const float4 *src, const uint32_t *perm, size_t n,
                 const Mat4f &T, double max_range, double sums[2]);

inline int fail(rsreg_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx->error_mutex);   // (the context's source worker thread reports through here too)
        ctx->last_error = what;
        if (e != hipSuccess) {
            ctx->last_error += ": ";
            ctx->last_error += hipGetErrorString(e);
        }
    }
    return code;
}

// Host-side record loops (32-byte AoS records <-> packed xyz in pinned staging) are memory-bound
// copies of tens of MB: split over the process's pool of host threads (workers.hpp).  f(lo, hi) handles records [lo, hi).
template <typename F> inline void host_parallel_for(size_t n, F f)
{
    const size_t pieces = std::min<size_t>(n / 32768 + 1, 4 * (host_pool().th.size() + 1));
    const std::function<void(size_t, size_t)> fn = f;
    host_pool().run(n, pieces, fn);
}

// 32-byte (or any stride) AoS records -> packed xyz in the pinned staging buffer
inline int pack_to_stage(rsreg_ctx *ctx, const void *points, size_t n, size_t stride)
{
    hipError_t e = ctx->h_stage.reserve(n * 12 + 16);
    if (e != hipSuccess) return fail(ctx, RSREG_ERR_ALLOC, "pinned staging", e);
    float *dst = ctx->h_stage.as<float>();
    const char *src = static_cast<const char *>(points);
    host_parallel_for(n, [=](size_t lo, size_t hi) {
        if (stride == 12) {
            std::memcpy(dst + 3 * lo, src + 12 * lo, (hi - lo) * 12);
        } else {
            for (size_t i = lo; i < hi; ++i) std::memcpy(dst + 3 * i, src + i * stride, 12);
        }
    });
    return RSREG_OK;
}

#define RSREG_HIP(ctx, expr)                                              \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) return rsreg::fail((ctx), RSREG_ERR_HIP, #expr, _e); \
    } while (0)

}  // namespace rsreg
