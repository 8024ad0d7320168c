// icp.hip — ICP half of the C ABI (include/rsreg.h): context, target grid build, the
// iteration loop of pcl::IterativeClosestPoint::computeTransformation, transformPointCloud.
//
// Reference call sites replaced: src/incremental_icp.hpp:46-49,57-63,
// src/icp_edge_based_registration.hpp:42-52,78-79,95,104,108-117,
// src/ndt_edge_based_registration.hpp:47-50,96-105.
#include <cstring>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <chrono>
#include <cstdlib>
#include <new>
#include <thread>
#include <vector>

#include "icp_kernels.hpp"
#include "icp_dense.hpp"
#include "cellsort.hpp"
#include "oscan.hpp"
#include "fitness_kernels.hpp"
#include "nn6_kernels.hpp"
#include "plane_kernels.hpp"
#include "rejector_kernels.hpp"
#include "gicp_kernels.hpp"
#include "cloud_ops.hpp"
#include "icp_grid_plan.hpp"

using namespace rsreg;

namespace {

inline uint32_t reduce_blocks(size_t n) { return (uint32_t)std::max<size_t>((n + kTile - 1) / kTile, 1); }  // depends on n only

hipEvent_t take_event(rsreg_ctx *ctx)
{
    if (ctx->ev_used == ctx->ev_pool.size()) {
        Event e;
        if (e.ensure(hipEventDefault) != hipSuccess) return nullptr;
        ctx->ev_pool.push_back(std::move(e));
    }
    return ctx->ev_pool[ctx->ev_used++];
}

struct ScopedEvents {  // records start/stop around a launch when profiling is on
    rsreg_ctx *ctx;
    std::vector<std::pair<size_t, size_t>> *list;
    size_t a = 0, b = 0;
    bool on;
    ScopedEvents(rsreg_ctx *c, std::vector<std::pair<size_t, size_t>> *l) : ctx(c), list(l), on(c->profiling)
    {
        if (!on) return;
        hipEvent_t e = take_event(ctx);
        a = ctx->ev_used - 1;
        if (e) (void)hipEventRecord(e, ctx->stream);
    }
    ~ScopedEvents()
    {
        if (!on) return;
        hipEvent_t e = take_event(ctx);
        b = ctx->ev_used - 1;
        if (e) (void)hipEventRecord(e, ctx->stream);
        list->push_back({a, b});
    }
};

double sum_events(rsreg_ctx *ctx, std::vector<std::pair<size_t, size_t>> &list)
{
    double ms = 0;
    for (auto &p : list) {
        float t = 0;
        if (hipEventElapsedTime(&t, ctx->ev_pool[p.first], ctx->ev_pool[p.second]) == hipSuccess) ms += t;
    }
    return ms;
}

float prune2_of(double max_dist)
{
    // squared search radius as a float that is never below the f64 gate PCL compares with
    const double gate2 = max_dist * max_dist;
    if (!(gate2 < (double)FLT_MAX)) return INFINITY;
    float f = (float)gate2;
    if ((double)f < gate2) f = std::nextafter(f, INFINITY);
    return f;
}

GridDev grid_dev(const rsreg_ctx *ctx, double max_dist)
{
    const GridParams &p = ctx->grid;
    GridDev g;
    g.ox = p.origin[0]; g.oy = p.origin[1]; g.oz = p.origin[2];
    g.inv_cell = p.inv_cell; g.cell = p.cell;
    g.dx = p.dims[0]; g.dy = p.dims[1]; g.dz = p.dims[2];
    g.bmask = p.table_mask;
    g.max_ring = p.max_ring;
    g.prune2 = prune2_of(max_dist);
    g.bricks = ctx->d_table.as<BrickEntry>();
    g.cellpos = ctx->d_cellpos.as<uint32_t>();
    g.pts = ctx->d_tgt_sorted.as<float4>();
    g.n_pts = p.dense ? 0u : p.n_points;   // (the brick hash's own count; a dense index is never searched through a GridDev)
    return g;
}

// bounding box + count of the finite points of a device-resident cloud (one host sync), on the given stream with
// the given scratch: d_misc (its kCounterWords are cleared), h_box (pinned, kBoxWords: the result), partial (kBoxPartialWords)
int device_bbox_on(rsreg_ctx *ctx, hipStream_t st, uint32_t *d_misc, uint32_t *h_box, uint32_t *partial, const char *d_pts, size_t n,
                   size_t stride, float mn[3], float mx[3], uint32_t *nfin)
{
    if (n == 0) {   // no kernel runs: the empty box
        for (int k = 0; k < 3; ++k) { mn[k] = ordered_float(0xffffffffu); mx[k] = ordered_float(0u); }
        *nfin = 0;
        return RSREG_OK;
    }
    const uint32_t nb = std::min<uint32_t>(div_up((uint32_t)n, kBlock), kBoxPartialGroups);
    k_bbox<<<nb, kBlock, 0, st>>>(d_pts, stride, (uint32_t)n, partial);
    RSREG_HIP(ctx, hipGetLastError());
    k_bbox_final<<<1, kBlock, 0, st>>>(partial, nb, h_box, d_misc);   // the box straight into the pinned host buffer (no copy queued); clears the counters
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    *nfin = h_box[6];
    for (int k = 0; k < 3; ++k) { mn[k] = ordered_float(h_box[k]); mx[k] = ordered_float(h_box[3 + k]); }
    return RSREG_OK;
}

// the scratch of the target's box (rsreg_ctx.hpp: the words of the small scratch buffers)
int reserve_box_scratch(rsreg_ctx *ctx)
{
    RSREG_HIP(ctx, ctx->d_misc.reserve(kMiscWords * sizeof(uint32_t)));
    RSREG_HIP(ctx, ctx->h_sums.reserve(kSumsBytes));
    RSREG_HIP(ctx, ctx->d_comm.reserve(kCommPartialsAt + kBoxPartialWords * sizeof(uint32_t)));
    return RSREG_OK;
}

int device_bbox(rsreg_ctx *ctx, const char *d_pts, size_t n, size_t stride, float mn[3], float mx[3], uint32_t *nfin)
{
    int rc = reserve_box_scratch(ctx);
    if (rc) return rc;
    return device_bbox_on(ctx, ctx->stream, ctx->d_misc.as<uint32_t>(), ctx->h_sums.as<uint32_t>(),
                          reinterpret_cast<uint32_t *>(ctx->d_comm.as<char>() + kCommPartialsAt), d_pts, n, stride, mn, mx, nfin);
}

// max_ring counts the rings that cover the gate (icp_grid_plan.hpp) -- unless that is the whole grid, where it says nothing about the
// gate.  True: the gate is at most max_ring cells.  The searches built for gates of at most four cells (the blocks search of the
// fused kernel, the sparse table) are chosen by max_ring <= 4 AND this: they carry no far path (icp_dense.hpp: nn_query_dense).
bool gate_in_rings(const GridParams &p) { return p.max_ring < std::max(p.dims[0], std::max(p.dims[1], p.dims[2])) + 1; }

DenseDev dense_dev(const rsreg_ctx *ctx, double max_dist)
{
    const GridParams &p = ctx->grid;
    DenseDev g;
    g.ox = p.origin[0]; g.oy = p.origin[1]; g.oz = p.origin[2];
    g.inv_cell = p.inv_cell; g.cell = p.cell;
    g.nx = p.dims[0]; g.ny = p.dims[1]; g.nz = p.dims[2];
    g.sx = p.dims[0] + 2;
    g.sxy = (p.dims[0] + 2) * (p.dims[1] + 2);
    g.max_ring = p.max_ring;
    g.prune2 = prune2_of(max_dist);
    g.start = ctx->d_dense.as<uint32_t>();
    g.pts = ctx->d_tgt_sorted.as<float4>();
    g.n_pts = p.n_points;
    g.table_bytes = (uint32_t)(((size_t)(p.dims[0] + 2) * (p.dims[1] + 2) * (p.dims[2] + 2) + 2) * 4);
    g.nbr = ctx->d_dense.as<uint32_t>() + g.table_bytes / 4;   // the occupancy words lie right behind the table (one memset clears both)
    g.pos_of = ctx->d_pos_of.as<uint32_t>();
#ifdef RSREG_DIAG   // (diagnostic builds only -- RSREG_CXXFLAGS=-DRSREG_DIAG: the shipped library has no switch that changes a result)
    g.debug_skip = tunables().debug_skip;
#endif
    // positions in cell units carry the rounding of (p - origin) * inv_cell, ~2^-23 of their size
    g.margin = std::min(kCellMargin, std::max(0.004f, 6.0e-7f * (float)std::max(p.dims[0], std::max(p.dims[1], p.dims[2]))));
    // how far the x order of a sorted run can be off: one bucket of the sort key (2^-xbits of a cell), plus the float
    // rounding of (x - ox) * inv_cell, which grows with the grid (ulp of the largest in-grid position)
    g.x_slack = p.cell * (std::ldexp(1.0f, -(p.xbits > 0 ? p.xbits : 16)) + 9.5367431640625e-7f * (float)std::max(p.dims[0], 1));
    return g;
}

// Dense-table index (icp_dense.hpp).  The grid geometry (ctx->grid) is already decided.
// KeyT: the sort key's type -- uint32_t when the cell id and at least 6 bits of x position fit 32 bits (build_dense).
template <typename KeyT>
int build_dense_keyed(rsreg_ctx *ctx, const char *d_pts, size_t n, size_t stride, double max_dist, uint32_t nfin, int id_bits)
{
    hipStream_t st = ctx->stream;
    GridParams &gp = ctx->grid;
    const size_t total = (size_t)(gp.dims[0] + 2) * (gp.dims[1] + 2) * (gp.dims[2] + 2);
    uint32_t *stats = ctx->d_misc.as<uint32_t>() + kMiscStats;
    uint32_t *h_stats = ctx->h_smisc.as<uint32_t>() + kHsCounts;   // (pinned words of the counts' own -- an alignment's sums land in h_sums)
    RSREG_HIP(ctx, ctx->d_keys.reserve(n * sizeof(KeyT)));
    RSREG_HIP(ctx, ctx->d_keys_alt.reserve(n * sizeof(KeyT)));
    const DenseDev g = dense_dev(ctx, max_dist);
    auto *keys = ctx->d_keys.as<KeyT>();
    auto *keys2 = ctx->d_keys_alt.as<KeyT>();
    auto *vals = ctx->d_vals.as<uint32_t>();
    auto *vals2 = ctx->d_vals_alt.as<uint32_t>();
    auto *flags = ctx->d_flags.as<unsigned long long>(), *scan = ctx->d_scan.as<unsigned long long>();   // keep | cstart << 32 and its scan
    uint32_t *cellslot = ctx->d_brick.as<uint32_t>(), *cellpos = ctx->d_cellpos.as<uint32_t>();
    uint32_t *table = ctx->d_dense.as<uint32_t>();
    const uint32_t xbits = (uint32_t)gp.xbits;
    // a table that is only read where an occupancy bit points is written by the scatter kernel, occupied cells only: no
    // clear, no scan of (nx+2)(ny+2)(nz+2) entries; the occupancy words behind it are OR-ed together and start from zero
    // (the occupancy words alone are cleared by the keys kernel on its way, unless that would be more than 64 words a thread)
    const bool occ_on_the_way = gp.table_sparse && (total + 2) <= 64ull * div_up((uint32_t)n, kBlock) * kBlock;
    if (!gp.table_sparse) RSREG_HIP(ctx, hipMemsetAsync(table, 0, (total + 2) * 4 * 2, st));
    else if (!occ_on_the_way) RSREG_HIP(ctx, hipMemsetAsync(table + (total + 2), 0, (total + 2) * 4, st));
    const unsigned end_bit = (unsigned)std::min<int>((int)sizeof(KeyT) * 8, (int)xbits + id_bits);
    // the library's own radix sort (osort.hpp; 32- and 64-bit keys alike since round 6), its state cleared by the keys kernel on
    // its way instead of by memsets
    const Radix32Plan plan = radix32_plan<KeyT>(n, 0, end_bit);
    // ... and then flag, scan and scatter are one launch too (compact.hpp), its look-back words cleared with the sort's state
    const bool scan_apart = tunables().scan_apart;
    const bool one_tail = !scan_apart && nfin < 0x7fffffffu;
    const CompactPlan cplan = compact_plan(nfin, plan.words);
    const uint32_t scratch_words = one_tail ? cplan.end : plan.words;
    const size_t sort_bytes = (size_t)scratch_words * 4;
    const size_t scan_bytes = oscan_scratch_bytes<unsigned long long>(nfin), tscan_bytes = oscan_scratch_bytes<uint32_t>(total + 1);
    // (the sort's state, then -- on the paths that scan apart -- the scans' sums behind it)
    const size_t off_scan = (sort_bytes + 255) & ~(size_t)255;
    RSREG_HIP(ctx, ctx->d_tmp.reserve(off_scan + std::max(scan_bytes, tscan_bytes) + 256));
    char *scan_scratch = ctx->d_tmp.as<char>() + off_scan;
    // (an even number of passes ends in the pair it started from: the keys are then written where the result belongs)
    const bool start_in_out = plan.ends_in_first;
    k_dense_keys<KeyT><<<div_up((uint32_t)n, kBlock), kBlock, 0, st>>>(d_pts, stride, (uint32_t)n, g, xbits, start_in_out ? keys2 : keys,
                                                                       start_in_out ? vals2 : vals, ctx->d_tmp.as<uint32_t>(), scratch_words,
                                                                       occ_on_the_way ? table + (total + 2) : nullptr,
                                                                       occ_on_the_way ? (uint32_t)(total + 2) : 0u);
    RSREG_HIP(ctx, hipGetLastError());
    {
        bool in_first = false;
        RSREG_HIP(ctx, radix32_sort_pairs<KeyT>(plan, ctx->d_tmp.as<uint32_t>(), start_in_out ? keys2 : keys, start_in_out ? keys : keys2,
                                                start_in_out ? vals2 : vals, start_in_out ? vals : vals2, n, 0, end_bit, st, &in_first));
        if (in_first != start_in_out) return fail(ctx, RSREG_ERR_STATE, "osort: the sorted pairs are not where they belong");
    }
    const uint32_t nbf = div_up(nfin, kBlock);
    if (one_tail) {
        uint32_t *scr = ctx->d_tmp.as<uint32_t>();
        k_dense_compact<KeyT><<<cplan.blocks, kCompactBlock, 0, st>>>(keys2, vals2, d_pts, stride, nfin, xbits, ctx->d_tgt_sorted.as<float4>(),
                                                                      ctx->d_pos_of.as<uint32_t>(), cellslot, cellpos, stats, h_stats,
                                                                      gp.table_sparse ? table : nullptr,
                                                                      reinterpret_cast<unsigned long long *>(scr + cplan.off_state), scr + cplan.off_ticket);
        RSREG_HIP(ctx, hipGetLastError());
    } else {
        k_dense_flag<KeyT><<<nbf, kBlock, 0, st>>>(keys2, vals2, d_pts, stride, nfin, xbits, flags);
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, (oscan<unsigned long long>(flags, scan, (size_t)nfin, 0ull, scan_scratch, st)));
        k_dense_scatter<KeyT><<<nbf, kBlock, 0, st>>>(keys2, vals2, d_pts, stride, nfin, xbits, flags, scan, ctx->d_tgt_sorted.as<float4>(),
                                                      ctx->d_pos_of.as<uint32_t>(), cellslot, cellpos, stats, h_stats,
                                                      gp.table_sparse ? table : nullptr);
        RSREG_HIP(ctx, hipGetLastError());
    }
    if (!gp.table_sparse) {
        k_dense_counts<<<nbf, kBlock, 0, st>>>(cellslot, cellpos, stats, table);
        RSREG_HIP(ctx, hipGetLastError());
        // counts -> first sorted point of every cell (in place), entry [total] = number of points
        RSREG_HIP(ctx, (oscan<uint32_t>(table, table, total + 1, 0u, scan_scratch, st)));
    }
    // occupancy word of every cell's 27-cell neighbourhood: a query never opens an empty cell
    k_dense_nbr<<<nbf, kBlock, 0, st>>>(cellslot, stats, g.sx, g.sxy, table + (total + 2));
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The same index by counting (cellsort.hpp): no sort, four launches + k_dense_nbr.  For grids a pass over all table
// entries is cheap for: at most 32 cells per point, or 16 M cells.  RSREG_COUNT_SORT=0: never.
bool count_sort_pays(size_t n, size_t total)
{
    return tunables().count_sort && total <= std::max<size_t>(32 * n, (size_t)16 << 20) && total < (1ull << 31);
}

// sources up to this many points (the one-launch load's default limit, tunables.hpp: plain_source_max) make their target's counting build leave
// the occupancy words out when the gate fits into ring 1
constexpr size_t kSmallSourceForTable = 65536;

int build_dense_counted(rsreg_ctx *ctx, const char *d_pts, size_t n, size_t stride, double max_dist, uint32_t nfin, bool with_nbr)
{
    hipStream_t st = ctx->stream;
    GridParams &gp = ctx->grid;
    const size_t total = (size_t)(gp.dims[0] + 2) * (gp.dims[1] + 2) * (gp.dims[2] + 2);
    uint32_t *h_counts = ctx->h_smisc.as<uint32_t>() + kHsCounts;   // pinned words of the counts' own
    // the counts are zero between builds (k_cc_scan puts them back); a new or larger buffer, or a build that did not
    // get to its end, starts from a memset
    RSREG_HIP(ctx, ctx->d_cnt.reserve((total + 16) * 4 + 2 * (size_t)kCcMaxSpans * 8));
    if (ctx->cnt_zero_ptr != ctx->d_cnt.ptr || ctx->cnt_zero_cap != ctx->d_cnt.cap || ctx->cnt_dirty) {
        RSREG_HIP(ctx, hipMemsetAsync(ctx->d_cnt.ptr, 0, ctx->d_cnt.cap, st));
        ctx->cnt_zero_ptr = ctx->d_cnt.ptr;
        ctx->cnt_zero_cap = ctx->d_cnt.cap;
    }
    ctx->cnt_dirty = true;
    RSREG_HIP(ctx, ctx->d_arrived.reserve(((size_t)nfin + 8) * sizeof(float4)));
    const DenseDev g = dense_dev(ctx, max_dist);
    uint32_t *cnt = ctx->d_cnt.as<uint32_t>() + 4u * kCcMaxSpans, *rank = ctx->d_vals.as<uint32_t>();   // (behind the two sets of per-span totals)
    uint32_t *cellslot = ctx->d_brick.as<uint32_t>(), *cellpos = ctx->d_cellpos.as<uint32_t>();
    uint32_t *table = ctx->d_dense.as<uint32_t>(), *occ = table + (total + 2);
    uint32_t *big = ctx->d_flags.as<uint32_t>();   // (n * 8 bytes: room for every cell beyond kCcSmall records)
    uint32_t *stats = ctx->d_misc.as<uint32_t>() + kMiscStats;
    // per-span totals of the counts (what k_cc_scan's workgroups start from): two sets used in turn, each cleared by the
    // counting kernel of the build before the one that fills it; they lie in front of the counts (zeroed with them)
    const uint32_t chunks = cc_span_chunks(total), spans = cc_spans(total), span = chunks * kCcChunk;
    auto *coarse_all = ctx->d_cnt.as<unsigned long long>();   // (at the head of the buffer, wherever the table ends)
    unsigned long long *coarse = coarse_all + (size_t)(ctx->cnt_flip ? kCcMaxSpans : 0), *coarse_next = coarse_all + (size_t)(ctx->cnt_flip ? 0 : kCcMaxSpans);
    ctx->cnt_flip = !ctx->cnt_flip;
    const uint32_t count_blocks = div_up((uint32_t)n, kCcTile);
    // the occupancy words are cleared by the counting kernel on its way, unless that would be more than 64 words a thread
    // (with_nbr false: an index without the words -- a small source's searches read them off the table, icp_dense.hpp:
    //  dense_occ_from_table; for a sparse cloud the words were half the build: 18 scattered atomics per occupied cell and a
    //  table's worth of zeroes)
    const bool occ_on_the_way = with_nbr && (total + 2) <= 64ull * count_blocks * kCcBlock;
    if (with_nbr && !occ_on_the_way) RSREG_HIP(ctx, hipMemsetAsync(occ, 0, (total + 2) * 4, st));
    k_cc_count<<<count_blocks, kCcBlock, 0, st>>>(d_pts, stride, (uint32_t)n, g, cnt, rank, coarse, span, occ_on_the_way ? occ : nullptr,
                                                   occ_on_the_way ? (uint32_t)(total + 2) : 0u, reinterpret_cast<uint32_t *>(coarse_next), 2u * kCcMaxSpans, stats);
    RSREG_HIP(ctx, hipGetLastError());
    k_cc_scan<<<spans, kCcScanBlock, 0, st>>>(cnt, (uint32_t)total, chunks, coarse, table, cellslot, cellpos, big, stats, h_counts);
    RSREG_HIP(ctx, hipGetLastError());
    const uint32_t nbf = div_up(nfin, kBlock), scatter_blocks = div_up((uint32_t)n, kBlock);
    // (one wave per crowded cell, the waves of the grid in turn; the grid covers every cell a cloud of nfin points can crowd)
    const uint32_t big_blocks = std::max(1u, std::min(div_up(nfin / (kCcSmall + 1u) + 1u, kBlock / 64), 2048u));
    // four dependent launches: scatter + occupancy words side by side (both need the scan only), then the in-cell order of the
    // small and of the crowded cells side by side
    if (with_nbr)
        k_cc_scatter_nbr<<<nbf + scatter_blocks, kBlock, 0, st>>>(d_pts, stride, (uint32_t)n, g, rank, table, ctx->d_arrived.as<float4>(), nbf, cellslot, stats, occ);
    else
        k_cc_scatter<<<scatter_blocks, kBlock, 0, st>>>(d_pts, stride, (uint32_t)n, g, rank, table, ctx->d_arrived.as<float4>());
    RSREG_HIP(ctx, hipGetLastError());
    k_cc_small_big<<<big_blocks + nbf, kBlock, 0, st>>>(ctx->d_arrived.as<float4>(), g, table, big, ctx->d_tgt_sorted.as<float4>(), ctx->d_pos_of.as<uint32_t>(), stats,
                                                        big_blocks);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The counts of a counting build that was queued and not waited for (build_dense): taken over from their pinned words once the
// stream has got there.  wait: wait for the stream first (somebody asks for the counts); false: the caller has just done so.
int target_counts(rsreg_ctx *ctx, bool wait)
{
    if (!ctx->counts_pending) return RSREG_OK;
    if (wait) RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->counts_pending = false;
    ctx->cnt_dirty = false;   // (k_cc_scan has put the counts back to zero)
    const uint32_t *h_counts = ctx->h_smisc.as<uint32_t>() + kHsCounts;
    GridParams &gp = ctx->grid;
    gp.n_cells = h_counts[0];
    gp.n_points = h_counts[1];
    rsreg_grid_info &gi = ctx->grid_info;
    gi.n_unique_points = gp.n_points;
    gi.n_cells = gp.n_cells;
    gi.index_bytes = (uint64_t)(gp.n_points + 4) * sizeof(float4) + (uint64_t)(ctx->counts_total + 1) * 2 * sizeof(uint32_t) + (uint64_t)ctx->counts_n * sizeof(uint32_t);
    return RSREG_OK;
}

int build_dense(rsreg_ctx *ctx, const char *d_pts, size_t n, size_t stride, double max_dist, uint32_t nfin, hipEvent_t ev0,
                hipEvent_t ev1)
{
    hipStream_t st = ctx->stream;
    GridParams &gp = ctx->grid;
    gp.dense = 1;
    const size_t total = (size_t)(gp.dims[0] + 2) * (gp.dims[1] + 2) * (gp.dims[2] + 2);
    RSREG_HIP(ctx, ctx->h_smisc.reserve(kHsWords * sizeof(uint32_t)));
    RSREG_HIP(ctx, ctx->d_vals.reserve(n * 4));
    RSREG_HIP(ctx, ctx->d_vals_alt.reserve(n * 4));
    RSREG_HIP(ctx, ctx->d_flags.reserve(n * 8));
    RSREG_HIP(ctx, ctx->d_scan.reserve(n * 8));
    RSREG_HIP(ctx, ctx->d_cellpos.reserve(((size_t)nfin + 2) * 4));
    RSREG_HIP(ctx, ctx->d_brick.reserve(((size_t)nfin + 2) * 4));
    RSREG_HIP(ctx, ctx->d_dense.reserve((total + 2) * 4 * 2));   // cell starts, then the neighbourhood occupancy words
    RSREG_HIP(ctx, ctx->d_tgt_sorted.reserve(((size_t)nfin + 8) * sizeof(float4)));
    RSREG_HIP(ctx, ctx->d_pos_of.reserve((n + 1) * 4));
    int id_bits = 1;
    while ((1ull << id_bits) <= total) ++id_bits;   // all-ones (non-finite) stays above every valid id
    const bool wide_keys = tunables().keys64, full_table = tunables().full_table;
    const bool narrow = !wide_keys && id_bits <= 26;   // at least 6 bits of x order inside a cell
    gp.xbits = narrow ? std::min(16, 32 - id_bits) : 16;
    // the searches of gates up to four cells go through the occupancy words only (icp_dense.hpp: dense_far_blocks);
    // the row search of wider or unbounded gates reads table entries of empty cells too and needs all of them
    // (... a gate of at most four cells, that is: max_ring of a grid of three cells a side is the whole grid, whatever the gate, and a
    //  far query's scan of every point reads the first and the last table entry -- icp_dense.hpp: nn_query_dense)
    gp.table_sparse = (gp.max_ring <= 4 && gate_in_rings(gp) && !full_table && !tunables().far_rows) ? 1 : 0;
    const uint32_t *h_counts = ctx->h_smisc.as<uint32_t>() + kHsCounts;
    const bool counted = count_sort_pays(n, total);
    if (counted) {
        gp.xbits = (int)kCcXBits;   // what the crowded cells are ordered by (g.x_slack follows)
        gp.table_sparse = 0;        // every table entry is written
        // a small source already loaded (the reference sets the source first: incremental_icp.hpp:57-58) and a gate inside
        // ring 1: no occupancy words -- every launch over this index then takes the instantiation that reads them off the table
        const bool small_source = ctx->have_source && ctx->n_source > 0 && ctx->n_source <= kSmallSourceForTable;
        gp.have_nbr = !(small_source && gp.max_ring <= 1 && tunables().nbr_from_table) ? 1 : 0;
        int rc = build_dense_counted(ctx, d_pts, n, stride, max_dist, nfin, gp.have_nbr != 0);
        if (rc) return rc;
        if (ctx->profiling) (void)hipEventRecord(ev1, st);
        // the build is queued, not waited for: the searches bound the record array by the number of finite points (the sorted
        // array holds at most that many, and the four far-away records behind its last one are inside the buffer either
        // way), and the two counts are taken over when somebody asks for them or has waited for the stream (target_counts)
        gp.n_cells = 0;
        gp.n_points = nfin;
        ctx->counts_pending = true;
        ctx->counts_total = total;
        ctx->counts_n = n;
        // ... unless the build's own time is wanted (profiling), or a source load is on its way on the context's other thread:
        // the caller's thread then has a wait in front of it anyway (join_source), and queueing the alignment's launches now
        // only gets in the way of the thread that is queueing the source's (measured: + 7 us per pair at 10^6 points)
        if (ctx->profiling || ctx->src_on_worker) {
            int rcc = target_counts(ctx, true);
            if (rcc) return rcc;
        }
    } else {
        gp.have_nbr = 1;
        int rc = narrow ? build_dense_keyed<uint32_t>(ctx, d_pts, n, stride, max_dist, nfin, id_bits)
                        : build_dense_keyed<unsigned long long>(ctx, d_pts, n, stride, max_dist, nfin, id_bits);
        if (rc) return rc;
        if (ctx->profiling) (void)hipEventRecord(ev1, st);
        RSREG_HIP(ctx, hipStreamSynchronize(st));   // (the scatter kernel left the two counts in pinned words of their own)
        gp.n_cells = h_counts[0];
        gp.n_points = h_counts[2];
    }
    gp.n_bricks = 0;
    rsreg_grid_info &gi = ctx->grid_info;
    for (int k = 0; k < 3; ++k) { gi.origin[k] = gp.origin[k]; gi.dims[k] = gp.dims[k]; }
    gi.cell_size = gp.cell;
    gi.n_unique_points = gp.n_points;   // (a counting build not yet waited for: the bound; target_counts puts the counts in)
    gi.n_cells = gp.n_cells;
    gi.max_points_per_cell = 0;   // dense mode: computed on demand by rsreg_icp_grid_info
    gi.index_kind = 1;
    gi.index_bytes = (uint64_t)(gp.n_points + 4) * sizeof(float4) + (uint64_t)(total + 1) * 2 * sizeof(uint32_t) + (uint64_t)n * sizeof(uint32_t);
    if (ctx->profiling) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) gi.ms_build = ms;
    }
    ctx->have_target = true;
    return RSREG_OK;
}

// Builds the grid from records already in HBM (d_pts/stride); keeps no pointer to them.
int build_grid(rsreg_ctx *ctx, const char *d_pts, size_t n, size_t stride, double max_dist, double refine = 1.0)
{
    hipStream_t st = ctx->stream;
    ctx->have_target = false;
    ctx->icp_fit_ok = false;   // (a new target: the fitness score waits for an alignment against it, and its index is rebuilt)
    ctx->fit_icp.built = false;
    ctx->counts_pending = false;   // (of a build nobody asked the counts of: this one's take their place; cnt_dirty stays as it is)
    ctx->tgt_cloud_id = 0;
    ctx->n_target_raw = n;
    std::memset(&ctx->grid_info, 0, sizeof(ctx->grid_info));
    std::memset(&ctx->grid, 0, sizeof(ctx->grid));
    ctx->gate_built_for = max_dist;
    ctx->tgt_rec = d_pts;   // (rsreg_gicp_set_target_lab* reads the records once more)
    ctx->tgt_rec_stride = stride;
    if (n > 0xfffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "target too large");

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (ctx->profiling) {
        ctx->ev_used = 0;
        ev0 = take_event(ctx);
        ev1 = take_event(ctx);
        (void)hipEventRecord(ev0, st);
    }
    float mn[3], mx[3];
    uint32_t nfin = 0;
    const rsreg::CloudBox known = ctx->next_tgt_box;   // (of the cloud handle this target comes from, if it has been measured before)
    ctx->next_tgt_box.valid = false;
    ctx->last_tgt_box.valid = false;
    const bool no_box_cache = !tunables().box_cache;
    if (known.valid && !no_box_cache && n > 0) {
        int rc = reserve_box_scratch(ctx);
        if (rc) return rc;
        for (int k = 0; k < 3; ++k) { mn[k] = known.mn[k]; mx[k] = known.mx[k]; }
        nfin = known.nfin;
    } else {
        int rc = device_bbox(ctx, d_pts, n, stride, mn, mx, &nfin);
        if (rc) return rc;
    }
    for (int k = 0; k < 3; ++k) { ctx->last_tgt_box.mn[k] = mn[k]; ctx->last_tgt_box.mx[k] = mx[k]; }
    ctx->last_tgt_box.nfin = nfin;
    ctx->last_tgt_box.valid = n > 0;
    ctx->last_tgt_box.exact = !(known.valid && !no_box_cache && n > 0) || known.exact;   // (measured just now, or what the handle knew)
    uint32_t *d_misc = ctx->d_misc.as<uint32_t>();
    uint32_t *h_misc = ctx->h_sums.as<uint32_t>();
    const size_t misc_bytes = kCounterWords * sizeof(uint32_t);
    ctx->grid_info.n_target_points = nfin;
    if (nfin == 0) {
        ctx->have_target = true;  // an empty index: every search comes back empty
        ctx->grid.cell = ctx->grid.inv_cell = 1.0f;
        RSREG_HIP(ctx, ctx->d_table.reserve(sizeof(BrickEntry)));
        RSREG_HIP(ctx, hipMemsetAsync(ctx->d_table.ptr, 0xff, sizeof(BrickEntry), st));
        RSREG_HIP(ctx, ctx->d_tgt_sorted.reserve(sizeof(float4)));
        RSREG_HIP(ctx, ctx->d_cellpos.reserve(16));
        return RSREG_OK;
    }

    // ---- the grid: cell, origin, dims, rings and the kind of index, decided by the host-only rule of icp_grid_plan.hpp.
    // `refine` (second pass only) shrinks the cells of a dense cloud towards ~8 points per occupied cell.
    static_assert(kIcpPlanMargin == kCellMargin, "icp_grid_plan.hpp counts the rings of a gate with the searches' margin");
    IcpGridInput plan_in;
    for (int k = 0; k < 3; ++k) { plan_in.mn[k] = mn[k]; plan_in.mx[k] = mx[k]; }
    plan_in.nfin = nfin;
    plan_in.max_dist = max_dist;
    plan_in.refine = refine;
    plan_in.cell_cap = tunables().cell_cap;
    plan_in.wide_cells = tunables().wide_cells;
    plan_in.dense_max_cells = tunables().dense_max_cells;
    const IcpGridPlan plan = icp_grid_plan(plan_in);
    GridParams &gp = ctx->grid;
    // a grid on which the searches' float32 bounds do not hold (a cell above 2^60 m, a box wider than a float) is built as before --
    // the target's box and records serve the fitness score, which has an index of its own -- and never searched (refuse_unserved)
    gp.unserved = plan.served ? 0 : 1;
    gp.cell = plan.cell;
    gp.inv_cell = plan.inv_cell;
    for (int k = 0; k < 3; ++k) { gp.origin[k] = plan.origin[k]; gp.dims[k] = plan.dims[k]; }
    gp.max_ring = plan.max_ring;
    if (plan.index_kind == 1) return build_dense(ctx, d_pts, n, stride, max_dist, nfin, ev0, ev1);

    // ---- sort by (brick, cell in brick, xyz hash)
    // (the brick path counts with atomics in the words k_bbox_final clears; the dense table's kernels only store there)
    if (known.valid && !no_box_cache && n > 0) RSREG_HIP(ctx, hipMemsetAsync(ctx->d_misc.ptr, 0, misc_bytes, st));
    RSREG_HIP(ctx, ctx->d_keys.reserve(n * 8));
    RSREG_HIP(ctx, ctx->d_keys_alt.reserve(n * 8));
    RSREG_HIP(ctx, ctx->d_vals.reserve(n * 4));
    RSREG_HIP(ctx, ctx->d_vals_alt.reserve(n * 4));
    RSREG_HIP(ctx, ctx->d_flags.reserve(n * 12));
    RSREG_HIP(ctx, ctx->d_scan.reserve(n * 12));
    RSREG_HIP(ctx, ctx->d_cellpos.reserve(((size_t)nfin + 2) * 4));
    RSREG_HIP(ctx, ctx->d_brick.reserve(((size_t)nfin + 2) * 20));
    RSREG_HIP(ctx, ctx->d_tgt_sorted.reserve(((size_t)nfin + 1) * sizeof(float4)));
    GridDev g = grid_dev(ctx, max_dist);
    const uint32_t nb = div_up((uint32_t)n, kBlock);
    auto *keys = ctx->d_keys.as<unsigned long long>();
    auto *keys2 = ctx->d_keys_alt.as<unsigned long long>();
    auto *vals = ctx->d_vals.as<uint32_t>();
    auto *vals2 = ctx->d_vals_alt.as<uint32_t>();
    k_cell_keys<<<nb, kBlock, 0, st>>>(d_pts, stride, (uint32_t)n, g, keys, vals);
    RSREG_HIP(ctx, hipGetLastError());
    // the library's own radix sort over all 64 key bits (osort.hpp), its state cleared by a memset in front; then three scans (oscan.hpp)
    uint32_t *keep = ctx->d_flags.as<uint32_t>(), *cstart = keep + n, *bstart = cstart + n;
    uint32_t *pos = ctx->d_scan.as<uint32_t>(), *cid = pos + n, *bid = cid + n;
    const size_t sort_bytes = (size_t)osort_plan<unsigned long long>(n, 0, 64).words * 4, scan_bytes = oscan_scratch_bytes<uint32_t>(nfin);
    RSREG_HIP(ctx, ctx->d_tmp.reserve(std::max(sort_bytes, scan_bytes) + 256));
    {
        bool in_first = false;
        RSREG_HIP(ctx, osort_pairs_cleared<unsigned long long>(ctx->d_tmp.as<uint32_t>(), keys, keys2, vals, vals2, n, 0, 64, st, &in_first));
        if (in_first) {   // (keys2 / vals2 below: the sorted pairs, wherever the passes have left them)
            std::swap(keys, keys2);
            std::swap(vals, vals2);
        }
    }
    const uint32_t nbf = div_up(nfin, kBlock);
    k_flag_runs<<<nbf, kBlock, 0, st>>>(keys2, vals2, d_pts, stride, nfin, keep, cstart, bstart);
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, (oscan<uint32_t>(keep, pos, (size_t)nfin, 0u, ctx->d_tmp.ptr, st)));
    RSREG_HIP(ctx, (oscan<uint32_t>(cstart, cid, (size_t)nfin, 0u, ctx->d_tmp.ptr, st)));
    RSREG_HIP(ctx, (oscan<uint32_t>(bstart, bid, (size_t)nfin, 0u, ctx->d_tmp.ptr, st)));
    // brick staging arrays: key[nfin+1] u64 | mask[nfin+1] u64 | base[nfin+1] u32
    auto *brickkey = ctx->d_brick.as<unsigned long long>();
    auto *brickmask = brickkey + (nfin + 1);
    auto *brickbase = reinterpret_cast<uint32_t *>(brickmask + (nfin + 1));
    RSREG_HIP(ctx, hipMemsetAsync(brickmask, 0, ((size_t)nfin + 1) * 8, st));
    k_scatter_sorted<<<nbf, kBlock, 0, st>>>(keys2, vals2, d_pts, stride, nfin, keep, cstart, bstart, pos, cid, bid,
                                             ctx->d_tgt_sorted.as<float4>(), ctx->d_cellpos.as<uint32_t>(), brickkey, brickmask,
                                             brickbase, d_misc + kMiscStats);
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(h_misc, d_misc, misc_bytes, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t *h_stats = h_misc + kMiscStats;   // (k_scatter_sorted's stats[0 .. 3], copied home with the head of d_misc)
    const uint32_t n_unique = h_stats[0], n_cells = h_stats[1], n_bricks = h_stats[3];
    gp.n_points = n_unique;
    gp.n_cells = n_cells;
    gp.n_bricks = n_bricks;

    // ---- hash table of occupied bricks, at most half full
    uint32_t slots = 64;
    while (slots < 2 * n_bricks) slots <<= 1;
    gp.table_mask = slots - 1;
    RSREG_HIP(ctx, ctx->d_table.reserve((size_t)slots * sizeof(BrickEntry)));
    RSREG_HIP(ctx, hipMemsetAsync(ctx->d_table.ptr, 0xff, (size_t)slots * sizeof(BrickEntry), st));
    k_brick_insert<<<div_up(n_bricks, kBlock), kBlock, 0, st>>>(brickkey, brickmask, brickbase, n_bricks,
                                                                ctx->d_table.as<BrickEntry>(), gp.table_mask);
    RSREG_HIP(ctx, hipGetLastError());
    k_max_cell_count<<<div_up(n_cells, kBlock), kBlock, 0, st>>>(ctx->d_cellpos.as<uint32_t>(), n_cells, d_misc + kMiscMaxCell);
    RSREG_HIP(ctx, hipGetLastError());
    if (ctx->profiling) (void)hipEventRecord(ev1, st);
    RSREG_HIP(ctx, hipMemcpyAsync(h_misc, d_misc, misc_bytes, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));

    rsreg_grid_info &gi = ctx->grid_info;
    for (int k = 0; k < 3; ++k) { gi.origin[k] = gp.origin[k]; gi.dims[k] = gp.dims[k]; }
    gi.cell_size = gp.cell;
    gi.n_unique_points = n_unique;
    gi.n_cells = n_cells;
    gi.max_points_per_cell = h_misc[kMiscMaxCell];
    gi.index_kind = 0;
    gi.index_bytes = (uint64_t)n_unique * sizeof(float4) + (uint64_t)slots * sizeof(BrickEntry) + ((uint64_t)n_cells + 1) * 4;
    if (ctx->profiling) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) gi.ms_build = ms;
    }
    ctx->have_target = true;
    // dense cloud: rebuild once with smaller cells (fewer candidates per query)
    const bool adaptive = tunables().adaptive_cell;
    if (adaptive && refine == 1.0 && n_cells > 0) {
        const double r = icp_refine_factor(n_unique, n_cells);
        if (r != 1.0) {
            const double ms_first = gi.ms_build;
            ctx->next_tgt_box = ctx->last_tgt_box;   // (the same records: no second measurement)
            int rc2 = build_grid(ctx, d_pts, n, stride, max_dist, r);
            if (rc2) return rc2;
            ctx->grid_info.ms_build += ms_first;
        }
    }
    return RSREG_OK;
}

// No index at all (icp_kernels.hpp: k_scan_nn): the target is only put into (x, y, index, z) records in the caller's
// order.  Chosen by rsreg_icp_set_target_cloud when the source that is already loaded has a handful of points;
// rsreg_icp_begin builds the real index after all if the alignment turns out to need it (`d_pts` must stay valid
// until then: the contract of cloud handles).
int scan_target(rsreg_ctx *ctx, const char *d_pts, size_t n, size_t stride, double max_dist)
{
    ctx->have_target = false;
    ctx->icp_fit_ok = false;
    ctx->fit_icp.built = false;
    ctx->tgt_cloud_id = 0;
    ctx->n_target_raw = n;
    std::memset(&ctx->grid_info, 0, sizeof(ctx->grid_info));
    std::memset(&ctx->grid, 0, sizeof(ctx->grid));
    ctx->gate_built_for = max_dist;
    ctx->tgt_rec = d_pts;
    ctx->tgt_rec_stride = stride;
    if (n > 0x7ffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "target too large");
    RSREG_HIP(ctx, ctx->d_tgt_sorted.reserve((n + 8) * sizeof(float4)));
    RSREG_HIP(ctx, ctx->d_scan_keys.reserve(kScanMaxSource * 8));
    k_scan_pack<<<div_up((uint32_t)n, kBlock), kBlock, 0, ctx->stream>>>(d_pts, stride, (uint32_t)n, ctx->d_tgt_sorted.as<float4>());
    RSREG_HIP(ctx, hipGetLastError());
    ctx->grid.dense = 2;
    ctx->grid.n_points = (uint32_t)n;
    ctx->scan_raw = d_pts;
    ctx->scan_stride = stride;
    ctx->grid_info.index_kind = 2;
    ctx->grid_info.n_unique_points = n;
    ctx->grid_info.index_bytes = (uint64_t)n * sizeof(float4);
    ctx->have_target = true;
    return RSREG_OK;
}

// The source load runs on its own stream; whoever needs its result (the number of distinct points, the source
// buffers) joins it first.
int join_source(rsreg_ctx *ctx)
{
    if (!ctx->src_pending) return RSREG_OK;
    ctx->src_pending = false;
    ctx->src_on_worker = false;
    const int rcw = ctx->source_enqueued();   // (the load's host side may still be running on the context's worker thread)
    if (rcw) {
        ctx->have_source = false;
        return rcw;
    }
    if (ctx->src_plain) {
        // one launch on the main stream, the caller's order, no merging: the number of queries IS the number of records, and
        // whatever reads the working copy is queued behind the launch on the same stream -- no wait on the caller's thread
        ctx->n_work = (uint32_t)ctx->n_source;
        return RSREG_OK;
    }
    RSREG_HIP(ctx, hipEventSynchronize(ctx->src.ev_done));
    ctx->n_work = ctx->h_smisc.as<uint32_t>()[kHsDistinct];
    return RSREG_OK;
}

// Sources of at most RSREG_PLAIN_SOURCE_MAX points are searched in the caller's order (k_source_plain), and never more than its
// workgroups have room for a partial box each (d_smisc: kBoxPartialGroups).  RSREG_SORT_SMALL=1: never.
constexpr size_t kPlainSourceLimit = (size_t)kBoxPartialGroups * kBlock;
bool source_is_small(size_t n)
{
    return n <= std::min<size_t>(tunables().plain_source_max, kPlainSourceLimit) && !tunables().sort_small;
}

// The part of a source load that queues work on src.stream (after one round trip for the bounding box); runs on the
// context's worker thread (rsreg_ctx.hpp: SourceWorker) or, with RSREG_NO_WORKER=1, on the caller's.
// `known`: the box of the cloud handle this source comes from, if the handle has one (by value: ctx->next_src_box belongs
// to the caller's thread alone)
int load_source_queue(rsreg_ctx *ctx, const char *d_raw, size_t n, size_t stride, const rsreg::CloudBox known)
{
    {
        RSREG_HIP(ctx, hipSetDevice(ctx->device));   // (this may be the context's worker thread)
        uint32_t *d_misc = ctx->d_smisc.as<uint32_t>(), *d_distinct = d_misc + kSmiscDistinct, *d_partials = d_misc + kSmiscPartials;
        uint32_t *h_words = ctx->h_smisc.as<uint32_t>(), *h_distinct = h_words + kHsDistinct;
        if (source_is_small(n)) {
            // one launch, the caller's order -- on the MAIN stream: the streams of a process share a few hardware queues,
            // and a kernel on the source stream can find itself behind a 0.4 ms voxel filter of a side stream
            hipStream_t st = ctx->stream;
            // (its box and finite count land in the pinned words kHsPlainBox behind the stamp `seq`; the ticket word lives in a buffer of its
            // own that is zero between launches)
            const bool box_too = tunables().box_cache;
            if (box_too && !ctx->d_plain_ticket.ptr) {
                RSREG_HIP(ctx, ctx->d_plain_ticket.reserve(64));
                RSREG_HIP(ctx, hipMemsetAsync(ctx->d_plain_ticket.ptr, 0, 64, st));
            }
            ctx->plain_box_seq = box_too ? ++ctx->plain_box_counter : 0u;
            k_source_plain<<<div_up((uint32_t)n, kBlock), kBlock, 0, st>>>(d_raw, stride, (uint32_t)n, ctx->d_src_all.as<float4>(), ctx->d_src.as<float4>(),
                                                                           ctx->d_perm.as<uint32_t>(), ctx->d_uniq_of.as<uint32_t>(),
                                                                           ctx->d_first.as<uint32_t>(), d_distinct, h_distinct,
                                                                           box_too ? d_partials : nullptr, ctx->d_plain_ticket.as<uint32_t>(), h_words + kHsPlainBox,
                                                                           ctx->plain_box_seq);
            RSREG_HIP(ctx, hipGetLastError());
            RSREG_HIP(ctx, hipEventRecord(ctx->src.ev_done, st));
            return RSREG_OK;
        }
        hipStream_t st = ctx->src.stream;
        RSREG_HIP(ctx, hipStreamWaitEvent(st, ctx->src.ev_main, 0));
        float mn[3], mx[3];
        uint32_t nfin = 0;
        const bool no_box_cache = !tunables().box_cache;
        if (known.valid && !no_box_cache) {   // (nothing of the load counts in the words k_bbox_final clears: the kernels below only store there)
            for (int k = 0; k < 3; ++k) { mn[k] = known.mn[k]; mx[k] = known.mx[k]; }
            nfin = known.nfin;
        } else {
            int rc = device_bbox_on(ctx, st, d_misc, h_words + kHsSrcBox, d_partials, d_raw, n, stride, mn, mx, &nfin);
            if (rc) return rc;
        }
        for (int k = 0; k < 3; ++k) { ctx->last_src_box.mn[k] = mn[k]; ctx->last_src_box.mx[k] = mx[k]; }
        ctx->last_src_box.nfin = nfin;
        ctx->last_src_box.valid = true;
        if (nfin == 0) { mn[0] = mn[1] = mn[2] = 0; mx[0] = mx[1] = mx[2] = 0; }
        double extent = 0;
        for (int k = 0; k < 3; ++k) extent = std::max(extent, (double)mx[k] - (double)mn[k]);
        // fine Morton resolution (a few mm): consecutive points then form compact blobs
        float cell = (float)std::max(tunables().cell_cap / 8.0, extent / 60000.0);
        // a 32-bit key (31 bits of Morton code + the invalid bit) halves the bytes the radix sort moves and saves it a pass
        // or two: the cell grows (by at most 2x: the search time moves by +- 1.5 % between 1.5 and 3 mm)
        // until the three axes need 31 bits together
        const bool wide_keys = tunables().keys64;
        auto axis_bits_of = [](double ext, double c) {
            int b = 1;
            while (b < 16 && (double)(1u << b) <= ext / c + 2.0) ++b;
            return b;
        };
        MortonBits mb{0, 0, 0};
        bool narrow = false;
        if (!wide_keys) {
            const int morton_bits = tunables().morton_bits;   // (23 + the invalid bit: three digit passes)
            for (double c = cell; c <= (morton_bits < 31 ? 64.0 : 2.0) * (double)cell + 1e-12; c *= 1.05) {
                mb = MortonBits{axis_bits_of((double)mx[0] - (double)mn[0], c), axis_bits_of((double)mx[1] - (double)mn[1], c),
                                axis_bits_of((double)mx[2] - (double)mn[2], c)};
                if (mb.x + mb.y + mb.z <= morton_bits && std::max(mb.x, std::max(mb.y, mb.z)) <= 12) {
                    narrow = true;
                    cell = (float)c;
                    break;
                }
            }
        }
        RSREG_HIP(ctx, ctx->d_skeys.reserve(n * 8));
        RSREG_HIP(ctx, ctx->d_skeys_alt.reserve(n * 8));
        RSREG_HIP(ctx, ctx->d_svals.reserve(n * 4));
        RSREG_HIP(ctx, ctx->d_sflags.reserve(n * 4));
        RSREG_HIP(ctx, ctx->d_sscan.reserve(n * 4));
        auto *vals = ctx->d_svals.as<uint32_t>();
        uint32_t *perm = ctx->d_perm.as<uint32_t>();
        uint32_t *keep = ctx->d_sflags.as<uint32_t>(), *pos = ctx->d_sscan.as<uint32_t>();
        const uint32_t nb = div_up((uint32_t)n, kBlock);
        size_t sort_bytes = 0;
        // (the sort's state at the head of d_stmp, the scan's sums behind it: the scan starts when the sort is done, but its
        // launches are queued before that)
        const size_t scan_bytes = oscan_scratch_bytes<uint32_t>(n);
        if (narrow) {
            auto *keys = ctx->d_skeys.as<uint32_t>();
            auto *keys2 = ctx->d_skeys_alt.as<uint32_t>();
            const unsigned sort_bits = (unsigned)(mb.x + mb.y + mb.z) + 1u;
            constexpr bool own_sort = true;   // (osort.hpp: the sort's state is cleared by the keys kernel, no memsets)
            const Radix32Plan plan = radix32_plan(n, 0, sort_bits);
            sort_bytes = (size_t)plan.words * 4;
            RSREG_HIP(ctx, ctx->d_stmp.reserve(std::max(sort_bytes, scan_bytes) + 256));
            // (an even number of passes ends in the pair it started from: the keys are then written where the result belongs)
            const bool start_in_out = plan.ends_in_first;
            uint32_t *keys_a = start_in_out ? keys2 : keys, *vals_a = start_in_out ? perm : vals;
            uint32_t *keys_b = start_in_out ? keys : keys2, *vals_b = start_in_out ? vals : perm;
            // the library's own sort over more than one workgroup's worth of pairs: its digit histograms are counted by the keys
            // kernel (two sets of counts in turn: the kernel clears the one the NEXT load will use, so no memset is queued;
            // a new buffer, or a load that did not get to its end, starts from one)
            const bool hist_on_the_way = own_sort && n > kOsTile;
            uint32_t *hist_now = nullptr;
            if (hist_on_the_way) {
                constexpr size_t set = OsKey<uint32_t>::max_passes * kOsDigits;
                const bool fresh = !ctx->d_shist.ptr;
                RSREG_HIP(ctx, ctx->d_shist.reserve(2 * set * 4));
                if (fresh || ctx->shist_dirty) RSREG_HIP(ctx, hipMemsetAsync(ctx->d_shist.ptr, 0, 2 * set * 4, st));
                ctx->shist_dirty = true;
                hist_now = ctx->d_shist.as<uint32_t>() + (ctx->shist_flip ? set : 0);
                uint32_t *hist_next = ctx->d_shist.as<uint32_t>() + (ctx->shist_flip ? 0 : set);
                ctx->shist_flip = !ctx->shist_flip;
                k_source_keys_hist<<<div_up((uint32_t)n, kOsHistBlock * kSkItems), kOsHistBlock, 0, st>>>(
                    d_raw, stride, (uint32_t)n, mn[0], mn[1], mn[2], 1.0f / cell, 1u << (sort_bits - 1u), mb, keys_a, vals_a, ctx->d_stmp.as<uint32_t>(), plan.words,
                    sort_bits, plan.passes, hist_now, hist_next);
            } else {
                k_source_keys<uint32_t><<<nb, kBlock, 0, st>>>(d_raw, stride, (uint32_t)n, mn[0], mn[1], mn[2], 1.0f / cell, 1u << (sort_bits - 1u), mb, keys_a, vals_a,
                                                               own_sort ? ctx->d_stmp.as<uint32_t>() : nullptr, own_sort ? plan.words : 0u);
            }
            RSREG_HIP(ctx, hipGetLastError());
            {
                bool in_first = false;
                RSREG_HIP(ctx, radix32_sort_pairs<uint32_t>(plan, ctx->d_stmp.as<uint32_t>(), keys_a, keys_b, vals_a, vals_b, n, 0, sort_bits, st, &in_first, hist_now));
                if (in_first != start_in_out) return fail(ctx, RSREG_ERR_STATE, "osort: the sorted pairs are not where they belong");
            }
            k_gather_source<uint32_t><<<nb, kBlock, 0, st>>>(d_raw, stride, (uint32_t)n, perm, ctx->d_src_all.as<float4>(), nullptr, keys2, keep);
            RSREG_HIP(ctx, hipGetLastError());
        } else {
            auto *keys = ctx->d_skeys.as<unsigned long long>();
            auto *keys2 = ctx->d_skeys_alt.as<unsigned long long>();
            // the sort only has to look at the bits the Morton codes of this extent can set (+ the invalid bit)
            const int axis_bits = axis_bits_of(extent, (double)cell);
            const unsigned sort_bits = 3u * (unsigned)axis_bits + 1u;
            const Radix32Plan plan = radix32_plan<unsigned long long>(n, 0, sort_bits);
            sort_bytes = (size_t)plan.words * 4;
            RSREG_HIP(ctx, ctx->d_stmp.reserve(std::max(sort_bytes, scan_bytes) + 256));
            const bool start_in_out = plan.ends_in_first;   // (as above: the sorted pairs must end in (keys2, perm))
            k_source_keys<unsigned long long><<<nb, kBlock, 0, st>>>(d_raw, stride, (uint32_t)n, mn[0], mn[1], mn[2], 1.0f / cell, 1ull << (3 * axis_bits), mb,
                                                                     start_in_out ? keys2 : keys, start_in_out ? perm : vals, ctx->d_stmp.as<uint32_t>(), plan.words);
            RSREG_HIP(ctx, hipGetLastError());
            {
                bool in_first = false;
                RSREG_HIP(ctx, radix32_sort_pairs<unsigned long long>(plan, ctx->d_stmp.as<uint32_t>(), start_in_out ? keys2 : keys, start_in_out ? keys : keys2,
                                                                      start_in_out ? perm : vals, start_in_out ? vals : perm, n, 0, sort_bits, st, &in_first));
                if (in_first != start_in_out) return fail(ctx, RSREG_ERR_STATE, "osort: the sorted pairs are not where they belong");
            }
            k_gather_source<unsigned long long><<<nb, kBlock, 0, st>>>(d_raw, stride, (uint32_t)n, perm, ctx->d_src_all.as<float4>(), nullptr, keys2, keep);
            RSREG_HIP(ctx, hipGetLastError());
        }
        RSREG_HIP(ctx, (oscan<uint32_t>(keep, pos, n, 0u, ctx->d_stmp.ptr, st)));
        k_source_unique<<<nb, kBlock, 0, st>>>(ctx->d_src_all.as<float4>(), (uint32_t)n, keep, pos, ctx->d_first.as<uint32_t>(),
                                               ctx->d_uniq_of.as<uint32_t>(), d_distinct, h_distinct,   // the number of distinct points: read at the join
                                               ctx->d_src.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipEventRecord(ctx->src.ev_done, st));
        ctx->shist_dirty = false;   // (everything of this load is queued: the counts' two sets are where the next load expects them)
    }
    return RSREG_OK;
}

// Loads the source: orders it spatially (Morton order of a few-mm grid, so the lanes of a wave
// query neighbouring cells) and merges exact copies of a point into one weighted point (the
// RealSense (0,0,0) pixels are ~11 % of a frame: they are searched once, not 10^5 times).
// d_perm: sorted position -> caller's index; d_uniq_of: sorted position -> distinct point.
// Everything after the bounding box (one host sync) is only queued -- on ctx->src.stream, behind whatever the
// main stream holds so far -- and joined by join_source: when the caller sets the source before the target (the
// reference's order, incremental_icp.hpp:57-58) the load runs beside the target's index build.
int load_source(rsreg_ctx *ctx, const char *d_raw, size_t n, size_t stride)
{
    if (n > 0xfffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "source too large");
    int rcj = join_source(ctx);   // (a load still in flight owns the buffers this one is about to fill)
    if (rcj) return rcj;
    ctx->last_src_box.valid = false;   // (of the load before this one: cloud.hip has taken it over by now)
    ctx->plain_box_seq = 0;
    // the box of the cloud this source comes from, if its handle knows it: taken over -- or dropped -- here, on the caller's
    // thread, after the load before this one has been joined; the worker's job gets a copy
    const rsreg::CloudBox known = ctx->next_src_box;
    ctx->next_src_box.valid = false;
    ctx->prep_join();
    RSREG_HIP(ctx, ctx->src.ensure());
    RSREG_HIP(ctx, ctx->d_src_all.reserve((n + 1) * sizeof(float4)));
    RSREG_HIP(ctx, ctx->d_src.reserve((n + 1) * sizeof(float4)));
    RSREG_HIP(ctx, ctx->d_cur.reserve((n + 1) * sizeof(float4)));
    RSREG_HIP(ctx, ctx->d_corr_pos.reserve((n + 1) * 4));
    RSREG_HIP(ctx, ctx->d_corr_d2.reserve((n + 1) * 4));
    RSREG_HIP(ctx, ctx->d_seed.reserve((n + 1) * 4));
    RSREG_HIP(ctx, ctx->d_perm.reserve((n + 1) * 4));
    RSREG_HIP(ctx, ctx->d_uniq_of.reserve((n + 1) * 4));
    RSREG_HIP(ctx, ctx->d_first.reserve((n + 2) * 4));
    RSREG_HIP(ctx, ctx->d_partials.reserve((size_t)reduce_blocks(n) * RSREG_NUM_SUMS * 8));
    {
        // the tile schedule's arrays lie at offsets that depend on the buffer's capacity only (tile_sched.hpp: sched_layout), so
        // that a schedule can be carried over to the next alignment; a new buffer starts from zero (the done counters go back
        // to zero by themselves) and without a schedule
        // (a larger buffer can come back at the address of the one just freed: the capacity says whether it is a new one)
        void *before = ctx->d_sched.ptr;
        const size_t cap_before = ctx->d_sched.cap;
        RSREG_HIP(ctx, ctx->d_sched.reserve(sched_layout(reduce_blocks(n)).words * 4));
        if (ctx->d_sched.ptr != before || ctx->d_sched.cap != cap_before) {
            RSREG_HIP(ctx, hipMemsetAsync(ctx->d_sched.ptr, 0, ctx->d_sched.cap, ctx->stream));
            sched_regrown(ctx->sched, sched_capacity(ctx->d_sched.cap));
        }
    }
    RSREG_HIP(ctx, ctx->d_sums.reserve(kSumsBytes));
    RSREG_HIP(ctx, ctx->h_sums.reserve(kSumsBytes));
    RSREG_HIP(ctx, ctx->d_smisc.reserve(kSmiscWords * sizeof(uint32_t)));
    RSREG_HIP(ctx, ctx->h_smisc.reserve(kHsWords * sizeof(uint32_t)));
    ctx->icp_fit_ok = false;   // (a new source: no fitness score until it is aligned)
    ctx->have_gicp_cs = false;   // (the covariances of the source before this one)
    ctx->have_lab_s = false;     // (and its colours)
    ctx->src_unmerged = false;
    ctx->src_nrm.have = false;   // (and its normals)
    ctx->gicp.active = 0;
    ctx->n_source = n;
    ctx->n_work = 0;
    ctx->src_cloud = nullptr;
    ctx->have_source = false;
    ctx->icp.active = 0;
    if (n) {
        // the raw cloud may have been produced (uploaded, filtered, transformed) on the main stream just now
        RSREG_HIP(ctx, hipEventRecord(ctx->src.ev_main, ctx->stream));
        const bool no_worker = !tunables().worker;
        ctx->src_on_worker = false;
        ctx->src_plain = source_is_small(n);
        if (no_worker || source_is_small(n)) {   // (a small source is one launch: not worth a hand-over)
            int rc = load_source_queue(ctx, d_raw, n, stride, known);
            if (rc) return rc;
        } else {
            ctx->src_on_worker = true;   // (until it is joined)
            // the rest -- a bounding-box round trip and ~25 launches -- on the context's worker thread: the caller goes on
            // (to the target's index build, in the reference's order of calls) while the source's queue is being filled
            if (!ctx->src_worker) ctx->src_worker.reset(new rsreg::SourceWorker());
            ctx->src_worker->post([ctx, d_raw, n, stride, known] { return load_source_queue(ctx, d_raw, n, stride, known); });
        }
        ctx->src_pending = true;
    }
    ctx->have_source = true;
    return RSREG_OK;
}

// DefaultConvergenceCriteria::hasConverged
bool criteria_has_converged(IcpState &s)
{
    const rsreg_icp_params &p = s.prm;
    if (s.state != RSREG_CONV_NOT_CONVERGED) { s.similar = 0; s.state = RSREG_CONV_NOT_CONVERGED; }
    bool is_similar = false;
    if (s.iterations >= p.max_iterations) { s.state = RSREG_CONV_ITERATIONS; return true; }
    if (p.criteria_mode == RSREG_CRITERIA_FIXED) return false;
    const double rot_thr = p.transformation_rotation_epsilon > 0 ? p.transformation_rotation_epsilon
                                                                  : 1.0 - p.transformation_epsilon;
    const double trans_thr = p.transformation_epsilon;
    const Mat4f &T = s.t_inc;
    const double cos_angle = 0.5 * ((double)T(0, 0) + (double)T(1, 1) + (double)T(2, 2) - 1.0);
    const double tsq = (double)T(0, 3) * T(0, 3) + (double)T(1, 3) * T(1, 3) + (double)T(2, 3) * T(2, 3);
    const int max_similar = 0;  // max_iterations_similar_transforms_
    if (cos_angle >= rot_thr && tsq <= trans_thr) {
        if (s.similar >= max_similar) { s.state = RSREG_CONV_TRANSFORM; return true; }
        is_similar = true;
    }
    if (std::fabs(s.cur_mse - s.prev_mse) < 1e-12) {
        if (s.similar >= max_similar) { s.state = RSREG_CONV_ABS_MSE; return true; }
        is_similar = true;
    }
    if (std::fabs(s.cur_mse - s.prev_mse) / s.prev_mse < p.euclidean_fitness_epsilon) {
        if (s.similar >= max_similar) { s.state = RSREG_CONV_REL_MSE; return true; }
        is_similar = true;
    }
    if (is_similar) ++s.similar; else s.similar = 0;
    s.prev_mse = s.cur_mse;
    return false;
}

int *seed_ptr(rsreg_ctx *ctx)
{
    return !tunables().seed ? nullptr : ctx->d_seed.as<int>();
}

// rsreg_icp_begin leaves "working copy = guess * source, no seeds" pending: the first search launch of the fused
// pipelines over the dense index does it on its way (launch_fused); whatever else touches the working copy first runs
// k_restart_source here.
int ensure_restarted(rsreg_ctx *ctx)
{
    IcpState &s = ctx->icp;
    if (!s.restart_pending) return RSREG_OK;
    s.restart_pending = false;
    const uint32_t n = (uint32_t)ctx->n_work;
    if (!n) return RSREG_OK;
    k_restart_source<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_src.as<float4>(), ctx->d_first.as<uint32_t>(), n, to_mat34(s.final_t), s.final_t.is_identity() ? 0 : 1,
                                                                    ctx->d_cur.as<float4>(), ctx->d_seed.as<int>());   // (and: no seeds yet)
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// diagnostic: per-wave start/end stamps of the last fused launch, dumped at rsreg_icp_end
unsigned long long *wave_times_ptr(rsreg_ctx *ctx, uint32_t n)
{
#ifndef RSREG_DIAG
    (void)ctx; (void)n;
    return nullptr;
#else
    if (!tunables().wave_times) return nullptr;
    if (ctx->d_brick.reserve(((size_t)n / 64 + 2) * 256 + (size_t)n * 4 + 64) != hipSuccess) return nullptr;   // (a scheduled launch has up to 2x the waves)
    return ctx->d_brick.as<unsigned long long>();
#endif
}

bool filters_on(const rsreg_icp_params &p)
{
    return p.use_reciprocal_correspondences != 0 || (p.trim_overlap_ratio > 0.0 && p.trim_overlap_ratio < 1.0);
}

// the pairs carry explicit weights (d_corr_w): one of the two filters, or a rejector chain, ran behind the search
bool weights_on(const rsreg_ctx *ctx) { return filters_on(ctx->icp.prm) || ctx->icp.chain.n > 0; }

// point-to-plane ICP (rsreg_estimation): the 32 sums and the 6-unknown solve take the place of the 17 sums and Umeyama
bool plane_on(const rsreg_icp_params &p) { return p.estimation == RSREG_ESTIMATION_POINT_TO_PLANE_LLS; }

// reciprocal check of one matched pair: is the source point the nearest source point of its target point?
template <bool kDense>
__global__ __launch_bounds__(kBlock) void k_recip_filter(const float4 *tgt, int *corr_pos, uint32_t *cw, uint32_t n, DenseDev gd, GridDev gh,
                                                         const float4 *child_pts, const uint32_t *perm, const uint32_t *first)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (kDense) dense_ring1_setup(gd);
    if (u >= n) return;
    const int pos = corr_pos[u];
    if (pos < 0) return;
    const float4 t = tgt[pos];
    const Best b = kDense ? nn_query_dense(gd, t.x, t.y, tgt_z(t), -1) : nn_query(gh, t.x, t.y, tgt_z(t), -1);
    // the index over the source keeps the lowest original index of equal points and prefers it among equidistant ones:
    // of the copies of a distinct source point only the first can be its target's nearest source point
    const bool ok = b.pos >= 0 && tgt_idx(child_pts[b.pos]) == perm[first[u]];
    cw[u] = ok ? 1u : 0u;
    if (!ok) corr_pos[u] = -1;
}

// Every correspondence search starts with this: a target whose grid is outside the served range (build_grid: unserved) is refused
// here, before a launch, not answered wrongly.  (One host comparison per launch; the kernels are the ones of every other grid.)
int refuse_unserved(rsreg_ctx *ctx, const rsreg_ctx *grid_of)
{
    if (!grid_of->grid.unserved) return RSREG_OK;
    return fail(ctx, RSREG_ERR_INVALID_ARG, "target outside the range the ICP search serves: cell above 2^60 m or box wider than a float (rsreg.h: rsreg_icp_set_target)");
}

// CorrespondenceRejectorTrimmed over the records in play.  flags == nullptr: rsreg_icp_params.trim_overlap_ratio, the records
// in play are the first cw[u] copies of every matched point and the cut lowers cw / corr_pos.  flags: the trim as an entry of
// the rejector chain -- one flag per record, *count_in of them set (known on the device: no counting pass), *count_out = how many the cut leaves.
int launch_trim(rsreg_ctx *ctx, float ratio, uint32_t *flags, const uint32_t *count_in, uint32_t *count_out)
{
    hipStream_t st = ctx->stream;
    const uint32_t ns = (uint32_t)ctx->n_source;
    uint32_t *cw = ctx->d_corr_w.as<uint32_t>();
    int *corr_pos = ctx->d_corr_pos.as<int>();
    // one key per ORIGINAL record, (d2, caller's index): ties at the cut go to the lowest index, also among the copies of
    // a distinct point on the merged (Morton-ordered) path -- the library's own 64-bit sort over the bits the keys use
    uint32_t idx_bits = 1;
    while (idx_bits < 32 && (ns - 1u) >> idx_bits) ++idx_bits;
    const unsigned sort_bits = 31u + idx_bits;
    RSREG_HIP(ctx, ctx->d_keys.reserve((size_t)ns * 8));
    RSREG_HIP(ctx, ctx->d_keys_alt.reserve((size_t)ns * 8));
    RSREG_HIP(ctx, ctx->d_vals.reserve((size_t)ns * 4));
    RSREG_HIP(ctx, ctx->d_vals_alt.reserve((size_t)ns * 4));
    auto *keys = ctx->d_keys.as<unsigned long long>(), *keys2 = ctx->d_keys_alt.as<unsigned long long>();
    uint32_t *vals = ctx->d_vals.as<uint32_t>(), *vals2 = ctx->d_vals_alt.as<uint32_t>();
    const Radix32Plan plan = radix32_plan<unsigned long long>(ns, 0, sort_bits);
    const size_t off_total = ((size_t)plan.words * 4 + 255) & ~(size_t)255;
    RSREG_HIP(ctx, ctx->d_tmp.reserve(off_total + 256));
    uint32_t *total = reinterpret_cast<uint32_t *>(ctx->d_tmp.as<char>() + off_total);
    if (!flags) RSREG_HIP(ctx, hipMemsetAsync(total, 0, 4, st));
    // (the keys are written into the pair the sort ends in, so that the result lies in (keys2, vals2); its state is
    // cleared by the keys kernel on its way)
    const bool start_in_out = plan.ends_in_first;
    unsigned long long *k_a = start_in_out ? keys2 : keys, *k_b = start_in_out ? keys : keys2;
    uint32_t *v_a = start_in_out ? vals2 : vals, *v_b = start_in_out ? vals : vals2;
    const uint32_t nbs = div_up(ns, kBlock);
    (flags ? k_trim_keys<true> : k_trim_keys<false>)<<<nbs, kBlock, 0, st>>>(corr_pos, flags ? flags : cw, ctx->d_corr_d2.as<float>(), ctx->d_perm.as<uint32_t>(),
                                                                             ctx->d_uniq_of.as<uint32_t>(), ctx->d_first.as<uint32_t>(), ns, idx_bits, k_a, v_a,
                                                                             ctx->d_tmp.as<uint32_t>(), plan.words);
    RSREG_HIP(ctx, hipGetLastError());
    {
        bool in_first = false;
        RSREG_HIP(ctx, radix32_sort_pairs<unsigned long long>(plan, ctx->d_tmp.as<uint32_t>(), k_a, k_b, v_a, v_b, ns, 0, sort_bits, st, &in_first));
        if ((in_first ? v_a : v_b) != vals2) return fail(ctx, RSREG_ERR_STATE, "osort: the sorted pairs are not where they belong");
    }
    if (flags) {
        k_trim_apply<true><<<nbs, kBlock, 0, st>>>(vals2, count_in, ns, ratio, ctx->d_uniq_of.as<uint32_t>(), ctx->d_first.as<uint32_t>(), flags, corr_pos, count_out);
    } else {
        k_trim_count<<<nbs, kBlock, 0, st>>>(keys2, ns, idx_bits, total);
        RSREG_HIP(ctx, hipGetLastError());
        k_trim_apply<false><<<nbs, kBlock, 0, st>>>(vals2, total, ns, ratio, ctx->d_uniq_of.as<uint32_t>(), ctx->d_first.as<uint32_t>(), cw, corr_pos, nullptr);
    }
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// the optional filters PCL's ICP applies between determineCorrespondences and the transformation estimate:
// reciprocal correspondences (CorrespondenceEstimation::determineReciprocalCorrespondences) and the trimmed rejector
int apply_filters(rsreg_ctx *ctx)
{
    IcpState &s = ctx->icp;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)ctx->n_work, ns = (uint32_t)ctx->n_source;
    if (!n) return RSREG_OK;
    RSREG_HIP(ctx, ctx->d_corr_w.reserve((size_t)n * 4 + 16));
    uint32_t *cw = ctx->d_corr_w.as<uint32_t>();
    int *corr_pos = ctx->d_corr_pos.as<int>();
    const uint32_t nb = div_up(n, kBlock);
    k_corr_weights<<<nb, kBlock, 0, st>>>(corr_pos, ctx->d_cur.as<float4>(), n, cw);
    RSREG_HIP(ctx, hipGetLastError());
    if (s.prm.use_reciprocal_correspondences) {
        // index the CURRENT source (it moves every iteration; PCL rebuilds its reciprocal kd-tree too), in the caller's order
        if (!ctx->recip) {
            int rc = rsreg_ctx_create(ctx->device, ctx->stream, &ctx->recip);
            if (rc) return fail(ctx, rc, "context of the reciprocal index");
        }
        RSREG_HIP(ctx, ctx->d_recip_pts.reserve(((size_t)ns + 1) * sizeof(float4)));
        k_recip_points<<<div_up(ns, kBlock), kBlock, 0, st>>>(ctx->d_cur.as<float4>(), ctx->d_perm.as<uint32_t>(), ctx->d_uniq_of.as<uint32_t>(), ns,
                                                           ctx->d_recip_pts.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
        rsreg_ctx *c = ctx->recip;
        int rc = build_grid(c, ctx->d_recip_pts.as<char>(), ns, sizeof(float4), s.prm.max_correspondence_distance, 1.0);
        if (rc) {
            std::string why;
            {
                std::lock_guard<std::mutex> lk(c->error_mutex);
                why = c->last_error;
            }
            return fail(ctx, rc, why.c_str());
        }
        if (int rcu = refuse_unserved(ctx, c)) return rcu;   // (the index over the source: the same range)
        if (c->grid.n_points) {   // (a bound while the child's counting build has not been waited for: never 0 for a cloud with a finite point)
            const DenseDev gd = c->grid.dense ? dense_dev(c, s.prm.max_correspondence_distance) : DenseDev{};
            const GridDev gh = grid_dev(c, s.prm.max_correspondence_distance);
            auto kern = c->grid.dense ? k_recip_filter<true> : k_recip_filter<false>;
            kern<<<nb, kBlock, 0, st>>>(ctx->d_tgt_sorted.as<float4>(), corr_pos, cw, n, gd, gh, c->d_tgt_sorted.as<float4>(),
                                        ctx->d_perm.as<uint32_t>(), ctx->d_first.as<uint32_t>());
            RSREG_HIP(ctx, hipGetLastError());
        }
    }
    if (s.prm.trim_overlap_ratio > 0.0 && s.prm.trim_overlap_ratio < 1.0) return launch_trim(ctx, (float)s.prm.trim_overlap_ratio, nullptr, nullptr, nullptr);
    return RSREG_OK;
}

// d_src_nrm_cur = the guess's 3 x 3 block * the source's normals as handed in: what rsreg_icp_begin leaves pending for a chain
// with the normal test, done by whoever touches the current normals first
int ensure_normals_restarted(rsreg_ctx *ctx)
{
    IcpState &s = ctx->icp;
    if (!s.normals_restart_pending) return RSREG_OK;
    s.normals_restart_pending = false;
    const uint32_t ns = (uint32_t)ctx->n_source;
    if (!ns) return RSREG_OK;
    RSREG_HIP(ctx, ctx->d_src_nrm_cur.reserve(((size_t)ns + 1) * sizeof(float4)));
    k_restart_normals<<<div_up(ns, kBlock), kBlock, 0, ctx->stream>>>(ctx->src_nrm.d.as<float4>(), ns, to_mat34(s.final_t), s.final_t.is_identity() ? 0 : 1,
                                                                     ctx->d_src_nrm_cur.as<float4>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// The rejector chain (include/rsreg.h: rsreg_icp_set_rejectors) behind apply_filters, all of it queued on the context's stream:
// flags per original record <- (corr_pos, cw); every entry rewrites them and leaves its count; the flags are counted back
// into cw / corr_pos.  Nothing is read back here: the counts and medians wait in d_rej_words for rsreg_icp_rejector_stats.
int apply_chain(rsreg_ctx *ctx)
{
    IcpState &s = ctx->icp;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)ctx->n_work, ns = (uint32_t)ctx->n_source;
    RSREG_HIP(ctx, ctx->d_rej_words.reserve(kRejWords * 4));
    uint32_t *words = ctx->d_rej_words.as<uint32_t>();
    RSREG_HIP(ctx, hipMemsetAsync(words, 0, kRejWords * 4, st));
    s.chain_stats = true;
    if (!n || !ns) return RSREG_OK;
    RSREG_HIP(ctx, ctx->d_rej_flags.reserve((size_t)ns * 4 + 16));
    uint32_t *flags = ctx->d_rej_flags.as<uint32_t>();
    uint32_t *cw = ctx->d_corr_w.as<uint32_t>();
    int *corr_pos = ctx->d_corr_pos.as<int>();
    const float *d2 = ctx->d_corr_d2.as<float>();
    const uint32_t *perm = ctx->d_perm.as<uint32_t>(), *uniq_of = ctx->d_uniq_of.as<uint32_t>(), *first = ctx->d_first.as<uint32_t>();
    const uint32_t nbs = div_up(ns, kBlock);
    const uint32_t nbg = rej_grid(ns);   // (the kernels that count, and the median's, which re-derive the select's state per workgroup: a bounded grid)
    uint32_t *cnt = words + kRejCnt;
    k_rej_flags_init<<<nbg, kBlock, 0, st>>>(corr_pos, cw, uniq_of, first, ns, flags, &cnt[0]);
    RSREG_HIP(ctx, hipGetLastError());
    for (int e = 0; e < s.chain.n; ++e) {
        const rsreg_rejector &r = s.chain.e[e];
        switch (r.kind) {
        case RSREG_REJECTOR_MEDIAN_DISTANCE: {
            uint32_t *hist = words + kRejHist + (uint32_t)e * kRejHistWords;
            for (uint32_t digit = 0; digit < kRejDigits; ++digit)
                k_rej_median_hist<<<nbg, kBlock, 0, st>>>(flags, d2, uniq_of, ns, digit, &cnt[e], hist);
            k_rej_median_apply<<<nbg, kBlock, 0, st>>>(flags, d2, uniq_of, ns, &cnt[e], hist, r.value, words + kRejMed + e, &cnt[e + 1]);
            break;
        }
        case RSREG_REJECTOR_ONE_TO_ONE: {
            const size_t nt = ctx->grid.n_points;   // (positions of the sorted target: the count, or its bound while a build's counts are pending)
            RSREG_HIP(ctx, ctx->d_rej_table.reserve((nt + 1) * 8));
            RSREG_HIP(ctx, hipMemsetAsync(ctx->d_rej_table.ptr, 0xff, (nt + 1) * 8, st));
            k_rej_o2o_min<<<nbg, kBlock, 0, st>>>(flags, corr_pos, d2, perm, uniq_of, ns, ctx->d_rej_table.as<unsigned long long>());
            k_rej_o2o_keep<<<nbg, kBlock, 0, st>>>(flags, corr_pos, d2, perm, uniq_of, ns, ctx->d_rej_table.as<unsigned long long>(), &cnt[e + 1]);
            break;
        }
        case RSREG_REJECTOR_SURFACE_NORMAL: {
            int rcn = ensure_normals_restarted(ctx);
            if (rcn) return rcn;
            k_rej_normal<<<nbg, kBlock, 0, st>>>(flags, corr_pos, perm, uniq_of, ns, ctx->d_tgt_sorted.as<float4>(), ctx->tgt_nrm.d.as<float4>(),
                                                 ctx->d_src_nrm_cur.as<float4>(), r.value, &cnt[e + 1]);
            break;
        }
        case RSREG_REJECTOR_TRIMMED: {
            int rct = launch_trim(ctx, (float)r.value, flags, &cnt[e], &cnt[e + 1]);
            if (rct) return rct;
            break;
        }
        default:
            return fail(ctx, RSREG_ERR_STATE, "rejector chain: unknown kind");
        }
        RSREG_HIP(ctx, hipGetLastError());
    }
    RSREG_HIP(ctx, hipMemsetAsync(cw, 0, (size_t)n * 4, st));
    k_rej_fold<<<nbs, kBlock, 0, st>>>(flags, uniq_of, ns, cw);
    RSREG_HIP(ctx, hipGetLastError());
    k_rej_fold_pos<<<div_up(n, kBlock), kBlock, 0, st>>>(cw, n, corr_pos);
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// the 6-D search of GICP6D is on (rsreg_gicp6d_begin): the pairs' positions then point into its own index's point array
bool six_on(const rsreg_ctx *ctx) { return ctx->gicp.active && ctx->gicp.six; }

// the (x, y, record, z) array corr_pos points into: the sorted target of the alignment's index, or the 6-D index's points
const float4 *pair_targets(const rsreg_ctx *ctx) { return six_on(ctx) ? ctx->g6.d_pts.as<float4>() : ctx->d_tgt_sorted.as<float4>(); }

int launch_search(rsreg_ctx *ctx)
{
    if (int rcu = refuse_unserved(ctx, ctx)) return rcu;
    ctx->icp.idle_after_sums = false;   // (something is queued on the main stream from here on)
    IcpState &s = ctx->icp;
    {
        int rcr = ensure_restarted(ctx);
        if (rcr) return rcr;
    }
    const uint32_t n = (uint32_t)ctx->n_work;
    const double gate2 = s.prm.max_correspondence_distance * s.prm.max_correspondence_distance;
    if (n) {
        ScopedEvents ev(ctx, &ctx->ev_nn);
        const GridDev g = grid_dev(ctx, s.prm.max_correspondence_distance);
        if (six_on(ctx)) {
            k_nn_search6<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), ctx->d_src6_col.as<float4>(), n, grid_dev(ctx->g6),
                                                                        ctx->d_g6_col.as<float4>(), g.prune2, gate2, ctx->d_corr_pos.as<int>(),
                                                                        ctx->d_corr_d2.as<float>());
        } else if (ctx->grid.dense == 2) {
            // the largest float that passes PCL's `if (distance > max_dist_sqr) continue` (compared in double)
            float gate_f = gate2 >= (double)FLT_MAX ? FLT_MAX : (float)gate2;
            if ((double)gate_f > gate2) gate_f = std::nextafterf(gate_f, 0.0f);
            unsigned long long *keys = ctx->d_scan_keys.as<unsigned long long>();
            const uint32_t nt = ctx->grid.n_points;
            RSREG_HIP(ctx, hipMemsetAsync(keys, 0xff, (size_t)n * 8, ctx->stream));
            if (nt)
                k_scan_nn<<<std::min(div_up(nt, kBlock), 2048u), kBlock, 0, ctx->stream>>>(ctx->d_tgt_sorted.as<float4>(), nt, ctx->d_cur.as<float4>(),
                                                                                          n, gate_f, keys);
            k_scan_finish<<<1, kScanMaxSource, 0, ctx->stream>>>(keys, ctx->d_cur.as<float4>(), n, ctx->d_corr_pos.as<int>(),
                                                                ctx->d_corr_d2.as<float>());
        } else if (ctx->grid.dense)
            (ctx->grid.have_nbr ? k_nn_search_dense<0> : k_nn_search_dense<3>)<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), n,
                                                                             dense_dev(ctx, s.prm.max_correspondence_distance), gate2,
                                                                             ctx->d_corr_pos.as<int>(), ctx->d_corr_d2.as<float>(),
                                                                             seed_ptr(ctx));
        else
            k_nn_search<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), n, g, gate2,
                                                                       ctx->d_corr_pos.as<int>(), ctx->d_corr_d2.as<float>(), seed_ptr(ctx));
        RSREG_HIP(ctx, hipGetLastError());
        s.n_nn_launches++;
    }
    if (weights_on(ctx)) {
        int rc = apply_filters(ctx);
        if (!rc && s.chain.n > 0) rc = apply_chain(ctx);
        if (rc) return rc;
    }
    s.have_search = true;
    return RSREG_OK;
}

// ---- the tail that brings an iteration's sums to the host, in two halves (the staged callers close their ev_reduce bracket
// between them): queue_final_reduce, then fetch_sums.  `count`: the 17 sums of a point-to-point iteration, the 32 of a
// point-to-plane or of a GICP one.
// where k_final_reduce leaves the sums the host is about to read: without a communicator straight in the pinned
// host buffer (no copy to queue behind the kernel), otherwise in HBM (the all-reduce works there)
double *host_sums_target(rsreg_ctx *ctx) { return ctx->comm ? ctx->d_sums.as<double>() : ctx->h_sums.as<double>(); }

// one workgroup per sum over the `nb` workgroups' partials
int queue_final_reduce(rsreg_ctx *ctx, const double *partials, uint32_t nb, int count)
{
    k_final_reduce<<<count, kReduceBlock, 0, ctx->stream>>>(partials, nb, host_sums_target(ctx));
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// (all-reduce,) copy where a communicator exists, wait, sums[0 .. count).  global: the sums of all ranks -- the 17 only: the
// alignments with 32 sums refuse more than one rank (icp_begin, rsreg_gicp_begin) and never ask
int fetch_sums(rsreg_ctx *ctx, double *sums, int count, bool global)
{
    if (global && ctx->comm) {   // also on a one-rank communicator: same calls, same stream order
        ScopedEvents ev(ctx, &ctx->ev_allreduce);
        int rc = rsreg_comm_allreduce_device_(ctx, ctx->d_sums.as<double>(), RSREG_NUM_SUMS);
        if (rc) return rc;
    }
    double *h = ctx->h_sums.as<double>();
    if (ctx->comm) RSREG_HIP(ctx, hipMemcpyAsync(h, ctx->d_sums.ptr, (size_t)count * 8, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->icp.idle_after_sums = true;
    (void)target_counts(ctx, false);
    std::memcpy(sums, h, (size_t)count * 8);
    return RSREG_OK;
}

int launch_sums(rsreg_ctx *ctx, double *sums, bool global)
{
    ctx->icp.idle_after_sums = false;   // (something is queued on the main stream from here on)
    {
        int rcr = ensure_restarted(ctx);
        if (rcr) return rcr;
    }
    const uint32_t n = (uint32_t)ctx->n_work;
    {
        ScopedEvents ev(ctx, &ctx->ev_reduce);
        if (weights_on(ctx))
            k_cov_reduce_w<<<reduce_blocks(n), kTile, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), ctx->d_corr_pos.as<int>(),
                                                                      ctx->d_corr_d2.as<float>(), ctx->d_corr_w.as<uint32_t>(),
                                                                      ctx->d_tgt_sorted.as<float4>(), n, ctx->d_partials.as<double>());
        else
            k_cov_reduce<<<reduce_blocks(n), kTile, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), ctx->d_corr_pos.as<int>(),
                                                                    ctx->d_corr_d2.as<float>(), ctx->d_tgt_sorted.as<float4>(), n,
                                                                    ctx->d_partials.as<double>());
        RSREG_HIP(ctx, hipGetLastError());
        int rc = queue_final_reduce(ctx, ctx->d_partials.as<double>(), reduce_blocks(n), RSREG_NUM_SUMS);
        if (rc) return rc;
    }
    return fetch_sums(ctx, sums, RSREG_NUM_SUMS, global);
}

// The 32 sums of a point-to-plane iteration (include/rsreg.h: RSREG_NUM_PLANE_SUMS) over the search's pairs: k_plane_reduce in
// the place of k_cov_reduce, k_final_reduce with a block per sum.  One rank only (rsreg_icp_begin): nothing is all-reduced.
int launch_plane_sums(rsreg_ctx *ctx, double *sums)
{
    ctx->icp.idle_after_sums = false;
    {
        int rcr = ensure_restarted(ctx);
        if (rcr) return rcr;
    }
    const uint32_t n = (uint32_t)ctx->n_work;
    const uint32_t nb = reduce_blocks(n);
    RSREG_HIP(ctx, ctx->d_plane_partials.reserve((size_t)nb * RSREG_NUM_PLANE_SUMS * 8));
    {
        ScopedEvents ev(ctx, &ctx->ev_reduce);
        k_plane_reduce<<<nb, kTile, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), ctx->d_corr_pos.as<int>(), ctx->d_corr_d2.as<float>(),
                                                      weights_on(ctx) ? ctx->d_corr_w.as<uint32_t>() : nullptr,
                                                      ctx->d_tgt_sorted.as<float4>(), ctx->tgt_nrm.d.as<float4>(), n,
                                                      ctx->d_plane_partials.as<double>());
        RSREG_HIP(ctx, hipGetLastError());
        int rc = queue_final_reduce(ctx, ctx->d_plane_partials.as<double>(), nb, RSREG_NUM_PLANE_SUMS);
        if (rc) return rc;
    }
    return fetch_sums(ctx, sums, RSREG_NUM_PLANE_SUMS, false);
}

// ---- tile schedule of the fused dense kernel (tile_sched.hpp: what it is for, its layout, state and launch rule) ----------
SchedCfg sched_cfg()
{
    const Tunables &t = tunables();
    SchedCfg c;
    c.on = t.sched;
    c.f4 = t.sched_f4;
    c.f2 = t.sched_f2;
    c.min_tiles = t.sched_min_tiles;
    c.at_launch = t.sched_at;
    return c;
}

static_assert(kSchedCostWords == kTileWaves, "the schedule buffer holds one cost word per wave of a tile");

struct SchedBufs {
    uint32_t *items, *cost, *done, *items_first;
};

SchedBufs sched_bufs(const rsreg_ctx *ctx)
{
    uint32_t *p = ctx->d_sched.as<uint32_t>();
    const SchedLayout l = sched_layout(ctx->sched.cap_tiles);   // (capacity, not this source's tiles: the arrays stay put from one alignment to the next)
    return SchedBufs{p + l.items, p + l.cost, p + l.done, p + l.items_first};
}

// The whole schedule in one workgroup (7 k tiles at 10^6 points; three kernels and a device-wide radix sort of 10-bit
// keys cost 35 us between two search launches, this one a few): a counting sort of the tiles by how long their slower
// wave ran in the timed launch, in steps of 0.64 us, longest first, then rank r -> its workgroups: the first n4 tiles
// get four, the next n2 two, the others one.  Tiles of one step come in whatever order the atomics hand out: the order
// of the workgroups decides when a tile runs, never what it computes.
// The list is XCD-aware: workgroups are dealt to the eight XCDs in turn (b and b + 8 share one, MI355X_MICROARCH.md
// "Workgroup dispatch"), and every XCD has a 4 MiB L2 of its own.  The tiles are in the source's Morton order, so a run of
// consecutive tiles is a compact piece of space: pieces of `deal` (RSREG_SCHED_XCD_DEAL, 32) consecutive tiles are dealt
// to eight runs in turn, each run is sorted longest first by itself, and the runs are dealt out to the workgroups in turn:
// workgroup b works on run b % 8 while that run lasts, so one XCD's L2 sees an eighth of the target's cells instead of all
// of them.  When a run is used up the others close ranks (no empty workgroups; those last tiles land on whatever XCD is
// next).  Which workgroup takes which tile never changes what a tile computes.
// Measured (profiles/r03_experiments/xcd_schedule_*) against one longest-first list for all XCDs: 300 k points 53.6 ->
// 48.7 us per launch (the eighth of the index fits the L2), 10^6 points level (96.9 against 96.5-98.3); pieces of 64+ tiles
// or eight contiguous runs of equal cost are slower at 10^6 (102-103 us: the heavy tiles of a crowded region then share
// one XCD's 256 workgroup slots); a few cost classes with the Morton order kept inside a class are slower the coarser the
// classes (97 -> 117 us).  (The single list and the equal-cost runs were forms of this kernel up to 730cb2e.)
__global__ __launch_bounds__(1024) void k_sched_build(const uint32_t *cost, uint32_t n_tiles, uint32_t n4, uint32_t n2, uint32_t total_items,
                                                      uint32_t deal, uint32_t *items, uint32_t *done)
{
    constexpr uint32_t kRuns = 8;
    __shared__ uint32_t bins[kRuns * 1024];
    __shared__ uint32_t part[16];
    __shared__ uint32_t run_first[kRuns + 1];   // rank, in run-major sorted order, of the first tile of a run
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t k = tid; k < kRuns * 1024u; k += 1024u) bins[k] = 0;
    __syncthreads();
    auto bucket_of = [&](uint32_t t) {   // 0 .. 1023, steps of 0.64 us, longer = larger
        uint32_t c = 0;
        for (int w = 0; w < kTileWaves; ++w) c = max(c, cost[t * kTileWaves + w]);
        return min(c >> 6, 1023u);
    };
    auto run_of = [&](uint32_t t) { return (t / deal) % kRuns; };
    // every thread owns a contiguous share of the tiles
    const uint32_t per = (n_tiles + 1023u) / 1024u, lo = min(n_tiles, tid * per), hi = min(n_tiles, lo + per);
    for (uint32_t t = lo; t < hi; ++t) {
        atomicAdd(&bins[run_of(t) * 1024u + (1023u - bucket_of(t))], 1u);
        done[t] = 0u;
    }
    __syncthreads();
    // exclusive scan of the 8 x 1024 bins, run-major: eight consecutive bins per thread
    {
        uint32_t v[8], sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = bins[tid * 8u + k]; sum += v[k]; }
        uint32_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(incl, off);
            if ((int)lane >= off) incl += u;
        }
        if (lane == 63u) part[wave] = incl;
        __syncthreads();
        uint32_t at = incl - sum;
        for (uint32_t w = 0; w < wave; ++w) at += part[w];
        if ((tid & 127u) == 0) run_first[tid >> 7] = at;   // (bin x * 1024 is thread 128 x's first)
        if (tid == 0) run_first[kRuns] = n_tiles;
#pragma unroll
        for (int k = 0; k < 8; ++k) { bins[tid * 8u + k] = at; at += v[k]; }
    }
    __syncthreads();
    // how long every run's list of workgroups is: its tiles, the first n4 / 8 of them four times, the next n2 / 8 twice
    uint32_t len[kRuns], r4[kRuns], r2[kRuns], used = 0;
#pragma unroll
    for (uint32_t x = 0; x < kRuns; ++x) {
        const uint32_t cnt = run_first[x + 1] - run_first[x];
        r4[x] = min(n4 / kRuns, cnt);
        r2[x] = min(n2 / kRuns, cnt - r4[x]);
        len[x] = cnt + 3u * r4[x] + r2[x];
        used += len[x];
    }
    auto place = [&](uint32_t x, uint32_t p) {   // list position p of run x -> workgroup: the runs dealt out in turn while they last
        uint32_t pos = 0;
#pragma unroll
        for (uint32_t y = 0; y < kRuns; ++y) pos += min(len[y], p + (y < x ? 1u : 0u));
        return pos;
    };
    for (uint32_t t = lo; t < hi; ++t) {
        const uint32_t b = bucket_of(t), x = run_of(t);
        const uint32_t r = atomicAdd(&bins[x * 1024u + (1023u - b)], 1u) - run_first[x];   // rank inside its run, longest first
        uint32_t lg, p;
        if (r < r4[x]) { lg = 2; p = 4u * r; }
        else if (r < r4[x] + r2[x]) { lg = 1; p = 4u * r4[x] + 2u * (r - r4[x]); }
        else { lg = 0; p = 4u * r4[x] + 2u * r2[x] + (r - r4[x] - r2[x]); }
        for (uint32_t q = 0; q < (1u << lg); ++q) items[place(x, p + q)] = t | q << 24 | lg << 28;
    }
    for (uint32_t k = used + tid; k < total_items; k += 1024u) items[k] = 0xffffffffu;   // (a run shorter than its share of the splits: nothing to do)
}

// first: the schedule of the alignments' FIRST launches (from a timed first launch; kept beside the steady one)
int build_schedule(rsreg_ctx *ctx, uint32_t n_tiles, bool first)
{
    const SchedCfg cfg = sched_cfg();
    if (n_tiles > ctx->sched.cap_tiles) return fail(ctx, RSREG_ERR_STATE, "tile schedule: more tiles than the schedule buffer was laid out for");
    const SchedBufs sb = sched_bufs(ctx);
    uint32_t n4 = (uint32_t)(cfg.f4 * n_tiles), n2 = (uint32_t)(cfg.f2 * n_tiles);
    n4 -= n4 % 8u;   // (an eighth of the splits to every run)
    n2 -= n2 % 8u;
    const uint32_t n_items = n_tiles + 3 * n4 + n2;
    k_sched_build<<<1, 1024, 0, ctx->stream>>>(sb.cost, n_tiles, n4, n2, n_items, tunables().sched_xcd_deal, first ? sb.items_first : sb.items, sb.done);
    RSREG_HIP(ctx, hipGetLastError());
    sched_built(ctx->sched, ctx->icp.sched, first, n_items, n_tiles);
#ifdef RSREG_DIAG
    if (!first && tunables().sched_verbose)
        std::fprintf(stderr, "[rsreg] tile schedule: %u tiles, %u searched by 4 lanes per query, %u by 2, %u workgroups\n", n_tiles, n4, n2, n_items);
#endif
    return RSREG_OK;
}

// fused pass: applies the pending increment (if any), searches, gates and reduces
int launch_fused(rsreg_ctx *ctx, double *sums, bool want_corr, bool device_loop = false)
{
    if (int rcu = refuse_unserved(ctx, ctx)) return rcu;
    ctx->icp.idle_after_sums = false;   // (something is queued on the main stream from here on)
    IcpState &s = ctx->icp;
    const uint32_t n = (uint32_t)ctx->n_work;
    const IcpDevState *dev = device_loop ? ctx->d_icp_state.as<IcpDevState>() : nullptr;
    const double gate2 = s.prm.max_correspondence_distance * s.prm.max_correspondence_distance;
    // the first launch of an alignment over the dense index reads the source itself, applies the guess and starts without
    // seeds: k_restart_source's work, one launch and a pass over the working copy saved (never with a schedule of this
    // alignment's own in place: that is built from one of its launches; a carried one may serve it, below)
    const bool restart_here = s.restart_pending && ctx->grid.dense && !s.sched.ready && !s.pending_transform;
    if (restart_here) {
        s.restart_pending = false;
    } else {
        int rcr = ensure_restarted(ctx);
        if (rcr) return rcr;
    }
    {
        ScopedEvents ev(ctx, &ctx->ev_nn);
        const GridDev g = grid_dev(ctx, s.prm.max_correspondence_distance);
        if (ctx->grid.dense) {
            unsigned long long *wt = wave_times_ptr(ctx, n);
            // (the search beyond ring 1 comes in two forms; each instantiation carries only the one its grid uses)
            const bool blocks = ctx->grid.max_ring <= 4 && gate_in_rings(ctx->grid) && !tunables().far_rows;
#ifdef RSREG_DIAG
            const bool light = tunables().wave_times_light;
            const bool tab = !ctx->grid.have_nbr;   // (an index without occupancy words: read off the table)
            auto kern = wt ? (light ? (tab ? k_icp_fused_dense<2, 3> : blocks ? k_icp_fused_dense<2, 1> : k_icp_fused_dense<2, 2>)
                                    : (tab ? k_icp_fused_dense<1, 3> : blocks ? k_icp_fused_dense<1, 1> : k_icp_fused_dense<1, 2>))
                           : (tab ? k_icp_fused_dense<0, 3> : blocks ? k_icp_fused_dense<0, 1> : k_icp_fused_dense<0, 2>);
#else
            const bool light = false;
            auto kern = !ctx->grid.have_nbr ? k_icp_fused_dense<0, 3> : blocks ? k_icp_fused_dense<0, 1> : k_icp_fused_dense<0, 2>;
#endif
            const SchedCfg cfg = sched_cfg();
            const uint32_t n_tiles = reduce_blocks(n);
            const SchedLaunch l = sched_next(cfg, ctx->sched, s.sched, n_tiles, restart_here, wt && !light);
            TileSched sc{};
            sc.n_tiles = n_tiles;
            if (l.eligible) {
                const SchedBufs sb = sched_bufs(ctx);
                sc.items = l.from == SchedLaunch::first ? sb.items_first : l.from == SchedLaunch::steady ? sb.items : nullptr;
                sc.cost = l.timed ? sb.cost : nullptr;
                sc.done = sb.done;
                sc.pos = ctx->d_corr_pos.as<int>();
                sc.d2 = ctx->d_corr_d2.as<float>();
                sc.n_items = l.n_items;
                sc.first_extra = l.first_extra;
            }
            kern<<<l.grid, kTile, 0, ctx->stream>>>(
                ctx->d_cur.as<float4>(), restart_here ? ctx->d_src.as<float4>() : nullptr, ctx->d_first.as<uint32_t>(), n, to_mat34(restart_here ? s.final_t : s.t_inc),
                restart_here ? (s.final_t.is_identity() ? 0 : 1) : (s.pending_transform ? 1 : 0),
                dense_dev(ctx, s.prm.max_correspondence_distance), gate2, want_corr ? ctx->d_corr_pos.as<int>() : nullptr,
                ctx->d_corr_d2.as<float>(), ctx->d_partials.as<double>(), seed_ptr(ctx), wt, dev, sc);
            RSREG_HIP(ctx, hipGetLastError());
            if (l.timed) {
                int rc = build_schedule(ctx, n_tiles, restart_here);
                if (rc) return rc;
                if (restart_here && cfg.at_launch == 0) {   // (RSREG_SCHED_AT=0: the steady schedule from the first launch's costs too)
                    rc = build_schedule(ctx, n_tiles, false);
                    if (rc) return rc;
                }
            }
            s.sched.fused_launches++;
            if (sc.items) s.n_sched_launches++;
        }
        else
            k_icp_fused<<<reduce_blocks(n), kTile, 0, ctx->stream>>>(
                ctx->d_cur.as<float4>(), n, to_mat34(s.t_inc), s.pending_transform ? 1 : 0, g, gate2,
                want_corr ? ctx->d_corr_pos.as<int>() : nullptr, ctx->d_corr_d2.as<float>(), ctx->d_partials.as<double>(),
                seed_ptr(ctx), dev);
        RSREG_HIP(ctx, hipGetLastError());
        s.n_nn_launches++;
    }
    s.pending_transform = false;
    // (no events of their own for what follows: in the fused pipelines ms_reduce is the time
    // between consecutive search kernels, read off the search kernels' events)
    s.have_search = want_corr;
    if (!device_loop) {   // the host loop: the sums come home
        int rc = queue_final_reduce(ctx, ctx->d_partials.as<double>(), reduce_blocks(n), RSREG_NUM_SUMS);
        if (rc) return rc;
        return fetch_sums(ctx, sums, RSREG_NUM_SUMS, true);
    }
    // the device loop: the sums stay on the device
    if (!ctx->comm) {   // final reduce + solve in one launch
        auto *st = ctx->d_icp_state.as<IcpDevState>();
        k_final_reduce_solve<<<RSREG_NUM_SUMS, kReduceBlock, 0, ctx->stream>>>(ctx->d_partials.as<double>(), reduce_blocks(n), ctx->d_sums.as<double>(),
                                                                          st, reinterpret_cast<unsigned int *>(st + 1));
        RSREG_HIP(ctx, hipGetLastError());
        return RSREG_OK;
    }
    k_final_reduce<<<RSREG_NUM_SUMS, kReduceBlock, 0, ctx->stream>>>(ctx->d_partials.as<double>(), reduce_blocks(n), ctx->d_sums.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    {   // all-reduce, solve, next pass
        ScopedEvents ev(ctx, &ctx->ev_allreduce);
        int rc = rsreg_comm_allreduce_device_(ctx, ctx->d_sums.as<double>(), RSREG_NUM_SUMS);
        if (rc) return rc;
    }
    k_icp_solve<<<1, 64, 0, ctx->stream>>>(ctx->d_sums.as<double>(), ctx->d_icp_state.as<IcpDevState>());
    RSREG_HIP(ctx, hipGetLastError());
    return RSREG_OK;
}

// RSREG_PIPELINE_DEVICE_LOOP with fixed-count criteria: every iteration is queued up front, the
// 136-byte state comes back once at the end.  Same kernels, same arithmetic as the host loop.
int run_device_loop(rsreg_ctx *ctx)
{
    IcpState &s = ctx->icp;
    RSREG_HIP(ctx, ctx->d_icp_state.reserve(sizeof(IcpDevState) + 16));   // + the reduce kernel's ticket
    RSREG_HIP(ctx, ctx->h_sums.reserve(1024));
    IcpDevState *h = ctx->h_sums.as<IcpDevState>();
    std::memset(h, 0, sizeof(IcpDevState) + 16);
    h->t_inc = to_mat34(Mat4f::identity());
    h->final_t = s.final_t;
    for (int k = 0; k < 9; ++k) h->svd_v[k] = (k % 4 == 0) ? 1.0 : 0.0;
    const auto t_q0 = std::chrono::steady_clock::now();
    RSREG_HIP(ctx, hipMemcpyAsync(ctx->d_icp_state.ptr, h, sizeof(IcpDevState) + 16, hipMemcpyHostToDevice, ctx->stream));
    const int iters = std::max(1, s.prm.max_iterations);
    int it = 0;
    for (; it < iters; ++it) {
        int rc = launch_fused(ctx, nullptr, false, true);
        if (rc) return rc;
    }
    RSREG_HIP(ctx, hipMemcpyAsync(h, ctx->d_icp_state.ptr, sizeof(IcpDevState), hipMemcpyDeviceToHost, ctx->stream));
    // (what queueing the whole loop took this thread: with several alignments in flight the threads share the runtime's launch path)
    ctx->host_timing.loop_enqueue = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_q0).count();
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s.idle_after_sums = true;
    (void)target_counts(ctx, false);
    std::memcpy(s.sums_last, h->sums_last, sizeof(s.sums_last));
    s.ncorr = h->ncorr;
    s.final_t = h->final_t;
    s.iterations = h->iterations;
    s.cur_mse = h->cur_mse;
    s.pending_transform = h->apply != 0;
    for (int c = 0; c < 4; ++c) { s.t_inc(0, c) = h->t_inc.r0[c]; s.t_inc(1, c) = h->t_inc.r1[c]; s.t_inc(2, c) = h->t_inc.r2[c]; }
    if (h->stopped) {
        s.state = RSREG_CONV_NO_CORRESPONDENCES;
        s.converged = 0;
    } else {
        s.state = RSREG_CONV_ITERATIONS;
        s.converged = 1;
    }
    return RSREG_OK;
}

int apply_pending_transform(rsreg_ctx *ctx)
{
    ctx->icp.idle_after_sums = false;   // (something is queued on the main stream from here on)
    IcpState &s = ctx->icp;
    {
        int rcr = ensure_restarted(ctx);
        if (rcr) return rcr;
    }
    if (!s.pending_transform) return RSREG_OK;
    const uint32_t n = (uint32_t)ctx->n_work;
    if (n) {
        ScopedEvents ev(ctx, &ctx->ev_transform);
        k_transform<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), n, to_mat34(s.t_inc));
        RSREG_HIP(ctx, hipGetLastError());
    }
    if (s.chain.has(RSREG_REJECTOR_SURFACE_NORMAL) && ctx->n_source) {   // the source's normals turn with it
        int rcn = ensure_normals_restarted(ctx);
        if (rcn) return rcn;
        k_rotate_normals<<<div_up((uint32_t)ctx->n_source, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_src_nrm_cur.as<float4>(), (uint32_t)ctx->n_source, to_mat34(s.t_inc));
        RSREG_HIP(ctx, hipGetLastError());
    }
    s.pending_transform = false;
    return RSREG_OK;
}

// result->sums_last of an iteration whose sums are not the 17 (point-to-plane, GICP): the layout stays, [0] the pairs and [16]
// their squared error are filled
void fill_sums_last(IcpState &s, double n, double err)
{
    std::memset(s.sums_last, 0, sizeof(s.sums_last));
    s.sums_last[0] = n;
    s.sums_last[16] = err;
}

// counts an iteration's pairs; true: fewer than the estimator's minimum, the alignment ends here without a transform
bool too_few_pairs(IcpState &s, double n, uint64_t min_pairs, int *done)
{
    s.ncorr = (uint64_t)(n + 0.5);
    if (s.ncorr >= min_pairs) return false;
    s.state = RSREG_CONV_NO_CORRESPONDENCES;
    s.converged = 0;
    *done = 1;
    return true;
}

// One iteration's update from its (global) sums, of which `n` is the number of pairs and `err` their squared error:
// solve(s) leaves the increment in s.t_inc, then compose + criteria; the transform of the source cloud itself is left
// pending so that the fused kernel can fold it into its pass.  (The caller has recorded the sums.)
template <typename Solve>
int update_with(rsreg_ctx *ctx, double n, double err, int *done, Solve solve)
{
    IcpState &s = ctx->icp;
    if (too_few_pairs(s, n, 3, done)) return RSREG_OK;   // min_number_correspondences_
    solve(s);
    s.pending_transform = true;
    s.final_t = mul(s.t_inc, s.final_t);
    s.iterations++;
    s.cur_mse = err / n;
    s.converged = criteria_has_converged(s) ? 1 : 0;
    s.have_search = false;
    *done = s.converged;
    return RSREG_OK;
}

// the 17 sums: Umeyama
int update_from_sums(rsreg_ctx *ctx, const double *sums, int *done)
{
    std::memcpy(ctx->icp.sums_last, sums, sizeof(ctx->icp.sums_last));
    return update_with(ctx, sums[0], sums[16], done, [sums](IcpState &s) { umeyama_from_sums(sums, s.t_inc, s.svd_v); });
}

// one point-to-plane iteration's 32 sums: TransformationEstimationPointToPlaneLLS (host_linalg.hpp: plane_solve_from_sums)
int update_from_plane_sums(rsreg_ctx *ctx, const double *sums, int *done)
{
    std::memcpy(ctx->icp.plane_sums_last, sums, sizeof(ctx->icp.plane_sums_last));
    fill_sums_last(ctx->icp, sums[0], sums[1]);
    return update_with(ctx, sums[0], sums[1], done, [sums](IcpState &s) { plane_solve_from_sums(sums, s.t_inc); });
}

// A host cloud on its way into HBM, packed xyz (PCL's ICP reads nothing else of a point): the caller's records are
// packed into pinned memory piece by piece (the pool of host threads, workers.hpp) and every piece goes over the PCIe link
// on the context's upload stream while the next one is being packed; `stage` / `ev`: the staging buffer of this kind of
// cloud (source / target: one each, so that the target is packed while the source is still on the link) and the event behind
// its last piece.  The stream `waiter` is made to wait for that event; the caller's buffer has been read when this returns.
int upload_packed(rsreg_ctx *ctx, PinnedBuf &stage, const Event &ev, DevBuf &d_raw, const void *points, size_t n, size_t stride,
                  hipStream_t waiter, double *ms_pack, double *ms_wait)
{
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    RSREG_HIP(ctx, ctx->h2d.ensure());
    RSREG_HIP(ctx, hipEventSynchronize(ev));   // (the staging buffer's last trip over the link is over; at once if it has made none)
    const auto t1 = clk::now();
    RSREG_HIP(ctx, stage.reserve(n * 12 + 16));
    RSREG_HIP(ctx, d_raw.reserve(n * 12 + 16));
    float *dst = stage.as<float>();
    const char *src = static_cast<const char *>(points);
    const size_t piece = (size_t)1 << 18;   // 3 MB of packed xyz: ~0.1 ms on the link
    for (size_t lo = 0; lo < n; lo += piece) {
        const size_t hi = std::min(n, lo + piece);
        host_parallel_for(hi - lo, [=](size_t a, size_t b) {
            if (stride == 12) {
                std::memcpy(dst + 3 * (lo + a), src + 12 * (lo + a), (b - a) * 12);
            } else {
                for (size_t i = lo + a; i < lo + b; ++i) std::memcpy(dst + 3 * i, src + i * stride, 12);
            }
        });
        RSREG_HIP(ctx, hipMemcpyAsync(d_raw.as<char>() + lo * 12, dst + 3 * lo, (hi - lo) * 12, hipMemcpyHostToDevice, ctx->h2d.stream));
    }
    RSREG_HIP(ctx, hipEventRecord(ev, ctx->h2d.stream));
    RSREG_HIP(ctx, hipStreamWaitEvent(waiter, ev, 0));
    const auto t2 = clk::now();
    if (ms_wait) *ms_wait = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (ms_pack) *ms_pack = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return RSREG_OK;
}

// One normal per record of the source (the target), three floats at normals + i * stride.  on_host: a host buffer, staged like
// the cloud itself -- packed into pinned memory of its own, over the link on the upload stream, the main stream behind it;
// otherwise records already in HBM, read on the context's stream.
int set_record_normals(rsreg_ctx *ctx, bool source, bool on_host, const void *normals, size_t n, size_t stride)
{
    if (!ctx || (n && !normals) || stride < 12 || (!on_host && (stride & 3))) return RSREG_ERR_INVALID_ARG;
    if (source) {
        if (!ctx->have_source) return fail(ctx, RSREG_ERR_NO_SOURCE, "rsreg_icp_set_source not called");
        if (n != ctx->n_source) return fail(ctx, RSREG_ERR_INVALID_ARG, "one normal per source record: the counts differ");
    } else {
        if (!ctx->have_target) return fail(ctx, RSREG_ERR_NO_TARGET, "rsreg_icp_set_target not called");
        if (n != ctx->n_target_raw) return fail(ctx, RSREG_ERR_INVALID_ARG, "one normal per target record: the counts differ");
    }
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    RecordNormals &r = source ? ctx->src_nrm : ctx->tgt_nrm;
    const char *d_rec = static_cast<const char *>(normals);
    if (on_host) {
        RSREG_HIP(ctx, ctx->h2d.ensure());
        RSREG_HIP(ctx, r.ev.ensure());
        RSREG_HIP(ctx, r.ev_packed.ensure());
        RSREG_HIP(ctx, hipStreamWaitEvent(ctx->h2d.stream, r.ev_packed, 0));   // (normals set before may still be read from d_raw)
        int rc = upload_packed(ctx, r.h, r.ev, r.d_raw, normals, n, stride, ctx->stream, nullptr, nullptr);
        if (rc) return rc;
        d_rec = r.d_raw.as<char>();
        stride = 12;
    }
    RSREG_HIP(ctx, r.d.reserve((n + 1) * sizeof(float4)));
    if (n) {
        k_pack_normals<<<div_up((uint32_t)n, kBlock), kBlock, 0, ctx->stream>>>(d_rec, stride, (uint32_t)n, r.d.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    r.have = true;
    if (on_host) RSREG_HIP(ctx, hipEventRecord(r.ev_packed, ctx->stream));
    return RSREG_OK;
}

// rsreg_icp_begin; need_index: the alignment runs the staged kernels over the index whatever the source's size (plane mode, GICP)
int icp_begin(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params, bool need_index, bool use_chain)
{
    if (!ctx || !params) return RSREG_ERR_INVALID_ARG;
    if (!ctx->have_target) return fail(ctx, RSREG_ERR_NO_TARGET, "rsreg_icp_set_target not called");
    if (!ctx->have_source) return fail(ctx, RSREG_ERR_NO_SOURCE, "rsreg_icp_set_source not called");
    if (params->max_iterations < 0 || !(params->max_correspondence_distance >= 0))
        return fail(ctx, RSREG_ERR_INVALID_ARG, "bad ICP parameters");
    if (params->max_correspondence_distance > ctx->gate_built_for)
        return fail(ctx, RSREG_ERR_INVALID_ARG, "max_correspondence_distance exceeds the one the target index was built for");
    // the filters need the whole source: each rank would trim its own block with its own cut and index only its own block for
    // the reciprocal search, a different answer from one GPU's (a global trim across ranks is not implemented)
    if (ctx->nranks > 1 && filters_on(*params))
        return fail(ctx, RSREG_ERR_INVALID_ARG, "reciprocal correspondences and the trimmed rejector need the whole source: not with more than one rank");
    const RejectorChain chain = use_chain ? ctx->rejectors : RejectorChain();
    if (ctx->nranks > 1 && chain.n > 0)
        return fail(ctx, RSREG_ERR_INVALID_ARG, "a rejector chain needs the whole source: not with more than one rank");
    if (chain.has(RSREG_REJECTOR_SURFACE_NORMAL) && !(ctx->tgt_nrm.have && ctx->src_nrm.have))
        return fail(ctx, RSREG_ERR_STATE, "the surface normal rejector needs rsreg_icp_set_source_normals and rsreg_icp_set_target_normals after the clouds are set");
    if (params->estimation != RSREG_ESTIMATION_SVD && params->estimation != RSREG_ESTIMATION_POINT_TO_PLANE_LLS)
        return fail(ctx, RSREG_ERR_INVALID_ARG, "unknown transformation estimation");
    if (plane_on(*params)) {
        // (the all-reduce of the 32 sums is not implemented, as a global trim is not)
        if (ctx->nranks > 1) return fail(ctx, RSREG_ERR_INVALID_ARG, "point-to-plane ICP: not with more than one rank");
        if (!ctx->tgt_nrm.have) return fail(ctx, RSREG_ERR_STATE, "point-to-plane ICP needs rsreg_icp_set_target_normals after rsreg_icp_set_target");
    }
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    {
        int rcj = join_source(ctx);
        if (rcj) return rcj;
    }
    if (ctx->grid.dense == 2 && (ctx->n_work > kScanMaxSource || filters_on(*params) || chain.n > 0 || need_index)) {
        // the target was set for a handful of queries (scan_target); this alignment needs the index after all
        if (!ctx->scan_raw) return fail(ctx, RSREG_ERR_NO_TARGET, "the target cloud was released before its index was built");
        int rcb = build_grid(ctx, ctx->scan_raw, ctx->n_target_raw, ctx->scan_stride, ctx->gate_built_for);
        if (rcb) return rcb;
    }
    IcpState &s = ctx->icp;
    s = IcpState();
    s.prm = *params;
    s.chain = chain;
    s.normals_restart_pending = chain.has(RSREG_REJECTOR_SURFACE_NORMAL);
    // the rings must cover THIS call's gate (it may be smaller than the one built for)
    s.final_t = Mat4f::identity();
    if (guess) std::memcpy(s.final_t.m, guess, sizeof(s.final_t.m));
    s.t_inc = Mat4f::identity();
    s.prev_mse = DBL_MAX;
    s.active = 1;
    ctx->ev_used = 0;
    ctx->ev_nn.clear();
    ctx->ev_reduce.clear();
    ctx->ev_transform.clear();
    ctx->ev_allreduce.clear();
    s.restart_pending = true;   // input_transformed = guess * input (App. A.2 prologue): ensure_restarted / launch_fused
    ctx->gicp.active = 0;
    return RSREG_OK;
}

// rsreg_icp_end.  source_records (nullable): the caller's source records, out_stride bytes each -- every record of aligned_out is
// then the WHOLE source record with xyz rewritten (what PCL's align(output) leaves: output = input, then xyz <- final * xyz),
// copied by the host threads that write the aligned positions anyway
int icp_end(rsreg_ctx *ctx, rsreg_icp_result *result, void *aligned_out, size_t out_stride, const void *source_records)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    IcpState &s = ctx->icp;
    if (!s.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_begin not called");
    const size_t n = ctx->n_source;
    if (aligned_out && n) {
        if (out_stride < 12) return RSREG_ERR_INVALID_ARG;
        RSREG_HIP(ctx, ctx->d_tmp.reserve(n * 12 + 16));
        RSREG_HIP(ctx, ctx->h_stage.reserve(n * 12 + 16));
        k_apply_final<<<div_up((uint32_t)n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_src_all.as<float4>(), (uint32_t)n, to_mat34(s.final_t),
                                                                                ctx->d_perm.as<uint32_t>(), ctx->d_tmp.as<float>());
        RSREG_HIP(ctx, hipGetLastError());
        // home in pieces: while piece k + 1 is on the link, piece k is written into the caller's records by the host's threads
        const auto t0 = std::chrono::steady_clock::now();
        const size_t piece = (size_t)1 << 18;
        const size_t pieces = (n + piece - 1) / piece;
        while (ctx->ev_home.size() < pieces) {
            Event e;
            RSREG_HIP(ctx, e.ensure());
            ctx->ev_home.push_back(std::move(e));
        }
        for (size_t k = 0; k < pieces; ++k) {
            const size_t lo = k * piece, hi = std::min(n, lo + piece);
            RSREG_HIP(ctx, hipMemcpyAsync(ctx->h_stage.as<char>() + lo * 12, ctx->d_tmp.as<char>() + lo * 12, (hi - lo) * 12, hipMemcpyDeviceToHost, ctx->stream));
            RSREG_HIP(ctx, hipEventRecord(ctx->ev_home[k], ctx->stream));
        }
        const float *src = ctx->h_stage.as<float>();
        char *dst = static_cast<char *>(aligned_out);
        const char *rec = static_cast<const char *>(source_records);
        // (the caller's records first, all of them, while the positions are still on the link: the positions then land in lines
        // the cores already own)
        // (icp_align has started that copy on a thread of its own, beside the iterations: it ends here)
        if (ctx->records_copy.joinable()) ctx->records_copy.join();
        else if (rec && rec != dst)
            host_parallel_for(n, [=](size_t a, size_t b) { std::memcpy(dst + a * out_stride, rec + a * out_stride, (b - a) * out_stride); });
        for (size_t k = 0; k < pieces; ++k) {
            const size_t lo = k * piece, hi = std::min(n, lo + piece);
            RSREG_HIP(ctx, hipEventSynchronize(ctx->ev_home[k]));
            host_parallel_for(hi - lo, [=](size_t a, size_t b) {
                const float one = 1.0f;
                for (size_t i = lo + a; i < lo + b; ++i) {
                    std::memcpy(dst + i * out_stride, src + 3 * i, 12);
                    if (out_stride >= 16) std::memcpy(dst + i * out_stride + 12, &one, 4);
                }
            });
        }
        ctx->host_timing.aligned_copy = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // (the usual end of an alignment: the last thing this thread did was wait for the sums, and nothing has been queued since)
    if (!(s.idle_after_sums && !(aligned_out && n))) RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)target_counts(ctx, false);
#ifdef RSREG_DIAG
    if (const char *sd_path = tunables().dump_seed) {   // dev: the position every query matched last, and the queries
        const size_t nq = ctx->n_work;
        std::vector<int> h(nq);
        std::vector<float> hq(nq * 4);
        (void)hipMemcpy(h.data(), ctx->d_seed.ptr, nq * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hq.data(), ctx->d_cur.ptr, nq * 16, hipMemcpyDeviceToHost);
        if (FILE *f = std::fopen(sd_path, "wb")) {
            std::fwrite(h.data(), 4, nq, f);
            std::fwrite(hq.data(), 4, nq * 4, f);
            const size_t np_ = ctx->grid.n_points;
            std::vector<float> hp(np_ * 4);
            (void)hipMemcpy(hp.data(), ctx->d_tgt_sorted.ptr, np_ * 16, hipMemcpyDeviceToHost);
            std::fwrite(hp.data(), 4, np_ * 4, f);
            std::fclose(f);
        }
    }
    if (const char *wt_path = tunables().wave_times) {
        if (ctx->grid.dense == 1 && ctx->n_work) {
            const bool light = tunables().wave_times_light;
            const size_t nw = light ? (size_t)(ctx->icp.sched.ready ? ctx->icp.sched.items : reduce_blocks(ctx->n_work)) * kTileWaves
                                    : (ctx->n_work + 63) / 64;
            std::vector<unsigned long long> h(16 * nw + (light ? 0 : (ctx->n_work + 1) / 2));   // wave records, then a uint32 of step counts per lane
            (void)hipMemcpy(h.data(), ctx->d_brick.ptr, h.size() * 8, hipMemcpyDeviceToHost);
            if (FILE *f = std::fopen(wt_path, "wb")) {
                std::fwrite(h.data(), 8, h.size(), f);
                std::fclose(f);
            }
        }
    }
#endif
    if (result) {
        std::memset(result, 0, sizeof(*result));
        std::memcpy(result->transform, s.final_t.m, 64);
        result->converged = s.converged;
        result->state = s.state;
        result->iterations = s.iterations;
        result->n_correspondences = s.ncorr;
        result->mse = s.cur_mse;
        std::memcpy(result->sums_last, s.sums_last, sizeof(s.sums_last));
        result->n_nn_launches = s.n_nn_launches;
        result->n_scheduled_launches = s.n_sched_launches;
        if (ctx->profiling) {
            result->ms_nn = sum_events(ctx, ctx->ev_nn);
#ifdef RSREG_DIAG
            if (tunables().dump_nn_ms) {   // diagnostic builds: duration of every search launch of this call
                std::fprintf(stderr, "[rsreg] search launches (us):");
                for (auto &p : ctx->ev_nn) {
                    float t = 0;
                    (void)hipEventElapsedTime(&t, ctx->ev_pool[p.first], ctx->ev_pool[p.second]);
                    std::fprintf(stderr, " %.1f", t * 1e3);
                }
                std::fprintf(stderr, "\n");
            }
#endif
            result->ms_reduce = sum_events(ctx, ctx->ev_reduce);
            if (ctx->ev_reduce.empty())   // fused pipelines: everything between two consecutive search kernels
                for (size_t k = 0; k + 1 < ctx->ev_nn.size(); ++k) {
                    float t = 0;
                    if (hipEventElapsedTime(&t, ctx->ev_pool[ctx->ev_nn[k].second], ctx->ev_pool[ctx->ev_nn[k + 1].first]) == hipSuccess)
                        result->ms_reduce += t;
                }
            result->ms_transform = sum_events(ctx, ctx->ev_transform);
            result->ms_allreduce = sum_events(ctx, ctx->ev_allreduce);   // (already inside ms_reduce in the fused pipelines)
            result->ms_total = result->ms_nn + result->ms_reduce + result->ms_transform;
        }
    }
    s.active = 0;
    ctx->icp_fit_ok = true;   // getFitnessScore: this alignment's source, final transform and target
    ctx->icp_fit_t = s.final_t;
    return RSREG_OK;
}

// rsreg_icp_align / rsreg_icp_align_records: begin, the iterations of the pipeline the parameters choose, end
int icp_align(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params, rsreg_icp_result *result, void *aligned_out, size_t out_stride,
              const void *source_records)
{
    const auto t_align0 = std::chrono::steady_clock::now();
    struct AlignClock {   // (whatever way the call ends: begin .. the last iteration + the aligned cloud's way home)
        rsreg_ctx *c;
        std::chrono::steady_clock::time_point t0;
        ~AlignClock() { if (c) c->host_timing.align = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - c->host_timing.aligned_copy; }
    } align_clock{ctx, t_align0};
    if (ctx) ctx->host_timing.aligned_copy = 0;
    // `output = input`: the caller's records go into the output on a thread of their own (the pool's threads under it) while this
    // thread queues and waits for the iterations; icp_end joins it before the aligned positions are written over the records
    struct CopyGuard {   // (an error on the way: the copy still owns aligned_out)
        rsreg_ctx *c;
        ~CopyGuard() { if (c && c->records_copy.joinable()) c->records_copy.join(); }
    } copy_guard{ctx};
    if (ctx && source_records && aligned_out && source_records != aligned_out && ctx->n_source && out_stride >= 12) {
        const size_t n_rec = ctx->n_source;
        const char *rec = static_cast<const char *>(source_records);
        char *dst = static_cast<char *>(aligned_out);
        ctx->records_copy = std::thread([=] {
            host_parallel_for(n_rec, [=](size_t a, size_t b) { std::memcpy(dst + a * out_stride, rec + a * out_stride, (b - a) * out_stride); });
        });
    }
    int rc = rsreg_icp_begin(ctx, guess, params);
    if (rc) return rc;
    int done = 0;
    double sums[RSREG_NUM_PLANE_SUMS];   // (the 17 of a point-to-point iteration, or the 32 of a point-to-plane one)
    const bool plane = plane_on(*params);     // point-to-plane: staged, with its own sums and solve
    const bool filtered = weights_on(ctx) || plane;   // the optional correspondence filters and the rejector chain run between the staged kernels
    const bool scan = ctx->grid.dense == 2;   // no index: the staged kernels (search over the whole target, sums)
    const bool fused = !filtered && !scan && (params->pipeline_mode == RSREG_PIPELINE_FUSED || params->pipeline_mode == RSREG_PIPELINE_DEVICE_LOOP);
    if (!filtered && !scan && params->pipeline_mode == RSREG_PIPELINE_DEVICE_LOOP && params->criteria_mode == RSREG_CRITERIA_FIXED) {
        rc = run_device_loop(ctx);
        if (rc) return rc;
        done = 1;
    }
    while (!done) {
        if (fused) {
            rc = launch_fused(ctx, sums, false);
        } else {
            rc = apply_pending_transform(ctx);
            if (!rc) rc = launch_search(ctx);
            if (!rc) rc = plane ? launch_plane_sums(ctx, sums) : launch_sums(ctx, sums, true);
        }
        if (rc) return rc;
        rc = plane ? update_from_plane_sums(ctx, sums, &done) : update_from_sums(ctx, sums, &done);
        if (rc) return rc;
    }
    return icp_end(ctx, result, aligned_out, out_stride, source_records);
}

// ---- GICP's helpers (the ABI's GICP section below says what an outer iteration is)
static_assert(RSREG_NUM_GICP_SUMS == RSREG_NUM_PLANE_SUMS, "k_gicp_reduce goes through plane_tile_reduce_store and k_final_reduce as the plane sums do");

// one covariance record per record of the source (the target): from the host (waited for: the buffer has been read) or from HBM
int gicp_set_covariances(rsreg_ctx *ctx, bool source, const void *host, const void *dev, size_t n, size_t stride)
{
    if (!ctx || (n && !host && !dev) || stride < 48 || (dev && (stride & 7))) return RSREG_ERR_INVALID_ARG;
    if (source) {
        if (!ctx->have_source) return fail(ctx, RSREG_ERR_NO_SOURCE, "rsreg_icp_set_source not called");
        if (n != ctx->n_source) return fail(ctx, RSREG_ERR_INVALID_ARG, "one covariance per source record: the counts differ");
    } else {
        if (!ctx->have_target) return fail(ctx, RSREG_ERR_NO_TARGET, "rsreg_icp_set_target not called");
        if (n != ctx->n_target_raw) return fail(ctx, RSREG_ERR_INVALID_ARG, "one covariance per target record: the counts differ");
    }
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf &d = source ? ctx->d_gicp_cs : ctx->d_gicp_ct;
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (an alignment before this one may still read the buffer)
    RSREG_HIP(ctx, d.reserve((n + 1) * 48));
    if (n && host) {
        RSREG_HIP(ctx, hipMemcpy2DAsync(d.ptr, 48, host, stride, 48, n, hipMemcpyHostToDevice, ctx->stream));
        RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else if (n) {
        k_gicp_pack_cov<<<div_up((uint32_t)n, kBlock), kBlock, 0, ctx->stream>>>(static_cast<const char *>(dev), stride, (uint32_t)n, d.as<double>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    (source ? ctx->have_gicp_cs : ctx->have_gicp_ct) = true;
    return RSREG_OK;
}

// GICP6D: one colour per record of the source (the target), three floats L', a', b' at the head of a record: from the host (waited
// for: the buffer has been read) or from HBM.  The source: a load that merged exact copies is taken apart again (k_source_unmerge).
// The target: the x, y, z of its records are taken over beside the colours -- the 6-D index is built from them (gicp6d_prepare).
int gicp_set_lab(rsreg_ctx *ctx, bool source, const void *host, const void *dev, size_t n, size_t stride)
{
    if (!ctx || (n && !host && !dev) || stride < 12 || (dev && (stride & 3))) return RSREG_ERR_INVALID_ARG;
    if (source) {
        if (!ctx->have_source) return fail(ctx, RSREG_ERR_NO_SOURCE, "rsreg_icp_set_source not called");
        if (n != ctx->n_source) return fail(ctx, RSREG_ERR_INVALID_ARG, "one colour per source record: the counts differ");
    } else {
        if (!ctx->have_target) return fail(ctx, RSREG_ERR_NO_TARGET, "rsreg_icp_set_target not called");
        if (n != ctx->n_target_raw) return fail(ctx, RSREG_ERR_INVALID_ARG, "one colour per target record: the counts differ");
        if (n && !ctx->tgt_rec) return fail(ctx, RSREG_ERR_STATE, "the target cloud's records have changed hands since rsreg_icp_set_target_cloud");
    }
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    if (source) {
        int rcj = join_source(ctx);
        if (rcj) return rcj;
    }
    DevBuf &d = source ? ctx->d_lab_s : ctx->d_lab_t;
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (an alignment before this one may still read the buffer)
    RSREG_HIP(ctx, d.reserve((n + 1) * sizeof(float4)));
    const uint32_t nb = div_up((uint32_t)n, kBlock);
    if (n && host) {
        RSREG_HIP(ctx, hipMemsetAsync(d.ptr, 0, n * sizeof(float4), ctx->stream));
        RSREG_HIP(ctx, hipMemcpy2DAsync(d.ptr, sizeof(float4), host, stride, 12, n, hipMemcpyHostToDevice, ctx->stream));
        RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else if (n) {
        k_nn6_pack3<<<nb, kBlock, 0, ctx->stream>>>(static_cast<const char *>(dev), stride, (uint32_t)n, d.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    if (source) {
        if (n && !ctx->src_plain && !ctx->src_unmerged) {
            k_source_unmerge<<<nb, kBlock, 0, ctx->stream>>>(ctx->d_src_all.as<float4>(), (uint32_t)n, ctx->d_src.as<float4>(), ctx->d_uniq_of.as<uint32_t>(),
                                                             ctx->d_first.as<uint32_t>());
            RSREG_HIP(ctx, hipGetLastError());
            ctx->n_work = n;
            ctx->src_unmerged = true;
        }
        ctx->have_lab_s = true;
    } else {
        RSREG_HIP(ctx, ctx->d_t6_xyz.reserve((n + 1) * sizeof(float4)));
        if (n) {
            k_nn6_pack3<<<nb, kBlock, 0, ctx->stream>>>(ctx->tgt_rec, ctx->tgt_rec_stride, (uint32_t)n, ctx->d_t6_xyz.as<float4>());
            RSREG_HIP(ctx, hipGetLastError());
            // exact 6-D copies of a record of lower index stay out of the index (nn6_kernels.hpp): a hash set at most half full
            uint32_t slots = 1024;
            while (slots < 2 * n && slots < 0x80000000u) slots <<= 1;
            if (slots < 2 * n) return fail(ctx, RSREG_ERR_INVALID_ARG, "GICP6D: target too large");
            RSREG_HIP(ctx, ctx->d_tmp.reserve((size_t)slots * 4));
            uint32_t *table = ctx->d_tmp.as<uint32_t>();
            RSREG_HIP(ctx, hipMemsetAsync(table, 0xff, (size_t)slots * 4, ctx->stream));
            k_nn6_copies_insert<<<nb, kBlock, 0, ctx->stream>>>(ctx->d_t6_xyz.as<float4>(), d.as<float4>(), (uint32_t)n, table, slots - 1u);
            RSREG_HIP(ctx, hipGetLastError());
            k_nn6_copies_drop<<<nb, kBlock, 0, ctx->stream>>>(ctx->d_t6_xyz.as<float4>(), d.as<float4>(), (uint32_t)n, table, slots - 1u);
            RSREG_HIP(ctx, hipGetLastError());
        }
        ctx->g6_built = false;
        ctx->have_lab_t = true;
    }
    return RSREG_OK;
}

// what rsreg_gicp6d_begin adds to rsreg_gicp_begin: the 6-D index over every finite target record (once per target and colours) and
// the two sides' colours times w (every begin: w is the call's)
int gicp6d_prepare(rsreg_ctx *ctx, float w)
{
    hipStream_t st = ctx->stream;
    const uint32_t nt = (uint32_t)ctx->n_target_raw, n = (uint32_t)ctx->n_work;
    if (!ctx->g6_built) {
        RSREG_HIP(ctx, ctx->h_g6.reserve(64));
        const Xyz4Records rd{ctx->d_t6_xyz.as<float4>()};
        PointGrid &gx = ctx->g6;
        int rc = grid_build_placed<FitGridPolicy>(ctx, gx, rd, nt, 1, ctx->h_g6.as<uint32_t>(), 0.0, [&](const PointGridDev &g, uint32_t *start, uint32_t *count, size_t) {
            k_nn6_scatter<<<div_up(nt, kBlock), kBlock, 0, st>>>(rd, nt, g, start, count, gx.d_pts.as<float4>());
            RSREG_HIP(ctx, hipGetLastError());
            return (int)RSREG_OK;
        });
        if (rc) return rc;
        ctx->g6_built = true;
    }
    const uint32_t np = ctx->g6.dims[0] ? ctx->g6.n_points : 0u;
    RSREG_HIP(ctx, ctx->d_g6_col.reserve(((size_t)np + 1) * sizeof(float4)));
    RSREG_HIP(ctx, ctx->d_src6_col.reserve(((size_t)n + 1) * sizeof(float4)));
    if (np) {
        k_nn6_target_colours<<<div_up(np, kBlock), kBlock, 0, st>>>(ctx->g6.d_pts.as<float4>(), np, ctx->d_lab_t.as<float4>(), w, ctx->d_g6_col.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    if (n) {
        k_nn6_source_colours<<<div_up(n, kBlock), kBlock, 0, st>>>(ctx->d_perm.as<uint32_t>(), ctx->d_first.as<uint32_t>(), n, ctx->d_lab_s.as<float4>(), w,
                                                                  ctx->d_src6_col.as<float4>());
        RSREG_HIP(ctx, hipGetLastError());
    }
    return RSREG_OK;
}

// the 32 sums at X (column-major double 4 x 4) over the pairs of the last search: launch_plane_sums with k_gicp_reduce
int gicp_launch_sums(rsreg_ctx *ctx, const double *X, double *sums)
{
    ctx->icp.idle_after_sums = false;
    const uint32_t n = (uint32_t)ctx->n_work;
    const uint32_t nb = reduce_blocks(n);
    RSREG_HIP(ctx, ctx->d_plane_partials.reserve((size_t)nb * RSREG_NUM_GICP_SUMS * 8));
    Mat34d Xr;
    for (int c = 0; c < 4; ++c) {
        Xr.r0[c] = X[c * 4 + 0];
        Xr.r1[c] = X[c * 4 + 1];
        Xr.r2[c] = X[c * 4 + 2];
    }
    {
        ScopedEvents ev(ctx, &ctx->ev_reduce);
        k_gicp_reduce<<<nb, kTile, 0, ctx->stream>>>(ctx->d_cur.as<float4>(), ctx->d_corr_pos.as<int>(), ctx->d_corr_d2.as<float>(), pair_targets(ctx),
                                                     ctx->d_gicp_m.as<double>(), Xr, n, ctx->d_plane_partials.as<double>());
        RSREG_HIP(ctx, hipGetLastError());
        int rc = queue_final_reduce(ctx, ctx->d_plane_partials.as<double>(), nb, RSREG_NUM_GICP_SUMS);
        if (rc) return rc;
    }
    return fetch_sums(ctx, sums, RSREG_NUM_GICP_SUMS, false);
}

void gicp_identity(double *X)
{
    for (int k = 0; k < 16; ++k) X[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

// C = A B, column-major double 4 x 4, entries ((a0 b0 + a1 b1) + a2 b2) + a3 b3
void gicp_mul(const double *A, const double *B, double *C)
{
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            C[c * 4 + r] = ((A[0 * 4 + r] * B[c * 4 + 0] + A[1 * 4 + r] * B[c * 4 + 1]) + A[2 * 4 + r] * B[c * 4 + 2]) + A[3 * 4 + r] * B[c * 4 + 3];
}

// x = scale * pinv(H) b and D = Delta(x), column-major; the rank of the solve (0: x = 0, D = I)
int gicp_step(const double *sums, double scale, double (&x)[6], double *D)
{
    const int rank = plane_unknowns_from_sums(sums, x);
    gicp_identity(D);
    if (rank == 0) return 0;
    for (int i = 0; i < 6; ++i) x[i] *= scale;
    double d12[12];
    plane_matrix_from_unknowns(x, d12);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) D[c * 4 + r] = d12[r * 4 + c];
    return rank;
}

// ---- getFitnessScore's helpers
// the float bound the search prunes with: never below max_range, so that no d2 with (double)d2 <= max_range is dropped
float fit_limit2(double max_range)
{
    if (!(max_range >= 0)) return -1.0f;   // (negative or NaN: nothing is in range)
    if (max_range >= (double)FLT_MAX) return __builtin_huge_valf();
    float f = (float)max_range;
    if ((double)f < max_range) f = std::nextafter(f, FLT_MAX);
    return f;
}

// this rank's (count, sum of d2) of the last ICP alignment (rsreg_icp_fitness_sums / _score)
int icp_fitness_block(rsreg_ctx *ctx, double max_range, double sums[2])
{
    if (!ctx->icp_fit_ok) return fail(ctx, RSREG_ERR_STATE, "no ICP alignment of the current source and target");
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = join_source(ctx);   // (nothing pending after an alignment; kept for the contract: the source's buffers are final)
    if (rc) return rc;
    rc = target_counts(ctx, true);   // (grid.n_points of a counting build nobody has waited for is only a bound)
    if (rc) return rc;
    const size_t n_tgt = ctx->grid.dense == 2 ? ctx->n_target_raw : ctx->grid.n_points;
    return fitness_sums(ctx, ctx->fit_icp, ctx->d_tgt_sorted.as<float4>(), n_tgt, ctx->d_src_all.as<float4>(), ctx->d_perm.as<uint32_t>(),
                        ctx->n_source, ctx->icp_fit_t, max_range, sums);
}

void fitness_result(const double sums[2], double *score, uint64_t *n_within)
{
    if (score) *score = sums[0] > 0 ? sums[1] / sums[0] : DBL_MAX;
    if (n_within) *n_within = (uint64_t)sums[0];
}

}  // namespace

// getFitnessScore's two sums (rsreg_ctx.hpp holds the contract; ndt.hip's score goes through here too)
int rsreg::fitness_sums(rsreg_ctx *ctx, PointGrid &fx, const float4 *tgt, size_t n_tgt, const float4 *src, const uint32_t *perm, size_t n,
                        const Mat4f &T, double max_range, double sums[2])
{
    hipStream_t st = ctx->stream;
    if (n_tgt > 0xfffffff0ull || n > 0xfffffff0ull) return fail(ctx, RSREG_ERR_INVALID_ARG, "cloud too large");
    if (!fx.built) {   // box (one round trip), counts and occupancy words, prefix sum, scatter: into fx's own buffers
        RSREG_HIP(ctx, ctx->h_fit.reserve(64));
        int rc = grid_build<FitGridPolicy>(ctx, fx, TargetRecords{tgt}, (uint32_t)n_tgt, 1, ctx->h_fit.as<uint32_t>());
        if (rc) return rc;
    }
    sums[0] = sums[1] = 0;
    if (n == 0) return RSREG_OK;
    const uint32_t nb = div_up((uint32_t)n, kBlock);
    RSREG_HIP(ctx, ctx->d_fit_d2.reserve(n * 4 + 16));
    RSREG_HIP(ctx, ctx->d_fit_partials.reserve((size_t)nb * 2 * 8));
    RSREG_HIP(ctx, ctx->d_fit_sums.reserve(64));
    RSREG_HIP(ctx, ctx->h_fit.reserve(64));
    k_fit_search<<<nb, kBlock, 0, st>>>(src, (uint32_t)n, to_mat34(T), perm, grid_dev(fx), fit_limit2(max_range), max_range,
                                        ctx->d_fit_d2.as<float>());
    RSREG_HIP(ctx, hipGetLastError());
    k_fit_tiles<<<nb, kBlock, 0, st>>>(ctx->d_fit_d2.as<float>(), (uint32_t)n, ctx->d_fit_partials.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    k_final_reduce<<<2, kReduceBlock, 0, st>>>(ctx->d_fit_partials.as<double>(), nb, ctx->d_fit_sums.as<double>());
    RSREG_HIP(ctx, hipGetLastError());
    double *h = ctx->h_fit.as<double>();
    RSREG_HIP(ctx, hipMemcpyAsync(h, ctx->d_fit_sums.ptr, 16, hipMemcpyDeviceToHost, st));
    RSREG_HIP(ctx, hipStreamSynchronize(st));
    sums[0] = h[0];
    sums[1] = h[1];
    return RSREG_OK;
}

// =============================================================================== C ABI
extern "C" {

int rsreg_version(void) { return RSREG_VERSION_MAJOR * 1000 + RSREG_VERSION_MINOR; }

const char *rsreg_status_string(int status)
{
    switch (status) {
        case RSREG_OK: return "ok";
        case RSREG_ERR_INVALID_ARG: return "invalid argument";
        case RSREG_ERR_EMPTY_CLOUD: return "empty cloud";
        case RSREG_ERR_HIP: return "HIP error";
        case RSREG_ERR_RCCL: return "RCCL error";
        case RSREG_ERR_NO_TARGET: return "no target set";
        case RSREG_ERR_NO_DEVICE: return "no usable HIP device";
        case RSREG_ERR_ALLOC: return "allocation failed";
        case RSREG_ERR_NO_SOURCE: return "no source set";
        case RSREG_ERR_STATE: return "call out of sequence";
        default: return "unknown status";
    }
}

// (the message is copied under the mutex the context's helper threads report under, into a buffer of the calling thread:
// the pointer stays valid until this thread's next call, whatever the helpers write meanwhile)
const char *rsreg_last_error(const rsreg_ctx *ctx)
{
    if (!ctx) return "null ctx";
    thread_local std::string copy;
    {
        std::lock_guard<std::mutex> lk(const_cast<rsreg_ctx *>(ctx)->error_mutex);
        copy = ctx->last_error;
    }
    return copy.c_str();
}

int rsreg_device_count(int *count)
{
    if (!count) return RSREG_ERR_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return RSREG_OK;
}

int rsreg_ctx_create(int device_id, void *stream, rsreg_ctx **out)
{
    rsreg::tunables_refresh();   // (the switches of csrc/tunables.hpp: as the environment has them now)
    if (!out) return RSREG_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RSREG_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return RSREG_ERR_INVALID_ARG;
    if (hipSetDevice(device_id) != hipSuccess) return RSREG_ERR_NO_DEVICE;
    rsreg_ctx *ctx = new (std::nothrow) rsreg_ctx();
    if (!ctx) return RSREG_ERR_ALLOC;
    ctx->device = device_id;
    if (stream) {
        ctx->stream = static_cast<hipStream_t>(stream);
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            delete ctx;
            return RSREG_ERR_HIP;
        }
        ctx->own_stream = true;
    }
    *out = ctx;
    return RSREG_OK;
}

int rsreg_ctx_destroy(rsreg_ctx *ctx)
{
    if (!ctx) return RSREG_OK;
    (void)hipSetDevice(ctx->device);
    ctx->prep_join();   // (rsreg_ctx_prepare's thread: what it made is released with everything else below)
    // The helper threads go first, in the order of who waits for whom -- a queued side job waits for the upload worker
    // (side_wait_input), an upload or a download for nothing of the others -- and every stream they fed is drained before
    // the context's members release themselves.
    if (ctx->src_worker) ctx->src_worker->shutdown();
    for (auto &w : ctx->side_workers)
        if (w) w->shutdown();
    if (ctx->up.worker) ctx->up.worker->shutdown();
    if (ctx->down.worker) ctx->down.worker->shutdown();
    (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t st : {(hipStream_t)ctx->src.stream, (hipStream_t)ctx->up.stream, (hipStream_t)ctx->down.stream, (hipStream_t)ctx->h2d.stream})
        if (st) (void)hipStreamSynchronize(st);
    for (rsreg_ctx::SideSet &ss : ctx->side_sets)
        if (ss.stream) (void)hipStreamSynchronize(ss.stream);
    rsreg_comm_destroy(ctx);
    if (ctx->recip) rsreg_ctx_destroy(ctx->recip);   // the child context of the reciprocal index runs on this context's stream: it goes first
    cloud_pool_clear(ctx);
    const hipStream_t own = ctx->own_stream ? ctx->stream : nullptr;
    delete ctx;
    if (own) (void)hipStreamDestroy(own);
    return RSREG_OK;
}

int rsreg_ctx_synchronize(rsreg_ctx *ctx)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)target_counts(ctx, false);
    return RSREG_OK;
}

int rsreg_ctx_set_profiling(rsreg_ctx *ctx, int enabled)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    ctx->profiling = enabled != 0;
    return RSREG_OK;
}

void rsreg_icp_params_default(rsreg_icp_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_iterations = 10;
    p->criteria_mode = RSREG_CRITERIA_PCL;
    p->pipeline_mode = RSREG_PIPELINE_FUSED;
    p->max_correspondence_distance = std::sqrt(DBL_MAX);
    p->transformation_epsilon = 0.0;
    p->transformation_rotation_epsilon = 0.0;
    p->euclidean_fitness_epsilon = -DBL_MAX;
}

void rsreg_icp_params_reference(rsreg_icp_params *p)
{
    if (!p) return;
    rsreg_icp_params_default(p);
    p->max_iterations = 100;                 // incremental_icp.hpp:46
    p->max_correspondence_distance = 0.01;   // :47
    p->transformation_epsilon = 1;           // :48
    p->euclidean_fitness_epsilon = 1000;     // :49
}

int rsreg_icp_set_target_device(rsreg_ctx *ctx, const void *d_points, size_t n, size_t stride, int is_dense,
                                double max_correspondence_distance)
{
    (void)is_dense;
    if (!ctx || (n && !d_points) || stride < 12 || (stride & 3)) return RSREG_ERR_INVALID_ARG;
    ctx->tgt_nrm.have = false;   // (of the target before this one)
    ctx->have_gicp_ct = false;
    ctx->have_lab_t = false;
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    return build_grid(ctx, static_cast<const char *>(d_points), n, stride, max_correspondence_distance);
}

// (internal, cloud.hip) a target for the handful of source points already loaded: no index, see scan_target
int rsreg_icp_set_target_scan_(rsreg_ctx *ctx, const void *d_points, size_t n, size_t stride, double max_correspondence_distance)
{
    ctx->tgt_nrm.have = false;
    ctx->have_gicp_ct = false;
    ctx->have_lab_t = false;
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    return scan_target(ctx, static_cast<const char *>(d_points), n, stride, max_correspondence_distance);
}

int rsreg_icp_set_target(rsreg_ctx *ctx, const void *points, size_t n, size_t stride, int is_dense,
                         double max_correspondence_distance)
{
    (void)is_dense;
    if (!ctx || (n && !points) || stride < 12) return RSREG_ERR_INVALID_ARG;
    ctx->tgt_nrm.have = false;   // (of the target before this one)
    ctx->have_gicp_ct = false;
    ctx->have_lab_t = false;
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    rsreg_host_timing &ht = ctx->host_timing;
    // a counting build that was queued and not waited for (build_dense) still reads d_tgt_raw on the main stream, and the
    // upload stream is ordered behind nothing: a second set_target with no alignment in between would overwrite the records
    // under k_cc_count / k_cc_scatter (a changed point re-derives another slot: a write past d_arrived).  Wait for it first.
    int rc = target_counts(ctx, true);
    if (rc) return rc;
    rc = upload_packed(ctx, ctx->h2d.h_tgt, ctx->h2d.ev_tgt, ctx->d_tgt_raw, points, n, stride, ctx->stream, &ht.target_pack, &ht.target_stage_wait);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    rc = build_grid(ctx, ctx->d_tgt_raw.as<char>(), n, 12, max_correspondence_distance);   // (behind the upload, by the stream's order)
    ht.target_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int rsreg_icp_set_source_device(rsreg_ctx *ctx, const void *d_points, size_t n, size_t stride, int is_dense)
{
    (void)is_dense;
    if (!ctx || (n && !d_points) || stride < 12 || (stride & 3)) return RSREG_ERR_INVALID_ARG;
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    return load_source(ctx, static_cast<const char *>(d_points), n, stride);
}

int rsreg_icp_set_source(rsreg_ctx *ctx, const void *points, size_t n, size_t stride, int is_dense)
{
    (void)is_dense;
    if (!ctx || (n && !points) || stride < 12) return RSREG_ERR_INVALID_ARG;
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = join_source(ctx);   // (a load still in flight reads d_src_raw)
    if (rc) return rc;
    // packed and sent piece by piece on the upload stream; the load itself (src.stream, the worker thread) starts behind the
    // event the main stream is made to wait for.  Nothing is waited for here: the caller goes on to rsreg_icp_set_target,
    // whose cloud is packed (into a staging buffer of its own) while this one is on the link and being sorted
    rsreg_host_timing &ht = ctx->host_timing;
    rc = upload_packed(ctx, ctx->h2d.h_src, ctx->h2d.ev_src, ctx->d_src_raw, points, n, stride, ctx->stream, &ht.source_pack, &ht.source_stage_wait);
    if (rc) return rc;
    return load_source(ctx, ctx->d_src_raw.as<char>(), n, 12);
}

int rsreg_icp_begin(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params)
{
    return icp_begin(ctx, guess, params, params && plane_on(*params), true);
}

int rsreg_icp_search(rsreg_ctx *ctx, int32_t *index_out, float *sqr_dist_out)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    if (!ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_begin not called");
    int rc = apply_pending_transform(ctx);
    if (rc) return rc;
    rc = launch_search(ctx);
    if (rc) return rc;
    const size_t n = ctx->n_source;
    if ((index_out || sqr_dist_out) && n) {
        RSREG_HIP(ctx, ctx->d_tmp.reserve(n * 8 + 32));
        int *d_idx = ctx->d_tmp.as<int>();
        float *d_d2 = reinterpret_cast<float *>(d_idx + n);
        // who keeps the match: the records the chain's flags leave, the first cw[u] copies the two filters leave, or every matched point
        const bool by_flags = ctx->icp.chain.n > 0, by_copies = !by_flags && filters_on(ctx->icp.prm);
        auto kern = by_flags ? k_export_corr<CorrKeep::flags> : by_copies ? k_export_corr<CorrKeep::copies> : k_export_corr<CorrKeep::matched>;
        const uint32_t *keep = by_flags ? ctx->d_rej_flags.as<uint32_t>() : by_copies ? ctx->d_corr_w.as<uint32_t>() : nullptr;
        kern<<<div_up((uint32_t)n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_corr_pos.as<int>(), ctx->d_corr_d2.as<float>(), keep, pair_targets(ctx),
                                                                      ctx->d_perm.as<uint32_t>(), ctx->d_uniq_of.as<uint32_t>(), ctx->d_first.as<uint32_t>(), (uint32_t)n,
                                                                      d_idx, d_d2);
        RSREG_HIP(ctx, hipGetLastError());
        if (index_out) RSREG_HIP(ctx, hipMemcpyAsync(index_out, d_idx, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (sqr_dist_out) RSREG_HIP(ctx, hipMemcpyAsync(sqr_dist_out, d_d2, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RSREG_OK;
}

int rsreg_icp_sums(rsreg_ctx *ctx, double sums[RSREG_NUM_SUMS])
{
    if (!ctx || !sums) return RSREG_ERR_INVALID_ARG;
    if (!ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_begin not called");
    if (plane_on(ctx->icp.prm)) return fail(ctx, RSREG_ERR_STATE, "point-to-plane alignment: rsreg_icp_plane_sums");
    if (!ctx->icp.have_search) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_search not called for this iteration");
    return launch_sums(ctx, sums, false);
}

int rsreg_umeyama_from_sums(const double sums[RSREG_NUM_SUMS], float t_out[16])
{
    if (!sums || !t_out) return RSREG_ERR_INVALID_ARG;
    Mat4f T;
    if (!umeyama_from_sums(sums, T)) return RSREG_ERR_INVALID_ARG;
    std::memcpy(t_out, T.m, sizeof(T.m));
    return RSREG_OK;
}

int rsreg_icp_update(rsreg_ctx *ctx, const double sums[RSREG_NUM_SUMS], float *t_inc_out, int *done)
{
    if (!ctx || !sums || !done) return RSREG_ERR_INVALID_ARG;
    if (!ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_begin not called");
    if (plane_on(ctx->icp.prm)) return fail(ctx, RSREG_ERR_STATE, "point-to-plane alignment: rsreg_icp_update_plane");
    int rc = update_from_sums(ctx, sums, done);
    if (rc) return rc;
    if (t_inc_out) std::memcpy(t_inc_out, ctx->icp.t_inc.m, 64);
    return RSREG_OK;
}

// ---- the records' normals (set_record_normals); the _device_ entries are internal (cloud.hip: rsreg_icp_set_*_normals_cloud)
int rsreg_icp_set_target_normals(rsreg_ctx *ctx, const void *normals, size_t n, size_t stride) { return set_record_normals(ctx, false, true, normals, n, stride); }
int rsreg_icp_set_target_normals_device_(rsreg_ctx *ctx, const void *d_normals, size_t n, size_t stride) { return set_record_normals(ctx, false, false, d_normals, n, stride); }
int rsreg_icp_set_source_normals(rsreg_ctx *ctx, const void *normals, size_t n, size_t stride) { return set_record_normals(ctx, true, true, normals, n, stride); }
int rsreg_icp_set_source_normals_device_(rsreg_ctx *ctx, const void *d_normals, size_t n, size_t stride) { return set_record_normals(ctx, true, false, d_normals, n, stride); }

// ---- the rejector chain (include/rsreg.h holds the contract; apply_chain above runs it)
int rsreg_icp_set_rejectors(rsreg_ctx *ctx, const rsreg_rejector *chain, int32_t n)
{
    if (!ctx || n < 0 || (n && !chain)) return RSREG_ERR_INVALID_ARG;
    if (n > kRejMax) return fail(ctx, RSREG_ERR_INVALID_ARG, "a rejector chain has at most 8 entries");
    RejectorChain c;
    for (int i = 0; i < n; ++i) {
        const double v = chain[i].value;
        switch (chain[i].kind) {
        case RSREG_REJECTOR_MEDIAN_DISTANCE:
            if (!(v >= 0.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "median distance rejector: the factor must not be NaN or negative");
            break;
        case RSREG_REJECTOR_ONE_TO_ONE:
            break;
        case RSREG_REJECTOR_SURFACE_NORMAL:
            break;
        case RSREG_REJECTOR_TRIMMED:
            if (!(v > 0.0 && v < 1.0)) return fail(ctx, RSREG_ERR_INVALID_ARG, "trimmed rejector: the overlap ratio must lie inside (0, 1)");
            break;
        default:
            return fail(ctx, RSREG_ERR_INVALID_ARG, "unknown rejector kind");
        }
        c.e[i] = chain[i];
    }
    c.n = n;
    ctx->rejectors = c;
    return RSREG_OK;
}

int rsreg_icp_rejector_stats(rsreg_ctx *ctx, rsreg_rejector_stat *stats, int32_t capacity, int32_t *n_out)
{
    if (!ctx || capacity < 0 || (capacity && !stats)) return RSREG_ERR_INVALID_ARG;
    const IcpState &s = ctx->icp;
    if (!s.chain_stats) return fail(ctx, RSREG_ERR_STATE, "no search with a rejector chain yet");
    if (n_out) *n_out = s.chain.n;
    uint32_t w[kRejHist];
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    RSREG_HIP(ctx, hipMemcpyAsync(w, ctx->d_rej_words.ptr, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int e = 0; e < s.chain.n && e < capacity; ++e) {
        float med;
        std::memcpy(&med, &w[kRejMed + e], 4);
        stats[e].n_in = w[kRejCnt + e];
        stats[e].n_out = w[kRejCnt + e + 1];
        stats[e].median_distance = s.chain.e[e].kind == RSREG_REJECTOR_MEDIAN_DISTANCE ? (double)med : 0.0;
        stats[e].reserved0 = 0.0;
    }
    return RSREG_OK;
}

int rsreg_icp_plane_sums(rsreg_ctx *ctx, double sums[RSREG_NUM_PLANE_SUMS])
{
    if (!ctx || !sums) return RSREG_ERR_INVALID_ARG;
    if (!ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_begin not called");
    if (!plane_on(ctx->icp.prm)) return fail(ctx, RSREG_ERR_STATE, "point-to-point alignment: rsreg_icp_sums");
    if (!ctx->icp.have_search) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_search not called for this iteration");
    return launch_plane_sums(ctx, sums);
}

int rsreg_icp_update_plane(rsreg_ctx *ctx, const double sums[RSREG_NUM_PLANE_SUMS], float *t_inc_out, int *done)
{
    if (!ctx || !sums || !done) return RSREG_ERR_INVALID_ARG;
    if (!ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_icp_begin not called");
    if (!plane_on(ctx->icp.prm)) return fail(ctx, RSREG_ERR_STATE, "point-to-point alignment: rsreg_icp_update");
    int rc = update_from_plane_sums(ctx, sums, done);
    if (rc) return rc;
    if (t_inc_out) std::memcpy(t_inc_out, ctx->icp.t_inc.m, 64);
    return RSREG_OK;
}

int rsreg_icp_plane_sums_last(rsreg_ctx *ctx, double sums[RSREG_NUM_PLANE_SUMS])
{
    if (!ctx || !sums) return RSREG_ERR_INVALID_ARG;
    std::memcpy(sums, ctx->icp.plane_sums_last, sizeof(ctx->icp.plane_sums_last));
    return RSREG_OK;
}

int rsreg_plane_solve_from_sums(const double sums[RSREG_NUM_PLANE_SUMS], float t_out[16], int *rank_out)
{
    if (!sums || !t_out) return RSREG_ERR_INVALID_ARG;
    Mat4f T;
    plane_solve_from_sums(sums, T, rank_out);
    std::memcpy(t_out, T.m, sizeof(T.m));
    return RSREG_OK;
}

int rsreg_icp_end(rsreg_ctx *ctx, rsreg_icp_result *result, void *aligned_out, size_t out_stride)
{
    return icp_end(ctx, result, aligned_out, out_stride, nullptr);
}

int rsreg_ctx_host_timing(rsreg_ctx *ctx, rsreg_host_timing *out)
{
    if (!ctx || !out) return RSREG_ERR_INVALID_ARG;
    *out = ctx->host_timing;
    return RSREG_OK;
}

int rsreg_icp_align(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params, rsreg_icp_result *result,
                    void *aligned_out, size_t out_stride)
{
    return icp_align(ctx, guess, params, result, aligned_out, out_stride, nullptr);
}

int rsreg_icp_align_records(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params, rsreg_icp_result *result,
                            const void *source_records, void *aligned_out, size_t stride)
{
    if (!source_records || !aligned_out) return RSREG_ERR_INVALID_ARG;
    return icp_align(ctx, guess, params, result, aligned_out, stride, source_records);
}

// ---------------------------------------------------------------------------------------------------------------------- GICP
// pcl::GeneralizedIterativeClosestPoint on the staged pipeline (include/rsreg.h holds the contract): the ICP state carries the
// transform, the search and the counters; an outer iteration is restart (cur = T * source) -> search -> k_gicp_mahalanobis ->
// { k_gicp_reduce at X -> host solve } -> T = float(X T).  One rank only: nothing is all-reduced.  (Its helpers: gicp_* above.)
void rsreg_gicp_params_default(rsreg_gicp_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_iterations = 200;
    p->max_inner_iterations = 20;
    p->k_correspondences = 20;
    p->max_correspondence_distance = 5.0;
    p->transformation_epsilon = 5e-4;
    p->rotation_epsilon = 2e-3;
    p->gicp_epsilon = 1e-3;
}

int rsreg_gicp_set_source_covariances(rsreg_ctx *ctx, const void *cov, size_t n, size_t stride)
{
    return gicp_set_covariances(ctx, true, cov, nullptr, n, stride);
}

int rsreg_gicp_set_target_covariances(rsreg_ctx *ctx, const void *cov, size_t n, size_t stride)
{
    return gicp_set_covariances(ctx, false, cov, nullptr, n, stride);
}

int rsreg_gicp_set_covariances_device_(rsreg_ctx *ctx, int source, const void *d_cov, size_t n, size_t stride)
{
    return gicp_set_covariances(ctx, source != 0, nullptr, d_cov, n, stride);
}

int rsreg_gicp_begin(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params)
{
    if (!ctx || !params) return RSREG_ERR_INVALID_ARG;
    if (params->max_iterations < 0 || params->max_inner_iterations < 0 || !(params->max_correspondence_distance >= 0) ||
        !(params->transformation_epsilon >= 0) || !(params->rotation_epsilon >= 0))
        return fail(ctx, RSREG_ERR_INVALID_ARG, "bad GICP parameters");
    if (ctx->nranks > 1) return fail(ctx, RSREG_ERR_INVALID_ARG, "GICP: not with more than one rank");
    if (ctx->have_target && ctx->have_source && !(ctx->have_gicp_cs && ctx->have_gicp_ct))
        return fail(ctx, RSREG_ERR_STATE, "GICP needs rsreg_gicp_set_source_covariances and rsreg_gicp_set_target_covariances after the clouds are set");
    rsreg_icp_params ip;
    rsreg_icp_params_default(&ip);
    ip.max_iterations = params->max_iterations;
    ip.criteria_mode = RSREG_CRITERIA_FIXED;
    ip.pipeline_mode = RSREG_PIPELINE_STAGED;
    ip.max_correspondence_distance = params->max_correspondence_distance;
    int rc = icp_begin(ctx, guess, &ip, true, false);   // (PCL's GICP loop consults no rejector)
    if (rc) return rc;
    ctx->gicp = GicpState();
    ctx->gicp.prm = *params;
    ctx->gicp.active = 1;
    return RSREG_OK;
}

int rsreg_gicp_search(rsreg_ctx *ctx, int32_t *index_out, float *sqr_dist_out)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    if (!ctx->gicp.active || !ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_gicp_begin not called");
    if (!ctx->have_gicp_cs || !ctx->have_gicp_ct || !ctx->have_target) return fail(ctx, RSREG_ERR_STATE, "a cloud was set after rsreg_gicp_begin: its covariances are gone");
    if (ctx->gicp.six && !(ctx->have_lab_s && ctx->have_lab_t)) return fail(ctx, RSREG_ERR_STATE, "a cloud was set after rsreg_gicp6d_begin: its colours are gone");
    IcpState &s = ctx->icp;
    s.restart_pending = true;   // the source under the whole current transform, from the records
    s.pending_transform = false;
    int rc = rsreg_icp_search(ctx, index_out, sqr_dist_out);
    if (rc) return rc;
    const uint32_t n = (uint32_t)ctx->n_work;
    if (n) {
        RSREG_HIP(ctx, ctx->d_gicp_m.reserve((size_t)n * 48 + 16));
        Mat34d R{};
        for (int c = 0; c < 3; ++c) {
            R.r0[c] = (double)s.final_t(0, c);
            R.r1[c] = (double)s.final_t(1, c);
            R.r2[c] = (double)s.final_t(2, c);
        }
        ScopedEvents ev(ctx, &ctx->ev_reduce);
        k_gicp_mahalanobis<<<div_up(n, kBlock), kBlock, 0, ctx->stream>>>(ctx->d_corr_pos.as<int>(), pair_targets(ctx), ctx->d_perm.as<uint32_t>(),
                                                                         ctx->d_first.as<uint32_t>(), ctx->d_gicp_cs.as<double>(), ctx->d_gicp_ct.as<double>(), R, n,
                                                                         ctx->d_gicp_m.as<double>());
        RSREG_HIP(ctx, hipGetLastError());
        s.idle_after_sums = false;
    }
    ctx->gicp.have_search = true;
    return RSREG_OK;
}

int rsreg_gicp_sums(rsreg_ctx *ctx, const double X[16], double sums[RSREG_NUM_GICP_SUMS])
{
    if (!ctx || !sums) return RSREG_ERR_INVALID_ARG;
    if (!ctx->gicp.active || !ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_gicp_begin not called");
    if (!ctx->gicp.have_search) return fail(ctx, RSREG_ERR_STATE, "rsreg_gicp_search not called for this iteration");
    double I[16];
    gicp_identity(I);
    return gicp_launch_sums(ctx, X ? X : I, sums);
}

int rsreg_gicp_step_from_sums(const double sums[RSREG_NUM_GICP_SUMS], double scale, double x_out[6], double delta_out[16], int *rank_out)
{
    if (!sums || !delta_out) return RSREG_ERR_INVALID_ARG;
    double x[6];
    const int rank = gicp_step(sums, scale, x, delta_out);
    if (x_out) std::memcpy(x_out, x, sizeof(x));
    if (rank_out) *rank_out = rank;
    return RSREG_OK;
}

int rsreg_gicp_update(rsreg_ctx *ctx, const double X[16], const double sums[RSREG_NUM_GICP_SUMS], int inner_evaluations, int *done)
{
    if (!ctx || !sums || !done) return RSREG_ERR_INVALID_ARG;
    if (!ctx->gicp.active || !ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_gicp_begin not called");
    IcpState &s = ctx->icp;
    GicpState &g = ctx->gicp;
    std::memcpy(g.sums_last, sums, sizeof(g.sums_last));
    fill_sums_last(s, sums[0], sums[1]);
    g.inner_evaluations += inner_evaluations;
    g.have_search = false;
    s.have_search = false;
    if (too_few_pairs(s, sums[0], 4, done)) return RSREG_OK;
    {
        double xs[6];
        g.rank_last = plane_unknowns_from_sums(sums, xs);
    }
    s.cur_mse = sums[1] / sums[0];
    double I[16], Td[16], Tn[16];
    gicp_identity(I);
    for (int k = 0; k < 16; ++k) Td[k] = (double)s.final_t.m[k];
    gicp_mul(X ? X : I, Td, Tn);
    Mat4f T_new = s.final_t;
    double delta = 0.0;
    const double rot_ratio = 1.0 / g.prm.rotation_epsilon, trans_ratio = 1.0 / g.prm.transformation_epsilon;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            T_new(r, c) = (float)Tn[c * 4 + r];
            const double diff = std::fabs((double)s.final_t(r, c) - (double)T_new(r, c));
            const double cd = diff == 0.0 ? 0.0 : diff * (c < 3 ? rot_ratio : trans_ratio);
            if (!(cd <= delta)) delta = cd;
        }
    s.final_t = T_new;
    s.iterations++;
    if (delta < 1.0) {
        s.state = RSREG_CONV_TRANSFORM;
        s.converged = 1;
    } else if (s.iterations >= g.prm.max_iterations) {
        s.state = RSREG_CONV_ITERATIONS;
        s.converged = 1;
    } else {
        s.state = RSREG_CONV_NOT_CONVERGED;
        s.converged = 0;
    }
    *done = s.converged;
    return RSREG_OK;
}

int rsreg_gicp_end(rsreg_ctx *ctx, rsreg_gicp_result *result, void *aligned_out, size_t out_stride)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    if (!ctx->gicp.active || !ctx->icp.active) return fail(ctx, RSREG_ERR_STATE, "rsreg_gicp_begin not called");
    rsreg_icp_result ir;
    int rc = icp_end(ctx, &ir, aligned_out, out_stride, nullptr);
    if (rc) return rc;
    const GicpState &g = ctx->gicp;
    if (result) {
        std::memset(result, 0, sizeof(*result));
        std::memcpy(result->transform, ir.transform, 64);
        result->converged = ir.converged;
        result->state = ir.state;
        result->iterations = ir.iterations;
        result->inner_evaluations = g.inner_evaluations;
        result->n_correspondences = ir.n_correspondences;
        result->mse = ir.mse;
        std::memcpy(result->sums_last, g.sums_last, sizeof(g.sums_last));
        result->ms_total = ir.ms_total;
        result->ms_nn = ir.ms_nn;
        result->ms_reduce = ir.ms_reduce;
        result->ms_transform = ir.ms_transform;
        result->n_nn_launches = ir.n_nn_launches;
        result->rank_last = g.rank_last;
    }
    ctx->gicp.active = 0;
    return RSREG_OK;
}

// the outer iterations of a GICP alignment that has begun (in three or in six dimensions), and its end
static int gicp_run(rsreg_ctx *ctx, const rsreg_gicp_params &prm, rsreg_gicp_result *result, void *aligned_out, size_t out_stride)
{
    int rc = RSREG_OK;
    int done = 0;
    while (!done) {
        rc = rsreg_gicp_search(ctx, nullptr, nullptr);
        if (rc) return rc;
        double X[16], S[RSREG_NUM_GICP_SUMS], Xc[16], Sc[RSREG_NUM_GICP_SUMS], D[16], x[6];
        gicp_identity(X);
        rc = gicp_launch_sums(ctx, X, S);
        if (rc) return rc;
        int evals = 0;
        // the step control of include/rsreg.h, decided by the sums alone
        while ((uint64_t)(S[0] + 0.5) >= 4 && evals < prm.max_inner_iterations) {
            double scale = 1.0;
            bool accepted = false;
            if (gicp_step(S, scale, x, D) == 0) break;
            while (evals < prm.max_inner_iterations) {
                gicp_mul(D, X, Xc);
                rc = gicp_launch_sums(ctx, Xc, Sc);
                if (rc) return rc;
                ++evals;
                if (Sc[3] <= S[3]) {
                    std::memcpy(X, Xc, sizeof(X));
                    std::memcpy(S, Sc, sizeof(S));
                    accepted = true;
                    break;
                }
                scale *= 0.5;
                (void)gicp_step(S, scale, x, D);
            }
            if (!accepted) break;
            bool small = true;
            for (int i = 0; i < 6; ++i) small = small && std::fabs(x[i]) <= (i < 3 ? prm.rotation_epsilon : prm.transformation_epsilon);
            if (small) break;
        }
        rc = rsreg_gicp_update(ctx, X, S, evals, &done);
        if (rc) return rc;
    }
    return rsreg_gicp_end(ctx, result, aligned_out, out_stride);
}

int rsreg_gicp_align(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, rsreg_gicp_result *result, void *aligned_out, size_t out_stride)
{
    int rc = rsreg_gicp_begin(ctx, guess, params);
    if (rc) return rc;
    return gicp_run(ctx, *params, result, aligned_out, out_stride);
}

// ---------------------------------------------------------------------------------------------------------------------- GICP6D
// pcl::GeneralizedIterativeClosestPoint6D: GICP whose correspondences are nearest neighbours in (x, y, z, w L', w a', w b')
// (include/rsreg.h holds the contract; nn6_kernels.hpp the search).  Everything behind the search is GICP's.
int rsreg_gicp_set_source_lab(rsreg_ctx *ctx, const void *lab, size_t n, size_t stride) { return gicp_set_lab(ctx, true, lab, nullptr, n, stride); }
int rsreg_gicp_set_target_lab(rsreg_ctx *ctx, const void *lab, size_t n, size_t stride) { return gicp_set_lab(ctx, false, lab, nullptr, n, stride); }
int rsreg_gicp_set_lab_device_(rsreg_ctx *ctx, int source, const void *d_lab, size_t n, size_t stride) { return gicp_set_lab(ctx, source != 0, nullptr, d_lab, n, stride); }

int rsreg_gicp6d_begin(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, double lab_weight)
{
    if (!ctx || !params) return RSREG_ERR_INVALID_ARG;
    if (!(lab_weight >= 0) || !std::isfinite(lab_weight)) return fail(ctx, RSREG_ERR_INVALID_ARG, "GICP6D: the colour weight must be finite and not negative");
    if (ctx->have_target && ctx->have_source && !(ctx->have_lab_s && ctx->have_lab_t))
        return fail(ctx, RSREG_ERR_STATE, "GICP6D needs rsreg_gicp_set_source_lab and rsreg_gicp_set_target_lab after the clouds are set");
    int rc = rsreg_gicp_begin(ctx, guess, params);
    if (rc) return rc;
    rc = gicp6d_prepare(ctx, (float)lab_weight);
    if (rc) {
        ctx->gicp.active = 0;
        ctx->icp.active = 0;
        return rc;
    }
    ctx->gicp.six = 1;
    ctx->gicp.lab_weight = (float)lab_weight;
    return RSREG_OK;
}

int rsreg_gicp6d_align(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, double lab_weight, rsreg_gicp_result *result, void *aligned_out,
                       size_t out_stride)
{
    int rc = rsreg_gicp6d_begin(ctx, guess, params, lab_weight);
    if (rc) return rc;
    return gicp_run(ctx, *params, result, aligned_out, out_stride);
}

int rsreg_icp_grid_info(rsreg_ctx *ctx, rsreg_grid_info *info)
{
    if (!ctx || !info) return RSREG_ERR_INVALID_ARG;
    if (!ctx->have_target) return RSREG_ERR_NO_TARGET;
    {
        int rcc = target_counts(ctx, true);   // (a counting build set_target did not wait for)
        if (rcc) return rcc;
    }
#ifdef RSREG_DIAG
    const bool want_max = tunables().grid_stats;   // (diagnostic builds: a pass over the occupied cells, only on request)
#else
    const bool want_max = false;
#endif
    if (want_max && ctx->grid.dense == 1 && ctx->grid_info.max_points_per_cell == 0 && ctx->grid.n_points > 0) {
        const size_t total = (size_t)(ctx->grid.dims[0] + 2) * (ctx->grid.dims[1] + 2) * (ctx->grid.dims[2] + 2);
        uint32_t *d = ctx->d_misc.as<uint32_t>() + kMiscMaxCount;
        uint32_t h = 0;
        RSREG_HIP(ctx, hipMemsetAsync(d, 0, 4, ctx->stream));
        (void)total;
        k_dense_max_count<<<256, kBlock, 0, ctx->stream>>>(ctx->d_cellpos.as<uint32_t>(), ctx->d_misc.as<uint32_t>() + kMiscStats, d);
        RSREG_HIP(ctx, hipGetLastError());
        RSREG_HIP(ctx, hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, ctx->stream));
        RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->grid_info.max_points_per_cell = h;
    }
    {
        int rcj = join_source(ctx);
        if (rcj) return rcj;
    }
    *info = ctx->grid_info;
    info->n_source_distinct = ctx->have_source ? (uint32_t)ctx->n_work : 0u;
    return RSREG_OK;
}

// pcl::transformPointCloud: whole records copied, xyz rewritten
int rsreg_transform_cloud(rsreg_ctx *ctx, const void *in, void *out, size_t n, size_t stride, int is_dense,
                          const float transform[16])
{
    (void)is_dense;  // non-finite points are left unchanged either way (xform of NaN stays NaN-free here)
    if (!ctx || !transform || (n && (!in || !out)) || stride < 12) return RSREG_ERR_INVALID_ARG;
    if (n == 0) return RSREG_OK;
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = pack_to_stage(ctx, in, n, stride);
    if (rc) return rc;
    RSREG_HIP(ctx, ctx->d_tmp.reserve(n * 12 + n * 16 + 64));
    char *d_raw = ctx->d_tmp.as<char>();
    float4 *d_pts = reinterpret_cast<float4 *>(d_raw + ((n * 12 + 15) & ~size_t(15)));
    RSREG_HIP(ctx, ctx->d_tmp.reserve(((n * 12 + 15) & ~size_t(15)) + n * 16 + 64));
    d_raw = ctx->d_tmp.as<char>();
    d_pts = reinterpret_cast<float4 *>(d_raw + ((n * 12 + 15) & ~size_t(15)));
    RSREG_HIP(ctx, hipMemcpyAsync(d_raw, ctx->h_stage.ptr, n * 12, hipMemcpyHostToDevice, ctx->stream));
    Mat4f T;
    std::memcpy(T.m, transform, 64);
    k_gather_source<uint32_t><<<div_up((uint32_t)n, kBlock), kBlock, 0, ctx->stream>>>(d_raw, 12, (uint32_t)n, nullptr, d_pts, nullptr);
    RSREG_HIP(ctx, hipGetLastError());
    k_apply_final<<<div_up((uint32_t)n, kBlock), kBlock, 0, ctx->stream>>>(d_pts, (uint32_t)n, to_mat34(T), nullptr,
                                                                            reinterpret_cast<float *>(d_raw));
    RSREG_HIP(ctx, hipGetLastError());
    RSREG_HIP(ctx, hipMemcpyAsync(ctx->h_stage.ptr, d_raw, n * 12, hipMemcpyDeviceToHost, ctx->stream));
    RSREG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const char *src = static_cast<const char *>(in);
    char *dst = static_cast<char *>(out);
    const float *xyz = ctx->h_stage.as<float>();
    host_parallel_for(n, [=](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            if (dst != src) std::memmove(dst + i * stride, src + i * stride, stride);
            std::memcpy(dst + i * stride, xyz + 3 * i, 12);
        }
    });
    return RSREG_OK;
}

// ---- getFitnessScore (fitness_sums and its helpers above)
int rsreg_icp_fitness_sums(rsreg_ctx *ctx, double max_range, double sums[2])
{
    if (!ctx || !sums) return RSREG_ERR_INVALID_ARG;
    return icp_fitness_block(ctx, max_range, sums);
}

int rsreg_icp_fitness_score(rsreg_ctx *ctx, double max_range, double *score, uint64_t *n_within)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    double sums[2];
    int rc = icp_fitness_block(ctx, max_range, sums);
    if (rc) return rc;
    if (ctx->nranks > 1) {   // (the same way as the 17 sums: every rank holds a block of the source)
        rc = rsreg_comm_allreduce_f64(ctx, sums, 2);
        if (rc) return rc;
    }
    fitness_result(sums, score, n_within);
    return RSREG_OK;
}

int rsreg_ndt_fitness_score(rsreg_ctx *ctx, double max_range, double *score, uint64_t *n_within)
{
    if (!ctx) return RSREG_ERR_INVALID_ARG;
    if (!ctx->ndt_fit_ok) return fail(ctx, RSREG_ERR_STATE, "no NDT alignment against the current NDT target");
    RSREG_HIP(ctx, hipSetDevice(ctx->device));
    double sums[2];
    int rc = fitness_sums(ctx, ctx->fit_ndt, ctx->d_ndt_tgt.as<float4>(), ctx->ndt_tgt_n, ctx->d_ndt_src.as<float4>(), nullptr, ctx->ndt_fit_n,
                          ctx->ndt_fit_t, max_range, sums);
    if (rc) return rc;
    fitness_result(sums, score, n_within);
    return RSREG_OK;
}

}  // extern "C"
