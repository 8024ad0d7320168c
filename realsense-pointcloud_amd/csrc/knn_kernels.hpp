// knn_kernels.hpp — exact k nearest neighbours of every point of a cloud within the same cloud: device code of
// pcl::StatisticalOutlierRemoval's first pass (include/rsreg.h: rsreg_cloud_knn_mean_distance, rsreg_cloud_sor).  Included by
// filters.hip only.
//
// PCL 1.9.1 (filters/impl/statistical_outlier_removal.hpp, recalled), per finite record:
//   searcher_->nearestKSearch(point, mean_k_ + 1, nn_indices, nn_dists);      // FLANN L2_Simple<float>, ascending
//   for (k = 1; k < mean_k_ + 1; ++k) dist_sum += sqrt(nn_dists[k]);          // double += float sqrt
//   distances[i] = static_cast<float>(dist_sum / mean_k_);
//
// The index (rsreg_ctx.hpp: KnnIndex, DESIGN.md §4, cloud filters) is a dense grid of cells over the finite points' box, numbered x
// fastest: the points of a run of cells along x are one run of the cell-sorted array.  One wave answers one query.  It walks
// shells of cells around the query's cell; the lanes fetch the starts of the shell's rows side by side, then the wave reads the
// points of every row that is neither empty nor beyond the bound, 64 at a time, 16 bytes a lane.  Distances not above the
// bound -- the (k + 1)-th smallest seen so far, +inf until then -- are appended to a buffer in LDS; a bitonic sort of that
// buffer keeps the k + 1 smallest and tightens the bound.  The walk ends when a lower bound of everything outside the visited cube
// exceeds the bound.  Only distance VALUES are kept: equal distances are equal values, so no tie order enters the result.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "records.hpp"

namespace rsreg {

constexpr int kKnnMaxK = 64;        // mean_k at most: k + 1 = 65 kept values and a batch of 64 new ones fit the buffer twice over
constexpr int kKnnBuf = 256;        // floats of LDS a wave selects in
constexpr int kKnnWave = 64;
constexpr float kKnnMargin = 0.03f; // slack (in cells) on every gap: the float rounding of the point -> cell assignment (1e-3 cells at 4 096 cells an axis)

struct KnnDev {
    float ox, oy, oz, inv_cell, cell;
    int dx, dy, dz;          // cells per axis (4 096 at most)
    uint32_t n;              // finite points indexed
    const uint32_t *start;   // per cell + 1: first point of the cell
    const float4 *pts;       // {x, y, z, bits(record index)}, cell by cell
};

// FLANN L2_Simple<float>: ((dx*dx + dy*dy) + dz*dz), no contraction (the form of icp_kernels.hpp: l2_simple)
__device__ __forceinline__ float knn_l2(float qx, float qy, float qz, float tx, float ty, float tz)
{
    const float dx = __fsub_rn(qx, tx), dy = __fsub_rn(qy, ty), dz = __fsub_rn(qz, tz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// position in cell units; the SAME expression places the points and the queries
__device__ __forceinline__ float knn_cell_pos(float p, float origin, float inv_cell) { return __fmul_rn(__fsub_rn(p, origin), inv_cell); }

__device__ __forceinline__ int knn_axis_cell(float p, float origin, float inv_cell, int d)
{
    return (int)fminf(fmaxf(floorf(knn_cell_pos(p, origin, inv_cell)), 0.0f), (float)(d - 1));
}

// lower bound (cells) on the distance along one axis from position u to the cells lo..hi
__device__ __forceinline__ float knn_gap(float u, int lo, int hi)
{
    return fmaxf(fmaxf((float)lo - u, u - (float)(hi + 1)) - kKnnMargin, 0.0f);
}

// A lower bound on the squared FLOAT distance to anything beyond the per-axis gaps.  The factor is fit_lb2's (fitness_kernels.hpp):
// the rounding of this sum (4 ulp), of cell * cell against 1 / inv_cell (2 ulp), of the position (3 ulp) and of knn_l2 itself
// (5 ulp) are 14 ulp of 2^-24 = 1e-6 < 4e-6.
__device__ __forceinline__ float knn_lb2(float gx, float gy, float gz, float cell2)
{
    return (gx * gx + gy * gy + gz * gz) * cell2 * 0.999996f;
}

__device__ __forceinline__ uint32_t knn_ordered(float f)   // (= float_ordered of icp_kernels.hpp; the way back: ordered_float)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ------------------------------------------------------------------------------ build
// box[0..2] = min, [3..5] = max (ordered uints), [6] = number of finite records; box = {~0 x 3, 0 x 5} on entry
__global__ __launch_bounds__(kBlock) void k_knn_bbox(const char *rec, size_t stride, uint32_t n, uint32_t *box)
{
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    uint32_t cnt = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float *p = rec_xyz(rec, stride, i);
        const float x = p[0], y = p[1], z = p[2];
        if (finite3(x, y, z)) {
            mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
            mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
            ++cnt;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], __shfl_down(mn[k], off));
            mx[k] = fmaxf(mx[k], __shfl_down(mx[k], off));
        }
        cnt += __shfl_down(cnt, off);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        for (int k = 0; k < 3; ++k) {
            atomicMin(&box[k], knn_ordered(mn[k]));
            atomicMax(&box[3 + k], knn_ordered(mx[k]));
        }
        atomicAdd(&box[6], cnt);
    }
}

__device__ __forceinline__ bool knn_point_cell(const KnnDev &g, float x, float y, float z, uint32_t &cell)
{
    if (!finite3(x, y, z)) return false;
    const int cx = knn_axis_cell(x, g.ox, g.inv_cell, g.dx), cy = knn_axis_cell(y, g.oy, g.inv_cell, g.dy),
              cz = knn_axis_cell(z, g.oz, g.inv_cell, g.dz);
    cell = ((uint32_t)cz * (uint32_t)g.dy + (uint32_t)cy) * (uint32_t)g.dx + (uint32_t)cx;
    return true;
}

// points per cell (count zero on entry); a non-finite record's distance is PCL's 0
__global__ __launch_bounds__(kBlock) void k_knn_count(const char *rec, size_t stride, uint32_t n, KnnDev g, uint32_t *count, float *dist)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    uint32_t c;
    if (knn_point_cell(g, p[0], p[1], p[2], c)) atomicAdd(&count[c], 1u);
    else dist[i] = 0.0f;
}

// each finite record to a free place of its cell (start = exclusive prefix of the counts; the counts go back to zero).  The order
// inside a cell is whatever the atomics make it: only distance values are read from the index.
__global__ __launch_bounds__(kBlock) void k_knn_scatter(const char *rec, size_t stride, uint32_t n, KnnDev g, const uint32_t *start,
                                                        uint32_t *count, float4 *sorted)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    const float x = p[0], y = p[1], z = p[2];
    uint32_t c;
    if (!knn_point_cell(g, x, y, z, c)) return;
    const uint32_t k = atomicSub(&count[c], 1u) - 1u;
    sorted[start[c] + k] = make_float4(x, y, z, __uint_as_float(i));
}

// ------------------------------------------------------------------------------ search
// Ascending bitonic sort of buf[0 .. n) (n = 64, 128 or 256 >= count, padded with +inf), by the one wave of the workgroup; then
// the k1 smallest stay: count = min(count, k1), bound = the k1-th smallest (+inf while there are fewer).
__device__ __forceinline__ void knn_select(float *buf, int lane, int k1, int &count, float &bound)
{
    const int n = count <= 64 ? 64 : (count <= 128 ? 128 : kKnnBuf);
    for (int i = count + lane; i < n; i += kKnnWave) buf[i] = __int_as_float(0x7f800000);
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n >> 1); t += kKnnWave) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const float a = buf[i], b = buf[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            __syncthreads();
        }
    }
    count = min(count, k1);
    bound = count >= k1 ? buf[k1 - 1] : __int_as_float(0x7f800000);
}

// One workgroup of ONE wave per query, queries in cell order (a grid-stride loop: the waves in flight work on neighbouring
// cells).  dist[record] = (float)(sum_{j = 1 .. k} (double)sqrtf(d2[j]) / k), d2 ascending, d2[0] (the point itself) dropped.
__global__ __launch_bounds__(kKnnWave) void k_knn_mean_distance(KnnDev g, int k, float *dist)
{
    __shared__ float buf[kKnnBuf];
    const int lane = (int)threadIdx.x, k1 = k + 1;
    const float inf = __int_as_float(0x7f800000), cell2 = g.cell * g.cell;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        const float ux = knn_cell_pos(q.x, g.ox, g.inv_cell), uy = knn_cell_pos(q.y, g.oy, g.inv_cell), uz = knn_cell_pos(q.z, g.oz, g.inv_cell);
        const int cx = knn_axis_cell(q.x, g.ox, g.inv_cell, g.dx), cy = knn_axis_cell(q.y, g.oy, g.inv_cell, g.dy),
                  cz = knn_axis_cell(q.z, g.oz, g.inv_cell, g.dz);
        const int rmax = max(max(max(cx, g.dx - 1 - cx), max(cy, g.dy - 1 - cy)), max(cz, g.dz - 1 - cz));
        int count = 0;
        float bound = inf;
        bool done = false, dirty = false;
        for (int r = 0; r <= rmax && !done; ++r) {
            const int side = 2 * r + 1, rows = side * side;
            for (int base = 0; base < rows && !done; base += kKnnWave) {
                const int row = base + lane;
                const int oy = row % side - r, oz = row / side - r, y = cy + oy, z = cz + oz;
                const bool in = row < rows && y >= 0 && y < g.dy && z >= 0 && z < g.dz;
                const bool face = abs(oy) == r || abs(oz) == r;   // a face row: every cell of it; else its two ends
                const float gy = knn_gap(uy, y, y), gz = knn_gap(uz, z, z);
                for (int pass = 0; pass < 2 && !done; ++pass) {
                    int x0, x1;
                    bool has = in;
                    if (face) {
                        x0 = max(cx - r, 0);
                        x1 = min(cx + r, g.dx - 1);
                        has = has && pass == 0;
                    } else {
                        x0 = x1 = pass == 0 ? cx - r : cx + r;
                        has = has && x0 >= 0 && x0 < g.dx;
                    }
                    const float lb = has ? knn_lb2(knn_gap(ux, x0, x1), gy, gz, cell2) : inf;
                    uint32_t s = 0, e = 0;
                    if (has && !(lb > bound)) {
                        const size_t c0 = ((size_t)z * (size_t)g.dy + (size_t)y) * (size_t)g.dx;
                        s = g.start[c0 + (size_t)x0];
                        e = g.start[c0 + (size_t)x1 + 1];
                    }
                    unsigned long long todo = __ballot(e > s);
                    while (todo && !done) {
                        const int l = __ffsll((long long)todo) - 1;
                        todo &= todo - 1;
                        const uint32_t ss = __shfl(s, l), ee = __shfl(e, l);
                        if (__shfl(lb, l) > bound) continue;   // (the bound has come down since the row was fetched)
                        for (uint32_t p = ss; p < ee; p += kKnnWave) {
                            if (count > kKnnBuf - kKnnWave) {
                                knn_select(buf, lane, k1, count, bound);
                                dirty = false;
                                if (count >= k1 && bound == 0.0f) {   // k + 1 copies of the query: nothing can change the values any more
                                    done = true;
                                    break;
                                }
                            }
                            const uint32_t i = p + (uint32_t)lane;
                            float d = inf;
                            bool ok = i < ee;
                            if (ok) {
                                const float4 t = g.pts[i];
                                d = knn_l2(q.x, q.y, q.z, t.x, t.y, t.z);
                                ok = d <= bound;
                            }
                            const unsigned long long m = __ballot(ok);
                            if (ok) buf[count + __popcll(m & lt)] = d;
                            count += __popcll(m);
                            dirty = dirty || m != 0ull;
                        }
                    }
                }
            }
            if (done) break;
            if (count >= k1) {
                if (dirty) {
                    knn_select(buf, lane, k1, count, bound);
                    dirty = false;
                }
                if (bound == 0.0f) break;
                // every cell not visited yet lies beyond one of the six faces of the cube of shell r
                float out = inf;
                if (cx + r + 1 < g.dx) out = fminf(out, knn_lb2(knn_gap(ux, cx + r + 1, g.dx - 1), 0.0f, 0.0f, cell2));
                if (cx - r - 1 >= 0) out = fminf(out, knn_lb2(knn_gap(ux, 0, cx - r - 1), 0.0f, 0.0f, cell2));
                if (cy + r + 1 < g.dy) out = fminf(out, knn_lb2(0.0f, knn_gap(uy, cy + r + 1, g.dy - 1), 0.0f, cell2));
                if (cy - r - 1 >= 0) out = fminf(out, knn_lb2(0.0f, knn_gap(uy, 0, cy - r - 1), 0.0f, cell2));
                if (cz + r + 1 < g.dz) out = fminf(out, knn_lb2(0.0f, 0.0f, knn_gap(uz, cz + r + 1, g.dz - 1), cell2));
                if (cz - r - 1 >= 0) out = fminf(out, knn_lb2(0.0f, 0.0f, knn_gap(uz, 0, cz - r - 1), cell2));
                if (out > bound) break;
            }
        }
        if (dirty) knn_select(buf, lane, k1, count, bound);
        __syncthreads();
        if (lane == 0) {
            double sum = 0.0;
            for (int i = 1; i < min(count, k1); ++i) sum += (double)(float)sqrt((double)buf[i]);   // ascending; the float sqrt, correctly rounded (through f64: 53 >= 2 * 24 + 2 bits), f64 sum
            dist[__float_as_uint(q.w)] = (float)(sum / (double)k);
        }
        __syncthreads();   // (the next query appends to the same buffer)
    }
}

// ------------------------------------------------------------------------------ threshold
// PCL's two sums as PCL adds them: one record after the other in input order, in double (a non-finite record adds its 0).
// Workgroup 0: sums[0] = sum of d; workgroup 1: sums[1] = sum of d * d.  One wave each: it loads 64 distances at a time (the
// next 64 are on their way meanwhile) and adds them in order, every lane the same chain.  The order is the contract, not a
// taste: var = (sq - sum * sum / n) / (n - 1) cancels, so the 1e-13 by which a tree of partial sums differs from the
// sequential sum of 3 * 10^5 values comes back 14 times larger in stddev (measured on a 307 k frame: 1.07e-12 relative).
// The chain of dependent f64 additions is the cost: about 2 us per 1 000 records.
__global__ __launch_bounds__(kKnnWave) void k_sor_sums(const float *dist, uint32_t n, double *sums)
{
    const uint32_t lane = threadIdx.x;
    const bool squares = blockIdx.x == 1;
    double acc = 0.0;
    float next = lane < n ? dist[lane] : 0.0f;
    for (uint32_t base = 0; base < n; base += kKnnWave) {
        double v = (double)next;
        const uint32_t ahead = base + kKnnWave + lane;
        next = ahead < n ? dist[ahead] : 0.0f;
        if (squares) v = v * v;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
#pragma unroll
        for (int i = 0; i < kKnnWave; ++i) {   // (beyond n: + 0.0, which changes nothing)
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, i);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), i);
            acc += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
    }
    if (lane == 0) sums[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------ flags and the ordered gather
// SOR: removed when distance > threshold (negative: when distance <= threshold); a non-finite record is never "valid": kept unless negative
__global__ __launch_bounds__(kBlock) void k_sor_flags(const char *rec, size_t stride, const float *dist, uint32_t n, double threshold, int negative,
                                                      uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    bool keep;
    if (!finite3(p[0], p[1], p[2])) keep = !negative;
    else {
        const bool above = (double)dist[i] > threshold;
        keep = negative ? above : !above;
    }
    flags[i] = keep ? 1u : 0u;
}

// PassThrough: a non-finite record is always removed; else removed when v < lo || v > hi (negative: when lo <= v <= hi)
__global__ __launch_bounds__(kBlock) void k_pass_flags(const char *rec, size_t stride, uint32_t n, int field, float lo, float hi, int negative,
                                                       uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    bool keep = false;
    if (finite3(p[0], p[1], p[2])) {
        const float v = p[field];
        const bool outside = v < lo || v > hi;
        keep = negative ? outside : !outside;
    }
    flags[i] = keep ? 1u : 0u;
}

// pos = exclusive prefix of flags: record i goes to place pos[i]; thread 0 leaves the number of kept records in *n_kept
__global__ __launch_bounds__(kBlock) void k_filter_gather(const char *rec, size_t stride, uint32_t n, const uint32_t *flags, const uint32_t *pos,
                                                          char *out, uint32_t *n_kept)
{
    const uint32_t words = (uint32_t)(stride / 4);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) *n_kept = pos[n - 1] + flags[n - 1];
    const uint32_t i = (uint32_t)(t / words), w = (uint32_t)(t % words);
    if (i >= n || !flags[i]) return;
    reinterpret_cast<uint32_t *>(out + (size_t)pos[i] * stride)[w] = reinterpret_cast<const uint32_t *>(rec + (size_t)i * stride)[w];
}

// keep_organized: every record stays, a removed one gets x = y = z = quiet NaN
__global__ __launch_bounds__(kBlock) void k_filter_organized(const char *rec, size_t stride, uint32_t n, const uint32_t *flags, char *out)
{
    const uint32_t words = (uint32_t)(stride / 4);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / words), w = (uint32_t)(t % words);
    if (i >= n) return;
    uint32_t v = reinterpret_cast<const uint32_t *>(rec + (size_t)i * stride)[w];
    if (w < 3 && !flags[i]) v = 0x7fc00000u;
    reinterpret_cast<uint32_t *>(out + (size_t)i * stride)[w] = v;
}

}  // namespace rsreg
