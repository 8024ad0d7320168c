// knn_kernels.hpp — exact k nearest neighbours of every point of a cloud within the same cloud: the one search under
// pcl::StatisticalOutlierRemoval's first pass (include/rsreg.h: rsreg_cloud_knn_mean_distance, rsreg_cloud_sor) and, through
// normals_kernels.hpp, under rsreg_cloud_knn and rsreg_cloud_normals; and the filters' flag / gather kernels.  Included by
// filters.hip only; the index itself, its build and the bounds the search prunes with are pointgrid.hpp's.
//
// PCL 1.9.1 (filters/impl/statistical_outlier_removal.hpp, recalled), per finite record:
//   searcher_->nearestKSearch(point, mean_k_ + 1, nn_indices, nn_dists);      // FLANN L2_Simple<float>, ascending
//   for (k = 1; k < mean_k_ + 1; ++k) dist_sum += sqrt(nn_dists[k]);          // double += float sqrt
//   distances[i] = static_cast<float>(dist_sum / mean_k_);
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "pointgrid.hpp"

namespace rsreg {

constexpr int kKnnMaxK = 64;        // mean_k at most: k + 1 = 65 kept elements and a batch of 64 new ones fit the buffer twice over
constexpr int kKnnBuf = 256;        // elements of LDS a wave selects in
constexpr int kKnnWave = 64;
// ------------------------------------------------------------------------------ search
// The index (rsreg_ctx.hpp: PointGrid, built with KnnGridPolicy) is a dense grid of cells over the finite points' box,
// numbered x fastest: the points of a run of cells along x are one run of the cell-sorted array.  One wave answers one query.  It walks
// shells of cells around the query's cell; the lanes fetch the starts of the shell's rows side by side, then the wave reads the
// points of every row that is neither empty nor beyond the bound, 64 at a time, 16 bytes a lane.  The candidates the bound
// takes -- the bound is the kept-th smallest element seen so far, none() until then -- are appended to a buffer in LDS; a
// bitonic sort of that buffer keeps the `kept` smallest and tightens the bound.  The walk ends when a lower bound of everything
// outside the visited cube exceeds the bound's distance.  The distance is float32 l2_simple throughout.
//
// What the selection sorts is the policy's; the two policies are everything in which the two searches differ.

// The value-only search: only squared distances are kept.  Equal distances are equal values, so no tie order enters the result,
// and a candidate AT the bound may be taken or left alike (it is taken).  Once `kept` zeros are held nothing can change the
// values any more: the walk ends there, which is what makes a pile of thousands of copies (the missing-depth records of a raw
// frame) cost each of its queries one refill.
struct KnnValues {
    using Elem = float;
    static constexpr bool kEndsAtZero = true;
    __device__ static Elem none() { return __int_as_float(0x7f800000); }
    __device__ static Elem make(float d2, uint32_t) { return d2; }
    __device__ static bool takes(Elem candidate, Elem bound) { return candidate <= bound; }
    __device__ static float d2(Elem e) { return e; }
};

// The identity-carrying search: a 64-bit key, float bits of d2 << 32 | original record index.  d2 >= 0, so its bit pattern orders
// like its value, and no two records share a key.  The `kept` smallest keys, ascending, are ascending by (d2, record index), and
// among the records whose d2 equals the kept-th smallest value the lowest indices: the project's tie rule ("ties: lowest index").
// So a candidate is taken when its KEY is below the bound, and nothing ends at a bound of 0: every record at distance 0 has to be
// seen before the lowest indices among them are known.  (A pile of m exact copies therefore costs m / 64 loads per query of the
// pile.)  The walk skips a cell only when its lower bound is ABOVE the bound's distance, so every record that ties with it is seen.
constexpr unsigned long long kKnnNoKey = ~0ull;   // above every key: the padding of the selection, the bound while fewer than `kept` are held
struct KnnKeys {
    using Elem = unsigned long long;
    static constexpr bool kEndsAtZero = false;
    __device__ static Elem none() { return kKnnNoKey; }
    __device__ static Elem make(float d2, uint32_t record) { return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)record; }
    __device__ static bool takes(Elem candidate, Elem bound) { return candidate < bound; }
    __device__ static float d2(Elem e) { return __uint_as_float((uint32_t)(e >> 32)); }   // (of a key: kKnnNoKey's high word is a NaN)
};

// Ascending bitonic sort of buf[0 .. n) (n = 64, 128 or 256 >= count, padded with none()), by the one wave of the workgroup; then
// the `kept` smallest stay: count = min(count, kept), bound = the kept-th smallest, bound_d2 its distance (none() and +inf while
// there are fewer: never d2(none())).
template <typename Sel>
__device__ __forceinline__ void knn_select(typename Sel::Elem *buf, int lane, int kept, int &count, typename Sel::Elem &bound, float &bound_d2)
{
    using Elem = typename Sel::Elem;
    const int n = count <= 64 ? 64 : (count <= 128 ? 128 : kKnnBuf);
    for (int i = count + lane; i < n; i += kKnnWave) buf[i] = Sel::none();
    __syncthreads();
    for (int s = 2; s <= n; s <<= 1) {
        for (int j = s >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n >> 1); t += kKnnWave) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const Elem a = buf[i], b = buf[l];
                const bool up = (i & s) == 0;
                if ((a > b) == up) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            __syncthreads();
        }
    }
    count = min(count, kept);
    bound = count >= kept ? buf[kept - 1] : Sel::none();
    bound_d2 = count >= kept ? Sel::d2(bound) : __int_as_float(0x7f800000);
}

// The `kept` smallest elements of the query q (a point of the index; its w carries its record) in buf[0 .. kept), ascending;
// returns how many there are (`kept`, when the index holds that many points).  Called by every lane of the one wave of the
// workgroup; buf: kKnnBuf elements of LDS.  Returns behind a barrier.
template <typename Sel>
__device__ __forceinline__ int knn_walk(const PointGridDev &g, const float4 q, int kept, typename Sel::Elem *buf, int lane)
{
    using Elem = typename Sel::Elem;
    const float inf = __int_as_float(0x7f800000);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const float ux = bound_pos(cell_pos(q.x, g.ox, g.inv_cell)), uy = bound_pos(cell_pos(q.y, g.oy, g.inv_cell)),
                uz = bound_pos(cell_pos(q.z, g.oz, g.inv_cell));
    const int cx = axis_cell(q.x, g.ox, g.inv_cell, g.dx), cy = axis_cell(q.y, g.oy, g.inv_cell, g.dy), cz = axis_cell(q.z, g.oz, g.inv_cell, g.dz);
    int count = 0;
    Elem bound = Sel::none();
    float bound_d2 = inf;
    bool done = false, dirty = false;   // done: Sel::kEndsAtZero only
    // shell r holds a cell while one of the six faces of its cube is inside the grid
    for (int r = 0; !done && (r <= cx || r <= cy || r <= cz || cx + r < g.dx || cy + r < g.dy || cz + r < g.dz); ++r) {
        // the rows of the shell's square that lie inside the grid (the others hold nothing: a record alone at the end of a grid of
        // 4 000 x 2 x 2 cells walks 4 000 shells of four rows each, not of (2 r + 1)^2)
        const int ny = min(cy + r, g.dy - 1) - max(cy - r, 0) + 1, rows = (min(cz + r, g.dz - 1) - (cz - r) + 1) * ny;
        for (int base = max(r - cz, 0) * ny; base < rows && !done; base += kKnnWave) {
            const int row = base + lane;
            const int y = max(cy - r, 0) + row % ny, z = cz - r + row / ny, oy = y - cy, oz = z - cz;
            const bool in = row < rows;
            const bool face = abs(oy) == r || abs(oz) == r;   // a face row: every cell of it; else its two ends
            const float gy = axis_gap(uy, y, y), gz = axis_gap(uz, z, z);
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
                const float lb = has ? grid_lb2(axis_gap(ux, x0, x1), gy, gz, g.cell) : inf;
                uint32_t s = 0, e = 0;
                if (has && !(lb > bound_d2)) {
                    const size_t c0 = ((size_t)z * (size_t)g.dy + (size_t)y) * (size_t)g.dx;
                    s = g.start[c0 + (size_t)x0];
                    e = g.start[c0 + (size_t)x1 + 1];
                }
                unsigned long long todo = __ballot(e > s);
                while (todo && !done) {
                    const int l = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const uint32_t ss = __shfl(s, l), ee = __shfl(e, l);
                    if (__shfl(lb, l) > bound_d2) continue;   // (the bound has come down since the row was fetched)
                    for (uint32_t p = ss; p < ee; p += kKnnWave) {
                        if (count > kKnnBuf - kKnnWave) {
                            knn_select<Sel>(buf, lane, kept, count, bound, bound_d2);
                            dirty = false;
                            if constexpr (Sel::kEndsAtZero) {
                                if (count >= kept && bound_d2 == 0.0f) {   // `kept` copies of the query
                                    done = true;
                                    break;
                                }
                            }
                        }
                        const uint32_t i = p + (uint32_t)lane;
                        Elem c = Sel::none();
                        bool ok = i < ee;
                        if (ok) {
                            const float4 t = g.pts[i];
                            c = Sel::make(l2_simple(q.x, q.y, q.z, t.x, t.y, t.z), __float_as_uint(t.w));
                            ok = Sel::takes(c, bound);
                        }
                        const unsigned long long m = __ballot(ok);
                        if (ok) buf[count + __popcll(m & lt)] = c;
                        count += __popcll(m);
                        dirty = dirty || m != 0ull;
                    }
                }
            }
        }
        if (done) break;
        if (count >= kept) {
            if (dirty) {
                knn_select<Sel>(buf, lane, kept, count, bound, bound_d2);
                dirty = false;
            }
            if constexpr (Sel::kEndsAtZero) {
                if (bound_d2 == 0.0f) break;
            }
            // every cell not visited yet lies beyond one of the six faces of the cube of shell r
            float out = inf;
            if (cx + r + 1 < g.dx) out = fminf(out, grid_lb2(axis_gap(ux, cx + r + 1, g.dx - 1), 0.0f, 0.0f, g.cell));
            if (cx - r - 1 >= 0) out = fminf(out, grid_lb2(axis_gap(ux, 0, cx - r - 1), 0.0f, 0.0f, g.cell));
            if (cy + r + 1 < g.dy) out = fminf(out, grid_lb2(0.0f, axis_gap(uy, cy + r + 1, g.dy - 1), 0.0f, g.cell));
            if (cy - r - 1 >= 0) out = fminf(out, grid_lb2(0.0f, axis_gap(uy, 0, cy - r - 1), 0.0f, g.cell));
            if (cz + r + 1 < g.dz) out = fminf(out, grid_lb2(0.0f, 0.0f, axis_gap(uz, cz + r + 1, g.dz - 1), g.cell));
            if (cz - r - 1 >= 0) out = fminf(out, grid_lb2(0.0f, 0.0f, axis_gap(uz, 0, cz - r - 1), g.cell));
            if (out > bound_d2) break;   // (strictly: a record AT the bound's distance may still carry a lower index)
        }
    }
    if (dirty) knn_select<Sel>(buf, lane, kept, count, bound, bound_d2);
    __syncthreads();
    return count;
}

// One workgroup of ONE wave per query, queries in cell order (a grid-stride loop: the waves in flight work on neighbouring
// cells).  dist[record] = (float)(sum_{j = 1 .. k} (double)sqrtf(d2[j]) / k), d2 ascending, d2[0] (the point itself) dropped.
__global__ __launch_bounds__(kKnnWave) void k_knn_mean_distance(PointGridDev g, int k, float *dist)
{
    __shared__ float buf[kKnnBuf];
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        const int count = knn_walk<KnnValues>(g, q, k + 1, buf, lane);
        if (lane == 0) {
            double sum = 0.0;
            for (int i = 1; i < count; ++i) sum += (double)(float)sqrt((double)buf[i]);   // ascending; the float sqrt, correctly rounded (through f64: 53 >= 2 * 24 + 2 bits), f64 sum
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
