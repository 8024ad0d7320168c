// fpfh_radius_kernels.hpp — pcl::FPFHEstimationOMP with setRadiusSearch over the exact radius search (radius_kernels.hpp:
// radius_walk_wave): device code of rsreg_cloud_spfh_radius and rsreg_cloud_fpfh_radius (include/rsreg.h, which holds the
// contract).  Included by filters.hip only; the pair features and the bins are fpfh_kernels.hpp's.
//
// A neighbourhood has no cap, so no neighbour list is kept: both passes walk the ball, one wave per finite record in cell order.
//   k_fpfh_radius_spfh    the hits of every 64-point read are packed into a queue in LDS (a ballot and a prefix count); whenever
//                         it holds 64 the whole wave takes one neighbour each -- the f64 pair features run with every lane busy,
//                         not with the few lanes of a read that hit.  The bins are counted with integer LDS adds, which commute:
//                         neither the queue's order nor lane timing enters.  Lane b then adds hist_incr to 0.0f cnt[b] times, one
//                         float addition after the other: the loop IS PCL's sequential +=, whatever the count.
//   k_fpfh_radius_weight  the hits of a read are handed round in ascending lane order, four at a time: lane b < 33 owns bin b, reads
//                         one 132-byte SPFH row per neighbour (coalesced), and adds the float32 product to its f64 sum.  The
//                         order -- rows of cells, a row's points, a read's lanes, all ascending -- is a function of the index
//                         alone, and the index places a cell's points in ascending record index.
// Nothing here uses a float atomic.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fpfh_kernels.hpp"
#include "radius_kernels.hpp"

namespace rsreg {

// the lanes below this one among the set bits of a ballot
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane)
{
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// The consumer of the first pass.  queue: 2 * kKnnWave points (fewer than 64 wait, a read adds at most 64); cnt: the 33 counts.
struct RadiusSpfhPairs {
    float4 *queue;
    uint32_t *cnt;
    const char *nrm;
    size_t nstride;
    float4 q;
    float nix, niy, niz;
    bool own;        // the record's own normal is finite: otherwise nothing is counted but m
    int lane;
    uint32_t queued = 0, m = 0;

    // the lanes below `have` take one queued neighbour each
    __device__ __forceinline__ void pairs(uint32_t have)
    {
        if ((uint32_t)lane < have) {
            const float4 t = queue[lane];
            const uint32_t nb = __float_as_uint(t.w);
            if (nb != __float_as_uint(q.w)) {
                const float *nj = rec_xyz(nrm, nstride, nb);
                const float pj[3] = {t.x, t.y, t.z};
                int bin[3];
                if (finite3(nj[0], nj[1], nj[2]) && fpfh_pair_bins(q.x, q.y, q.z, nix, niy, niz, pj, nj, bin)) {
                    atomicAdd(&cnt[bin[0]], 1u);
                    atomicAdd(&cnt[kFpfhBins + bin[1]], 1u);
                    atomicAdd(&cnt[2 * kFpfhBins + bin[2]], 1u);
                }
            }
        }
    }
    __device__ __forceinline__ void operator()(const float4 t, bool hit)
    {
        const unsigned long long mask = __ballot(hit);
        const uint32_t hits = (uint32_t)__popcll(mask);
        m += hits;
        if (!own || !hits) return;   // (the whole wave alike)
        if (hit) queue[queued + (uint32_t)lanes_below(mask, lane)] = t;   // (queued < 64: below 2 * kKnnWave)
        queued += hits;
        if (queued >= (uint32_t)kKnnWave) {
            __syncthreads();
            pairs((uint32_t)kKnnWave);
            const uint32_t rest = queued - (uint32_t)kKnnWave;
            float4 keep = t;
            if ((uint32_t)lane < rest) keep = queue[kKnnWave + lane];
            __syncthreads();
            if ((uint32_t)lane < rest) queue[lane] = keep;
            queued = rest;
        }
    }
    __device__ __forceinline__ void finish()
    {
        __syncthreads();
        pairs(queued);
        __syncthreads();
    }
};

// The SPFH row of the indexed point q (q.w: its record) by one wave: row `record` of spfh, the 33 floats; count[record] (nullable) = m,
// the neighbours within the radius, the record itself among them.  queue, cnt: the workgroup's LDS (RadiusSpfhPairs); the barrier at
// the end lets the next row clear the counts.
__device__ __forceinline__ void radius_spfh_row(const PointGridDev &g, const RadiusQuery rq, const char *nrm, size_t nstride, const float4 q, float4 *queue,
                                                uint32_t *cnt, int lane, float *spfh, uint32_t *count)
{
    const size_t record = (size_t)__float_as_uint(q.w);
    const float *ni = rec_xyz(nrm, nstride, record);
    RadiusSpfhPairs f{queue, cnt, nrm, nstride, q, ni[0], ni[1], ni[2], false, lane};
    f.own = finite3(f.nix, f.niy, f.niz);
    if (lane < kFpfhRow) cnt[lane] = 0u;
    __syncthreads();
    radius_walk_wave(g, q, rq, lane, f);
    f.finish();
    if (lane < kFpfhRow) {
        // m == 1: no pair, no addition -- the infinite increment is never used
        const float hist_incr = __fdiv_rn(100.0f, (float)(f.m - 1u));
        const uint32_t c = cnt[lane];
        float acc = 0.0f;
        for (uint32_t u = 0; u < c; ++u) acc = __fadd_rn(acc, hist_incr);
        spfh[record * kFpfhRow + (size_t)lane] = acc;
    }
    if (count && lane == 0) count[record] = f.m;
    __syncthreads();   // (the counts have been read: the next row may clear them)
}

// One workgroup of ONE wave per finite record, queries in cell order (the grid-stride loop of k_normals_radius): radius_spfh_row of
// every indexed point.  The rows and counts of records not visited (non-finite ones) have been zeroed before the launch.
__global__ __launch_bounds__(kKnnWave) void k_fpfh_radius_spfh(PointGridDev g, RadiusQuery rq, const char *nrm, size_t nstride, float *spfh, uint32_t *count)
{
    __shared__ float4 queue[2 * kKnnWave];
    __shared__ uint32_t cnt[kFpfhRow];
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) radius_spfh_row(g, rq, nrm, nstride, g.pts[j], queue, cnt, lane, spfh, count);
}

// The consumer of the second pass: lane b < 33 owns bin b.
struct RadiusFpfhWeigh {
    const float *spfh;
    float4 q;
    int lane;
    double h = 0.0;

    __device__ __forceinline__ void operator()(const float4 t, bool hit)
    {
        // d2 != 0 leaves out the record itself and exact copies
        const float d2 = l2_simple(q.x, q.y, q.z, t.x, t.y, t.z);
        const float w = __fdiv_rn(1.0f, d2);
        const uint32_t tag = __float_as_uint(t.w);
        unsigned long long todo = __ballot(hit && d2 != 0.0f);
        while (todo) {
            // four neighbours at a time, in ascending lane order: their rows are in flight together
            bool on[4];
            float wa[4], s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                on[u] = todo != 0ull;
                const int l = on[u] ? __ffsll((long long)todo) - 1 : 0;
                todo &= todo - 1ull;   // (0 stays 0)
                const uint32_t nb = __shfl(tag, l);
                wa[u] = __shfl(w, l);
                s[u] = (on[u] && lane < kFpfhRow) ? spfh[(size_t)nb * kFpfhRow + (size_t)lane] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (on[u]) h = h + (double)__fmul_rn(s[u], wa[u]);
        }
    }
};

// One workgroup of ONE wave per finite record, queries in cell order.  out: record `record`'s 33 floats; a record whose own normal
// is not finite gets quiet NaNs and sets *any_nan, and so does every row the arithmetic leaves a NaN in.  The rows of non-finite
// records have been written before the launch (k_fpfh_radius_not_finite).
__global__ __launch_bounds__(kKnnWave) void k_fpfh_radius_weight(PointGridDev g, RadiusQuery rq, const char *nrm, size_t nstride, const float *spfh, float *out,
                                                                 uint32_t *any_nan)
{
#pragma clang fp contract(off)
    __shared__ double hs[kFpfhRow];
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        const size_t record = (size_t)__float_as_uint(q.w);
        const float *ni = rec_xyz(nrm, nstride, record);
        if (!finite3(ni[0], ni[1], ni[2])) {   // (the whole wave alike)
            if (lane < kFpfhRow) out[record * kFpfhRow + (size_t)lane] = __uint_as_float(0x7fc00000u);
            if (lane == 0) *any_nan = 1u;
            continue;
        }
        RadiusFpfhWeigh f{spfh, q, lane};
        radius_walk_wave(g, q, rq, lane, f);
        if (lane < kFpfhRow) hs[lane] = f.h;
        __syncthreads();
        bool is_nan = false;
        if (lane < kFpfhRow) {
            const int t = lane / kFpfhBins;
            double sum = 0.0;
#pragma unroll
            for (int b = 0; b < kFpfhBins; ++b) sum = sum + hs[t * kFpfhBins + b];
            const float r = (float)(f.h * (sum != 0.0 ? 100.0 / sum : 0.0));
            out[record * kFpfhRow + (size_t)lane] = r;
            is_nan = r != r;
        }
        if (__ballot(is_nan) != 0ull && lane == 0) *any_nan = 1u;
        __syncthreads();   // (the sums have been read: the next record may overwrite them)
    }
}

// the rows of the records the index does not hold: 33 quiet NaNs each; one thread per float
__global__ __launch_bounds__(kBlock) void k_fpfh_radius_not_finite(const char *rec, size_t stride, uint32_t n, float *out)
{
    const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= (size_t)n * kFpfhRow) return;
    const float *p = rec_xyz(rec, stride, at / kFpfhRow);
    if (!finite3(p[0], p[1], p[2])) out[at] = __uint_as_float(0x7fc00000u);
}

}  // namespace rsreg
