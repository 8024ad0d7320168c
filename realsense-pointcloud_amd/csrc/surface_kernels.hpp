// surface_kernels.hpp — setSearchSurface: the exact radius search of the records of one cloud (the queries) in another (the surface),
// and its consumers -- counts, pcl::NormalEstimation and pcl::FPFHEstimationOMP with setRadiusSearch (include/rsreg.h, which holds
// the contract: rsreg_cloud_radius_count_surface, rsreg_cloud_normals_radius_surface, rsreg_cloud_fpfh_radius_surface,
// rsreg_cloud_spfh_radius_surface).  Included by filters.hip only.  The index is radius_kernels.hpp's, built over the SURFACE; the
// walks, the moments, the SPFH row and the weighting are radius_kernels.hpp's and fpfh_radius_kernels.hpp's, unchanged.
//
// A query is not an indexed point: it comes from its own cloud, and radius_walk clamps the box of cells of one that lies outside
// the grid (radius_axis_cells).  The host sorts the finite queries by the surface cell they fall in (k_radius_cell_keys against
// the surface's grid, osort.hpp) and the kernels go through that order, one wave per query: neighbouring waves read the same
// rows of cells.  The order decides nothing else -- every sum of a query runs in the walk order of the surface's index, and every
// row lands at the query's own record.  Non-finite queries carry the key above every cell and end the loop.
//   k_surface_count_mark    m per query, and a plain store of 1 into mark[surface record] for every hit (every writer of a word
//                           writes the same value: no atomic)
//   k_surface_needed        the marks in the order of the index, for the prefix sum that numbers the needed records
//   k_surface_list          the places in the index of the needed records, ascending
//   k_surface_spfh          radius_spfh_row of the listed records only: the bytes rsreg_cloud_spfh_radius gives them
//   k_surface_fpfh_weight   RadiusFpfhWeigh over the queries: no normal of the query is looked at; m = 0 gives NaNs
//   k_surface_normals       RadiusMoments about the query, wave_sum_fixed, normal_from_sums
// Nothing here uses a float atomic.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fpfh_radius_kernels.hpp"

namespace rsreg {

// the queries of a call: their records, and (key, record) sorted by key -- the surface cell, no_cell for a non-finite record
struct SurfaceQueries {
    const char *rec;
    size_t stride;
    const uint32_t *keys, *order;
    uint32_t n, no_cell;
    // the j-th query in cell order as a walk takes it: x, y, z and its record as the tag; false from the first non-finite one on
    __device__ __forceinline__ bool at(uint32_t j, float4 &q) const
    {
        if (keys[j] == no_cell) return false;
        const uint32_t i = order[j];
        const float *p = rec_xyz(rec, stride, i);
        q = make_float4(p[0], p[1], p[2], __uint_as_float(i));
        return true;
    }
};

struct SurfaceCountMark {
    uint32_t *mark;
    uint32_t n = 0;
    __device__ __forceinline__ void operator()(const float4 &t)
    {
        ++n;
        mark[__float_as_uint(t.w)] = 1u;
    }
};

// One workgroup of ONE wave per finite query.  count[query record] = m, its neighbours in the surface (the words of non-finite
// queries have been zeroed before the launch); mark (nullable: counts only), zero on entry: 1 for every surface record that is a
// neighbour of a query.
__global__ __launch_bounds__(kKnnWave) void k_surface_count_mark(PointGridDev g, RadiusQuery rq, SurfaceQueries sq, uint32_t *count, uint32_t *mark)
{
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < sq.n; j += gridDim.x) {
        float4 q;
        if (!sq.at(j, q)) break;
        uint32_t m;
        if (mark) {
            SurfaceCountMark c{mark};
            radius_walk(g, q, rq, lane, c);
            m = c.n;
        } else {
            RadiusCount c;
            radius_walk(g, q, rq, lane, c);
            m = c.n;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
        if (lane == 0) count[__float_as_uint(q.w)] = m;
    }
}

// flags[j] = whether the point j of the index is needed
__global__ __launch_bounds__(kBlock) void k_surface_needed(PointGridDev g, const uint32_t *mark, uint32_t *flags)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    flags[j] = mark[__float_as_uint(g.pts[j].w)];
}

// incl: the inclusive prefix sum of k_surface_needed's flags.  list[u] = the u-th needed point of the index.
__global__ __launch_bounds__(kBlock) void k_surface_list(const uint32_t *incl, uint32_t n, uint32_t *list)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t here = incl[j], before = j ? incl[j - 1] : 0u;
    if (here != before) list[before] = j;
}

// One workgroup of ONE wave per listed point of the surface's index: k_fpfh_radius_spfh's row, the record's neighbourhood in the
// surface and the surface's normals.  Rows that are not listed are not written.
__global__ __launch_bounds__(kKnnWave) void k_surface_spfh(PointGridDev g, RadiusQuery rq, const char *nrm, size_t nstride, const uint32_t *list, uint32_t n_list,
                                                           float *spfh)
{
    __shared__ float4 queue[2 * kKnnWave];
    __shared__ uint32_t cnt[kFpfhRow];
    const int lane = (int)threadIdx.x;
    for (uint32_t u = blockIdx.x; u < n_list; u += gridDim.x) radius_spfh_row(g, rq, nrm, nstride, g.pts[list[u]], queue, cnt, lane, spfh, nullptr);
}

// One workgroup of ONE wave per finite query: k_fpfh_radius_weight's sums over the query's neighbours in the surface.  count: what
// k_surface_count_mark left; m = 0 gives 33 quiet NaNs and sets *any_nan, and so does every row the arithmetic leaves a NaN in.
// The rows of non-finite queries have been written before the launch (k_fpfh_radius_not_finite).
__global__ __launch_bounds__(kKnnWave) void k_surface_fpfh_weight(PointGridDev g, RadiusQuery rq, SurfaceQueries sq, const uint32_t *count, const float *spfh,
                                                                  float *out, uint32_t *any_nan)
{
#pragma clang fp contract(off)
    __shared__ double hs[kFpfhRow];
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < sq.n; j += gridDim.x) {
        float4 q;
        if (!sq.at(j, q)) break;
        const size_t record = (size_t)__float_as_uint(q.w);
        if (count[record] == 0u) {   // (the whole wave alike)
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
        __syncthreads();   // (the sums have been read: the next query may overwrite them)
    }
}

// One workgroup of ONE wave per finite query: k_normals_radius with q taken from the query cloud -- the covariance about the query
// over its m neighbours in the surface, the flip towards the viewpoint from the query.  m < 3: four quiet NaNs, and *any_nan = 1.
__global__ __launch_bounds__(kKnnWave) void k_surface_normals(PointGridDev g, RadiusQuery rq, SurfaceQueries sq, float vpx, float vpy, float vpz, float *out,
                                                              uint32_t *any_nan)
{
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < sq.n; j += gridDim.x) {
        float4 q;
        if (!sq.at(j, q)) break;
        RadiusMoments a;
        a.qx = (double)q.x; a.qy = (double)q.y; a.qz = (double)q.z;
        radius_walk(g, q, rq, lane, a);
        uint32_t m = a.n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
        if (m < 3u) {
            if (lane < 8) out[(size_t)__float_as_uint(q.w) * 8 + (size_t)lane] = (lane < 3 || lane == 4) ? __uint_as_float(0x7fc00000u) : 0.0f;
            if (lane == 0) *any_nan = 1u;
            continue;
        }
        const double sx = wave_sum_fixed(a.sx), sy = wave_sum_fixed(a.sy), sz = wave_sum_fixed(a.sz);
        const double sxx = wave_sum_fixed(a.sxx), sxy = wave_sum_fixed(a.sxy), sxz = wave_sum_fixed(a.sxz);
        const double syy = wave_sum_fixed(a.syy), syz = wave_sum_fixed(a.syz), szz = wave_sum_fixed(a.szz);
        normal_from_sums(q, (double)m, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, vpx, vpy, vpz, lane, out);
    }
}

// every row of a call whose surface holds no finite record: `row` floats each, quiet NaN where the row's bit of nan_mask is set, else 0
__global__ __launch_bounds__(kBlock) void k_surface_no_neighbours(float *out, size_t words, uint32_t row, unsigned long long nan_mask)
{
    const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= words) return;
    out[at] = (nan_mask >> (at % row)) & 1ull ? __uint_as_float(0x7fc00000u) : 0.0f;
}

}  // namespace rsreg
