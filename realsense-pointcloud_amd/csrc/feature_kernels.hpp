// feature_kernels.hpp — exact k-nearest-neighbour search across two clouds in descriptor space (33 floats a row, what
// rsreg_cloud_fpfh writes) and the correspondence lists over it: device code of rsreg_cloud_feature_knn and
// rsreg_cloud_feature_correspondences (include/rsreg.h, which holds the contract).  Included by features.hip only.
//
// No index: a k-d tree in 33 dimensions is a linear scan with overhead, and the point grid is three-dimensional.  Every query row
// meets every target row, 33 subtractions, 33 multiplications and 32 additions a pair in the contract's order.
//   k_fm_valid     one thread per row: whether its 33 floats are finite, and how many rows are.
//   k_fm_search<K> one wave per workgroup, ONE LANE PER QUERY ROW (33 VGPRs, loaded once), one slice of the target (feature_plan.hpp)
//                  in tiles of 64 rows staged in LDS.  Every lane reads the same LDS address -- a broadcast, no bank conflict; rows
//                  are padded to 36 floats so that a row is eight ds_read_b128 and one ds_read_b32 -- and kFmFlight target rows are in
//                  flight at once: the order INSIDE a pair is the contract's, independent pairs interleave.  Each lane keeps its K
//                  best (d2 bits << 32 | target index) keys in registers, ascending, by a fully unrolled compare-exchange
//                  insertion behind the guard "d2 bits above the worst kept: skip".  The key is monotone in (d2, index): d2 >= +0
//                  and never NaN between valid rows (a difference that overflows gives +inf, never inf - inf).
//                  K == 1: the slices merge by a 64-bit integer atomicMin on the query's key.  K > 1: every slice leaves its K
//                  keys, and
//   k_fm_merge<K>  one thread per query selects the k smallest of its slices' keys -- the keys are unique, so the selection is
//                  exact -- and writes indices and distances (an invalid query: -1 and 0).
//   k_fm_corr_*    correspondence rules on the forward (and reverse) K = 1 keys: flags, then -- behind oscan.hpp's prefix sum -- the
//                  ordered gather and the 8-byte count.
// Nothing here uses a float atomic: a minimum of unique integer keys does not depend on the order it is taken in.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rsreg.h"
#include "feature_plan.hpp"

namespace rsreg {

constexpr int kFmDim = 33;                 // floats of a descriptor row (pcl::FPFHSignature33)
constexpr int kFmRowPad = 36;              // floats a staged row takes in LDS: 144 bytes, 16-byte aligned
constexpr int kFmLanes = 64;               // threads of a search workgroup: one wave
constexpr int kFmFlight = 2;               // target rows whose pairs a lane has in flight at once
constexpr uint32_t kFmBlock = 256;         // threads of the one-thread-per-row kernels
constexpr unsigned long long kFmNone = ~0ull;
static_assert(kFmQueries == (uint32_t)kFmLanes && kFmTile % kFmFlight == 0 && kFmTile <= (uint32_t)kFmLanes, "one lane a query; a lane a tile row's flag; rows kFmFlight at a time");

__device__ __forceinline__ bool fm_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// valid[i] = all 33 floats of row i are finite (DefaultPointRepresentation::isValid); *count += the rows that are
__global__ __launch_bounds__(kFmBlock) void k_fm_valid(const char *rec, size_t stride, uint32_t n, uint32_t *valid, uint32_t *count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const float *r = reinterpret_cast<const float *>(rec + (size_t)i * stride);
        ok = true;
#pragma unroll
        for (int b = 0; b < kFmDim; ++b) ok = ok & fm_finite(r[b]);
        valid[i] = ok ? 1u : 0u;
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(count, (uint32_t)__popcll(m));
}

// best[0 .. K) ascending; `key` differs from every key in it (another target index) or the slot is still kFmNone
template <int K> __device__ __forceinline__ void fm_insert(unsigned long long (&best)[K], unsigned long long key)
{
    if (key < best[K - 1]) {
        best[K - 1] = key;
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            const unsigned long long a = best[j - 1], b = best[j];
            const bool sw = b < a;
            best[j - 1] = sw ? b : a;
            best[j] = sw ? a : b;
        }
    }
}

// one more bin of a pair: d += (q - t) * (q - t), three roundings
__device__ __forceinline__ float fm_bin(float d, float q, float t)
{
    const float diff = __fsub_rn(q, t);
    return __fadd_rn(d, __fmul_rn(diff, diff));
}

// Workgroup b: query block b / slices, target slice b % slices.  K == 1: out = one key per query, kFmNone before the launch, merged
// by atomicMin.  K > 1: out = K keys per (slice, query), key j of slice s of query i at ((s * K + j) * nq + i), all written.
template <int K> __global__ __launch_bounds__(kFmLanes) void k_fm_search(const char *qrec, size_t qstride, const uint32_t *qvalid, uint32_t nq,
                                                                         const char *trec, size_t tstride, const uint32_t *tvalid, uint32_t nt,
                                                                         uint32_t slices, unsigned long long *out)
{
    __shared__ __attribute__((aligned(16))) float s_row[kFmTile * kFmRowPad];
    __shared__ uint32_t s_ok[kFmTile];
    const uint32_t lane = threadIdx.x;
    const uint32_t qb = blockIdx.x / slices, s = blockIdx.x - qb * slices;
    const uint32_t t_lo = feature_slice_begin(s, slices, nt), t_hi = feature_slice_begin(s + 1, slices, nt);
    const uint32_t i = qb * kFmQueries + lane;
    const bool live = i < nq && qvalid[i] != 0;   // (a lane past the end or on an invalid row walks along and keeps nothing)
    float q[kFmDim];
    {
        const float *r = reinterpret_cast<const float *>(qrec + (size_t)(i < nq ? i : nq - 1) * qstride);
#pragma unroll
        for (int b = 0; b < kFmDim; ++b) q[b] = r[b];
    }
    unsigned long long best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = kFmNone;

    for (uint32_t t0 = t_lo; t0 < t_hi; t0 += kFmTile) {
        const uint32_t rows = t_hi - t0 < kFmTile ? t_hi - t0 : kFmTile;
        __syncthreads();   // (the tile before has been read)
        for (uint32_t e = lane; e < rows * kFmDim; e += kFmLanes) {
            const uint32_t r = e / kFmDim, c = e - r * kFmDim;
            s_row[r * kFmRowPad + c] = *reinterpret_cast<const float *>(trec + (size_t)(t0 + r) * tstride + (size_t)c * 4);
        }
        if (lane < kFmTile) s_ok[lane] = lane < rows ? tvalid[t0 + lane] : 0u;   // (rows past the slice: never a candidate)
        __syncthreads();
        for (uint32_t r = 0; r < rows; r += kFmFlight) {
            const float *p = s_row + r * kFmRowPad;
            float d[kFmFlight];
            {   // bin 0: 0.0f + x is x for every x >= +0, the first addition of the contract is the square itself
#pragma unroll
                for (int j = 0; j < kFmFlight; ++j) {
                    const float diff = __fsub_rn(q[0], p[j * kFmRowPad]);
                    d[j] = __fmul_rn(diff, diff);
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float4 a[kFmFlight];
#pragma unroll
                for (int j = 0; j < kFmFlight; ++j) a[j] = *reinterpret_cast<const float4 *>(p + j * kFmRowPad + 4 * c);
#pragma unroll
                for (int j = 0; j < kFmFlight; ++j) {
                    if (c > 0) d[j] = fm_bin(d[j], q[4 * c], a[j].x);
                    d[j] = fm_bin(d[j], q[4 * c + 1], a[j].y);
                    d[j] = fm_bin(d[j], q[4 * c + 2], a[j].z);
                    d[j] = fm_bin(d[j], q[4 * c + 3], a[j].w);
                }
            }
#pragma unroll
            for (int j = 0; j < kFmFlight; ++j) d[j] = fm_bin(d[j], q[32], p[j * kFmRowPad + 32]);
#pragma unroll
            for (int j = 0; j < kFmFlight; ++j) {
                const uint32_t bits = __float_as_uint(d[j]);
                if (live && s_ok[r + j] != 0 && bits <= (uint32_t)(best[K - 1] >> 32))
                    fm_insert<K>(best, ((unsigned long long)bits << 32) | (unsigned long long)(t0 + r + (uint32_t)j));
            }
        }
    }
    if (K == 1) {
        if (live && best[0] != kFmNone) atomicMin(&out[i], best[0]);
    } else if (i < nq) {
#pragma unroll
        for (int j = 0; j < K; ++j) out[((size_t)s * K + j) * nq + i] = best[j];
    }
}

// keys: `lists` keys per query, key e of query i at keys[e * nq + i] (kFmNone: no candidate).  The k <= K smallest, ascending, to
// row i of index_out / d2_out (each nullable); a query that is not valid gets -1 and 0.
template <int K> __global__ __launch_bounds__(kFmBlock) void k_fm_merge(const unsigned long long *keys, uint32_t lists, const uint32_t *qvalid, uint32_t nq,
                                                                        int k, int32_t *index_out, float *d2_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    unsigned long long best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = kFmNone;
    const bool ok = qvalid[i] != 0;
    if (ok)
        for (uint32_t e = 0; e < lists; ++e) {
            const unsigned long long key = keys[(size_t)e * nq + i];
            if (key != kFmNone) fm_insert<K>(best, key);
        }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) {
            const bool hit = ok && best[j] != kFmNone;
            if (index_out) index_out[(size_t)i * k + j] = hit ? (int32_t)(uint32_t)best[j] : -1;
            if (d2_out) d2_out[(size_t)i * k + j] = hit ? __uint_as_float((uint32_t)(best[j] >> 32)) : 0.0f;
        }
    }
}

// flags[i] = source row i keeps its match: fwd[i] is its nearest valid target row (kFmNone: none, or the row is not valid), kept
// unless (double)d2 > max_sqr; rev (nullable: not reciprocal) holds every target row's nearest valid source row, and the match is
// kept only if that row is i and its distance passes the same test.
__global__ __launch_bounds__(kFmBlock) void k_fm_corr_flags(const unsigned long long *fwd, const unsigned long long *rev, uint32_t ns, double max_sqr,
                                                            uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const unsigned long long key = fwd[i];
    bool keep = key != kFmNone && !((double)__uint_as_float((uint32_t)(key >> 32)) > max_sqr);
    if (keep && rev) {
        const unsigned long long back = rev[(uint32_t)key];
        keep = back != kFmNone && !((double)__uint_as_float((uint32_t)(back >> 32)) > max_sqr) && (uint32_t)back == i;
    }
    flags[i] = keep ? 1u : 0u;
}

// pos: the exclusive prefix sum of flags.  The kept matches in the order of their source rows, the first `capacity` of them; *count =
// how many there are.
__global__ __launch_bounds__(kFmBlock) void k_fm_corr_gather(const unsigned long long *fwd, const uint32_t *flags, const uint32_t *pos, uint32_t ns,
                                                             unsigned long long capacity, rsreg_correspondence *out, unsigned long long *count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    if (flags[i] && pos[i] < capacity) {
        const unsigned long long key = fwd[i];
        rsreg_correspondence c;
        c.index_query = (int32_t)i;
        c.index_match = (int32_t)(uint32_t)key;
        c.distance = __uint_as_float((uint32_t)(key >> 32));
        out[pos[i]] = c;
    }
    if (i == ns - 1) *count = (unsigned long long)pos[i] + flags[i];
}

}  // namespace rsreg
