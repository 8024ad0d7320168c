// prerej_kernels.hpp — the kernels of pcl::SampleConsensusPrerejective (prerej.hip; C ABI and contract: include/rsreg.h, "pose from
// descriptor neighbours"): hypotheses from three source records and a random one of each one's k nearest descriptors, thrown away on
// a cheap edge-length test, the survivors scored against the WHOLE target cloud by an exact nearest-point search.
//
//   k_prerej_hypotheses   one lane per hypothesis: six draws, the six points, the polygon test, 17 sums, umeyama_from_sums -> a
//                         3 x 4 table row, a valid flag, the sample
//   k_prerej_score        THE HOT PATH: for every valid row of a slice of the table, the inliers of a tile of source records and
//                         the two waves' sums of their d2 (one exact nearest-neighbour query per (hypothesis, source record))
//   k_prerej_final        one lane per hypothesis: its partials added in ascending group order
//   k_prerej_flags        the inlier flags of the source records under one transform (the winner's)
//   k_prerej_emit         the flagged record numbers, compacted in ascending order (positions: oscan.hpp)
//
// The search is pointgrid.hpp's fit_nearest over a block-major PointGrid of the target (FitGridPolicy): exact at any range and for
// queries far outside the target's box, which is where a random pose throws the source.
#pragma once

#include "records.hpp"
#include "pointgrid.hpp"
#include "prerej_plan.hpp"
#include "prerej_score.hpp"

namespace rsreg {

constexpr int kPrejLanes = 256;   // the one-item-a-lane kernels' workgroup

// the target's records for the grid build: x, y, z at the head of a record of any stride; an indexed point carries no tag
struct PrejRecords {
    const char *rec;
    size_t stride;
    __device__ __forceinline__ float3 xyz(uint32_t i) const
    {
        const float *p = rec_xyz(rec, stride, i);
        return make_float3(p[0], p[1], p[2]);
    }
    __device__ __forceinline__ float tag(uint32_t) const { return 0.0f; }
    __device__ __forceinline__ void not_finite(uint32_t) const {}
};

// Hypothesis h0 + j (j < count) of the contract.  table[12 * j ..] = the rows of its transform, valid[j] = 1 when it has one
// (otherwise the row is NaN and valid[j] = 0), sample[8 * j ..] = its three source records and its three target records (-1 x 6
// when the draws gave none: an ineligible record).  nbr: ns rows of k target records, a row of -1 for an ineligible source record;
// the host has checked every other entry against nt.
__global__ __launch_bounds__(64) void k_prerej_hypotheses(const char *src, size_t sstride, uint32_t ns, const char *tgt, size_t tstride, const int32_t *nbr,
                                                          uint32_t k, unsigned long long seed, unsigned long long h0, uint32_t count, float sim2,
                                                          float *table, uint32_t *valid, int32_t *sample)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const unsigned long long h = h0 + j;
    uint32_t id[3];
    int32_t match[3] = {-1, -1, -1};
    bool ok = true;
    for (int d = 0; d < 3; ++d) id[d] = sac_draw(seed, h, (uint32_t)d, ns);
    for (int d = 0; d < 3; ++d) {
        const uint32_t col = sac_draw(seed, h, 3u + (uint32_t)d, k);
        const int32_t *row = nbr + (size_t)id[d] * k;
        if (row[0] < 0) ok = false; else match[d] = row[col];
    }
    ok = ok && id[0] != id[1] && id[0] != id[2] && id[1] != id[2];
    Mat4f T;
    bool good = false;
    if (ok) {
        float P[3][3], Q[3][3];
        for (int d = 0; d < 3; ++d) {
            const float *p = rec_xyz(src, sstride, id[d]), *q = rec_xyz(tgt, tstride, (size_t)match[d]);
            for (int c = 0; c < 3; ++c) { P[d][c] = p[c]; Q[d][c] = q[c]; }
            ok = ok && finite3(P[d][0], P[d][1], P[d][2]) && finite3(Q[d][0], Q[d][1], Q[d][2]);
        }
        // the polygon test (CorrespondenceRejectorPoly::thresholdPolygon): squared edge lengths, the smaller over the larger, float32
        for (int a = 0; a < 3 && ok; ++a) {
            const int b = (a + 1) % 3;
            const float ds = l2_simple(P[a][0], P[a][1], P[a][2], P[b][0], P[b][1], P[b][2]);
            const float dt = l2_simple(Q[a][0], Q[a][1], Q[a][2], Q[b][0], Q[b][1], Q[b][2]);
            const float sim = ds < dt ? __fdiv_rn(ds, dt) : __fdiv_rn(dt, ds);
            ok = sim >= sim2;   // (NaN, which 0 / 0 gives, fails)
        }
        if (ok) {
            double s[RSREG_NUM_SUMS];
            for (int i = 0; i < RSREG_NUM_SUMS; ++i) s[i] = 0.0;
            for (int d = 0; d < 3; ++d) {   // (the sums of k_sac_hypotheses: a weight of one, in pair order)
                const double p[3] = {P[d][0], P[d][1], P[d][2]}, q[3] = {Q[d][0], Q[d][1], Q[d][2]};
                s[0] += 1.0;
                for (int c = 0; c < 3; ++c) { s[1 + c] += p[c]; s[4 + c] += q[c]; }
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) s[7 + r * 3 + c] += q[r] * p[c];
                s[16] += (double)l2_simple(P[d][0], P[d][1], P[d][2], Q[d][0], Q[d][1], Q[d][2]);
            }
            good = umeyama_from_sums(s, T);
        }
    }
    const float nan = __uint_as_float(0x7fc00000u);
    float *row = table + (size_t)j * 12;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) row[r * 4 + c] = good ? T(r, c) : nan;
    valid[j] = good ? 1u : 0u;
    int32_t *s8 = sample + (size_t)j * 8;
    const bool drawn = match[0] >= 0 && match[1] >= 0 && match[2] >= 0;
    for (int d = 0; d < 3; ++d) {
        s8[d] = drawn ? (int32_t)id[d] : -1;
        s8[3 + d] = drawn ? match[d] : -1;
    }
    s8[6] = s8[7] = 0;
}

// Workgroup b: tile b % tiles of the source against slice b / tiles of the table (prerej_plan.hpp).  A lane keeps its record in
// registers for the whole slice.  The row and its valid flag are read through addresses that depend on the workgroup and the loop
// counter alone, i.e. by the scalar unit, once a wave; an invalid row is skipped by both waves without a search.  A wave's count
// of one hypothesis is a ballot's population count, a scalar; lane j keeps the one of the chunk's j-th hypothesis, so a chunk costs
// a wave one integer atomicAdd instruction.  A wave's d2 sum goes to a place of its own, partials[(h * tiles + tile) * 2 + wave]:
// no float atomics, one writer a word.  valid == nullptr: every row is scored.
__global__ __launch_bounds__(kPrejBlock) void k_prerej_score(const char *__restrict__ src, size_t sstride, uint32_t ns, const float *__restrict__ table,
                                                             const uint32_t *__restrict__ valid, uint32_t H, uint32_t tiles, uint32_t slice_chunks,
                                                             PointGridDev g, float limit2, uint32_t *__restrict__ counts, double *__restrict__ partials)
{
    const uint32_t tile = prerej_group_tile(blockIdx.x, tiles), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float nan = __uint_as_float(0x7fc00000u);
    float px = nan, py = nan, pz = nan;
    const size_t i = (size_t)tile * kPrejTile + threadIdx.x;
    if (i < ns) {
        const float *p = rec_xyz(src, sstride, i);
        px = p[0]; py = p[1]; pz = p[2];
    }
    uint32_t h_first, h_end;
    prerej_group_slice(blockIdx.x, tiles, slice_chunks, H, &h_first, &h_end);
    for (uint32_t h0 = h_first; h0 < h_end; h0 += kPrejChunk) {
        const uint32_t m = h_end - h0 < kPrejChunk ? h_end - h0 : kPrejChunk;
        uint32_t mine = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t h = h0 + j;
            if (valid && !valid[h]) continue;   // (uniform: the address is)
            const float *row = table + (size_t)h * 12;
            Mat34 T;
#pragma unroll
            for (int c = 0; c < 4; ++c) { T.r0[c] = row[c]; T.r1[c] = row[4 + c]; T.r2[c] = row[8 + c]; }
            const float d2 = prerej_d2(T, px, py, pz, g, limit2);
            const bool in = d2 < limit2;
            const uint32_t c = (uint32_t)__popcll(__ballot(in));
            mine = lane == j ? c : mine;
            const double s = prerej_wave_sum(in ? (double)d2 : 0.0);
            if (lane == 0) partials[((size_t)h * tiles + tile) * 2 + wave] = s;
        }
        if (lane < m && mine) atomicAdd(&counts[h0 + lane], mine);
    }
}

// sums[h] = the partials of hypothesis h: a group is wave 0 + wave 1, the groups are added in ascending order starting from group
// 0's value; 0.0 for an invalid hypothesis, whose partials nobody wrote
__global__ __launch_bounds__(kPrejLanes) void k_prerej_final(const double *partials, const uint32_t *valid, uint32_t H, uint32_t tiles, double *sums)
{
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    double t = 0.0;
    if (!valid || valid[h]) {
        const double *p = partials + (size_t)h * tiles * 2;
        t = p[0] + p[1];
        for (uint32_t gi = 1; gi < tiles; ++gi) t += p[2 * (size_t)gi] + p[2 * (size_t)gi + 1];
    }
    sums[h] = t;
}

// flags[i] = source record i is an inlier under T
__global__ __launch_bounds__(kPrejLanes) void k_prerej_flags(const char *src, size_t sstride, uint32_t ns, Mat34 T, PointGridDev g, float limit2, uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const float *p = rec_xyz(src, sstride, i);
    flags[i] = prerej_d2(T, p[0], p[1], p[2], g, limit2) < limit2 ? 1u : 0u;
}

// out[pos[i]] = i for the flagged records whose position is below `room`; *found = how many are flagged
__global__ __launch_bounds__(kPrejLanes) void k_prerej_emit(const uint32_t *flags, const uint32_t *pos, uint32_t ns, unsigned long long room, int32_t *out,
                                                            unsigned long long *found)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    if (flags[i] && pos[i] < room) out[pos[i]] = (int32_t)i;
    if (i == ns - 1) *found = (unsigned long long)pos[i] + flags[i];
}

}  // namespace rsreg
