// sac_kernels.hpp — the kernels of RANSAC over a correspondence list (sac.hip; C ABI and contract: include/rsreg.h, "pose from
// correspondences"): pcl::registration::CorrespondenceRejectorSampleConsensus and TransformationEstimationSVD.
//
//   k_sac_gather       the 12-byte correspondences -> six coordinate planes (source x y z, target x y z), padded to whole tiles
//   k_sac_hypotheses   one lane per hypothesis: draw three pairs, check them, 17 sums, umeyama_from_sums -> a 3 x 4 table row
//   k_sac_count        THE HOT PATH: counts[h] += pairs of a tile within the threshold under hypothesis h
//   k_sac_flags        the inlier flags under one transform (what the winner, or a refit, keeps)
//   k_sac_sums + k_sac_final   the 17 sums over the flagged pairs, f64, in a fixed tree (TransformationEstimationSVD)
//   k_sac_emit         the flagged correspondences, compacted in input order (positions: oscan.hpp)
//
// A pair with a point that is not finite holds NaN in all six planes, and so does the padding behind the last pair: every
// comparison against a NaN is false, so such a pair is never an inlier, never sampled and never summed, without a bound or a flag.
#pragma once

#include "records.hpp"
#include "sac_plan.hpp"

namespace rsreg {

constexpr int kSacLanes = 256;        // the one-item-a-lane kernels' workgroup
constexpr int kSacSumTile = 128;      // pairs a workgroup of k_sac_sums adds: two waves, the tree of the ICP sums (icp_kernels.hpp)
constexpr int kSacFinalBlock = 256;

// (the contract's generator, sac_draw: records.hpp)

__global__ __launch_bounds__(kSacLanes) void k_sac_gather(const rsreg_correspondence *corr, uint32_t n, const char *src, size_t sstride, const char *tgt,
                                                          size_t tstride, float *planes, uint32_t pitch)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pitch) return;
    const float nan = __uint_as_float(0x7fc00000u);
    float v[6] = {nan, nan, nan, nan, nan, nan};
    if (i < n) {
        const rsreg_correspondence c = corr[i];   // (the indices were checked on the host)
        const float *p = rec_xyz(src, sstride, (size_t)c.index_query), *q = rec_xyz(tgt, tstride, (size_t)c.index_match);
        const float px = p[0], py = p[1], pz = p[2], qx = q[0], qy = q[1], qz = q[2];
        if (finite3(px, py, pz) && finite3(qx, qy, qz)) { v[0] = px; v[1] = py; v[2] = pz; v[3] = qx; v[4] = qy; v[5] = qz; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) planes[(size_t)k * pitch + i] = v[k];
}

// sample[4 * j .. 4 * j + 3] = the three pair indices of hypothesis h0 + j and the try that gave them (-1 x 4: sixteen bad tries);
// table[12 * j ..] = the rows of its transform (an invalid hypothesis: NaN, which no pair is within any threshold of)
__global__ __launch_bounds__(64) void k_sac_hypotheses(const float *planes, uint32_t pitch, uint32_t n, unsigned long long seed, unsigned long long h0,
                                                       uint32_t count, double min_sample_sqr, float *table, int32_t *sample)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const unsigned long long h = h0 + j;
    const float *px = planes, *py = planes + pitch, *pz = planes + 2 * (size_t)pitch, *qx = planes + 3 * (size_t)pitch, *qy = planes + 4 * (size_t)pitch,
                *qz = planes + 5 * (size_t)pitch;
    Mat4f T;
    int found = -1;
    uint32_t id[3] = {0, 0, 0};
    for (uint32_t t = 0; t < kSacTries && found < 0; ++t) {
        for (int k = 0; k < 3; ++k) id[k] = sac_draw(seed, h, 3 * t + k, n);
        if (id[0] == id[1] || id[0] == id[2] || id[1] == id[2]) continue;
        float P[3][3], Q[3][3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            P[k][0] = px[id[k]]; P[k][1] = py[id[k]]; P[k][2] = pz[id[k]];
            Q[k][0] = qx[id[k]]; Q[k][1] = qy[id[k]]; Q[k][2] = qz[id[k]];
            ok = ok && finite3(P[k][0], P[k][1], P[k][2]) && finite3(Q[k][0], Q[k][1], Q[k][2]);
        }
        if (!ok) continue;
        for (int a = 0; a < 2; ++a)
            for (int b = a + 1; b < 3; ++b) ok = ok && (double)l2_simple(P[a][0], P[a][1], P[a][2], P[b][0], P[b][1], P[b][2]) > min_sample_sqr;
        if (!ok) continue;
        double s[RSREG_NUM_SUMS];
        for (int k = 0; k < RSREG_NUM_SUMS; ++k) s[k] = 0.0;
        for (int k = 0; k < 3; ++k) {   // (accum_pair of icp_kernels.hpp with a weight of one, in pair order)
            const double p[3] = {P[k][0], P[k][1], P[k][2]}, q[3] = {Q[k][0], Q[k][1], Q[k][2]};
            s[0] += 1.0;
            for (int c = 0; c < 3; ++c) { s[1 + c] += p[c]; s[4 + c] += q[c]; }
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) s[7 + r * 3 + c] += q[r] * p[c];
            s[16] += (double)l2_simple(P[k][0], P[k][1], P[k][2], Q[k][0], Q[k][1], Q[k][2]);
        }
        if (umeyama_from_sums(s, T)) found = (int)t;
    }
    const float nan = __uint_as_float(0x7fc00000u);
    float *row = table + (size_t)j * 12;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) row[r * 4 + c] = found >= 0 ? T(r, c) : nan;
    for (int k = 0; k < 3; ++k) sample[4 * (size_t)j + k] = found >= 0 ? (int32_t)id[k] : -1;
    sample[4 * (size_t)j + 3] = found;
}

// the contract's score of one pair: xform in records.hpp's order, then L2_Simple, every operation rounded once in float32
__device__ __forceinline__ bool sac_within(const Mat34 &m, float px, float py, float pz, float qx, float qy, float qz, float thr_up)
{
    const float3 t = xform(m, px, py, pz);
    return l2_simple(t.x, t.y, t.z, qx, qy, qz) < thr_up;   // (thr_up: the least float >= threshold^2, so this IS (double)d2 < threshold^2)
}

// Workgroup b: tile b % tiles of the pairs against slice b / tiles of the table (sac_plan.hpp).  A lane keeps its kSacPairsPerLane
// pairs in registers for the whole slice.  The table's rows are read through addresses that depend on the workgroup and the loop
// counter alone, i.e. by the scalar unit, once a wave.  A wave's count of one hypothesis is a ballot's population count, a scalar;
// lane j of the wave keeps the one of the chunk's j-th hypothesis, so a chunk of 64 costs a wave ONE integer add in LDS, and the
// workgroup one integer atomicAdd a hypothesis in HBM.
__global__ __launch_bounds__(kSacBlock) void k_sac_count(const float *__restrict__ planes, uint32_t pitch, const float *__restrict__ table, uint32_t H,
                                                         uint32_t tiles, uint32_t slice_chunks, float thr_up, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t s_cnt[kSacChunk];
    const uint32_t tile = sac_group_tile(blockIdx.x, tiles), lane = threadIdx.x & 63u;
    float px[kSacPairsPerLane], py[kSacPairsPerLane], pz[kSacPairsPerLane], qx[kSacPairsPerLane], qy[kSacPairsPerLane], qz[kSacPairsPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kSacPairsPerLane; ++k) {
        const size_t i = (size_t)tile * kSacTile + k * kSacBlock + threadIdx.x;   // (< pitch = tiles * kSacTile: the planes are padded)
        px[k] = planes[i]; py[k] = planes[pitch + i]; pz[k] = planes[2 * (size_t)pitch + i];
        qx[k] = planes[3 * (size_t)pitch + i]; qy[k] = planes[4 * (size_t)pitch + i]; qz[k] = planes[5 * (size_t)pitch + i];
    }
    uint32_t h_first, h_end;
    sac_group_slice(blockIdx.x, tiles, slice_chunks, H, &h_first, &h_end);
    for (uint32_t h0 = h_first; h0 < h_end; h0 += kSacChunk) {
        const uint32_t m = h_end - h0 < kSacChunk ? h_end - h0 : kSacChunk;
        if (threadIdx.x < kSacChunk) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const float *row = table + (size_t)(h0 + j) * 12;
            Mat34 T;
#pragma unroll
            for (int c = 0; c < 4; ++c) { T.r0[c] = row[c]; T.r1[c] = row[4 + c]; T.r2[c] = row[8 + c]; }
            uint32_t c = 0;
#pragma unroll
            for (uint32_t k = 0; k < kSacPairsPerLane; ++k) c += (uint32_t)__popcll(__ballot(sac_within(T, px[k], py[k], pz[k], qx[k], qy[k], qz[k], thr_up)));
            mine = lane == j ? c : mine;
        }
        if (mine) atomicAdd(&s_cnt[lane], mine);
        __syncthreads();
        if (threadIdx.x < m) {
            const uint32_t v = s_cnt[threadIdx.x];
            if (v) atomicAdd(&counts[h0 + threadIdx.x], v);
        }
    }
}

// flags[i] = pair i is within the threshold under T; word[0] += the flags set, word[1] += the flags that differ from old[i]
// (old nullable)
__global__ __launch_bounds__(kSacLanes) void k_sac_flags(const float *planes, uint32_t pitch, uint32_t n, Mat34 T, float thr_up, const uint32_t *old,
                                                         uint32_t *flags, uint32_t *word)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false, differs = false;
    if (i < n) {
        in = sac_within(T, planes[i], planes[pitch + i], planes[2 * (size_t)pitch + i], planes[3 * (size_t)pitch + i], planes[4 * (size_t)pitch + i],
                        planes[5 * (size_t)pitch + i], thr_up);
        differs = old && (old[i] != 0u) != in;
        flags[i] = in ? 1u : 0u;
    }
    const uint32_t a = (uint32_t)__popcll(__ballot(in)), b = (uint32_t)__popcll(__ballot(differs));
    if ((threadIdx.x & 63u) == 0) {
        if (a) atomicAdd(&word[0], a);
        if (b) atomicAdd(&word[1], b);
    }
}

// The 17 sums (include/rsreg.h: RSREG_NUM_SUMS; p the source point, q the target point, [16] the squared distance of the pair
// as it stands) over the finite pairs whose flag is set (flags nullable: every finite pair).  The gathering twin of k_cov_reduce
// / tile_reduce_store / k_final_reduce (icp_kernels.hpp), the same halving order: pair i belongs to lane i % 64 of wave
// (i / 64) % 2 of workgroup i / 128; a wave's 64 terms of a sum meet by recursive halving across lane bit 5, 4, .. 0; the
// workgroup adds wave 0 + wave 1 into partials[k][workgroup]; k_sac_final's thread t adds the partials t, t + 256, .. in ascending
// order, a wave folds its lanes with offsets 32, 16, .. 1, thread 0 adds the four waves in order.  The order is a function of n alone.
__global__ __launch_bounds__(kSacSumTile) void k_sac_sums(const float *planes, uint32_t pitch, uint32_t n, const uint32_t *flags, double *partials)
{
    __shared__ double shr[kSacSumTile / 64][RSREG_NUM_SUMS];
    double a[RSREG_NUM_SUMS];
    for (int k = 0; k < RSREG_NUM_SUMS; ++k) a[k] = 0.0;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (!flags || flags[i])) {
        const float P[3] = {planes[i], planes[pitch + i], planes[2 * (size_t)pitch + i]};
        const float Q[3] = {planes[3 * (size_t)pitch + i], planes[4 * (size_t)pitch + i], planes[5 * (size_t)pitch + i]};
        if (finite3(P[0], P[1], P[2]) && finite3(Q[0], Q[1], Q[2])) {
            a[0] = 1.0;
            for (int c = 0; c < 3; ++c) { a[1 + c] = (double)P[c]; a[4 + c] = (double)Q[c]; }
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) a[7 + r * 3 + c] = (double)Q[r] * (double)P[c];
            a[16] = (double)l2_simple(P[0], P[1], P[2], Q[0], Q[1], Q[2]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0, cnt = RSREG_NUM_SUMS;
    double v9[9], v5[5], v3[3], v2[2], v1[1], v0[1];
    halve_sums<RSREG_NUM_SUMS>(a, v9, lane, 32, base, cnt);
    halve_sums<9>(v9, v5, lane, 16, base, cnt);
    halve_sums<5>(v5, v3, lane, 8, base, cnt);
    halve_sums<3>(v3, v2, lane, 4, base, cnt);
    halve_sums<2>(v2, v1, lane, 2, base, cnt);
    halve_sums<1>(v1, v0, lane, 1, base, cnt);
    if (cnt >= 1) shr[wave][base] = v0[0];   // exactly one lane ends up owning each of the 17 sums
    __syncthreads();
    if (threadIdx.x < RSREG_NUM_SUMS) partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = shr[0][threadIdx.x] + shr[1][threadIdx.x];
}

// 17 workgroups: workgroup k adds sum k over all slabs, fixed order
__global__ __launch_bounds__(kSacFinalBlock) void k_sac_final(const double *partials, uint32_t nblocks, double *sums)
{
    __shared__ double shf[kSacFinalBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *src = partials + (size_t)blockIdx.x * nblocks;
    double v = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += kSacFinalBlock) v += src[b];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) shf[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = shf[0];
        for (int w = 1; w < kSacFinalBlock / 64; ++w) t += shf[w];
        sums[blockIdx.x] = t;
    }
}

// out[pos[i]] = corr[i] for the flagged pairs whose position is below `room`; *found = how many are flagged
__global__ __launch_bounds__(kSacLanes) void k_sac_emit(const rsreg_correspondence *corr, const uint32_t *flags, const uint32_t *pos, uint32_t n,
                                                        unsigned long long room, rsreg_correspondence *out, unsigned long long *found)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flags[i] && pos[i] < room) out[pos[i]] = corr[i];
    if (i == n - 1) *found = (unsigned long long)pos[i] + flags[i];
}

}  // namespace rsreg
