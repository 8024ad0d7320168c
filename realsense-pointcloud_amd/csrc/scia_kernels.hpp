// scia_kernels.hpp — the kernels of pcl::SampleConsensusInitialAlignment (scia.hip; C ABI and contract: include/rsreg.h, "pose from
// descriptor neighbours, scored by a robust error"): hypotheses from nr_samples source records that keep a minimum distance from
// one another, each paired with a random one of its k nearest descriptors; NO hypothesis is thrown away, every one is scored over
// EVERY source record by a bounded penalty of its exact nearest-point distance.
//
//   k_scia_hypotheses   one lane per hypothesis: the sequential rejection loop over 56 candidate draws, the neighbour draws, 17 sums,
//                       umeyama_from_sums -> a 3 x 4 table row, a valid word, 16 sample words
//   k_scia_score        THE HOT PATH: for every valid row of a slice of the table, the two waves' sums of the error terms of a tile
//                       of source records (one exact nearest-neighbour query per (hypothesis, source record))
//
// k_scia_score has k_prerej_score's shape (prerej_kernels.hpp) without its ballot, counts and atomics, writes the same `partials`
// layout, and k_prerej_final (launched through prerej_final, cloud_ops.hpp) adds them.  The grid is prerej_plan.hpp's.
#pragma once

#include "records.hpp"
#include "pointgrid.hpp"
#include "prerej_plan.hpp"
#include "prerej_score.hpp"

namespace rsreg {

constexpr int kSciaMaxSamples = 8;      // nr_samples at most: the sample lives in registers
constexpr uint32_t kSciaDraws = 56;     // candidate draws of a hypothesis: draws 0 .. 55; the neighbour draws are 56 .. 63
constexpr int kSciaTruncated = 0, kSciaHuber = 1;   // rsreg_scia_error_function

// Hypothesis h0 + j (j < count) of the contract.  table[12 * j ..] = the rows of its transform, valid[j] = 1 when it has one
// (otherwise the row is NaN and valid[j] = 0), sample[16 * j ..] = its source records, sample[16 * j + 8 ..] = their target records,
// -1 behind nr of each (-1 x 16 when the 56 draws did not fill the sample).  nbr: ns rows of k target records, a row of -1 for an
// ineligible source record; the host has checked every other entry against nt.  msd2 = min_sample_distance^2, a double.
// The sample is indexed by unrolled loops alone, so that it stays in registers.
__global__ __launch_bounds__(64) void k_scia_hypotheses(const char *src, size_t sstride, uint32_t ns, const char *tgt, size_t tstride, const int32_t *nbr,
                                                        uint32_t k, unsigned long long seed, unsigned long long h0, uint32_t count, int nr, double msd2,
                                                        float *table, uint32_t *valid, int32_t *sample)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const unsigned long long h = h0 + j;
    uint32_t id[kSciaMaxSamples];
    float P[kSciaMaxSamples][3];
#pragma unroll
    for (int s = 0; s < kSciaMaxSamples; ++s) { id[s] = 0u; P[s][0] = P[s][1] = P[s][2] = 0.0f; }
    int n = 0;
    for (uint32_t d = 0; d < kSciaDraws && n < nr; ++d) {
        const uint32_t c = sac_draw(seed, h, d, ns);
        if (nbr[(size_t)c * k] < 0) continue;
        const float *p = rec_xyz(src, sstride, c);
        const float x = p[0], y = p[1], z = p[2];
        if (!finite3(x, y, z)) continue;
        bool ok = true;
#pragma unroll
        for (int s = 0; s < kSciaMaxSamples; ++s)
            if (s < n) ok = ok && id[s] != c && (double)l2_simple(x, y, z, P[s][0], P[s][1], P[s][2]) >= msd2;
        if (!ok) continue;
#pragma unroll
        for (int s = 0; s < kSciaMaxSamples; ++s)
            if (s == n) { id[s] = c; P[s][0] = x; P[s][1] = y; P[s][2] = z; }
        ++n;
    }
    const bool filled = n == nr;
    int32_t match[kSciaMaxSamples];
    bool ok = filled;
    double s17[RSREG_NUM_SUMS];
#pragma unroll
    for (int i = 0; i < RSREG_NUM_SUMS; ++i) s17[i] = 0.0;
#pragma unroll
    for (int s = 0; s < kSciaMaxSamples; ++s) {
        match[s] = -1;
        if (filled && s < nr) {
            match[s] = nbr[(size_t)id[s] * k + sac_draw(seed, h, kSciaDraws + (uint32_t)s, k)];
            const float *q = rec_xyz(tgt, tstride, (size_t)match[s]);
            const float qx = q[0], qy = q[1], qz = q[2];
            ok = ok && finite3(qx, qy, qz);
            // (the sums of k_sac_hypotheses: a weight of one, in pair order; a pair that is not finite ends the hypothesis anyway)
            const double pd[3] = {P[s][0], P[s][1], P[s][2]}, qd[3] = {qx, qy, qz};
            s17[0] += 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) { s17[1 + c] += pd[c]; s17[4 + c] += qd[c]; }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) s17[7 + r * 3 + c] += qd[r] * pd[c];
            s17[16] += (double)l2_simple(P[s][0], P[s][1], P[s][2], qx, qy, qz);
        }
    }
    Mat4f T;
    const bool good = ok && umeyama_from_sums(s17, T);
    const float nan = __uint_as_float(0x7fc00000u);
    float *row = table + (size_t)j * 12;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) row[r * 4 + c] = good ? T(r, c) : nan;
    valid[j] = good ? 1u : 0u;
    int32_t *s16 = sample + (size_t)j * 16;
#pragma unroll
    for (int s = 0; s < kSciaMaxSamples; ++s) {
        s16[s] = filled && s < nr ? (int32_t)id[s] : -1;
        s16[8 + s] = match[s];
    }
}

// the contract's term of one finite source record whose nearest squared distance is e (+inf: none)
template <int kFn> __device__ __forceinline__ double scia_term(float e, float thr)
{
    if (kFn == kSciaTruncated) return (e < __int_as_float(0x7f800000) && e <= thr) ? (double)__fdiv_rn(e, thr) : 1.0;
    const double ed = (double)e, td = (double)thr;
    return ed <= td ? __dmul_rn(__dmul_rn(0.5, ed), ed) : __dmul_rn(__dmul_rn(0.5, td), __dsub_rn(__dmul_rn(2.0, ed), td));
}

// Workgroup b: tile b % tiles of the source against slice b / tiles of the table (prerej_plan.hpp).  A lane keeps its record in
// registers for the whole slice.  The row and its valid word are read through addresses that depend on the workgroup and the loop
// counter alone, i.e. by the scalar unit, once a wave; an invalid row is skipped by both waves without a search.  A lane's term stays
// in registers; a wave's sum goes to a place of its own, partials[(h * tiles + tile) * 2 + wave]: no atomics, one writer a word.
// The truncated term does not change beyond thr, so its search stops there; Huber's is unbounded.  valid == nullptr: every row.
template <int kFn>
__global__ __launch_bounds__(kPrejBlock) void k_scia_score(const char *__restrict__ src, size_t sstride, uint32_t ns, const float *__restrict__ table,
                                                           const uint32_t *__restrict__ valid, uint32_t H, uint32_t tiles, uint32_t slice_chunks,
                                                           PointGridDev g, float thr, double *__restrict__ partials)
{
    const uint32_t tile = prerej_group_tile(blockIdx.x, tiles), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float nan = __uint_as_float(0x7fc00000u);
    float px = nan, py = nan, pz = nan;
    const size_t i = (size_t)tile * kPrejTile + threadIdx.x;
    if (i < ns) {
        const float *p = rec_xyz(src, sstride, i);
        px = p[0]; py = p[1]; pz = p[2];
    }
    const bool fin = finite3(px, py, pz);   // (a record that is not finite, or past the end: a term of +0.0)
    const float limit2 = kFn == kSciaTruncated ? thr : __int_as_float(0x7f800000);
    uint32_t h_first, h_end;
    prerej_group_slice(blockIdx.x, tiles, slice_chunks, H, &h_first, &h_end);
    for (uint32_t h = h_first; h < h_end; ++h) {
        if (valid && !valid[h]) continue;   // (uniform: the address is)
        const float *row = table + (size_t)h * 12;
        Mat34 T;
#pragma unroll
        for (int c = 0; c < 4; ++c) { T.r0[c] = row[c]; T.r1[c] = row[4 + c]; T.r2[c] = row[8 + c]; }
        const float e = prerej_d2(T, px, py, pz, g, limit2);
        const double s = prerej_wave_sum(fin ? scia_term<kFn>(e, thr) : 0.0);
        if (lane == 0) partials[((size_t)h * tiles + tile) * 2 + wave] = s;
    }
}

}  // namespace rsreg
