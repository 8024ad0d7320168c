// plane_seg_kernels.hpp — the kernels of the RANSAC plane segmentation and of ExtractIndices (segment.hip; C ABI and contract:
// include/rsreg.h, "plane segmentation"): pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE and SAC_RANSAC,
// pcl::ExtractIndices.  (plane_kernels.hpp is something else: the sums of point-to-plane ICP.)
//
//   k_plane_hypotheses   one lane per hypothesis: draw three records, the cross product, the unit normal, the axis test -> a table row
//   k_plane_count        THE HOT PATH: counts[h] += records of a tile within the threshold of plane h
//   k_plane_flags        the inlier flags under one model (the winner's, the refined model's, rsreg_cloud_plane_filter's)
//   k_plane_sums + k_plane_final   the ten sums over the flagged records, f64 relative to p0, in the fixed tree of k_sac_sums
//   k_plane_emit         the flagged records' indices, ascending (positions: oscan.hpp)
//   k_extract_gather / k_extract_clear   ExtractIndices: whole records by index; the flags of the named records cleared
//
// The records are read from the cloud as it lies, at its stride: k_plane_count loads a lane's records once for a whole slice of
// the table, so a gather into coordinate planes would cost a pass and a buffer to save nothing.
#pragma once

#include "records.hpp"
#include "plane_seg_plan.hpp"

namespace rsreg {

constexpr int kPlaneLanes = 256;        // the one-item-a-lane kernels' workgroup
constexpr int kPlaneSumTile = 128;      // records a workgroup of k_plane_sums adds: two waves, the tree of k_sac_sums
constexpr int kPlaneFinalBlock = 256;
constexpr int kPlaneSums = RSREG_NUM_PLANE_SEG_SUMS;

struct PlaneAxis {   // SACMODEL_PERPENDICULAR_PLANE: on != 0 when eps_angle > 0 and the axis is not zero
    double x, y, z, cos_eps;
    int on;
};

// the contract's test of one record against one model: float32, every operation rounded once, |dist| < thr_up with thr_up the
// least float >= threshold, which IS (double)|dist| < threshold.  A coordinate that is not finite makes dist inf or NaN.
__device__ __forceinline__ bool plane_within(float a, float b, float c, float d, float x, float y, float z, float thr_up)
{
    const float dist = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), d);
    return fabsf(dist) < thr_up;
}

// table[j] = the model of hypothesis h0 + j (NaN x 4 for an INVALID one, which no record is within any threshold of);
// sample[4 j .. 4 j + 3] = the three records of its good try and the try (-1 x 4: sixteen bad tries); valid[j] = good try and axis test
__global__ __launch_bounds__(64) void k_plane_hypotheses(const char *rec, size_t stride, uint32_t n, unsigned long long seed, unsigned long long h0,
                                                         uint32_t count, PlaneAxis axis, float4 *table, int32_t *sample, uint32_t *valid)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const unsigned long long h = h0 + j;
    int found = -1;
    uint32_t id[3] = {0, 0, 0};
    float A = 0.f, B = 0.f, Cc = 0.f, D = 0.f;
    for (uint32_t t = 0; t < kPlaneTries && found < 0 && n >= 3; ++t) {
        for (int k = 0; k < 3; ++k) id[k] = sac_draw(seed, h, 3 * t + k, n);
        if (id[0] == id[1] || id[0] == id[2] || id[1] == id[2]) continue;
        float P[3][3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            const float *p = rec_xyz(rec, stride, id[k]);
            P[k][0] = p[0]; P[k][1] = p[1]; P[k][2] = p[2];
            ok = ok && finite3(P[k][0], P[k][1], P[k][2]);
        }
        if (!ok) continue;
        const float ux = __fsub_rn(P[1][0], P[0][0]), uy = __fsub_rn(P[1][1], P[0][1]), uz = __fsub_rn(P[1][2], P[0][2]);
        const float vx = __fsub_rn(P[2][0], P[0][0]), vy = __fsub_rn(P[2][1], P[0][1]), vz = __fsub_rn(P[2][2], P[0][2]);
        const float nx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
        const float ny = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
        const float nz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
        const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz));
        if (!(isfinite(n2) && n2 > 0.0f)) continue;
        // correctly rounded float sqrt and divide: the double result rounded to float is the float result (53 >= 2 * 24 + 2)
        const float l = (float)sqrt((double)n2);
        A = (float)((double)nx / (double)l);
        B = (float)((double)ny / (double)l);
        Cc = (float)((double)nz / (double)l);
        D = -__fadd_rn(__fadd_rn(__fmul_rn(A, P[0][0]), __fmul_rn(B, P[0][1])), __fmul_rn(Cc, P[0][2]));
        found = (int)t;
    }
    bool good = found >= 0;
    if (good && axis.on) {
        const double a = A, b = B, c = Cc;
        const double cs = fabs((a * axis.x + b * axis.y) + c * axis.z) /
                          (sqrt((a * a + b * b) + c * c) * sqrt((axis.x * axis.x + axis.y * axis.y) + axis.z * axis.z));
        good = cs >= axis.cos_eps;
    }
    const float nan = __uint_as_float(0x7fc00000u);
    table[j] = good ? make_float4(A, B, Cc, D) : make_float4(nan, nan, nan, nan);
    for (int k = 0; k < 3; ++k) sample[4 * (size_t)j + k] = found >= 0 ? (int32_t)id[k] : -1;
    sample[4 * (size_t)j + 3] = found;
    valid[j] = good ? 1u : 0u;
}

// Workgroup b: tile b % tiles of the records against slice b / tiles of the table (plane_seg_plan.hpp).  A lane keeps its
// kPlaneRecordsPerLane records in registers for the whole slice (a record that is not finite, or past the cloud, as NaN).  A row
// of the table is four floats at an address that depends on the workgroup and the loop counter alone, i.e. it comes in by the
// scalar unit, once a wave.  A wave's count of one hypothesis is a ballot's population count, a scalar; lane j of the wave keeps
// the one of the chunk's j-th hypothesis, so a chunk of 64 costs a wave ONE integer add in LDS, and the workgroup one integer
// atomicAdd a hypothesis in HBM.
__global__ __launch_bounds__(kPlaneBlock) void k_plane_count(const char *__restrict__ rec, size_t stride, uint32_t n, const float4 *__restrict__ table,
                                                             uint32_t H, uint32_t tiles, uint32_t slice_chunks, float thr_up, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t s_cnt[kPlaneChunk];
    const uint32_t tile = plane_group_tile(blockIdx.x, tiles), lane = threadIdx.x & 63u;
    const float nan = __uint_as_float(0x7fc00000u);
    float x[kPlaneRecordsPerLane], y[kPlaneRecordsPerLane], z[kPlaneRecordsPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kPlaneRecordsPerLane; ++k) {
        const size_t i = (size_t)tile * kPlaneTile + k * kPlaneBlock + threadIdx.x;
        x[k] = y[k] = z[k] = nan;
        if (i < n) {
            const float *p = rec_xyz(rec, stride, i);
            const float px = p[0], py = p[1], pz = p[2];
            if (finite3(px, py, pz)) { x[k] = px; y[k] = py; z[k] = pz; }
        }
    }
    uint32_t h_first, h_end;
    plane_group_slice(blockIdx.x, tiles, slice_chunks, H, &h_first, &h_end);
    for (uint32_t h0 = h_first; h0 < h_end; h0 += kPlaneChunk) {
        const uint32_t m = h_end - h0 < kPlaneChunk ? h_end - h0 : kPlaneChunk;
        if (threadIdx.x < kPlaneChunk) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const float4 r = table[h0 + j];
            uint32_t c = 0;
#pragma unroll
            for (uint32_t k = 0; k < kPlaneRecordsPerLane; ++k) c += (uint32_t)__popcll(__ballot(plane_within(r.x, r.y, r.z, r.w, x[k], y[k], z[k], thr_up)));
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

// flags[i] = (record i is an inlier of the model) != negative
__global__ __launch_bounds__(kPlaneLanes) void k_plane_flags(const char *rec, size_t stride, uint32_t n, float4 m, float thr_up, int negative, uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = rec_xyz(rec, stride, i);
    const float px = p[0], py = p[1], pz = p[2];
    const bool in = finite3(px, py, pz) && plane_within(m.x, m.y, m.z, m.w, px, py, pz, thr_up);
    flags[i] = in != (negative != 0) ? 1u : 0u;
}

// The ten sums over the flagged records, e = (double)p - (double)p0: [0] their number, [1..3] sum e, [4..9] sum of e.x e.x, e.x e.y,
// e.x e.z, e.y e.y, e.y e.z, e.z e.z.  The tree is k_sac_sums' (sac_kernels.hpp), unchanged: record i is term i % 64 of wave
// (i / 64) % 2 of workgroup i / 128; a wave's 64 terms meet by recursive halving across lane bit 5, 4, .. 0; the workgroup adds
// wave 0 + wave 1 into partials[k][workgroup]; k_plane_final is k_sac_final.  A record that is not flagged is a term of +0.
// p0 is record i0 of the cloud (i0 < n), read here; workgroup 0 leaves its three floats in p0_out for the host's solve.
__global__ __launch_bounds__(kPlaneSumTile) void k_plane_sums(const char *rec, size_t stride, uint32_t n, const uint32_t *flags, uint32_t i0, double *partials,
                                                             float *p0_out)
{
    const float *q = rec_xyz(rec, stride, i0);
    const float p0x = q[0], p0y = q[1], p0z = q[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) { p0_out[0] = p0x; p0_out[1] = p0y; p0_out[2] = p0z; }
    __shared__ double shr[kPlaneSumTile / 64][kPlaneSums];
    double a[kPlaneSums];
    for (int k = 0; k < kPlaneSums; ++k) a[k] = 0.0;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flags[i]) {
        const float *p = rec_xyz(rec, stride, i);
        const double ex = (double)p[0] - (double)p0x, ey = (double)p[1] - (double)p0y, ez = (double)p[2] - (double)p0z;
        a[0] = 1.0;
        a[1] = ex; a[2] = ey; a[3] = ez;
        a[4] = ex * ex; a[5] = ex * ey; a[6] = ex * ez; a[7] = ey * ey; a[8] = ey * ez; a[9] = ez * ez;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0, cnt = kPlaneSums;
    double v5[5], v3[3], v2[2], v1[1], w1[1], v0[1];
    halve_sums<kPlaneSums>(a, v5, lane, 32, base, cnt);
    halve_sums<5>(v5, v3, lane, 16, base, cnt);
    halve_sums<3>(v3, v2, lane, 8, base, cnt);
    halve_sums<2>(v2, v1, lane, 4, base, cnt);
    halve_sums<1>(v1, w1, lane, 2, base, cnt);
    halve_sums<1>(w1, v0, lane, 1, base, cnt);
    if (cnt >= 1) shr[wave][base] = v0[0];   // exactly one lane ends up owning each of the ten sums
    __syncthreads();
    if (threadIdx.x < kPlaneSums) partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = shr[0][threadIdx.x] + shr[1][threadIdx.x];
}

// ten workgroups: workgroup k adds sum k over all slabs, fixed order (k_sac_final's)
__global__ __launch_bounds__(kPlaneFinalBlock) void k_plane_final(const double *partials, uint32_t nblocks, double *sums)
{
    __shared__ double shf[kPlaneFinalBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *src = partials + (size_t)blockIdx.x * nblocks;
    double v = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += kPlaneFinalBlock) v += src[b];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) shf[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = shf[0];
        for (int w = 1; w < kPlaneFinalBlock / 64; ++w) t += shf[w];
        sums[blockIdx.x] = t;
    }
}

// out[pos[i]] = i for the flagged records whose position is below `room`; *found = how many are flagged
__global__ __launch_bounds__(kPlaneLanes) void k_plane_emit(const uint32_t *flags, const uint32_t *pos, uint32_t n, unsigned long long room, int32_t *out,
                                                            unsigned long long *found)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flags[i] && pos[i] < room) out[pos[i]] = (int32_t)i;
    if (i == n - 1) *found = (unsigned long long)pos[i] + flags[i];
}

// ExtractIndices, positive: word w of out record j = word w of in record index[j] (the indices were checked on the host)
__global__ __launch_bounds__(kBlock) void k_extract_gather(const char *rec, size_t stride, const int32_t *index, uint32_t m, char *out)
{
    const size_t words = stride / 4, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)m * words) return;
    const size_t j = t / words, w = t % words;
    reinterpret_cast<uint32_t *>(out)[t] = reinterpret_cast<const uint32_t *>(rec + (size_t)index[j] * stride)[w];
}

// ExtractIndices, negative: the flags of the named records cleared (the flags start as ones; a record named twice is cleared twice)
__global__ __launch_bounds__(kBlock) void k_extract_clear(const int32_t *index, uint32_t m, uint32_t *flags)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) flags[index[j]] = 0u;
}

}  // namespace rsreg
