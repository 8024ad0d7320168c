// fpfh_kernels.hpp — pcl::FPFHEstimation (setKSearch) over the exact k-nearest-neighbour search (knn_kernels.hpp:
// knn_walk<KnnKeys>): device code of rsreg_cloud_spfh and rsreg_cloud_fpfh (include/rsreg.h, which holds the contract).
// Included by filters.hip only.
//
// PCL 1.9.1 (features/impl/fpfh.hpp: computePointSPFHSignature, weightPointSPFHSignature; pfh_tools.cpp: computePairFeatures),
// recalled.  Two passes over the cloud:
//   k_fpfh_spfh    one wave per finite record, in cell order: the search, then lane a takes neighbour a -- its index and d2 go
//                  to row `record` of nn_idx / nn_d2 (pass 2 reads them: nothing is searched twice), its three pair features are
//                  computed in f64 and counted in 33 words of LDS with integer adds, which commute: no lane timing enters.  A bin
//                  hit by c pairs holds 0.0f + hist_incr c times, read from a table the workgroup fills once.
//   k_fpfh_weight  one wave per record, in record order: lane b < 33 owns one bin and adds SPFH[N(i)[a]][b] / d2[a] over the
//                  neighbours in their order (each step one 132-byte row); the three normalising sums are sequential by contract
//                  (11 k float additions each, neighbour-major): three lanes add them from the products staged in LDS.
// Nothing here uses a float atomic; every sum runs in an order the contract names.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "knn_kernels.hpp"

namespace rsreg {

constexpr int kFpfhBins = 11;               // per feature
constexpr int kFpfhRow = 3 * kFpfhBins;     // floats of a pcl::FPFHSignature33

// floor(scaled), clamped to [0, 10] (a NaN goes to 0)
__device__ __forceinline__ int fpfh_bin(double scaled)
{
    return (int)fmin(fmax(floor(scaled), 0.0), (double)(kFpfhBins - 1));
}

// The three bins of the pair (p_i, n_i), (p_j, n_j), all in f64 without contraction (include/rsreg.h: "pair features"); false
// when the pair is skipped: coincident points, or a dp parallel to the source normal.  The normals are finite.
__device__ __forceinline__ bool fpfh_pair_bins(float pix, float piy, float piz, float nix, float niy, float niz, const float *pj, const float *nj, int (&bin)[3])
{
#pragma clang fp contract(off)
    double dx = (double)pj[0] - (double)pix, dy = (double)pj[1] - (double)piy, dz = (double)pj[2] - (double)piz;
    const double f4 = sqrt((dx * dx + dy * dy) + dz * dz);
    if (f4 == 0.0) return false;
    double n1x = nix, n1y = niy, n1z = niz, n2x = nj[0], n2y = nj[1], n2z = nj[2];
    const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / f4, a2 = ((n2x * dx + n2y * dy) + n2z * dz) / f4;
    double f3 = a1;
    if (fabs(a1) < fabs(a2)) {   // PCL: acos(fabs(a1)) > acos(fabs(a2)) -- the other point becomes the source
        double t;
        t = n1x; n1x = n2x; n2x = t;
        t = n1y; n1y = n2y; n2y = t;
        t = n1z; n1z = n2z; n2z = t;
        dx = -dx;
        dy = -dy;
        dz = -dz;
        f3 = -a2;
    }
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;   // v = dp x n1
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    if (vn == 0.0) return false;
    vx = vx / vn;
    vy = vy / vn;
    vz = vz / vn;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;   // w = n1 x v
    const double f2 = (vx * n2x + vy * n2y) + vz * n2z;
    const double f1 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
    constexpr double kPi = 3.14159265358979323846, kInvTwoPi = 1.0 / (2.0 * kPi);
    bin[0] = fpfh_bin(11.0 * ((f1 + kPi) * kInvTwoPi));
    bin[1] = fpfh_bin(11.0 * ((f2 + 1.0) * 0.5));
    bin[2] = fpfh_bin(11.0 * ((f3 + 1.0) * 0.5));
    return true;
}

// One workgroup of ONE wave per finite record, queries in cell order (the shape of k_normals).  Row `record` of nn_idx / nn_d2:
// the k neighbours, ascending (d2, index); row `record` of spfh: the 33 floats.  The rows of records not visited (non-finite
// ones) have been zeroed before the launch; a finite record whose normal is not finite writes its zeros here.
__global__ __launch_bounds__(kKnnWave) void k_fpfh_spfh(PointGridDev g, int k, float hist_incr, const char *rec, size_t stride, const char *nrm,
                                                        size_t nstride, int32_t *nn_idx, float *nn_d2, float *spfh)
{
    __shared__ unsigned long long buf[kKnnBuf];
    __shared__ uint32_t cnt[kFpfhRow];
    __shared__ float tab[kKnnWave];   // tab[c] = 0.0f + hist_incr, c times: PCL's sequential += of equal increments
    const int lane = (int)threadIdx.x;
    {
        float acc = 0.0f, mine = 0.0f;
        for (int c = 1; c < kKnnWave; ++c) {
            acc = __fadd_rn(acc, hist_incr);
            if (c == lane) mine = acc;
        }
        tab[lane] = mine;
    }
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        const size_t record = (size_t)__float_as_uint(q.w);
        if (lane < kFpfhRow) cnt[lane] = 0u;
        knn_walk<KnnKeys>(g, q, k, buf, lane);   // (returns behind a barrier: the zeros and, the first time, the table are in place)
        const float *ni = rec_xyz(nrm, nstride, record);
        const float nix = ni[0], niy = ni[1], niz = ni[2];
        if (lane < k) {
            const unsigned long long key = buf[lane];
            const uint32_t nb = (uint32_t)key;
            const size_t at = record * (size_t)k + (size_t)lane;
            nn_idx[at] = (int32_t)nb;
            nn_d2[at] = __uint_as_float((uint32_t)(key >> 32));
            if ((size_t)nb != record && finite3(nix, niy, niz)) {
                const float *nj = rec_xyz(nrm, nstride, nb);
                int bin[3];
                if (finite3(nj[0], nj[1], nj[2]) && fpfh_pair_bins(q.x, q.y, q.z, nix, niy, niz, rec_xyz(rec, stride, nb), nj, bin)) {
                    atomicAdd(&cnt[bin[0]], 1u);
                    atomicAdd(&cnt[kFpfhBins + bin[1]], 1u);
                    atomicAdd(&cnt[2 * kFpfhBins + bin[2]], 1u);
                }
            }
        }
        __syncthreads();
        if (lane < kFpfhRow) spfh[record * kFpfhRow + (size_t)lane] = tab[cnt[lane]];   // (at most k - 1 <= 63 pairs hit a bin)
        __syncthreads();   // (the keys and the counts have been read: the next query may append and clear)
    }
}

// One workgroup of ONE wave per record, in record order.  out: record i's 33 floats; a record that is not finite or whose own
// normal is not finite gets quiet NaNs and sets *any_nan; so does every row the arithmetic leaves a NaN in.  PCL's order (include/rsreg.h): for a, for t, for b: val = SPFH * w,
// sum_t += val, h[t][b] += val; then h *= 100 / sum_t.  Lane b adds its own h in neighbour order; lane t < 3 adds sum_t over
// (a, b) from the products staged in LDS.
__global__ __launch_bounds__(kKnnWave) void k_fpfh_weight(const char *rec, size_t stride, const char *nrm, size_t nstride, uint32_t n, int k,
                                                          const int32_t *nn_idx, const float *nn_d2, const float *spfh, float *out, uint32_t *any_nan)
{
    __shared__ float stage[kKnnMaxK * kFpfhRow];
    __shared__ float wl[kKnnMaxK];
    __shared__ float sums[3];
    const int lane = (int)threadIdx.x;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const float *p = rec_xyz(rec, stride, i), *m = rec_xyz(nrm, nstride, i);
        if (!finite3(p[0], p[1], p[2]) || !finite3(m[0], m[1], m[2])) {   // (the whole wave alike)
            if (lane < kFpfhRow) out[(size_t)i * kFpfhRow + (size_t)lane] = __uint_as_float(0x7fc00000u);
            if (lane == 0) *any_nan = 1u;
            continue;
        }
        int32_t nb = 0;
        float w = 0.0f;   // 0: the neighbour is skipped (the record itself and exact copies); 1 / d2 is never 0 for a finite d2
        if (lane < k) {
            const size_t at = (size_t)i * (size_t)k + (size_t)lane;
            nb = nn_idx[at];
            const float d2 = nn_d2[at];
            w = d2 == 0.0f ? 0.0f : __fdiv_rn(1.0f, d2);
        }
        wl[lane] = w;
        float h = 0.0f;
        for (int a = 0; a < k; ++a) {
            const float wa = __shfl(w, a);
            const int32_t na = __shfl(nb, a);
            if (wa == 0.0f) continue;
            if (lane < kFpfhRow) {
                const float val = __fmul_rn(spfh[(size_t)(uint32_t)na * kFpfhRow + (size_t)lane], wa);
                h = __fadd_rn(h, val);
                stage[a * kFpfhRow + lane] = val;
            }
        }
        __syncthreads();
        if (lane < 3) {
            float s = 0.0f;
            for (int a = 0; a < k; ++a) {
                if (wl[a] == 0.0f) continue;
#pragma unroll
                for (int b = 0; b < kFpfhBins; ++b) s = __fadd_rn(s, stage[a * kFpfhRow + lane * kFpfhBins + b]);
            }
            if (s != 0.0f) s = (float)(100.0 / (double)s);
            sums[lane] = s;
        }
        __syncthreads();
        // a finite record gets NaNs by the arithmetic too (1 / d2 = +inf for a denormal d2, and 0 * inf; inf - inf of overflowed
        // products): the flag is raised for every row that holds one -- a ballot, one plain store of the same word by one lane
        bool is_nan = false;
        if (lane < kFpfhRow) {
            const float r = __fmul_rn(h, sums[lane / kFpfhBins]);
            out[(size_t)i * kFpfhRow + (size_t)lane] = r;
            is_nan = r != r;
        }
        if (__ballot(is_nan) != 0ull && lane == 0) *any_nan = 1u;
        __syncthreads();   // (the staged products and the weights have been read: the next record may overwrite them)
    }
}

}  // namespace rsreg
