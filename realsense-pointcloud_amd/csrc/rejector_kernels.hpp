// rejector_kernels.hpp — device code of the correspondence rejector chain (include/rsreg.h: rsreg_icp_set_rejectors): PCL's
// CorrespondenceRejectorMedianDistance, ...OneToOne and ...SurfaceNormal between the staged search and the sums, and the source
// normals that move with the source.  Included by icp.hip behind icp_kernels.hpp.
//
// The chain works on ORIGINAL source records: one in-play flag per record j (sorted position: uniq_of[j] = its distinct point u,
// perm[j] = the caller's index), because after the normal test the copies of a point still in play need not be the first ones.
// k_rej_flags_init makes the flags from what the search and the two filters in front left (corr_pos, cw: a prefix of u's
// copies), every rejector rewrites them, k_rej_fold counts them back into cw[u] so that the sums kernels need no second form.
// Every kernel that writes flags counts the ones it leaves set into a word of its own (integer atomics: the same total in any
// order); nothing here adds floats, so the same chain on the same pairs leaves the same flags on any context at any launch.
#pragma once

#include "icp_kernels.hpp"

namespace rsreg {

constexpr int kRejMax = 8;              // entries of a chain (rsreg.h)
constexpr uint32_t kRejDigits = 4;      // the median's select: four 8-bit digits of the d2 bits, most significant first
// the chain's words in HBM: cnt[0] = records in play in front of the chain, cnt[e + 1] = behind entry e; med[e] = entry e's
// median (float bits); then 4 x 256 digit counts per entry
constexpr uint32_t kRejCnt = 0, kRejMed = kRejMax + 1, kRejHist = 32, kRejHistWords = kRejDigits * 256;
constexpr uint32_t kRejWords = kRejHist + kRejMax * kRejHistWords;

// Every kernel below that rewrites the flags runs a bounded grid over the records in strides (rej_grid) and adds what it left set
// to its count word once per WORKGROUP: a count word is one address, atomics on one address are served one after the other
// (~11 ns each on this part), and one per wave made k_rej_flags_init 178 us at 10^6 records, 16 k atomics on the way.
constexpr uint32_t kRejMaxBlocks = 512;
inline uint32_t rej_grid(uint32_t n_source) { return std::min(div_up(n_source, kBlock), kRejMaxBlocks); }

// the workgroup's sum of `kept`, added to *dst by one thread (every thread of the workgroup calls this)
__device__ __forceinline__ void rej_block_count(uint32_t kept, uint32_t *dst)
{
    __shared__ uint32_t s_part[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) kept += __shfl_down(kept, off);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += s_part[w];
        if (t) atomicAdd(dst, t);
    }
}

// flags[j] = record j is in play behind the search, the reciprocal test and trim_overlap_ratio: its point has a match and it
// is among the first cw[u] copies (the rule of k_export_corr<CorrKeep::copies>)
__global__ __launch_bounds__(kBlock) void k_rej_flags_init(const int *corr_pos, const uint32_t *cw, const uint32_t *uniq_of, const uint32_t *first,
                                                           uint32_t n_source, uint32_t *flags, uint32_t *cnt_out)
{
    uint32_t kept = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_source; j += gridDim.x * blockDim.x) {
        const uint32_t u = uniq_of[j];
        const bool in_play = corr_pos[u] >= 0 && j - first[u] < cw[u];
        flags[j] = in_play ? 1u : 0u;
        kept += in_play ? 1u : 0u;
    }
    rej_block_count(kept, cnt_out);
}

// ---- MEDIAN_DISTANCE: the d2 at rank floor(m / 2) of the records in play, by a radix select over the bits of the float
// (squared distances are >= +0, +inf included: their bits order like the values).  Digit q's counts are taken over the records
// whose higher digits equal the ones already chosen; every workgroup re-derives those from the finished counts of the digits
// before (a 256-entry prefix sum each), so no state is handed from launch to launch but the counts themselves.
// Returns the chosen digits (`digits` of them, most significant first); m == 0: 0.
__device__ __forceinline__ uint32_t rej_select_prefix(const uint32_t *hist, uint32_t digits, uint32_t m)
{
    __shared__ uint32_t s_scan[kBlock];
    __shared__ uint32_t s_pk[2];   // the digits chosen so far, the rank among the records that share them
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s_pk[0] = 0; s_pk[1] = m / 2u; }
    for (uint32_t q = 0; q < digits; ++q) {
        __syncthreads();
        const uint32_t c = hist[q * 256u + tid];
        s_scan[tid] = c;
        __syncthreads();
        for (uint32_t off = 1; off < 256u; off <<= 1) {
            const uint32_t v = tid >= off ? s_scan[tid - off] : 0u;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const uint32_t incl = s_scan[tid], excl = incl - c, k = s_pk[1];
        __syncthreads();   // (every thread has read the rank before the one that holds it writes the next)
        if (c && excl <= k && k < incl) { s_pk[0] = (s_pk[0] << 8) | tid; s_pk[1] = k - excl; }
    }
    __syncthreads();
    return s_pk[0];
}

static_assert(kBlock == 256, "the select's digit counts are one per thread of a workgroup");

// the counts of digit `digit` (0: the top byte) over the records in play that carry the digits chosen before; hist: zero before
// the chain's first launch
__global__ __launch_bounds__(kBlock) void k_rej_median_hist(const uint32_t *flags, const float *corr_d2, const uint32_t *uniq_of, uint32_t n_source,
                                                            uint32_t digit, const uint32_t *m_p, uint32_t *hist)
{
    __shared__ uint32_t s_hist[256];
    const uint32_t m = *m_p;
    if (m == 0) return;   // (the whole grid alike)
    const uint32_t prefix = rej_select_prefix(hist, digit, m);
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t shift = 24u - 8u * digit;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_source; j += gridDim.x * blockDim.x) {
        if (!flags[j]) continue;
        const uint32_t bits = __float_as_uint(corr_d2[uniq_of[j]]);
        if (digit == 0 || (bits >> (shift + 8u)) == prefix) atomicAdd(&s_hist[(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = s_hist[threadIdx.x];
    if (c) atomicAdd(&hist[digit * 256u + threadIdx.x], c);
}

// a record stays iff (double)d2 <= (double)median * factor, in IEEE double as written (a NaN product drops everything)
__global__ __launch_bounds__(kBlock) void k_rej_median_apply(uint32_t *flags, const float *corr_d2, const uint32_t *uniq_of, uint32_t n_source,
                                                             const uint32_t *m_p, const uint32_t *hist, double factor, uint32_t *med_out,
                                                             uint32_t *cnt_out)
{
    const uint32_t m = *m_p;
    if (m == 0) return;   // (nothing in play: nothing happens, the median stays 0)
    const uint32_t med_bits = rej_select_prefix(hist, kRejDigits, m);
    if (blockIdx.x == 0 && threadIdx.x == 0) *med_out = med_bits;
    const double bound = (double)__uint_as_float(med_bits) * factor;
    uint32_t kept = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_source; j += gridDim.x * blockDim.x) {
        if (!flags[j]) continue;
        const bool keep = (double)corr_d2[uniq_of[j]] <= bound;
        if (!keep) flags[j] = 0u;
        kept += keep ? 1u : 0u;
    }
    rej_block_count(kept, cnt_out);
}

// ---- ONE_TO_ONE: of the records in play that share a target position the one with the smallest (d2, caller's index) stays.
// table: one key per position of the sorted target, all ones before the launch; key = d2 bits << 32 | caller's index (the
// order Best relies on; +inf under an infinite gate is a key like any other).  Every copy of a merged point competes by itself.
__device__ __forceinline__ unsigned long long rej_o2o_key(float d2, uint32_t orig) { return ((unsigned long long)__float_as_uint(d2) << 32) | orig; }

// A record does not compete when the lane before it holds a smaller key for the same position: someone better is known.  The
// copies of a merged point are neighbours in j in the caller's order, and so are a plain source's runs of missing depth, all
// at (0, 0, 0) and all matched to one target point: of such a run the first lane of a wave alone goes to memory (10^5 atomics on
// one address took 1.2 ms at 10^6 records).  And nobody competes who reads a key in the table that already beats its own: the
// table only ever falls.
__global__ __launch_bounds__(kBlock) void k_rej_o2o_min(const uint32_t *flags, const int *corr_pos, const float *corr_d2, const uint32_t *perm,
                                                        const uint32_t *uniq_of, uint32_t n_source, unsigned long long *table)
{
    const uint32_t stride = gridDim.x * blockDim.x, lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * blockDim.x; base < n_source; base += stride) {   // (the same trips for every lane of a wave)
        const uint32_t j = base + threadIdx.x;
        const bool flag = j < n_source && flags[j] != 0u;
        unsigned long long key = ~0ull;
        int pos = -1;
        if (flag) {
            const uint32_t u = uniq_of[j];
            key = rej_o2o_key(corr_d2[u], perm[j]);
            pos = corr_pos[u];
        }
        const unsigned long long key_before = __shfl_up(key, 1);
        const int pos_before = __shfl_up(pos, 1);
        if (!flag || (lane > 0 && pos_before == pos && key_before < key)) continue;
        unsigned long long *slot = &table[pos];
        if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(slot, key);
    }
}

__global__ __launch_bounds__(kBlock) void k_rej_o2o_keep(uint32_t *flags, const int *corr_pos, const float *corr_d2, const uint32_t *perm,
                                                         const uint32_t *uniq_of, uint32_t n_source, const unsigned long long *table,
                                                         uint32_t *cnt_out)
{
    uint32_t kept = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_source; j += gridDim.x * blockDim.x) {
        if (!flags[j]) continue;
        const uint32_t u = uniq_of[j];
        const bool keep = table[corr_pos[u]] == rej_o2o_key(corr_d2[u], perm[j]);
        if (!keep) flags[j] = 0u;
        kept += keep ? 1u : 0u;
    }
    rej_block_count(kept, cnt_out);
}

// ---- SURFACE_NORMAL: a record stays iff (double)((sx*tx + sy*ty) + sz*tz) > threshold: float products and sums, each rounded
// once; s = the record's CURRENT normal (caller's order), t = the matched target record's normal.  A NaN score drops the record.
__global__ __launch_bounds__(kBlock) void k_rej_normal(uint32_t *flags, const int *corr_pos, const uint32_t *perm, const uint32_t *uniq_of,
                                                       uint32_t n_source, const float4 *tgt, const float4 *tgt_normals, const float4 *src_normals,
                                                       double threshold, uint32_t *cnt_out)
{
    uint32_t kept = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_source; j += gridDim.x * blockDim.x) {
        if (!flags[j]) continue;
        const float4 s = src_normals[perm[j]];
        const float4 t = tgt_normals[tgt_idx(tgt[corr_pos[uniq_of[j]]])];
        const float score = __fadd_rn(__fadd_rn(__fmul_rn(s.x, t.x), __fmul_rn(s.y, t.y)), __fmul_rn(s.z, t.z));
        const bool keep = (double)score > threshold;
        if (!keep) flags[j] = 0u;
        kept += keep ? 1u : 0u;
    }
    rej_block_count(kept, cnt_out);
}

// ---- the flags back into cw / corr_pos.  cw: zero before the launch.  The copies of a point are neighbours in j, so a wave
// adds one number per point it covers (a frame's 10^5 copies of (0, 0, 0) are 1 600 atomics, not 10^5).
__global__ __launch_bounds__(kBlock) void k_rej_fold(const uint32_t *flags, const uint32_t *uniq_of, uint32_t n_source, uint32_t *cw)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool in = j < n_source;
    const uint32_t u = in ? uniq_of[j] : 0xffffffffu;
    const bool flag = in && flags[j] != 0u;
    const uint32_t before = __shfl_up(u, 1);
    const bool head = lane == 0 || u != before;
    const unsigned long long heads = __ballot(head), set = __ballot(flag);
    if (!head || !in) return;
    const unsigned long long above = heads & ~((2ull << lane) - 1ull);   // (lane 63: 2 << 63 wraps to 0, the mask to nothing above)
    const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;
    const unsigned long long upto = end >= 64u ? ~0ull : ((1ull << end) - 1ull);
    const uint32_t c = (uint32_t)__popcll(set & upto & ~((1ull << lane) - 1ull));
    if (c) atomicAdd(&cw[u], c);
}

// a point none of whose copies is in play has no match any more
__global__ __launch_bounds__(kBlock) void k_rej_fold_pos(const uint32_t *cw, uint32_t n, int *corr_pos)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n && cw[u] == 0u) corr_pos[u] = -1;
}

// (determineCorrespondences' list behind the chain, the records whose flag is set: icp_kernels.hpp, k_export_corr<CorrKeep::flags>)

// ---- the source's normals, one float4 {nx, ny, nz, 0} per source RECORD in the caller's order.  They turn with the source:
// by the guess when an alignment begins, by every increment after it -- xform's arithmetic without the translation,
// (r0*x + r1*y) + r2*z, every operation rounded once; a NaN goes through as it is.
__device__ __forceinline__ float4 rotate_normal(const Mat34 &m, const float4 &v)
{
    const float ox = __fadd_rn(__fadd_rn(__fmul_rn(m.r0[0], v.x), __fmul_rn(m.r0[1], v.y)), __fmul_rn(m.r0[2], v.z));
    const float oy = __fadd_rn(__fadd_rn(__fmul_rn(m.r1[0], v.x), __fmul_rn(m.r1[1], v.y)), __fmul_rn(m.r1[2], v.z));
    const float oz = __fadd_rn(__fadd_rn(__fmul_rn(m.r2[0], v.x), __fmul_rn(m.r2[1], v.y)), __fmul_rn(m.r2[2], v.z));
    return make_float4(ox, oy, oz, 0.0f);
}

// cur = guess's 3 x 3 block * the normals as handed in (apply_guess 0: a copy)
__global__ __launch_bounds__(kBlock) void k_restart_normals(const float4 *in, uint32_t n, Mat34 guess, int apply_guess, float4 *cur)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 v = in[i];
    cur[i] = apply_guess ? rotate_normal(guess, v) : v;
}

// beside k_transform: the increment's 3 x 3 block, in place
__global__ __launch_bounds__(kBlock) void k_rotate_normals(float4 *cur, uint32_t n, Mat34 T)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cur[i] = rotate_normal(T, cur[i]);
}

}  // namespace rsreg
