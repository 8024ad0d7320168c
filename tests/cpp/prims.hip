// prims.hip — test-only harness around the library's three primitives, as the product compiles them: the radix sort
// (osort.hpp), the device-wide prefix sums (oscan.hpp) and the one-launch compaction's block scan and look-back
// (compact.hpp).  A shared library of extern "C" entry points on host arrays, loaded by tests/prims_check.py (ctypes),
// built by tests/test_primitives_gpu.py into tests/cpp/_build/ with the library's own flags plus -shared -I<csrc>.
//
// Every entry point returns a hipError_t (0: success).  Every device buffer an output is read from has 64 guard elements
// behind it (and `offset` elements in front of a scan's), filled with a known byte; the entry points report whether the
// primitive left them alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "compact.hpp"
#include "oscan.hpp"
#include "osort.hpp"

using namespace rsreg;

namespace {

constexpr size_t kGuard = 64;
constexpr unsigned char kFill = 0xCD, kDirty = 0xFF;

#define CK(x)                                     \
    do {                                          \
        const hipError_t e_ = (x);                \
        if (e_ != hipSuccess) return (int)e_;     \
    } while (0)

struct Dev {
    void *p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};

// the host side of a guard check: `count` bytes from `at` in device memory are all `fill`
hipError_t guard_intact(const void *dev, size_t count, unsigned char fill, bool *ok)
{
    std::vector<unsigned char> h(count);
    if (count) {
        const hipError_t e = hipMemcpy(h.data(), dev, count, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
    }
    for (unsigned char c : h)
        if (c != fill) { *ok = false; break; }
    return hipSuccess;
}

// the kernel in front of a sort, as the product's key-writing kernels are: writes the keys (xor `flip`) and the values,
// and clears `words` words of the sort's scratch on its way (osort_clear)
template <typename K>
__global__ __launch_bounds__(256) void k_keys(const K *ksrc, const uint32_t *vsrc, K *keys, uint32_t *vals, size_t n, K flip, uint32_t *clear,
                                              uint32_t words)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, threads = gridDim.x * blockDim.x;
    for (size_t i = t; i < n; i += threads) {
        keys[i] = ksrc[i] ^ flip;
        vals[i] = vsrc[i];
    }
    if (clear) osort_clear(clear, words, t, threads);
}

// The buffers of one sort: the staging copy of the input, the two pairs the passes ping-pong between (guards behind), the scratch.
template <typename K> struct SortBufs {
    Dev ksrc, vsrc, ka, kb, va, vb, scratch, hist;
    size_t n = 0;
    OsortPlan plan;

    hipError_t init(const K *keys, const uint32_t *vals, size_t n_, unsigned begin_bit, unsigned end_bit)
    {
        n = n_;
        plan = osort_plan<K>(n, begin_bit, end_bit);
        hipError_t e;
        if ((e = ksrc.alloc(n * sizeof(K))) || (e = vsrc.alloc(n * 4)) || (e = ka.alloc((n + kGuard) * sizeof(K))) ||
            (e = kb.alloc((n + kGuard) * sizeof(K))) || (e = va.alloc((n + kGuard) * 4)) || (e = vb.alloc((n + kGuard) * 4)) ||
            (e = scratch.alloc((size_t)plan.words * 4)) || (e = hist.alloc((size_t)plan.passes * kOsDigits * 4)))
            return e;
        if ((e = hipMemset(ka.p, kFill, (n + kGuard) * sizeof(K))) || (e = hipMemset(kb.p, kFill, (n + kGuard) * sizeof(K))) ||
            (e = hipMemset(va.p, kFill, (n + kGuard) * 4)) || (e = hipMemset(vb.p, kFill, (n + kGuard) * 4)) ||
            (e = hipMemset(scratch.p, kDirty, (size_t)plan.words * 4)) || (e = hipMemset(hist.p, kDirty, (size_t)plan.passes * kOsDigits * 4)))
            return e;
        if (n && ((e = hipMemcpy(ksrc.p, keys, n * sizeof(K), hipMemcpyHostToDevice)) || (e = hipMemcpy(vsrc.p, vals, n * 4, hipMemcpyHostToDevice))))
            return e;
        return hipDeviceSynchronize();   // (the fills are on the null stream; the sorts run on streams that do not wait for it)
    }

    void keys_kernel(hipStream_t st, K flip, uint32_t *clear, uint32_t words)
    {
        k_keys<K><<<256, 256, 0, st>>>(ksrc.as<K>(), vsrc.as<uint32_t>(), ka.as<K>(), va.as<uint32_t>(), n, flip, clear, words);
    }

    hipError_t sort(hipStream_t st, unsigned begin_bit, unsigned end_bit, bool *in_first, const uint32_t *hist_ready = nullptr)
    {
        return osort_pairs<K>(plan, scratch.as<uint32_t>(), ka.as<K>(), kb.as<K>(), va.as<uint32_t>(), vb.as<uint32_t>(), n, begin_bit, end_bit, st,
                              in_first, hist_ready);
    }

    // the sorted pairs out of the pair they ended in; *guards_ok &= every pair's guard elements untouched
    hipError_t read(bool in_first, K *keys_out, uint32_t *vals_out, bool *guards_ok)
    {
        hipError_t e;
        if (n && ((e = hipMemcpy(keys_out, in_first ? ka.p : kb.p, n * sizeof(K), hipMemcpyDeviceToHost)) ||
                  (e = hipMemcpy(vals_out, in_first ? va.p : vb.p, n * 4, hipMemcpyDeviceToHost))))
            return e;
        if ((e = guard_intact(ka.as<K>() + n, kGuard * sizeof(K), kFill, guards_ok)) || (e = guard_intact(kb.as<K>() + n, kGuard * sizeof(K), kFill, guards_ok)) ||
            (e = guard_intact(va.as<uint32_t>() + n, kGuard * 4, kFill, guards_ok)) || (e = guard_intact(vb.as<uint32_t>() + n, kGuard * 4, kFill, guards_ok)))
            return e;
        return hipSuccess;
    }
};

// mode 0: osort_pairs_cleared on a scratch block full of 0xFF;
// mode 1: the product's pattern -- a key-writing kernel clears the dirty scratch block (osort_clear), then osort_pairs;
// mode 2: hist_ready -- the digit histograms `hist` (passes x 256) come from the host, the key kernel clears only the look-back
//         words and tickets, the scratch's histogram region stays 0xFF;
// mode 3: two sorts in a row on one scratch block, each behind its own key kernel: first the complemented keys, then the keys.
// info: [0] *in_first, [1] osort_ends_in_first(plan, n), [2] radix32_plan(...).ends_in_first, [3] guards intact
template <typename K>
int sort_case(const K *keys, const uint32_t *vals, size_t n, unsigned begin_bit, unsigned end_bit, int mode, const uint32_t *hist, K *keys_out,
              uint32_t *vals_out, int *info)
{
    SortBufs<K> b;
    CK(b.init(keys, vals, n, begin_bit, end_bit));
    Stream st;
    CK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    bool in_first = false;
    if (mode == 0) {
        if (n) {
            CK(hipMemcpy(b.ka.p, keys, n * sizeof(K), hipMemcpyHostToDevice));
            CK(hipMemcpy(b.va.p, vals, n * 4, hipMemcpyHostToDevice));
            CK(hipDeviceSynchronize());
        }
        CK(osort_pairs_cleared<K>(b.scratch.template as<uint32_t>(), b.ka.template as<K>(), b.kb.template as<K>(), b.va.template as<uint32_t>(),
                                  b.vb.template as<uint32_t>(), n, begin_bit, end_bit, st.s, &in_first));
    } else if (mode == 1) {
        b.keys_kernel(st.s, (K)0, b.scratch.template as<uint32_t>(), b.plan.words);
        CK(b.sort(st.s, begin_bit, end_bit, &in_first));
    } else if (mode == 2) {
        if (b.plan.passes) CK(hipMemcpy(b.hist.p, hist, (size_t)b.plan.passes * kOsDigits * 4, hipMemcpyHostToDevice));
        b.keys_kernel(st.s, (K)0, b.scratch.template as<uint32_t>() + b.plan.off_ticket, b.plan.words - b.plan.off_ticket);
        CK(b.sort(st.s, begin_bit, end_bit, &in_first, b.hist.template as<uint32_t>()));
    } else if (mode == 3) {
        b.keys_kernel(st.s, ~(K)0, b.scratch.template as<uint32_t>(), b.plan.words);
        CK(b.sort(st.s, begin_bit, end_bit, &in_first));
        b.keys_kernel(st.s, (K)0, b.scratch.template as<uint32_t>(), b.plan.words);
        CK(b.sort(st.s, begin_bit, end_bit, &in_first));
    } else {
        return (int)hipErrorInvalidValue;
    }
    CK(hipStreamSynchronize(st.s));
    bool guards = true;
    CK(b.read(in_first, keys_out, vals_out, &guards));
    if (mode == 2 && b.plan.passes) CK(guard_intact(b.scratch.p, (size_t)b.plan.off_ticket * 4, kDirty, &guards));   // (hist_ready: never written)
    info[0] = in_first;
    info[1] = osort_ends_in_first<K>(b.plan, n);
    info[2] = radix32_plan<K>(n, begin_bit, end_bit).ends_in_first;
    info[3] = guards;
    return 0;
}

// Four sorts on four streams, each with its own buffers and scratch, all queued (key kernel + sort, the product's pattern)
// before the first synchronize.  keys / vals: the four inputs one after the other (ns[0] + ... + ns[3]), the outputs likewise.
template <typename K>
int sort_streams(const K *keys, const uint32_t *vals, const size_t *ns, unsigned begin_bit, unsigned end_bit, K *keys_out, uint32_t *vals_out,
                 int *info /* 4 x in_first, then guards intact */)
{
    SortBufs<K> b[4];
    Stream st[4];
    bool in_first[4] = {};
    size_t at = 0;
    for (int s = 0; s < 4; ++s) {
        CK(b[s].init(keys + at, vals + at, ns[s], begin_bit, end_bit));
        CK(hipStreamCreateWithFlags(&st[s].s, hipStreamNonBlocking));
        at += ns[s];
    }
    for (int s = 0; s < 4; ++s) {
        b[s].keys_kernel(st[s].s, (K)0, b[s].scratch.template as<uint32_t>(), b[s].plan.words);
        CK(b[s].sort(st[s].s, begin_bit, end_bit, &in_first[s]));
    }
    for (int s = 0; s < 4; ++s) CK(hipStreamSynchronize(st[s].s));
    bool guards = true;
    at = 0;
    for (int s = 0; s < 4; ++s) {
        CK(b[s].read(in_first[s], keys_out + at, vals_out + at, &guards));
        info[s] = in_first[s];
        at += ns[s];
    }
    info[4] = guards;
    return 0;
}

// osort_pairs with arguments it must reject, on a stream under capture: whatever it queued would become a node of the captured
// graph (which is never instantiated, so nothing runs).  which: 0 n = 2^30; 1 end_bit above the key width (begin_bit 8: the
// passes still fit); 2 a plan for 10 000 pairs, called with 20 000; 3 a plan for 100, called with 5 000; 4 a plan for 5 000,
// called with 100.  out: [0] the hipError_t, [1] nodes captured, [2] the stream idle afterwards, [3] *in_first
template <typename K> int sort_bad_args(int which, int *out)
{
    constexpr unsigned kBits = sizeof(K) * 8;
    size_t n = 10000, plan_n = 10000;
    unsigned begin_bit = 0, end_bit = kBits;
    switch (which) {
    case 0: n = plan_n = 1ull << 30; break;
    case 1: begin_bit = 8; end_bit = kBits + 1; break;
    case 2: n = 20000; break;
    case 3: plan_n = 100; n = 5000; break;
    case 4: plan_n = 5000; n = 100; break;
    default: return (int)hipErrorInvalidValue;
    }
    const OsortPlan plan = osort_plan<K>(plan_n, begin_bit, end_bit);
    Dev keys, vals, scratch;
    CK(keys.alloc(2 * kGuard * sizeof(K)));
    CK(vals.alloc(2 * kGuard * 4));
    CK(scratch.alloc(kGuard * 4));
    Stream st;
    CK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    CK(hipStreamBeginCapture(st.s, hipStreamCaptureModeRelaxed));
    bool in_first = false;
    const hipError_t err = osort_pairs<K>(plan, scratch.as<uint32_t>(), keys.as<K>(), keys.as<K>() + kGuard, vals.as<uint32_t>(), vals.as<uint32_t>() + kGuard,
                                          n, begin_bit, end_bit, st.s, &in_first);
    hipGraph_t graph = nullptr;
    CK(hipStreamEndCapture(st.s, &graph));
    size_t nodes = 0;
    const hipError_t ge = hipGraphGetNodes(graph, nullptr, &nodes);
    (void)hipGraphDestroy(graph);
    CK(ge);
    out[0] = (int)err;
    out[1] = (int)nodes;
    out[2] = hipStreamQuery(st.s) == hipSuccess;
    out[3] = in_first;
    return 0;
}

// oscan<T, kInclusive> of n values that start `offset` elements into their buffer (in place: out = in); the scratch is 0xFF.
// guards: [0] the `offset` elements in front of the output and 64 behind it untouched, [1] the input unchanged (not in place)
template <typename T, bool kInclusive>
int scan_case(const T *in, T *out, size_t n, size_t offset, int inplace, T init, int *guards)
{
    const size_t total = offset + n + kGuard;
    Dev din, dout, scratch;
    CK(din.alloc(total * sizeof(T)));
    CK(hipMemset(din.p, kFill, total * sizeof(T)));
    if (!inplace) {
        CK(dout.alloc(total * sizeof(T)));
        CK(hipMemset(dout.p, kFill, total * sizeof(T)));
    }
    CK(scratch.alloc(oscan_scratch_bytes<T>(n)));
    CK(hipMemset(scratch.p, kDirty, oscan_scratch_bytes<T>(n)));
    if (n) CK(hipMemcpy(din.as<T>() + offset, in, n * sizeof(T), hipMemcpyHostToDevice));
    CK(hipDeviceSynchronize());
    T *o = (inplace ? din.as<T>() : dout.as<T>());
    Stream st;
    CK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    CK((oscan<T, kInclusive>(din.as<T>() + offset, o + offset, n, init, scratch.p, st.s)));
    CK(hipStreamSynchronize(st.s));
    if (n) CK(hipMemcpy(out, o + offset, n * sizeof(T), hipMemcpyDeviceToHost));
    bool ok = true;
    CK(guard_intact(o, offset * sizeof(T), kFill, &ok));
    CK(guard_intact(o + offset + n, kGuard * sizeof(T), kFill, &ok));
    guards[0] = ok;
    guards[1] = 1;
    if (!inplace && n) {
        std::vector<T> back(n);
        CK(hipMemcpy(back.data(), din.as<T>() + offset, n * sizeof(T), hipMemcpyDeviceToHost));
        guards[1] = std::memcmp(back.data(), in, n * sizeof(T)) == 0;
    }
    return 0;
}

// ---- compaction: the counting half of k_dense_compact (icp_dense.hpp), built from compact.hpp's own pieces

__global__ __launch_bounds__(256) void k_cs_clear(uint32_t *scratch, uint32_t from, uint32_t to)
{
    for (uint32_t w = from + blockIdx.x * blockDim.x + threadIdx.x; w < to; w += gridDim.x * blockDim.x) scratch[w] = 0u;
}

// Every element's exclusive pair of counts (flags a, flags b) and the totals; no scatter, so a wrong count writes nothing
// out of place.  The element that is the last one writes the totals (as k_dense_compact does).
__global__ __launch_bounds__(kCompactBlock) void k_cs_counts(const uint8_t *fa, const uint8_t *fb, uint32_t n, unsigned long long *state,
                                                             uint32_t *ticket, uint32_t *excl_a, uint32_t *excl_b, uint32_t *totals)
{
    __shared__ uint32_t s_bid;
    __shared__ unsigned long long s_wave[kCompactBlock / 64];
    __shared__ unsigned long long s_excl;
    if (threadIdx.x == 0) s_bid = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t bid = s_bid;
    const uint32_t i0 = (bid * kCompactBlock + threadIdx.x) * kCompactItems;
    unsigned long long f[kCompactItems], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCompactItems; ++j) {
        const uint32_t i = i0 + j;
        f[j] = i < n ? (unsigned long long)(fa[i] != 0) | (unsigned long long)(fb[i] != 0) << 32 : 0ull;
        mine += f[j];
    }
    unsigned long long total;
    unsigned long long run = compact_block_scan(mine, s_wave, total);
    run += compact_lookback(state, bid, total, &s_excl);
#pragma unroll
    for (uint32_t j = 0; j < kCompactItems; ++j) {
        const uint32_t i = i0 + j;
        if (i >= n) break;
        excl_a[i] = (uint32_t)run;
        excl_b[i] = (uint32_t)(run >> 32);
        run += f[j];
        if (i == n - 1) {
            totals[0] = (uint32_t)run;
            totals[1] = (uint32_t)(run >> 32);
        }
    }
}

}  // namespace

extern "C" {

int prims_device_count(int *count) { return (int)hipGetDeviceCount(count); }

int prims_osort_u32(const uint32_t *keys, const uint32_t *vals, size_t n, unsigned begin_bit, unsigned end_bit, int mode, const uint32_t *hist,
                    uint32_t *keys_out, uint32_t *vals_out, int *info)
{
    return sort_case<uint32_t>(keys, vals, n, begin_bit, end_bit, mode, hist, keys_out, vals_out, info);
}

int prims_osort_u64(const unsigned long long *keys, const uint32_t *vals, size_t n, unsigned begin_bit, unsigned end_bit, int mode, const uint32_t *hist,
                    unsigned long long *keys_out, uint32_t *vals_out, int *info)
{
    return sort_case<unsigned long long>(keys, vals, n, begin_bit, end_bit, mode, hist, keys_out, vals_out, info);
}

int prims_osort_streams_u32(const uint32_t *keys, const uint32_t *vals, const size_t *ns, unsigned begin_bit, unsigned end_bit, uint32_t *keys_out,
                            uint32_t *vals_out, int *info)
{
    return sort_streams<uint32_t>(keys, vals, ns, begin_bit, end_bit, keys_out, vals_out, info);
}

int prims_osort_streams_u64(const unsigned long long *keys, const uint32_t *vals, const size_t *ns, unsigned begin_bit, unsigned end_bit,
                            unsigned long long *keys_out, uint32_t *vals_out, int *info)
{
    return sort_streams<unsigned long long>(keys, vals, ns, begin_bit, end_bit, keys_out, vals_out, info);
}

int prims_osort_bad_args(int key_bits, int which, int *out)
{
    return key_bits == 64 ? sort_bad_args<unsigned long long>(which, out) : sort_bad_args<uint32_t>(which, out);
}

int prims_oscan_u32(const uint32_t *in, uint32_t *out, size_t n, int inclusive, size_t offset, int inplace, uint32_t init, int *guards)
{
    return inclusive ? scan_case<uint32_t, true>(in, out, n, offset, inplace, init, guards) : scan_case<uint32_t, false>(in, out, n, offset, inplace, init, guards);
}

int prims_oscan_u64(const unsigned long long *in, unsigned long long *out, size_t n, int inclusive, size_t offset, int inplace, unsigned long long init,
                    int *guards)
{
    return inclusive ? scan_case<unsigned long long, true>(in, out, n, offset, inplace, init, guards)
                     : scan_case<unsigned long long, false>(in, out, n, offset, inplace, init, guards);
}

// flags a / b: n bytes each (nonzero: set); `at`: the first scratch word the plan may use.  guards: [0] the scratch words in
// front of `at` and behind the plan's end untouched, [1] the 64 elements behind both outputs untouched
int prims_compact_counts(const uint8_t *fa, const uint8_t *fb, size_t n, uint32_t at, uint32_t *excl_a, uint32_t *excl_b, uint32_t *totals, int *guards)
{
    const CompactPlan p = compact_plan(n, at);
    const size_t words = (size_t)p.end + kGuard;
    Dev dfa, dfb, dea, deb, dtot, scratch;
    CK(dfa.alloc(n));
    CK(dfb.alloc(n));
    CK(dea.alloc((n + kGuard) * 4));
    CK(deb.alloc((n + kGuard) * 4));
    CK(dtot.alloc(2 * 4));
    CK(scratch.alloc(words * 4));
    CK(hipMemset(dea.p, kFill, (n + kGuard) * 4));
    CK(hipMemset(deb.p, kFill, (n + kGuard) * 4));
    CK(hipMemset(dtot.p, kDirty, 2 * 4));
    CK(hipMemset(scratch.p, kDirty, words * 4));
    if (n) {
        CK(hipMemcpy(dfa.p, fa, n, hipMemcpyHostToDevice));
        CK(hipMemcpy(dfb.p, fb, n, hipMemcpyHostToDevice));
    }
    CK(hipDeviceSynchronize());
    Stream st;
    CK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    uint32_t *s = scratch.as<uint32_t>();
    k_cs_clear<<<64, 256, 0, st.s>>>(s, p.off_state, p.end);
    if (p.blocks)
        k_cs_counts<<<p.blocks, kCompactBlock, 0, st.s>>>(dfa.as<uint8_t>(), dfb.as<uint8_t>(), (uint32_t)n,
                                                         reinterpret_cast<unsigned long long *>(s + p.off_state), s + p.off_ticket, dea.as<uint32_t>(),
                                                         deb.as<uint32_t>(), dtot.as<uint32_t>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st.s));
    if (n) {
        CK(hipMemcpy(excl_a, dea.p, n * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(excl_b, deb.p, n * 4, hipMemcpyDeviceToHost));
    }
    CK(hipMemcpy(totals, dtot.p, 2 * 4, hipMemcpyDeviceToHost));
    bool ok = true;
    CK(guard_intact(s, (size_t)at * 4, kDirty, &ok));
    CK(guard_intact(s + p.end, kGuard * 4, kDirty, &ok));
    guards[0] = ok;
    ok = true;
    CK(guard_intact(dea.as<uint32_t>() + n, kGuard * 4, kFill, &ok));
    CK(guard_intact(deb.as<uint32_t>() + n, kGuard * 4, kFill, &ok));
    guards[1] = ok;
    return 0;
}

}  // extern "C"
