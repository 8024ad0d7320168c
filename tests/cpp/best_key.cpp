// best_key.cpp — the ordering the dense search's running best relies on (csrc/icp_dense.hpp: DBest): for keys
// d_bits << 32 | index with d a squared distance (0 ... +inf: bits 0 ... 0x7f800000), the minimum of two keys read as IEEE
// doubles (the candidate's through fabs, a source modifier on the GPU) is the minimum of the keys as unsigned 64-bit integers.  All pairs of the edge patterns (tests/test_best_key_cpu.py),
// then pseudo-random pairs.  Prints "best_key ok: <pairs> pairs" or the first mismatches.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static double as_double(uint64_t k)
{
    double d;
    std::memcpy(&d, &k, 8);
    return d;
}

static uint64_t as_bits(double d)
{
    uint64_t k;
    std::memcpy(&k, &d, 8);
    return k;
}

static int check(uint64_t a, uint64_t b, int &bad)
{
    volatile double da = as_double(a), db = as_double(b);   // (volatile: the minimum is taken at run time, in the FPU's own mode)
    const uint64_t got = as_bits(std::fmin(da, std::fabs(db))), want = a < b ? a : b;   // (the candidate goes in as |key|, as in dconsider)
    if (got != want && bad++ < 10) std::printf("mismatch: fmin(%016llx, %016llx) = %016llx, min = %016llx\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)got, (unsigned long long)want);
    if (!std::isfinite((double)da) || std::signbit((double)da)) {
        if (bad++ < 10) std::printf("not a finite non-negative double: %016llx\n", (unsigned long long)a);
    }
    return 1;
}

int main()
{
    const uint32_t d_bits[] = {0u, 1u, 0x007fffffu, 0x00800000u, 0x3f800000u, 0x7f7fffffu, 0x7f800000u};   // 0, least and largest subnormal, least normal, 1, FLT_MAX, +inf
    const uint32_t index[] = {0u, 1u, 0xfffffffeu, 0xffffffffu};
    std::vector<uint64_t> keys;
    for (uint32_t d : d_bits)
        for (uint32_t i : index) keys.push_back((uint64_t)d << 32 | i);
    int bad = 0;
    long long pairs = 0;
    for (uint64_t a : keys)
        for (uint64_t b : keys) pairs += check(a, b, bad);   // (equal d with every pair of indices, and a == b, are among them)
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int n = 0; n < 2000000; ++n) {
        const uint64_t r = next(), q = next();
        const uint64_t a = ((r >> 32) % 0x7f800001ull) << 32 | (uint32_t)r;
        uint64_t b = ((q >> 32) % 0x7f800001ull) << 32 | (uint32_t)q;
        if (n % 4 == 0) b = (a & 0xffffffff00000000ull) | (uint32_t)q;   // equal d
        if (n % 64 == 1) b = 0x7f800000ffffffffull;                       // the start value
        pairs += check(a, b, bad);
    }
    // a distance that came out as a NaN (default pattern, either sign) never wins, whatever the best: |key| is a finite double above the start value
    for (uint32_t d : {0x7fc00000u, 0xffc00000u})
        for (uint64_t best : keys) {
            volatile double db = as_double(best), dk = as_double((uint64_t)d << 32 | 5u);
            if (as_bits(std::fmin(db, std::fabs(dk))) != best && bad++ < 10) std::printf("a NaN distance won: d bits %08x against %016llx\n", d, (unsigned long long)best);
            ++pairs;
        }
    if (bad) return 1;
    std::printf("best_key ok: %lld pairs\n", pairs);
    return 0;
}
