// lab_kernels.hpp — RGB -> normalised CIE L*a*b*, the colour half of pcl::GeneralizedIterativeClosestPoint6D's 6-D point
// (include/rsreg.h: "GICP6D" holds the contract).  Included by cloud.hip only.
//
// PCL's RGB2Lab goes through two tables (256 entries of sRGB -> linear, 4000 of the CIE f()); behind the tables a colour is
// nine multiplies, six adds, two divides, three table reads and the scaling, each rounded once.  The host function and the
// kernel below run the SAME function over the SAME tables, so their bytes agree.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "records.hpp"

namespace rsreg {

constexpr int kLabSrgbEntries = 256, kLabFEntries = 4000;

struct LabTables {
    float srgb[kLabSrgbEntries];
    float f[kLabFEntries];
};

// computed once, in double, rounded to float (PCL fills both with powf in float: the header's stated deviation)
inline const LabTables &lab_tables()
{
    static const LabTables tables = [] {
        LabTables t;
        for (int i = 0; i < kLabSrgbEntries; ++i) {
            const double f = (double)i / 255.0;
            t.srgb[i] = (float)(f > 0.04045 ? std::pow((f + 0.055) / 1.055, 2.4) : f / 12.92);
        }
        for (int i = 0; i < kLabFEntries; ++i) {
            const double f = (double)i / 4000.0;
            t.f[i] = (float)(f > 0.008856 ? std::cbrt(f) : 7.787 * f + 16.0 / 116.0);
        }
        return t;
    }();
    return tables;
}

// one rounding per operation on both sides (the host's translation unit is built without contraction)
RSREG_HD inline float lab_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    volatile float r = a * b;
    return r;
#endif
}
RSREG_HD inline float lab_add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    volatile float r = a + b;
    return r;
#endif
}
RSREG_HD inline float lab_sub(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    volatile float r = a - b;
    return r;
#endif
}
RSREG_HD inline float lab_div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    volatile float r = a / b;
    return r;
#endif
}

RSREG_HD inline int lab_f_index(float v)
{
    const int i = (int)lab_mul(v, 4000.0f);
    return i < 0 ? 0 : (i > kLabFEntries - 1 ? kLabFEntries - 1 : i);   // (PCL does not clamp: white reads one past its table)
}

RSREG_HD inline float lab_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rgba: r = bits 16-23, g = 8-15, b = 0-7 (PCL's packed rgb word); out = L / 100, a / 120, b / 120
RSREG_HD inline void lab_from_rgb(const float *S, const float *F, uint32_t rgba, float &Ln, float &an, float &bn)
{
    const float r = S[(rgba >> 16) & 255u], g = S[(rgba >> 8) & 255u], b = S[rgba & 255u];
    const float x = lab_add(lab_add(lab_mul(r, 0.412453f), lab_mul(g, 0.357580f)), lab_mul(b, 0.180423f));
    const float y = lab_add(lab_add(lab_mul(r, 0.212671f), lab_mul(g, 0.715160f)), lab_mul(b, 0.072169f));
    const float z = lab_add(lab_add(lab_mul(r, 0.019334f), lab_mul(g, 0.119193f)), lab_mul(b, 0.950227f));
    const float fx = F[lab_f_index(lab_div(x, 0.95047f))], fy = F[lab_f_index(y)], fz = F[lab_f_index(lab_div(z, 1.08883f))];
    float L = lab_sub(lab_mul(116.0f, fy), 16.0f);
    if (L > 100.0f) L = 100.0f;
    const float A = lab_clamp(lab_mul(500.0f, lab_sub(fx, fy)), -120.0f, 120.0f);
    const float B = lab_clamp(lab_mul(200.0f, lab_sub(fy, fz)), -120.0f, 120.0f);
    Ln = lab_div(L, 100.0f);
    an = lab_div(A, 120.0f);
    bn = lab_div(B, 120.0f);
}

// record i of `out` = {L', a', b', 0} of the packed rgb word at byte 16 of record i of `rec`; the colour does not depend on x, y, z
// (tables: the 256 + 4000 floats of lab_tables() in HBM)
__global__ __launch_bounds__(kBlock) void k_cloud_lab(const char *rec, size_t stride, uint32_t n, const float *tables, float4 *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t rgba = *reinterpret_cast<const uint32_t *>(rec + (size_t)i * stride + 16);
    float L, a, b;
    lab_from_rgb(tables, tables + kLabSrgbEntries, rgba, L, a, b);
    out[i] = make_float4(L, a, b, 0.0f);
}

}  // namespace rsreg
