// prerej_score.hpp — what one lane of a pose-scoring kernel does with one source record, and how a wave adds its 64 terms: shared
// by k_prerej_score (prerej_kernels.hpp) and k_scia_score (scia_kernels.hpp), which live in different translation units.
#pragma once

#include "records.hpp"
#include "pointgrid.hpp"

namespace rsreg {

// a wave's 64 terms, met pairwise across lane bit 5, 4, .. 0: lane 0 holds the sum
__device__ __forceinline__ double prerej_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// the contract's score of one source record under one transform: xform in records.hpp's order, the exact nearest float32 d2 within
// limit2 (= the least float >= max_range^2), +inf where p' is not finite or nothing is that near; an inlier iff d2 < limit2
__device__ __forceinline__ float prerej_d2(const Mat34 &m, float px, float py, float pz, const PointGridDev &g, float limit2)
{
    const float3 t = xform(m, px, py, pz);   // (a record that is not finite, or past the end: NaN in, NaN out)
    if (!finite3(t.x, t.y, t.z)) return __int_as_float(0x7f800000);
    return fit_nearest(g, t.x, t.y, t.z, limit2);
}

}  // namespace rsreg
