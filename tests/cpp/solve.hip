// solve.hip — test-only harness around the two device forms of the Umeyama solve, as the product compiles them
// (csrc/icp_kernels.hpp included as it is): umeyama_from_sums on one lane of a wave (what k_icp_solve runs) and
// umeyama_wave on a full 64-lane wave (what k_final_reduce_solve runs).  A shared library with one extern "C" entry point
// on host arrays, loaded by tests/umeyama_cases.py (ctypes), built into tests/cpp/_build/ with the library's own flags plus
// -shared -I<csrc> -I<include>.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icp_kernels.hpp"

using namespace rsreg;

namespace {

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

// one wave per case: sums[17] and the V to start from in, from each form the 4 x 4 (column-major), the V it leaves and
// whether it solved out
__global__ __launch_bounds__(64) void k_solve_cases(const double *sums, const double *v_in, int n, float *t_lane, double *v_lane, int *ok_lane,
                                                    float *t_wave, double *v_wave, int *ok_wave)
{
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (c >= n) return;   // (uniform over the wave)
    double s[RSREG_NUM_SUMS];
#pragma unroll
    for (int k = 0; k < RSREG_NUM_SUMS; ++k) s[k] = sums[(size_t)c * RSREG_NUM_SUMS + k];
    if (lane == 0) {
        double v[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) v[i] = v_in[(size_t)c * 9 + i];
        Mat4f t = Mat4f::identity();
        ok_lane[c] = umeyama_from_sums(s, t, v) ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t_lane[(size_t)c * 16 + i] = t.m[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) v_lane[(size_t)c * 9 + i] = v[i];
    }
    // all 64 lanes again
    double v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = v_in[(size_t)c * 9 + i];
    Mat4f t = Mat4f::identity();
    const bool solved = umeyama_wave(s, t, v);
    if (lane == 0) {
        ok_wave[c] = solved ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t_wave[(size_t)c * 16 + i] = t.m[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) v_wave[(size_t)c * 9 + i] = v[i];
    }
}

}  // namespace

// n cases.  Returns a hipError_t (0: success).
extern "C" int solve_cases(const double *sums, const double *v_in, int n, float *t_lane, double *v_lane, int *ok_lane, float *t_wave,
                           double *v_wave, int *ok_wave)
{
    if (n <= 0) return 0;
    const size_t N = (size_t)n;
    Dev d_sums, d_vin, d_tl, d_vl, d_ol, d_tw, d_vw, d_ow;
    CK(d_sums.alloc(N * RSREG_NUM_SUMS * 8));
    CK(d_vin.alloc(N * 9 * 8));
    CK(d_tl.alloc(N * 16 * 4));
    CK(d_vl.alloc(N * 9 * 8));
    CK(d_ol.alloc(N * 4));
    CK(d_tw.alloc(N * 16 * 4));
    CK(d_vw.alloc(N * 9 * 8));
    CK(d_ow.alloc(N * 4));
    CK(hipMemcpy(d_sums.p, sums, N * RSREG_NUM_SUMS * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_vin.p, v_in, N * 9 * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d_tl.p, 0xFF, N * 16 * 4));
    CK(hipMemset(d_tw.p, 0xFF, N * 16 * 4));
    CK(hipMemset(d_vl.p, 0xFF, N * 9 * 8));
    CK(hipMemset(d_vw.p, 0xFF, N * 9 * 8));
    CK(hipMemset(d_ol.p, 0xFF, N * 4));
    CK(hipMemset(d_ow.p, 0xFF, N * 4));
    k_solve_cases<<<(unsigned)n, 64>>>(d_sums.as<double>(), d_vin.as<double>(), n, d_tl.as<float>(), d_vl.as<double>(), d_ol.as<int>(),
                                       d_tw.as<float>(), d_vw.as<double>(), d_ow.as<int>());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(t_lane, d_tl.p, N * 16 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(v_lane, d_vl.p, N * 9 * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ok_lane, d_ol.p, N * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(t_wave, d_tw.p, N * 16 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(v_wave, d_vw.p, N * 9 * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ok_wave, d_ow.p, N * 4, hipMemcpyDeviceToHost));
    return 0;
}
