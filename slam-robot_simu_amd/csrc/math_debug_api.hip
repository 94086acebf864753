// math_debug_api.hip -- slam_debug_math: each routine of fastmath.hpp run on
// the device, one lane per argument, so that a test can hold the compiled
// device code (the fma_k / fma_kk inline assembly, the 1.5 2^52 shift read
// from kdm's low word, v_ldexp_f64 into the subnormals, the frexp builtins,
// the v_rsq_f64 / v_rcp_f64 seeds, the LDS staging of the three tables, the
// range selects and the hand-off to the library sincos) to a host restatement
// bit for bit (tests/test_gpu_fastmath.py, tests/fastmath_ref.py).  The kernel
// calls the very inline functions the production kernels call; the tables
// reach them the way production stages them: rng_tabs_stage for the RNG
// tables, the plain exp table for exp_tab and (t.x / 2, t.y) for exp_nhalf
// (pf_device.inl, likelihood_lanes).
#include "device_mem.hpp"

namespace slam {

template <int FN>
__global__ __launch_bounds__(256) void debug_math_kernel(const int64_t n, const double* __restrict__ in,
                                                         double* __restrict__ out) {
    constexpr bool kRng = FN == SLAM_MATH_HEADING_SINCOS_TAB || FN == SLAM_MATH_RNG_LOG_TAB ||
                          FN == SLAM_MATH_RNG_SINCOS2PI_TAB;
    constexpr bool kExp = FN == SLAM_MATH_EXP_TAB || FN == SLAM_MATH_EXP_TAB_NONPOS;
    constexpr bool kExpHalf = FN == SLAM_MATH_EXP_NHALF || FN == SLAM_MATH_EXP_NHALF_NONPOS;
    __shared__ RngTabsLds s_rng;
    __shared__ double2 s_etab[64];
    RngTabs T{nullptr, nullptr, nullptr};
    if (kRng) T = rng_tabs_stage(&s_rng, (int)threadIdx.x, 256);
    if ((kExp || kExpHalf) && threadIdx.x < 64) {
        const double2 t = kExpTab64[threadIdx.x];
        s_etab[threadIdx.x] = kExpHalf ? make_double2(t.x * 0.5, t.y) : t;
    }
    __syncthreads();                       // every lane of the block, before the bounds test
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = in[4 * i], b = in[4 * i + 1], c = in[4 * i + 2], d = in[4 * i + 3];
    double r0 = 0.0, r1 = 0.0;
    switch (FN) {
    case SLAM_MATH_FAST_SINCOS: fast_sincos(a, &r0, &r1); break;
    case SLAM_MATH_SMALL_SINCOS: small_sincos(a, &r0, &r1); break;
    case SLAM_MATH_ROTATE_SC: rotate_sc(a, b, c, d, &r0, &r1); break;
    case SLAM_MATH_HEADING_SINCOS_TAB: heading_sincos_tab(a, T, &r0, &r1); break;
    case SLAM_MATH_EXP_LEAN: r0 = exp_lean(a); break;
    case SLAM_MATH_EXP_TAB: r0 = exp_tab<false>(a, s_etab); break;
    case SLAM_MATH_EXP_TAB_NONPOS: r0 = exp_tab<true>(a, s_etab); break;
    case SLAM_MATH_EXP_NHALF: r0 = exp_nhalf<false>(a, s_etab); break;
    case SLAM_MATH_EXP_NHALF_NONPOS: r0 = exp_nhalf<true>(a, s_etab); break;
    case SLAM_MATH_SQRT_POS: r0 = sqrt_pos(a); break;
    case SLAM_MATH_RNG_LOG_TAB: r0 = rng_log_tab((uint32_t)a, T); break;
    case SLAM_MATH_RNG_SINCOS2PI_TAB: rng_sincos2pi_tab((uint32_t)a, T, &r0, &r1); break;
    case SLAM_MATH_RNG_LOG_SCALED: r0 = rng_log_scaled(a, (int)b); break;
    // the word's uniform as bm_pair forms it (common.hpp)
    case SLAM_MATH_RNG_SINCOS2PI: rng_sincos2pi(((double)(uint32_t)a + 1.0) * 0x1p-32, &r0, &r1); break;
    }
    out[2 * i] = r0;
    out[2 * i + 1] = r1;
}

template <int FN>
void launch_debug_math(unsigned grid, int64_t n, const double* in, double* out) {
    debug_math_kernel<FN><<<grid, 256>>>(n, in, out);
}

}  // namespace slam

using namespace slam;

extern "C" int slam_debug_math(int device, int32_t fn, int64_t n, const double* in, double* out) {
    SLAM_ARG_CHECK(in && out && n >= 0 && n <= (int64_t(1) << 26) && fn >= 0 && fn < SLAM_MATH_COUNT,
                   "slam_debug_math: bad arguments");
    if (n == 0) return SLAM_OK;
    int ndev = 0;
    SLAM_HIP_TRY(hipGetDeviceCount(&ndev));
    SLAM_ARG_CHECK(device >= 0 && device < ndev, "slam_debug_math: no such HIP device");
    SLAM_HIP_TRY(hipSetDevice(device));
    DeviceMem mem;
    double* d = nullptr;                   // n x 4 operands, then n x 2 results
    const int rc = mem.alloc(&d, 6 * (size_t)n);
    if (rc) return rc;
    double* d_out = d + 4 * n;
    hipError_t e = hipMemcpy(d, in, 4 * n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)((n + 255) / 256);
        switch (fn) {
#define SLAM_MATH_CASE(F) case F: launch_debug_math<F>(grid, n, d, d_out); break
        SLAM_MATH_CASE(SLAM_MATH_FAST_SINCOS);
        SLAM_MATH_CASE(SLAM_MATH_SMALL_SINCOS);
        SLAM_MATH_CASE(SLAM_MATH_ROTATE_SC);
        SLAM_MATH_CASE(SLAM_MATH_HEADING_SINCOS_TAB);
        SLAM_MATH_CASE(SLAM_MATH_EXP_LEAN);
        SLAM_MATH_CASE(SLAM_MATH_EXP_TAB);
        SLAM_MATH_CASE(SLAM_MATH_EXP_TAB_NONPOS);
        SLAM_MATH_CASE(SLAM_MATH_EXP_NHALF);
        SLAM_MATH_CASE(SLAM_MATH_EXP_NHALF_NONPOS);
        SLAM_MATH_CASE(SLAM_MATH_SQRT_POS);
        SLAM_MATH_CASE(SLAM_MATH_RNG_LOG_TAB);
        SLAM_MATH_CASE(SLAM_MATH_RNG_SINCOS2PI_TAB);
        SLAM_MATH_CASE(SLAM_MATH_RNG_LOG_SCALED);
        SLAM_MATH_CASE(SLAM_MATH_RNG_SINCOS2PI);
#undef SLAM_MATH_CASE
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, 2 * n * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SLAM_ERR_HIP, std::string("slam_debug_math: ") + hipGetErrorString(e));
    return SLAM_OK;
}
