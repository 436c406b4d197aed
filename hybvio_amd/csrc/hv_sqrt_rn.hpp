// The correctly rounded binary32 square root of the min-eigenvalue corner response, shared by gftt.hip (GPU-GFTT) and
// gftt_legacy.hip (GFTT): both reproduce cv::cornerMinEigenVal as oracle/gftt_oracle.c evaluates it, to the bit.
#pragma once
#include <hip/hip_runtime.h>

namespace hv {

// sqrtf for the response, correctly rounded as the oracle's. With contraction off the compiler's own expansion also scales
// arguments below 2^-96 and tests the class of the input, about 16 instructions; the detector's arguments are sums of squares
// and almost never that small. Here 0 and everything from 2^-96 up take the hardware approximation (1 ulp) and the choice
// between it and its two neighbours by the sign of their residuals x - n * s, each one explicit fma (a single rounding, not a
// contraction): from 2^-96 up the lowest bit of n * s is at least 2^-142, so a non-zero residual never rounds to zero. For 0
// the lower neighbour is a NaN and the upper one leaves a residual of -0: both comparisons fail and 0 stays. Arguments in
// (0, 2^-96) -- the square of a one-ulp difference of two sums near 2^-25 is exactly 2^-96, so they can occur -- take sqrtf.
__device__ __forceinline__ bool sqrt_arg_tiny(float x) { return __float_as_uint(x) - 1u < 0x0F800000u - 1u; }   // 0 < x < 2^-96
__device__ __forceinline__ float sqrt_rn_normal(float x)
{
    const float s = __builtin_amdgcn_sqrtf(x);
    const float lo = __uint_as_float(__float_as_uint(s) - 1u), hi = __uint_as_float(__float_as_uint(s) + 1u);
    const float res_lo = __builtin_fmaf(-lo, s, x), res_hi = __builtin_fmaf(-hi, s, x);
    float r = res_lo <= 0.f ? lo : s;
    r = res_hi > 0.f ? hi : r;
    return r;
}
__device__ __forceinline__ float sqrt_rn(float x)
{
    if (__builtin_expect(sqrt_arg_tiny(x), 0)) return sqrtf(x);
    return sqrt_rn_normal(x);
}

}  // namespace hv
