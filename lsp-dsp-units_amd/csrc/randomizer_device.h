// lsp::dspu::Randomizer on the device (reference: src/main/util/Randomizer.cpp:108-143), with nothing of a bank in it: one step of
// one generator, the draw as a float, and the three shaped functions of random().  The reference is recorded with contraction
// off, so nothing here may contract (the pragma below holds to the end of the including file, which is what every bit-exact
// kernel of this library sets for itself anyway).
//
// The transcendentals are S*: the float64 function of the float32 argument, rounded once to float32.  The reference's bits there
// are its C library's; tests hold a sample to the interval that S* and its float32 neighbours span.  sqrtf and the float division
// are correctly rounded on both sides (sqrtf, not __fsqrt_rn: that one is the native instruction here, an ulp off now and then).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#pragma clang fp contract(off)

namespace mi_rand
{
    constexpr double RAND_RANGE = 2.32830643654e-10;        // :26, the literal and not 2^-32
    constexpr double RAND_LAMBDA = 2.718281828459045 * 1.4142135623730951;      // M_E * M_SQRT2, a double product
    constexpr float  EXP_LAMBDA = 46.722748f;               // expf(float(RAND_LAMBDA)), bits 0x423AE418
    constexpr double TWO_PI = 2.0 * 3.141592653589793;      // 2.0f * M_PI
    constexpr double HALF_SQRT2 = 1.4142135623730951 * 0.5; // M_SQRT2 * RAND_T

    // :113 in uint32_t.  The shifted truncated product makes the map non-affine: there is no jump-ahead
    __device__ __forceinline__ uint32_t step(uint32_t last, uint32_t mul1, uint32_t mul2, uint32_t add)
    {
        return mul1 * last + ((mul2 * last) >> 16) + add;
    }

    // :114: one float64 product rounded once; 0.0f for 0, 1.0f from 0xFFFFFF80 on
    __device__ __forceinline__ float linear(uint32_t last)
    {
        return __double2float_rn(__uint2double_rn(last) * RAND_RANGE);
    }

    __device__ __forceinline__ float exp_star(float x) { return __double2float_rn(exp(double(x))); }
    __device__ __forceinline__ float log_star(float x) { return __double2float_rn(log(double(x))); }
    __device__ __forceinline__ float cos_star(float x) { return __double2float_rn(cos(double(x))); }

    // RND_EXP, :125
    __device__ __forceinline__ float exponential(float rv)
    {
        const float x = __double2float_rn(RAND_LAMBDA * double(rv));
        return __fdiv_rn(exp_star(x) - 1.0f, EXP_LAMBDA - 1.0f);
    }

    // RND_TRIANGLE, :128-130: the first branch is a float64 product, the second all float
    __device__ __forceinline__ float triangle(float rv)
    {
        if (rv <= 0.5f)
            return __double2float_rn(HALF_SQRT2 * double(sqrtf(rv)));
        return 1.0f - sqrtf(4.0f - 2.0f * (1.0f + rv)) * 0.5f;
    }

    // RND_GAUSSIAN, :132-138: rv from the first draw, rv2 from the second.  rv == 0 gives Inf * cos: kept
    __device__ __forceinline__ float gaussian(float rv, float rv2)
    {
        const float arg = __double2float_rn(TWO_PI * double(rv2));
        return sqrtf(-2.0f * log_star(rv)) * cos_star(arg);
    }
} // namespace mi_rand
