// gut_fixed.h — what the image-space stages share: the fixed-point unit of the integer adjoints and the
// per-view Adam element.  ONE copy of each, so that the environment map and the bilateral grids scale by the same rule and the
// exposures and the grids step by the same arithmetic.
#pragma once
#include "gut_internal.h"

namespace gut {

__device__ __forceinline__ float pow2f_env(int s) { return __uint_as_float((uint32_t)(s + 127) << 23); }   // s in -126..126
__device__ __forceinline__ float finite_or_zero_env(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 0.0f : x; }

// The exponent s of the fixed-point unit 2^-s (DESIGN.md §17's rule with pixels in the place of tiles): the largest finite |c| has
// the bits max_bits, |c| < 2^e with e read from the exponent field, and s = 40 - e less the bits by which the view has more than
// 2^22 pixels.  A pixel's weights sum to 1, so a cell's total stays below 2^62 (+ the roundings).  Clamped so that 2^s and
// 2^-s are normal floats; a cotangent of zeros takes s = 0.
__device__ __forceinline__ int env_scale_exponent(uint32_t max_bits, uint64_t pixels) {
    if (max_bits == 0u) return 0;
    const int e = max((int)(max_bits >> 23), 1) - 126;
    const int extra = pixels > (1ull << 22) ? (64 - (int)__clzll((long long)(pixels - 1ull)) - 22) : 0;   // ceil(log2(pixels)) - 22
    return min(max(40 - e - extra, -126), 126);
}

// One element of a per-view Adam step at the view's visit t (already advanced): the moments in place, the betas held in float32,
// 1 - beta^t formed in double from them and rounded once.  No contraction, whatever the unit is built with, so that a host form can
// follow it bit for bit.
__device__ __forceinline__ void view_adam_element(float g, float* __restrict__ p, float* __restrict__ m1, float* __restrict__ m2, int32_t t,
                                                  float lr, float beta1, float beta2, float eps) {
#pragma clang fp contract(off)
    const float m = beta1 * m1[0] + (1.0f - beta1) * g;
    const float v = beta2 * m2[0] + ((1.0f - beta2) * g) * g;
    m1[0] = m;
    m2[0] = v;
    const float c1 = (float)(1.0 - pow((double)beta1, (double)t)), c2 = (float)(1.0 - pow((double)beta2, (double)t));
    p[0] = p[0] - (lr * (m / c1)) / (sqrtf(v / c2) + eps);
}

}  // namespace gut
