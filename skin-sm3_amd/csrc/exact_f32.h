// What the attribution kernels (attr.hip, rise.hip) and the corruption kernels (corrupt.hip) share and must keep bit-identical:
// separately rounded f32 operations, the blend built from them, the Philox4x32-10 generator and the normals made from its words.
#pragma once
#include <math.h>

#include "common.h"

// Contraction is switched off inside each body: plain + and * compiled under the default contraction are still fused by the
// backend after inlining, and the numpy restatements in the tests depend on every product and sum being rounded on its own.
static __device__ __forceinline__ float fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
static __device__ __forceinline__ float fsub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
static __device__ __forceinline__ float fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// base + alpha * (x - base), three separately rounded operations
static __device__ __forceinline__ float blend(float x, float b, float alpha) {
    return fadd(b, fmul(alpha, fsub(x, b)));
}

// counter (c0, c1, c2, c3), key (k0, k1) -> four random words (Salmon et al., SC 2011)
static __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// two standard normals from two words: u = (w + 0.5) * 2^-32 in (0, 1), r = sqrt(-2 log(u_a)), z = r * cos(2 pi u_b), r * sin(2 pi
// u_b) in float64, rounded to f32 once (sm3_attr_noise's rule, which sm3_corrupt_pointwise follows)
static __device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const double ua = ((double)wa + 0.5) * 0x1p-32, ub = ((double)wb + 0.5) * 0x1p-32;
    const double r = sqrt(-2.0 * log(ua));
    double s, co;
    sincospi(2.0 * ub, &s, &co);
    z0 = (float)(r * co), z1 = (float)(r * s);
}
