// Grad-CAM (Selvaraju et al. 2017) of an encoder stage: the two steps after the engine has the stage output A [N, h*w, C]
// (NHWC, storage type) and the gradients G of T target logits with respect to it.
//
//   sm3_cam_alpha: alpha[t, n, c] = (sum over p of G[t, n, p, c]) / (h*w).  One thread per (t, n, c) adds the positions in
//                  ascending order; consecutive threads read consecutive channels (coalesced).
//   sm3_cam_maps:  low[n, t, p] = ReLU(sum over c of alpha[t, n, c] * A[n, p, c]), then the bilinear upsample to H x W
//                  (F.interpolate(mode="bilinear", align_corners=False)) and (cam - min) / (1e-7 + max(cam - min)) per map.
//                  Two launches: one wave per row (n, p) for the low-resolution maps -- lane l owns channels 8l .. 8l+7 of
//                  every 512-channel chunk and adds them in ascending order, then a fixed xor butterfly adds the 64 lane sums
//                  -- and one 1024-thread workgroup per (n, t) map for the upsample, whose min / max (exact, so order-free) are reduced
//                  in LDS before the second pass writes the normalised map.
// No atomics anywhere: every output is written once by a fixed order of operations that depends on its own inputs only, so
// equal inputs give equal bits across calls, grids and batch positions.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTChunk = 8;  // targets accumulated per pass over a row of A
constexpr int kUpThreads = 1024;  // one workgroup per map: 16 waves, so that N * T maps fill the CUs
constexpr int kUpWaves = kUpThreads / 64;

template <typename T>
__device__ __forceinline__ void load8(const T* p, float v[8]);

template <>
__device__ __forceinline__ void load8<float>(const float* p, float v[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}

template <>
__device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float v[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

template <>
__device__ __forceinline__ void load8<f16_t>(const f16_t* p, float v[8]) {
    const f16x8 h = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
}

template <typename T>
__global__ void __launch_bounds__(kThreads) cam_alpha_kernel(const T* __restrict__ g, float* __restrict__ alpha, int64_t TN,
                                                             int HW, int C) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // (t * N + n) * C + c
    if (i >= TN * C) return;
    const int64_t tn = i / C;
    const int c = (int)(i - tn * C);
    const T* p = g + tn * HW * C + c;
    float s = 0.f;
#pragma unroll 8
    for (int q = 0; q < HW; ++q) s += ElemTraits<T>::load(p + (int64_t)q * C);
    alpha[i] = s / (float)HW;
}

// one wave per row r = n * HW + p of A
template <typename T>
__global__ void __launch_bounds__(kThreads) cam_low_kernel(const T* __restrict__ a, const float* __restrict__ alpha,
                                                           float* __restrict__ low, int N, int HW, int C, int Tn) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= (int64_t)N * HW) return;  // wave-uniform
    const int n = (int)(r / HW);
    const int p = (int)(r - (int64_t)n * HW);
    const T* row = a + r * C;
    for (int t0 = 0; t0 < Tn; t0 += kTChunk) {
        const int nt = min(kTChunk, Tn - t0);
        float acc[kTChunk];
#pragma unroll
        for (int j = 0; j < kTChunk; ++j) acc[j] = 0.f;
        for (int c0 = lane * 8; c0 < C; c0 += 64 * 8) {
            float v[8];
            load8<T>(row + c0, v);
#pragma unroll
            for (int j = 0; j < kTChunk; ++j) {
                if (j < nt) {
                    const float* al = alpha + ((int64_t)(t0 + j) * N + n) * C + c0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[j] = fmaf(v[e], al[e], acc[j]);
                }
            }
        }
        // fixed butterfly: every lane ends with the same sum (a + b == b + a)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int j = 0; j < kTChunk; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
        }
        if (lane < nt) {
            float s = acc[0];
#pragma unroll
            for (int j = 1; j < kTChunk; ++j) s = lane == j ? acc[j] : s;
            low[((int64_t)n * Tn + t0 + lane) * HW + p] = relu_f32(s);
        }
    }
}

// PyTorch's upsample_bilinear2d (align_corners=False, no scale factor) at output position (oy, ox).  No contraction: both
// passes of cam_upsample_kernel must round every value the same way (so that no value falls below the map's minimum).  On the
// last row / column the neighbour is the pixel itself and it gets the whole weight: a constant edge stays exactly constant
// (l0 * v + l1 * v may round away from v), and a 1 x 1 map upsamples to an exactly constant map.
__device__ __forceinline__ float bilinear(const float* __restrict__ m, int h, int w, float sh, float sw, int oy, int ox) {
#pragma clang fp contract(off)
    const float yr = fmaxf(sh * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float xr = fmaxf(sw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)yr, h - 1), x0 = min((int)xr, w - 1);  // (the clamp never binds; it keeps reads in the map)
    const int yp = y0 < h - 1 ? 1 : 0, xp = x0 < w - 1 ? 1 : 0;
    const float ly1 = yp ? yr - (float)y0 : 0.f, lx1 = xp ? xr - (float)x0 : 0.f;
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float* r0 = m + (int64_t)y0 * w + x0;
    const float* r1 = r0 + (int64_t)yp * w;
    return ly0 * (lx0 * r0[0] + lx1 * r0[xp]) + ly1 * (lx0 * r1[0] + lx1 * r1[xp]);
}

// one workgroup per map (n, t): min / max of the upsampled map, then the normalised map
__global__ void __launch_bounds__(kUpThreads) cam_upsample_kernel(const float* __restrict__ low, float* __restrict__ maps,
                                                                  int h, int w, int H, int W) {
    __shared__ float smin[kUpWaves], smax[kUpWaves];
    const float* m = low + (int64_t)blockIdx.x * h * w;
    float* out = maps + (int64_t)blockIdx.x * H * W;
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int P = H * W;
    float mn = INFINITY, mx = -INFINITY;
    for (int q = threadIdx.x; q < P; q += kUpThreads) {
        const float v = bilinear(m, h, w, sh, sw, q / W, q % W);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    // min and max are exact: the reduction order does not change them
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) smin[threadIdx.x >> 6] = mn, smax[threadIdx.x >> 6] = mx;
    __syncthreads();
    mn = smin[0], mx = smax[0];
#pragma unroll
    for (int i = 1; i < kUpWaves; ++i) mn = fminf(mn, smin[i]), mx = fmaxf(mx, smax[i]);
    const float den = 1e-7f + (mx - mn);  // max(cam - min) = max - min: subtracting mn is monotone
    for (int q = threadIdx.x; q < P; q += kUpThreads) out[q] = (bilinear(m, h, w, sh, sw, q / W, q % W) - mn) / den;
}

constexpr int64_t kMax31 = 0x7fffffffLL;

}  // namespace

extern "C" int sm3_cam_alpha(int dtype, const void* g, float* alpha, int T, int N, int HW, int C, void* stream) {
    if (!g || !alpha || T < 1 || N < 1 || HW < 1 || C < 1) return SM3_EINVAL;
    if ((int64_t)T * N * C > kMax31 * 64 || (int64_t)T * N * HW > kMax31) return SM3_EINVAL;
    if (!SM3_DTYPE_OK(dtype)) return SM3_EDTYPE;
    const int64_t TN = (int64_t)T * N;
    const dim3 grid((uint32_t)((TN * C + kThreads - 1) / kThreads));
#define CAM_ALPHA(E)                                                                                                       \
    hipLaunchKernelGGL(cam_alpha_kernel<E>, grid, dim3(kThreads), 0, (hipStream_t)stream, static_cast<const E*>(g), alpha, \
                       TN, HW, C)
    SM3_DISPATCH_DTYPE(dtype, CAM_ALPHA);
#undef CAM_ALPHA
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_cam_maps(int dtype, const void* a, const float* alpha, float* low, float* maps, int N, int T, int h, int w,
                            int C, int H, int W, void* stream) {
    if (!a || !alpha || !low || !maps || N < 1 || T < 1 || h < 1 || w < 1 || C < 1 || H < 1 || W < 1) return SM3_EINVAL;
    if ((int64_t)h * w > kMax31 || (int64_t)H * W > kMax31 || (int64_t)N * h * w > kMax31 ||
        (int64_t)N * T > kMax31 || (int64_t)N * T * h * w > kMax31 * 64)
        return SM3_EINVAL;
    if (!SM3_DTYPE_OK(dtype)) return SM3_EDTYPE;
    if (C % 8 || (reinterpret_cast<uintptr_t>(a) & 15)) return SM3_EALIGN;
    const int HW = h * w;
    const dim3 grid((uint32_t)(((int64_t)N * HW + kWaves - 1) / kWaves));
#define CAM_LOW(E)                                                                                                             \
    hipLaunchKernelGGL(cam_low_kernel<E>, grid, dim3(kThreads), 0, (hipStream_t)stream, static_cast<const E*>(a), alpha, low, \
                       N, HW, C, T)
    SM3_DISPATCH_DTYPE(dtype, CAM_LOW);
#undef CAM_LOW
    SM3_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_upsample_kernel, dim3((uint32_t)((int64_t)N * T)), dim3(kUpThreads), 0, (hipStream_t)stream, low, maps,
                       h, w, H, W);
    SM3_CHECK_LAUNCH();
    return 0;
}
