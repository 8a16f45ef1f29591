// Pixel-level attributions (Integrated Gradients, Sundararajan et al. 2017; SmoothGrad, Smilkov et al. 2017): the four
// streaming steps around the encoders' forward and data-only backward (sm3hip/attr.py).  x: one modality's images, [N][E]
// f32 with E = 3 * H * W (NCHW rows).
//
//   sm3_attr_path:       out[j][n][e] = base + alpha_k * (x - base), k = k0 + j, alpha_k = (2k + 1) / (2 * steps) (midpoint
//                        rule), as fadd(base, fmul(alpha, fsub(x, base))): three separately rounded f32 operations, never an
//                        FMA, so that a numpy restatement gives equal bits.
//   sm3_attr_noise:      out[j][n][e] = fadd(x, fmul(sigma[n], z)), z a standard normal that is a function of (seed, sample,
//                        n, e) alone: Philox4x32-10 with key = the 64-bit seed (low word first) and counter (e / 4, n, sample,
//                        0), sample = k0 + j * stride; Box-Muller on the word pairs (w0, w1) and (w2, w3) -- u = (w + 0.5) *
//                        2^-32 in (0, 1), r = sqrt(-2 log(u_a)), z = r * cos(2 pi u_b), r * sin(2 pi u_b) -- in float64
//                        (log, sqrt, sincospi), rounded to f32 once; element e takes lane e % 4.
//   sm3_attr_accumulate: acc[n][e] = (((acc + w * f(g[0])) + w * f(g[1])) + ...), f = identity or square, ascending j, each
//                        product and each sum rounded separately.  One thread owns four consecutive elements over all j, so the
//                        result does not depend on how the steps were cut into calls.
//   sm3_attr_finish:     attr = (x - base) * acc (mode 0, IG) or acc (mode 1, SmoothGrad); maps[t][n][p] = the sum over the
//                        channels (ascending) of |attr|; sums[t][n] = the sum of attr over all elements in float64: a thread
//                        adds its 4 positions x C channels (channel-major, positions ascending), a fixed xor butterfly adds
//                        the 64 lanes, the waves' sums are added in wave order, the workgroup's partial is stored plainly, and a
//                        second launch adds the partials of a row in index order.
// No atomics: every output is written once by a fixed order of operations on its own inputs.
#include <math.h>

#include "exact_f32.h"

// Contraction off for the file: every product and sum below is rounded on its own (the numpy restatements in the tests
// depend on it).  The toolchain's fadd / fmul are plain + and * compiled under the default contraction, which the
// backend still fuses after inlining, so the three operations are written in exact_f32.h (shared with rise.hip).
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kMax31 = 0x7fffffffLL;

__global__ void __launch_bounds__(kThreads) attr_path_kernel(const float4* __restrict__ x, const float4* __restrict__ base,
                                                             int base_n, float4* __restrict__ out, int64_t NE4, int64_t E4,
                                                             int k0, int c, int steps) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // j * NE4 + (n * E4 + e4)
    if (i >= NE4 * c) return;
    const int j = (int)(i / NE4);
    const int64_t r = i - (int64_t)j * NE4;
    const float alpha = (float)(2 * (k0 + j) + 1) / (float)(2 * steps);
    const float4 v = x[r];
    const float4 b = base[base_n == 1 ? r % E4 : r];
    out[i] = make_float4(blend(v.x, b.x, alpha), blend(v.y, b.y, alpha), blend(v.z, b.z, alpha), blend(v.w, b.w, alpha));
}

__global__ void __launch_bounds__(kThreads) attr_noise_kernel(const float4* __restrict__ x, const float* __restrict__ sigma,
                                                              float4* __restrict__ out, int64_t NE4, int64_t E4, int k0, int c,
                                                              int stride, uint32_t key0, uint32_t key1) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // j * NE4 + (n * E4 + e4)
    if (i >= NE4 * c) return;
    const int j = (int)(i / NE4);
    const int64_t r = i - (int64_t)j * NE4;
    const int n = (int)(r / E4);
    const uint32_t e4 = (uint32_t)(r - (int64_t)n * E4);
    uint32_t w[4];
    philox4x32_10(e4, (uint32_t)n, (uint32_t)(k0 + j * stride), 0u, key0, key1, w);
    float4 z;
    box_muller(w[0], w[1], z.x, z.y);
    box_muller(w[2], w[3], z.z, z.w);
    const float s = sigma[n];
    const float4 v = x[r];
    out[i] = make_float4(fadd(v.x, fmul(s, z.x)), fadd(v.y, fmul(s, z.y)),
                         fadd(v.z, fmul(s, z.z)), fadd(v.w, fmul(s, z.w)));
}

template <bool kSquared>
__device__ __forceinline__ float step(float a, float g, float w) {
    return fadd(a, fmul(w, kSquared ? fmul(g, g) : g));
}

template <bool kSquared>
__global__ void __launch_bounds__(kThreads) attr_accumulate_kernel(const float4* __restrict__ g, float4* __restrict__ acc,
                                                                   int c, int64_t NE4, float w) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= NE4) return;
    float4 a = acc[i];
    auto add = [&](const float4& v) {
        a.x = step<kSquared>(a.x, v.x, w), a.y = step<kSquared>(a.y, v.y, w);
        a.z = step<kSquared>(a.z, v.z, w), a.w = step<kSquared>(a.w, v.w, w);
    };
    int j = 0;
    for (; j + 4 <= c; j += 4) {  // four loads in flight; the sums stay in ascending j
        const float4 v0 = g[i + (int64_t)j * NE4], v1 = g[i + (int64_t)(j + 1) * NE4];
        const float4 v2 = g[i + (int64_t)(j + 2) * NE4], v3 = g[i + (int64_t)(j + 3) * NE4];
        add(v0), add(v1), add(v2), add(v3);
    }
    for (; j < c; ++j) add(g[i + (int64_t)j * NE4]);
    acc[i] = a;
}

// grid (blocks per row, T * N); a thread owns positions 4q .. 4q + 3 of every channel of row (t, n)
template <int kMode>
__global__ void __launch_bounds__(kThreads) attr_finish_kernel(const float4* __restrict__ acc, const float4* __restrict__ x,
                                                               const float4* __restrict__ base, int base_n,
                                                               float4* __restrict__ attr, float4* __restrict__ maps,
                                                               double* __restrict__ partials, int N, int C, int HW4) {
    __shared__ double red[kWaves];
    const int tn = blockIdx.y, n = tn % N;
    const int q = blockIdx.x * kThreads + threadIdx.x;
    double s = 0.0;
    if (q < HW4) {
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ch = 0; ch < C; ++ch) {
            const int64_t o = ((int64_t)tn * C + ch) * HW4 + q;
            float4 a = acc[o];
            if (kMode == 0) {
                const int64_t xo = ((int64_t)n * C + ch) * HW4 + q;
                const float4 v = x[xo];
                const float4 b = base[base_n == 1 ? (int64_t)ch * HW4 + q : xo];
                a = make_float4(fmul(fsub(v.x, b.x), a.x), fmul(fsub(v.y, b.y), a.y),
                                fmul(fsub(v.z, b.z), a.z), fmul(fsub(v.w, b.w), a.w));
            }
            attr[o] = a;
            m.x = fadd(m.x, fabsf(a.x)), m.y = fadd(m.y, fabsf(a.y));
            m.z = fadd(m.z, fabsf(a.z)), m.w = fadd(m.w, fabsf(a.w));
            s = (((s + (double)a.x) + (double)a.y) + (double)a.z) + (double)a.w;
        }
        maps[(int64_t)tn * HW4 + q] = m;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);  // every lane ends with the same sum (a + b == b + a)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
#pragma unroll
        for (int i = 1; i < kWaves; ++i) t += red[i];
        partials[(int64_t)tn * gridDim.x + blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kThreads) attr_sums_kernel(const double* __restrict__ partials, double* __restrict__ sums,
                                                             int TN, int blocks) {
    const int tn = blockIdx.x * kThreads + threadIdx.x;
    if (tn >= TN) return;
    const double* p = partials + (int64_t)tn * blocks;
    double t = p[0];
    int b = 1;
    for (; b + 8 <= blocks; b += 8) {  // eight loads in flight; the sum stays in index order
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[b + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) t += v[i];
    }
    for (; b < blocks; ++b) t += p[b];
    sums[tn] = t;
}

inline bool misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}

}  // namespace

extern "C" int sm3_attr_path(const float* x, const float* base, int base_n, float* out, int N, int64_t E, int k0, int c,
                             int steps, void* stream) {
    if (!x || !base || !out || N < 1 || E < 1 || c < 1 || steps < 1 || k0 < 0 || (base_n != 1 && base_n != N))
        return SM3_EINVAL;
    if (steps > (1 << 23) || (int64_t)k0 + c > steps) return SM3_EINVAL;  // 2k + 1 and 2 * steps exact in f32
    if (E > kMax31 * 4 || (int64_t)N * (E / 4 + 1) > kMax31 || (int64_t)c * N * (E / 4 + 1) > kMax31 * kThreads)
        return SM3_EINVAL;
    if (E % 4 || misaligned(x, base, out)) return SM3_EALIGN;
    const int64_t E4 = E / 4, NE4 = N * E4;
    const dim3 grid((uint32_t)((NE4 * c + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(attr_path_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<const float4*>(base), base_n, reinterpret_cast<float4*>(out), NE4, E4, k0, c, steps);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_attr_noise(const float* x, const float* sigma, float* out, int N, int64_t E, int k0, int c, int stride,
                              uint64_t seed, void* stream) {
    if (!x || !sigma || !out || N < 1 || E < 1 || c < 1 || k0 < 0 || stride < 1) return SM3_EINVAL;
    if ((int64_t)k0 + (int64_t)(c - 1) * stride > kMax31) return SM3_EINVAL;
    if (E > kMax31 * 4 || (int64_t)N * (E / 4 + 1) > kMax31 || (int64_t)c * N * (E / 4 + 1) > kMax31 * kThreads)
        return SM3_EINVAL;
    if (E % 4 || misaligned(x, out)) return SM3_EALIGN;
    const int64_t E4 = E / 4, NE4 = N * E4;
    const dim3 grid((uint32_t)((NE4 * c + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(attr_noise_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x),
                       sigma, reinterpret_cast<float4*>(out), NE4, E4, k0, c, stride, (uint32_t)seed, (uint32_t)(seed >> 32));
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_attr_accumulate(const float* g, float* acc, int c, int N, int64_t E, float weight, int squared,
                                   void* stream) {
    if (!g || !acc || c < 1 || N < 1 || E < 1 || (squared != 0 && squared != 1)) return SM3_EINVAL;
    if (E > kMax31 * 4 || (int64_t)N * (E / 4 + 1) > kMax31 || (int64_t)c * N * (E / 4 + 1) > kMax31 * kThreads)
        return SM3_EINVAL;
    if (E % 4 || misaligned(g, acc)) return SM3_EALIGN;
    const int64_t NE4 = N * (E / 4);
    const dim3 grid((uint32_t)((NE4 + kThreads - 1) / kThreads));
    if (squared)
        hipLaunchKernelGGL(attr_accumulate_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(acc), c, NE4, weight);
    else
        hipLaunchKernelGGL(attr_accumulate_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(acc), c, NE4, weight);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_attr_finish_blocks(int HW) { return HW < 1 ? SM3_EINVAL : (int)(((int64_t)HW / 4 + kThreads - 1) / kThreads); }

extern "C" int sm3_attr_finish(const float* acc, const float* x, const float* base, int base_n, float* attr, float* maps,
                               double* sums, double* partials, int T, int N, int C, int HW, int mode, void* stream) {
    if (!acc || !attr || !maps || !sums || !partials || T < 1 || N < 1 || C < 1 || HW < 1 || (mode != 0 && mode != 1))
        return SM3_EINVAL;
    if (mode == 0 && (!x || !base || (base_n != 1 && base_n != N))) return SM3_EINVAL;
    if ((int64_t)T * N > 65535 || (int64_t)T * N * C * (HW / 4 + 1) > kMax31 * kThreads) return SM3_EINVAL;
    if (HW % 4 || misaligned(acc, attr, maps) || (mode == 0 && misaligned(x, base)) ||
        ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(partials)) & 7))
        return SM3_EALIGN;
    const int HW4 = HW / 4, blocks = sm3_attr_finish_blocks(HW), TN = T * N;
    const dim3 grid((uint32_t)blocks, (uint32_t)TN);
#define ATTR_FINISH(M)                                                                                                     \
    hipLaunchKernelGGL(attr_finish_kernel<M>, grid, dim3(kThreads), 0, (hipStream_t)stream,                                \
                       reinterpret_cast<const float4*>(acc), reinterpret_cast<const float4*>(x),                           \
                       reinterpret_cast<const float4*>(base), base_n, reinterpret_cast<float4*>(attr),                     \
                       reinterpret_cast<float4*>(maps), partials, N, C, HW4)
    if (mode == 0)
        ATTR_FINISH(0);
    else
        ATTR_FINISH(1);
#undef ATTR_FINISH
    SM3_CHECK_LAUNCH();
    hipLaunchKernelGGL(attr_sums_kernel, dim3((uint32_t)((TN + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, partials, sums, TN, blocks);
    SM3_CHECK_LAUNCH();
    return 0;
}
