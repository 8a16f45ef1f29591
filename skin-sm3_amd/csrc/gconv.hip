// Grouped 3 x 3 convolution (ResNeXt's conv2: reference src/models/resnet.py:142-146, conv3x3(width, width, stride, groups)),
// NHWC, pad 1, G groups of cg = C / G channels, in the three arithmetic modes (bf16 / f16 inputs with f32 accumulation, exact
// f32).  Forward with the BatchNorm statistic partials of sm3_conv_gather_gemm, data gradient (stride 1 and 2), weight gradient
// as fixed-order plain-store slabs + sm3_slab_reduce (no float atomics), and the filter-bank layout.
//
// Design: these layers move ~18 FLOP per byte at cg = 4 and a few hundred at cg = 64, so the kernels are
// direct VALU convolutions rather than MFMA tiles -- no block-diagonal padding of the group's K to the 32-wide MFMA operand.  One
// lane owns one output channel; a wave covers 64 consecutive channels, so the activation vector of a group (cg contiguous
// channels of one pixel) is a broadcast load and the filter banks are laid out channel-fastest ([tap][k][C]) so that every
// weight load of a wave is one coalesced 128- (16-bit) or 256-byte (f32) line.  Each weight load is reused for kRU output
// rows.  Every sum has a fixed order (tap-major, then channel), so each launch is a function of its inputs.
#include "common.h"

namespace {

constexpr int kStatRows = 128;  // rows per BatchNorm partial row: sm3_conv_partial_rows
constexpr int kRU = 4;          // output rows per pass over the filter taps
constexpr int kDgradRows = 16;  // input pixels per data-gradient workgroup

template <typename T>
__device__ __forceinline__ void load4(const T* p, float* f);
template <>
__device__ __forceinline__ void load4<float>(const float* p, float* f) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}
template <>
__device__ __forceinline__ void load4<bf16_t>(const bf16_t* p, float* f) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    f[0] = bf16_to_f32((uint16_t)(v.x & 0xffffu)); f[1] = bf16_to_f32((uint16_t)(v.x >> 16));
    f[2] = bf16_to_f32((uint16_t)(v.y & 0xffffu)); f[3] = bf16_to_f32((uint16_t)(v.y >> 16));
}
template <>
__device__ __forceinline__ void load4<f16_t>(const f16_t* p, float* f) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    f[0] = f16_to_f32((uint16_t)(v.x & 0xffffu)); f[1] = f16_to_f32((uint16_t)(v.x >> 16));
    f[2] = f16_to_f32((uint16_t)(v.y & 0xffffu)); f[3] = f16_to_f32((uint16_t)(v.y >> 16));
}

template <typename T>
__device__ __forceinline__ void store1(T* p, float v);
template <>
__device__ __forceinline__ void store1<float>(float* p, float v) { *p = v; }
template <>
__device__ __forceinline__ void store1<bf16_t>(bf16_t* p, float v) { p->v = f32_to_bf16(v); }
template <>
__device__ __forceinline__ void store1<f16_t>(f16_t* p, float v) { p->v = f32_to_f16(v); }

// y[r][co] = sum_{tap, k < CG} x[pixel(r, tap)][g*CG + k] * w[co][tap][k], g = co / CG.  Workgroup: one wave, 64 channels x 128
// rows (one BatchNorm partial row: the sums of the ROUNDED outputs and of their squares, as the dense kernel's epilogue).
template <typename T, int CG>
__global__ __launch_bounds__(64) void gconv_fwd_kernel(const T* __restrict__ x, const T* __restrict__ wf, T* __restrict__ y,
                                                       float* __restrict__ part, int M, int H, int W, int Ho, int Wo, int C,
                                                       int s) {
    const int co = blockIdx.y * 64 + threadIdx.x;
    const int cbase = co / CG * CG;
    const long r0 = (long)blockIdx.x * kStatRows;
    const long rend = min((long)M, r0 + kStatRows);
    const int HoWo = Ho * Wo;
    float s1 = 0.f, s2 = 0.f;
    for (long r = r0; r < rend; r += kRU) {
        int n[kRU], oy[kRU], ox[kRU];
        bool ok[kRU];
#pragma unroll
        for (int u = 0; u < kRU; ++u) {
            ok[u] = r + u < rend;
            const int rr = (int)(ok[u] ? r + u : r);
            n[u] = rr / HoWo;
            const int rem = rr - n[u] * HoWo;
            oy[u] = rem / Wo;
            ox[u] = rem - oy[u] * Wo;
        }
        float acc[kRU];
#pragma unroll
        for (int u = 0; u < kRU; ++u) acc[u] = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            const T* xp[kRU];
            bool in[kRU];
#pragma unroll
            for (int u = 0; u < kRU; ++u) {
                const int iy = oy[u] * s - 1 + ky, ix = ox[u] * s - 1 + kx;
                in[u] = ok[u] && iy >= 0 && iy < H && ix >= 0 && ix < W;
                xp[u] = x + (((long)n[u] * H + (in[u] ? iy : 0)) * W + (in[u] ? ix : 0)) * C + cbase;
            }
            const T* wp = wf + (long)tap * CG * C + co;
#pragma unroll
            for (int k4 = 0; k4 < CG / 4; ++k4) {
                float wv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) wv[i] = ElemTraits<T>::load(wp + (long)(k4 * 4 + i) * C);
#pragma unroll
                for (int u = 0; u < kRU; ++u) {
                    if (in[u]) {
                        float xv[4];
                        load4<T>(xp[u] + k4 * 4, xv);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[u] = fmaf(xv[i], wv[i], acc[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kRU; ++u) {
            if (ok[u]) {
                const float v = ElemTraits<T>::round(acc[u]);
                store1<T>(y + (r + u) * C + co, v);
                s1 += v;
                s2 = fmaf(v, v, s2);
            }
        }
    }
    if (part) {
        part[((long)blockIdx.x * 2 + 0) * C + co] = s1;
        part[((long)blockIdx.x * 2 + 1) * C + co] = s2;
    }
}

// dx[p][ci] = sum_{tap, j < CG} dy[out(p, tap)][g*CG + j] * w[g*CG + j][tap][ci - g*CG], g = ci / CG, over the output pixels
// (oy, ox) with oy*s - 1 + ky = iy, ox*s - 1 + kx = ix (stride 2: the taps of the pixel's parity class only).
template <typename T, int CG>
__global__ __launch_bounds__(64) void gconv_dgrad_kernel(const T* __restrict__ dy, const T* __restrict__ wd, T* __restrict__ dx,
                                                         int Mi, int H, int W, int Ho, int Wo, int C, int s) {
    const int ci = blockIdx.y * 64 + threadIdx.x;
    const int cbase = ci / CG * CG;
    const long r0 = (long)blockIdx.x * kDgradRows;
    const long rend = min((long)Mi, r0 + kDgradRows);
    const int HW = H * W;
    for (long r = r0; r < rend; r += kRU) {
        int n[kRU], iy[kRU], ix[kRU];
        bool ok[kRU];
#pragma unroll
        for (int u = 0; u < kRU; ++u) {
            ok[u] = r + u < rend;
            const int rr = (int)(ok[u] ? r + u : r);
            n[u] = rr / HW;
            const int rem = rr - n[u] * HW;
            iy[u] = rem / W;
            ix[u] = rem - iy[u] * W;
        }
        float acc[kRU];
#pragma unroll
        for (int u = 0; u < kRU; ++u) acc[u] = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            const T* gp[kRU];
            bool in[kRU];
            bool any = false;
#pragma unroll
            for (int u = 0; u < kRU; ++u) {
                const int ty = iy[u] + 1 - ky, tx = ix[u] + 1 - kx;
                const int oy = ty / s, ox = tx / s;  // ty, tx >= 0 is checked first
                in[u] = ok[u] && ty >= 0 && tx >= 0 && oy * s == ty && ox * s == tx && oy < Ho && ox < Wo;
                gp[u] = dy + (((long)n[u] * Ho + (in[u] ? oy : 0)) * Wo + (in[u] ? ox : 0)) * C + cbase;
                any |= in[u];
            }
            if (!any) continue;  // uniform over the wave: every lane has the same pixels
            const T* wp = wd + (long)tap * CG * C + ci;
#pragma unroll
            for (int j4 = 0; j4 < CG / 4; ++j4) {
                float wv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) wv[i] = ElemTraits<T>::load(wp + (long)(j4 * 4 + i) * C);
#pragma unroll
                for (int u = 0; u < kRU; ++u) {
                    if (in[u]) {
                        float gv[4];
                        load4<T>(gp[u] + j4 * 4, gv);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[u] = fmaf(gv[i], wv[i], acc[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kRU; ++u)
            if (ok[u]) store1<T>(dx + (r + u) * C + ci, acc[u]);
    }
}

// Slab z of the weight gradient: slab[z][co][tap][k] = sum over the output rows [z*R, (z+1)*R) of dy[r][co] * x[pixel(r, tap)]
// [g*CG + k], rows in ascending order.  One lane per (co, tap) holds the CG sums of its group's input channels.
template <typename T, int CG>
__global__ __launch_bounds__(64) void gconv_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                         float* __restrict__ slabs, int M, int H, int W, int Ho, int Wo, int C,
                                                         int s, int R) {
    const int co = blockIdx.x * 64 + threadIdx.x;
    const int tap = blockIdx.y, ky = tap / 3, kx = tap - ky * 3;
    const int cbase = co / CG * CG;
    const long r0 = (long)blockIdx.z * R;
    const long rend = min((long)M, r0 + R);
    const int HoWo = Ho * Wo;
    float acc[CG];
#pragma unroll
    for (int k = 0; k < CG; ++k) acc[k] = 0.f;
    int n = (int)(r0 / HoWo);
    int rem = (int)(r0 - (long)n * HoWo);
    int oy = rem / Wo, ox = rem - oy * Wo;
    for (long r = r0; r < rend; ++r) {
        const int iy = oy * s - 1 + ky, ix = ox * s - 1 + kx;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {  // uniform over the wave
            const float g = ElemTraits<T>::load(dy + r * C + co);
            const T* xp = x + (((long)n * H + iy) * W + ix) * C + cbase;
#pragma unroll
            for (int k4 = 0; k4 < CG / 4; ++k4) {
                float xv[4];
                load4<T>(xp + k4 * 4, xv);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[k4 * 4 + i] = fmaf(g, xv[i], acc[k4 * 4 + i]);
            }
        }
        if (++ox == Wo) {
            ox = 0;
            if (++oy == Ho) { oy = 0; ++n; }
        }
    }
    float* out = slabs + (long)blockIdx.z * C * 9 * CG + ((long)co * 9 + tap) * CG;
#pragma unroll
    for (int k4 = 0; k4 < CG / 4; ++k4)
        *reinterpret_cast<float4*>(out + k4 * 4) = make_float4(acc[k4 * 4], acc[k4 * 4 + 1], acc[k4 * 4 + 2], acc[k4 * 4 + 3]);
}

// master [C][9][cg] fp32 (OHWI) -> forward bank wf[tap][k][co] and data-gradient bank wd[tap][j][g*cg + k] = w[g*cg + j][tap][k]
template <typename T>
__global__ __launch_bounds__(256) void gconv_weight_prep_kernel(const float* __restrict__ m, T* __restrict__ wf,
                                                                T* __restrict__ wd, int C, int cg, const int* __restrict__ only_if) {
    if (only_if && *only_if == 0) return;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * 9 * cg) return;
    const int k = (int)(e % cg);
    const int tap = (int)(e / cg % 9);
    const int co = (int)(e / (9L * cg));
    const float v = m[e];
    store1<T>(wf + ((long)tap * cg + k) * C + co, v);
    const int g = co / cg, j = co - g * cg;
    store1<T>(wd + ((long)tap * cg + j) * C + g * cg + k, v);
}

// host-side checks shared by every entry point: SM3_EINVAL / SM3_EALIGN / SM3_EDTYPE before any launch
int check_geom(int dtype, int N, int H, int W, int C, int groups, int stride) {
    if (!SM3_DTYPE_OK(dtype)) return SM3_EDTYPE;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || groups <= 0 || C % groups) return SM3_EINVAL;
    if (stride != 1 && stride != 2) return SM3_EINVAL;
    const int cg = C / groups;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) return SM3_EINVAL;
    if (C % 64) return SM3_EALIGN;
    if ((long)N * H * W * C >= (1L << 31)) return SM3_EINVAL;  // element offsets of one tensor stay below 2^31 ...
    return 0;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

#define SM3_GCONV_CG(cg, CALL)           \
    do {                                 \
        switch (cg) {                    \
            case 4: CALL(4); break;      \
            case 8: CALL(8); break;      \
            case 16: CALL(16); break;    \
            case 32: CALL(32); break;    \
            default: CALL(64); break;    \
        }                                \
    } while (0)

}  // namespace

extern "C" int sm3_gconv_weight_prep(int dtype, const float* master, void* w_fwd, void* w_dgrad, int C, int groups,
                                     const int* only_if, void* stream) {
    if (!master || !w_fwd || !w_dgrad) return SM3_EINVAL;
    const int rc = check_geom(dtype, 1, 1, 1, C, groups, 1);
    if (rc) return rc;
    const int cg = C / groups;
    const long n = (long)C * 9 * cg;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(T)                                                                                                   \
    hipLaunchKernelGGL(gconv_weight_prep_kernel<T>, dim3(blocks), dim3(256), 0, st, master, (T*)w_fwd, (T*)w_dgrad, C, \
                       cg, only_if)
    SM3_DISPATCH_DTYPE(dtype, LAUNCH);
#undef LAUNCH
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_gconv_fwd(int dtype, const void* x, const void* w_fwd, void* y, float* stat_partials, int N, int H, int W,
                             int C, int groups, int stride, void* stream) {
    if (!x || !w_fwd || !y) return SM3_EINVAL;
    const int rc = check_geom(dtype, N, H, W, C, groups, stride);
    if (rc) return rc;
    if (misaligned(x) || misaligned(y) || misaligned(w_fwd)) return SM3_EALIGN;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long M = (long)N * Ho * Wo;
    const int cg = C / groups;
    const dim3 grid((unsigned)((M + kStatRows - 1) / kStatRows), (unsigned)(C / 64));
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_CG(CG)                                                                                                        \
    hipLaunchKernelGGL((gconv_fwd_kernel<T_, CG>), grid, dim3(64), 0, st, (const T_*)x, (const T_*)w_fwd, (T_*)y, stat_partials, \
                       (int)M, H, W, Ho, Wo, C, stride)
#define LAUNCH(T)          \
    {                      \
        using T_ = T;      \
        SM3_GCONV_CG(cg, LAUNCH_CG); \
    }
    SM3_DISPATCH_DTYPE(dtype, LAUNCH);
#undef LAUNCH
#undef LAUNCH_CG
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_gconv_dgrad(int dtype, const void* dy, const void* w_dgrad, void* dx, int N, int H, int W, int C, int groups,
                               int stride, void* stream) {
    if (!dy || !w_dgrad || !dx) return SM3_EINVAL;
    const int rc = check_geom(dtype, N, H, W, C, groups, stride);
    if (rc) return rc;
    if (misaligned(dy) || misaligned(dx) || misaligned(w_dgrad)) return SM3_EALIGN;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long Mi = (long)N * H * W;
    const int cg = C / groups;
    const dim3 grid((unsigned)((Mi + kDgradRows - 1) / kDgradRows), (unsigned)(C / 64));
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_CG(CG)                                                                                                      \
    hipLaunchKernelGGL((gconv_dgrad_kernel<T_, CG>), grid, dim3(64), 0, st, (const T_*)dy, (const T_*)w_dgrad, (T_*)dx, \
                       (int)Mi, H, W, Ho, Wo, C, stride)
#define LAUNCH(T)          \
    {                      \
        using T_ = T;      \
        SM3_GCONV_CG(cg, LAUNCH_CG); \
    }
    SM3_DISPATCH_DTYPE(dtype, LAUNCH);
#undef LAUNCH
#undef LAUNCH_CG
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_gconv_wgrad_slabs(int N, int H, int W, int stride, int slab_capacity) {
    if (N <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2) || slab_capacity < 1) return SM3_EINVAL;
    const long M = (long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    long R = (M + slab_capacity - 1) / slab_capacity;
    if (R < 64) R = 64;
    return (int)((M + R - 1) / R);
}

extern "C" int sm3_gconv_wgrad_det(int dtype, const void* x, const void* dy, float* dw, float* slabs, int slab_capacity, int N,
                                   int H, int W, int C, int groups, int stride, void* stream) {
    if (!x || !dy || !dw || !slabs || slab_capacity < 1) return SM3_EINVAL;
    const int rc = check_geom(dtype, N, H, W, C, groups, stride);
    if (rc) return rc;
    if (misaligned(x) || misaligned(dy) || misaligned(dw) || misaligned(slabs)) return SM3_EALIGN;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long M = (long)N * Ho * Wo;
    const int nslabs = sm3_gconv_wgrad_slabs(N, H, W, stride, slab_capacity);
    const long R = (M + nslabs - 1) / nslabs;  // the partition sm3_gconv_wgrad_slabs counted: a function of M and the capacity
    const int cg = C / groups;
    const dim3 grid((unsigned)(C / 64), 9u, (unsigned)nslabs);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_CG(CG)                                                                                                        \
    hipLaunchKernelGGL((gconv_wgrad_kernel<T_, CG>), grid, dim3(64), 0, st, (const T_*)x, (const T_*)dy, slabs, (int)M, H, W, \
                       Ho, Wo, C, stride, (int)R)
#define LAUNCH(T)          \
    {                      \
        using T_ = T;      \
        SM3_GCONV_CG(cg, LAUNCH_CG); \
    }
    SM3_DISPATCH_DTYPE(dtype, LAUNCH);
#undef LAUNCH
#undef LAUNCH_CG
    SM3_CHECK_LAUNCH();
    return sm3_slab_reduce(slabs, nslabs, (int64_t)C * 9 * cg, dw, 1, stream);
}
