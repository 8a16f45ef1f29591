// RISE black-box saliency (Petsiuk, Das, Saenko: Randomized Input Sampling for Explanation of Black-box Models, BMVC 2018):
// the three steps around the encoders' eval-mode forward (sm3hip/rise.py).  Mask i of modality m is the paper's "s x s binary
// grid, upsampled bilinearly to (s + 1) cells, cropped at a random shift", in integers: with cells ch = ceil(H / s), cw =
// ceil(W / s) and a corner grid of G x G bits, G = s + 2,
//
//     mask_i[y][x] = (float)A / (float)(ch * cw),   Y = y + oy, X = x + ox, gy = Y / ch, ry = Y % ch, gx = X / cw, rx = X % cw,
//     A = (ch - ry) (cw - rx) g[gy][gx] + (ch - ry) rx g[gy][gx + 1] + ry (cw - rx) g[gy + 1][gx] + ry rx g[gy + 1][gx + 1]
//
// -- one correctly rounded f32 division of two integers below 2^24.  A mask is never stored: the two streaming kernels
// regenerate its values from a 144-byte table row.
//
//   sm3_rise_table:      row j (kRow = 36 words) of mask i = i0 + j: words 0 .. 31 the grid bits (bit gy * G + gx of the row,
//                        little-endian in the words), word 32 oy, word 33 ox, words 34 and 35 zero.  Philox4x32-10 as attr.hip
//                        has it, key = the 64-bit seed (low word first), counter (q, i, m, 1): grid bit 4q + l = word l of call
//                        q < thr, thr = floor(p * 2^32); call ceil(G * G / 4) gives oy = (w0 * ch) >> 32, ox = (w1 * cw) >> 32.
//                        A function of (seed, m, i, H, W, s, p) alone.
//   sm3_rise_compose:    out[j][n][ch][p] = fadd(b, fmul(mask_j[p], fsub(x, b))): three separately rounded f32 operations, the
//                        three channels of a pixel with the pixel's mask value.  One thread owns 4 consecutive flat pixels of
//                        one image and a group of kGroup masks: x and base are read once per channel and group, the 4 mask
//                        values once per mask; 16-byte non-temporal stores.
//   sm3_rise_accumulate: maps[n][t][p] = (((0 + w[0][r] * mask_0[p]) + w[1][r] * mask_1[p]) + ...) / d, r = n * T + t, ascending
//                        i over ALL M masks in one launch, every product and sum rounded on its own, d = (float)(M * p).  A
//                        thread owns 4 pixels x a tile of kRowTile rows; the accumulators never leave registers, the weights of a mask
//                        are the same for the whole wave (scalar operands), a chunk of table rows is staged in LDS.
// y / ch and y % ch are fixed per pixel; the shift adds at most one carry, so no kernel divides per mask.  No atomics.
#include "exact_f32.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;    // table, compose
constexpr int kAccThreads = 64;  // accumulate: one wave per workgroup, the problem has few pixels (12 544 quads at 224^2)
constexpr int kRow = 36;         // words per table row
constexpr int kGroup = 8;        // masks per compose thread
#ifndef SM3_RISE_ROW_TILE
#define SM3_RISE_ROW_TILE 8
#endif
constexpr int kRowTile = SM3_RISE_ROW_TILE;  // rows per accumulation thread (-DSM3_RISE_ROW_TILE=4 / 16: the variants of DESIGN.md 8.5)
constexpr int kChunk = 32;       // table rows staged in LDS at a time by the accumulation
constexpr int kMaxMasks = 1 << 20;
constexpr int kMaxCompose = kGroup * 65535;  // masks per compose launch: the groups are one grid axis
constexpr int kMaxHW = 1 << 24;  // A <= ch * cw <= H * W: exact in f32

// one thread per table word
__global__ void __launch_bounds__(kThreads) rise_table_kernel(uint32_t* __restrict__ table, int i0, int c, uint32_t m, int G,
                                                              int ch, int cw, uint32_t thr, uint32_t key0, uint32_t key1) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= c * kRow) return;
    const int j = t / kRow, word = t - j * kRow;
    const uint32_t i = (uint32_t)(i0 + j);
    const int GG = G * G;
    uint32_t v = 0u, w[4];
    if (word < 32) {
#pragma unroll 1
        for (int k = 0; k < 8; ++k) {
            const int q = 8 * word + k;
            if (4 * q >= GG) break;
            philox4x32_10((uint32_t)q, i, m, 1u, key0, key1, w);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (4 * q + l < GG && w[l] < thr) v |= 1u << (4 * k + l);
        }
    } else if (word < 34) {
        philox4x32_10((uint32_t)((GG + 3) / 4), i, m, 1u, key0, key1, w);
        v = word == 32 ? (uint32_t)(((uint64_t)w[0] * (uint32_t)ch) >> 32) : (uint32_t)(((uint64_t)w[1] * (uint32_t)cw) >> 32);
    }
    table[t] = v;
}

// what a pixel keeps for all masks: its cell and its place inside the cell
struct Pixel {
    int cy, ry, cx, rx;
};

__device__ __forceinline__ Pixel pixel_at(int p, int W, int ch, int cw) {
    const int y = p / W, x = p - y * W;
    Pixel px;
    px.cy = y / ch, px.ry = y - px.cy * ch;
    px.cx = x / cw, px.rx = x - px.cx * cw;
    return px;
}

// bits j and j + 1 of a table row (j + 1 < G * G <= 1024).  The word index is clamped: a table that sm3_rise_table did not
// write cannot make a read leave the row.
__device__ __forceinline__ uint32_t two_bits(const uint32_t* row, int j) {
    const int k = min(max(j >> 5, 0), 31);
    const uint64_t w = (uint64_t)row[k] | ((uint64_t)row[k + 1] << 32);
    return (uint32_t)(w >> (j & 31)) & 3u;
}

__device__ __forceinline__ float mask_value(const uint32_t* row, const Pixel& px, int oy, int ox, int G, int ch, int cw,
                                            float D) {
    int Y = px.ry + oy, gy = px.cy;
    if (Y >= ch) Y -= ch, ++gy;
    int X = px.rx + ox, gx = px.cx;
    if (X >= cw) X -= cw, ++gx;
    const int j = gy * G + gx;
    const uint32_t top = two_bits(row, j), bot = two_bits(row, j + G);
    const int a = (cw - X) * (int)(top & 1u) + X * (int)(top >> 1);
    const int b = (cw - X) * (int)(bot & 1u) + X * (int)(bot >> 1);
    return (float)((ch - Y) * a + Y * b) / D;
}

// grid (ceil(HW4 / kThreads), N, ceil(c / kGroup)); table: the rows of the c masks
__global__ void __launch_bounds__(kThreads) rise_compose_kernel(const uint4* __restrict__ x, const uint4* __restrict__ base,
                                                                int base_n, const uint32_t* __restrict__ table,
                                                                uint4* __restrict__ out, int N, int HW4, int W, int G, int ch,
                                                                int cw, float D, int c) {
    __shared__ uint32_t rows[kGroup * kRow];
    const int j0 = blockIdx.z * kGroup, nj = min(kGroup, c - j0);
    for (int k = threadIdx.x; k < nj * kRow; k += kThreads) rows[k] = table[(int64_t)j0 * kRow + k];
    __syncthreads();
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= HW4) return;
    const int n = blockIdx.y;
    Pixel px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = pixel_at(4 * q + e, W, ch, cw);
    uint4 xv[3], bv[3];
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
        xv[cc] = x[((int64_t)n * 3 + cc) * HW4 + q];
        bv[cc] = base[((int64_t)(base_n == 1 ? 0 : n) * 3 + cc) * HW4 + q];
    }
    for (int jj = 0; jj < nj; ++jj) {
        const uint32_t* row = rows + jj * kRow;
        const int oy = (int)min(row[32], (uint32_t)(ch - 1)), ox = (int)min(row[33], (uint32_t)(cw - 1));
        float mv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) mv[e] = mask_value(row, px[e], oy, ox, G, ch, cw, D);
        uint4* o = out + ((int64_t)(j0 + jj) * N + n) * 3 * HW4 + q;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            const float r0 = blend(__uint_as_float(xv[cc].x), __uint_as_float(bv[cc].x), mv[0]);
            const float r1 = blend(__uint_as_float(xv[cc].y), __uint_as_float(bv[cc].y), mv[1]);
            const float r2 = blend(__uint_as_float(xv[cc].z), __uint_as_float(bv[cc].z), mv[2]);
            const float r3 = blend(__uint_as_float(xv[cc].w), __uint_as_float(bv[cc].w), mv[3]);
            stg16<true>(o + (int64_t)cc * HW4,
                        make_uint4(__float_as_uint(r0), __float_as_uint(r1), __float_as_uint(r2), __float_as_uint(r3)));
        }
    }
}

// One tile of rows over all M masks.  kFull: every row of the tile exists, so a mask's kRT weights are one unconditional
// wave-uniform load (scalar registers); the last tile of a row count that kRT does not divide takes them one by one.
template <int kRT, bool kFull>
__device__ __forceinline__ void accumulate_tile(const uint32_t* __restrict__ table, const float* __restrict__ weights,
                                                uint32_t* rows, const Pixel (&px)[4], float (&acc)[kRT][4], int r0, int R, int M,
                                                int G, int ch, int cw, float D) {
    for (int i0 = 0; i0 < M; i0 += kChunk) {
        const int ni = min(kChunk, M - i0);
        __syncthreads();
        for (int k = threadIdx.x; k < ni * kRow; k += kAccThreads) rows[k] = table[(int64_t)i0 * kRow + k];
        __syncthreads();
        for (int ii = 0; ii < ni; ++ii) {
            const float* wi = weights + (int64_t)(i0 + ii) * R + r0;
            float wk[kRT];
#pragma unroll
            for (int k = 0; k < kRT; ++k) wk[k] = (kFull || r0 + k < R) ? wi[k] : 0.f;
            const uint32_t* row = rows + ii * kRow;
            const int oy = (int)min(row[32], (uint32_t)(ch - 1)), ox = (int)min(row[33], (uint32_t)(cw - 1));
            float mv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) mv[e] = mask_value(row, px[e], oy, ox, G, ch, cw, D);
#pragma unroll
            for (int k = 0; k < kRT; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[k][e] = fadd(acc[k][e], fmul(wk[k], mv[e]));
        }
    }
}

// grid (ceil(HW4 / kAccThreads), ceil(R / kRT)); rows r = n * T + t, weights [M][R]
template <int kRT>
__global__ void __launch_bounds__(kAccThreads) rise_accumulate_kernel(const uint32_t* __restrict__ table,
                                                                      const float* __restrict__ weights,
                                                                      float* __restrict__ maps, int64_t stride_n,
                                                                      int64_t stride_t, int T, int R, int M, int HW4, int W,
                                                                      int G, int ch, int cw, float D, float d) {
    __shared__ uint32_t rows[kChunk * kRow];
    const int q = blockIdx.x * kAccThreads + threadIdx.x;
    const bool active = q < HW4;
    const int r0 = blockIdx.y * kRT;  // the same for the whole workgroup
    Pixel px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = pixel_at(active ? 4 * q + e : 0, W, ch, cw);
    float acc[kRT][4];
#pragma unroll
    for (int k = 0; k < kRT; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.f;
    if (r0 + kRT <= R)
        accumulate_tile<kRT, true>(table, weights, rows, px, acc, r0, R, M, G, ch, cw, D);
    else
        accumulate_tile<kRT, false>(table, weights, rows, px, acc, r0, R, M, G, ch, cw, D);
    if (!active) return;
#pragma unroll
    for (int k = 0; k < kRT; ++k) {
        const int r = r0 + k;
        if (r >= R) break;
        const int n = r / T, t = r - n * T;
        float4* o = reinterpret_cast<float4*>(maps + n * stride_n + t * stride_t + 4 * (int64_t)q);
        *o = make_float4(acc[k][0] / d, acc[k][1] / d, acc[k][2] / d, acc[k][3] / d);
    }
}

inline bool misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}

// the image and the grid: 1 <= s <= min(H, W, 30), H * W <= 2^24
inline bool bad_geometry(int H, int W, int s) {
    return H < 1 || W < 1 || (int64_t)H * W > kMaxHW || s < 1 || s > 30 || s > H || s > W;
}

}  // namespace

extern "C" int sm3_rise_table(uint32_t* table, int i0, int c, int modality, int H, int W, int s, double p, uint64_t seed,
                              void* stream) {
    if (!table || i0 < 0 || c < 1 || (int64_t)i0 + c > kMaxMasks || (modality != 0 && modality != 1) || bad_geometry(H, W, s))
        return SM3_EINVAL;
    if (!(p > 0.0 && p < 1.0)) return SM3_EINVAL;
    const uint32_t thr = (uint32_t)(p * 4294967296.0);  // floor: p * 2^32 is exact and below 2^32
    if (thr == 0u) return SM3_EINVAL;
    if (misaligned(table)) return SM3_EALIGN;
    const int ch = (H + s - 1) / s, cw = (W + s - 1) / s;
    const dim3 grid((uint32_t)(((int64_t)c * kRow + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(rise_table_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, table, i0, c, (uint32_t)modality, s + 2,
                       ch, cw, thr, (uint32_t)seed, (uint32_t)(seed >> 32));
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_rise_compose(const float* x, const float* base, int base_n, const uint32_t* table, float* out, int N, int H,
                                int W, int s, int c, void* stream) {
    if (!x || !base || !table || !out || N < 1 || N > 65535 || c < 1 || c > kMaxCompose || (base_n != 1 && base_n != N) ||
        bad_geometry(H, W, s))
        return SM3_EINVAL;
    const int HW = H * W;
    if (HW % 4 || misaligned(x, base, table, out)) return SM3_EALIGN;
    const int HW4 = HW / 4, ch = (H + s - 1) / s, cw = (W + s - 1) / s;
    const dim3 grid((uint32_t)((HW4 + kThreads - 1) / kThreads), (uint32_t)N, (uint32_t)((c + kGroup - 1) / kGroup));
    hipLaunchKernelGGL(rise_compose_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(x),
                       reinterpret_cast<const uint4*>(base), base_n, table, reinterpret_cast<uint4*>(out), N, HW4, W, s + 2, ch,
                       cw, (float)(ch * cw), c);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_rise_accumulate(const uint32_t* table, const float* weights, float* maps, int64_t stride_n, int64_t stride_t,
                                   int N, int T, int M, int H, int W, int s, double p, void* stream) {
    if (!table || !weights || !maps || N < 1 || T < 1 || M < 1 || M > kMaxMasks || stride_n < 0 || stride_t < 0 ||
        bad_geometry(H, W, s))
        return SM3_EINVAL;
    if (!(p > 0.0 && p < 1.0)) return SM3_EINVAL;
    const int64_t R = (int64_t)N * T;
    constexpr int rt = kRowTile;
    if ((R + rt - 1) / rt > 65535) return SM3_EINVAL;  // grid.y
    const int HW = H * W;
    if (HW % 4 || stride_n % 4 || stride_t % 4 || misaligned(table, maps) || (reinterpret_cast<uintptr_t>(weights) & 3))
        return SM3_EALIGN;
    const int HW4 = HW / 4, ch = (H + s - 1) / s, cw = (W + s - 1) / s;
    const float d = (float)((double)M * p);
    const dim3 grid((uint32_t)((HW4 + kAccThreads - 1) / kAccThreads), (uint32_t)((R + rt - 1) / rt));
    hipLaunchKernelGGL(rise_accumulate_kernel<kRowTile>, grid, dim3(kAccThreads), 0, (hipStream_t)stream, table, weights, maps,
                       stride_n, stride_t, T, (int)R, M, HW4, W, s + 2, ch, cw, (float)(ch * cw), d);
    SM3_CHECK_LAUNCH();
    return 0;
}
