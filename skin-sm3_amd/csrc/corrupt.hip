// Image corruptions for the robustness report (sm3hip/corrupt.py, whose module text is the specification).  x, out: [B][3][H][W]
// f32 in [0, 1] -- the resampled image before Normalize.  Every output element is a function of (image, operation, parameter,
// seed, case id, modality) alone: nothing depends on the batch, the chunk or the position in a launch.
//
//   sm3_corrupt_pointwise: gaussian_noise, impulse_noise, colour_cast.  One thread owns four consecutive elements of one image's
//                          [3][H][W] row (one Philox4x32-10 call; the last thread of an image owns the 3 H W % 4 tail).  Element
//                          words: counter (e / 4, case, modality << 16 | code << 8 | severity, 7), word e % 4; case word:
//                          counter (0xFFFFFFFF, case, code << 8 | severity, 7), word 0; key = the seed, low word first.
//   sm3_corrupt_taps:      out = (sum of x at the table's (dy, dx) offsets, in table order, every add rounded) / count, with
//                          clamped coordinates.  A workgroup of 32 x 8 threads stages one 32 x 32 output tile plus a halo of 10 --
//                          52 x 52 source pixels, each read from HBM once per tile -- in LDS (row stride 53 dwords; the 32 lanes of
//                          a half-wave read 32 consecutive dwords for every tap, so no tap conflicts), then every thread walks the
//                          taps for its 4 pixels.  The tables travel in the kernel arguments, the cases' table numbers too, 64
//                          cases per launch, so every table read is wave-uniform.
//   sm3_corrupt_pixelate:  every pixel -> the mean of its f x f block (blocks anchored at (0, 0), row-major sum, one division by
//                          the number of in-image pixels).  A workgroup owns a tile of (32 / f) * f pixels a side: the tile is read
//                          once into LDS, one thread sums one block, every thread stores 4 pixels.
//   sm3_corrupt_jpeg:      a 4:4:4 baseline JPEG round trip in integers.  One wave owns one 8 x 8 block of the three channels, lane
//                          = pixel; the colour conversion, the two DCT passes, the quantisation and the way back pass through LDS
//                          only.  int32 where the bounds allow it (the first DCT pass: 8 * 4017 * 128 < 2^22), int64 elsewhere
//                          (second pass < 2^37, the inverse < 2^42).
// No atomics: every output is written once by a fixed order of operations on its own inputs.
#include "exact_f32.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMax31 = 0x7fffffffLL;
constexpr int kOpGaussian = 0, kOpImpulse = 1, kOpCast = 10;  // corrupt.CORRUPTIONS' codes
constexpr uint32_t kStream = 7u;                              // the last counter word (resample.philox_words lists them)

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// i = n * E4c + e4: thread e4 of image n owns elements 4 e4 .. 4 e4 + 3 (fewer at the tail)
__global__ void __launch_bounds__(kThreads) corrupt_pointwise_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                     const int32_t* __restrict__ ids, int64_t E, int64_t E4c,
                                                                     int64_t total, int HW, int op, float fparam, uint32_t T,
                                                                     uint32_t c2, uint32_t key0, uint32_t key1, int vec) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t n = i / E4c;
    const uint32_t e4 = (uint32_t)(i - n * E4c);
    const int64_t e0 = 4 * (int64_t)e4;
    const int cnt = (int)(E - e0 < 4 ? E - e0 : 4);
    const uint32_t id = (uint32_t)ids[n];
    const float* src = x + n * E + e0;
    float* dst = out + n * E + e0;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        for (int k = 0; k < cnt; ++k) v[k] = src[k];
    }
    uint32_t w[4];
    if (op == kOpCast) {
        philox4x32_10(0xFFFFFFFFu, id, c2 & 0xFFFFu, kStream, key0, key1, w);
        const bool cool = w[0] & 1u;
        const float hi = fadd(1.f, fparam), lo = fsub(1.f, fparam);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ch = (int)((e0 + k) / HW);
            const float g = ch == 1 ? 1.f : ((ch == 0) != cool ? hi : lo);
            v[k] = clamp01(fmul(v[k], g));
        }
    } else {
        philox4x32_10(e4, id, c2, kStream, key0, key1, w);
        if (op == kOpGaussian) {
            float z[4];
            box_muller(w[0], w[1], z[0], z[1]);
            box_muller(w[2], w[3], z[2], z[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = clamp01(fadd(v[k], fmul(fparam, z[k])));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = w[k] < T ? 0.f : ((uint64_t)w[k] + T >= 0x100000000ull ? 1.f : v[k]);
        }
    }
    if (vec) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < cnt; ++k) dst[k] = v[k];
    }
}

// ---- blur by tap tables ---------------------------------------------------------------------------------------------------
constexpr int kTile = 32, kRows = 8;             // 32 x 8 threads, 4 tile rows per thread
constexpr int kHalo = 10;                        // the largest offset of any table
constexpr int kSide = kTile + 2 * kHalo;         // 52
constexpr int kStride = kSide + 1;               // 53 dwords
constexpr int kTapStore = 336;                   // taps of all tables of a call (the disk of radius 10 has 317, 8 lines of 21: 168)
constexpr int kMaxTables = 8;
constexpr int kCaseChunk = 64;                   // cases per launch

struct TapArgs {
    int16_t dy[kTapStore], dx[kTapStore];
    int32_t first[kMaxTables], count[kMaxTables];
    uint8_t table_of[kCaseChunk];
};

// grid (3 * tiles_y * tiles_x, cases of the chunk)
__global__ void __launch_bounds__(kTile* kRows) corrupt_taps_kernel(const float* __restrict__ x, float* __restrict__ out, int H,
                                                                     int W, int tiles_x, int tiles_y, TapArgs a) {
    __shared__ float tile[kSide * kStride];
    const int j = threadIdx.x, i0 = threadIdx.y;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    const int ch = b / tiles_y;
    const int y0 = ty * kTile, x0 = tx * kTile;
    const int64_t plane = ((int64_t)blockIdx.y * 3 + ch) * H * W;
    const float* src = x + plane;
    for (int p = i0 * kTile + j; p < kSide * kSide; p += kTile * kRows) {
        const int r = p / kSide, c = p - r * kSide;
        const int gy = min(max(y0 - kHalo + r, 0), H - 1), gx = min(max(x0 - kHalo + c, 0), W - 1);
        tile[r * kStride + c] = src[(int64_t)gy * W + gx];
    }
    __syncthreads();
    const int tb = a.table_of[blockIdx.y];
    const int t0 = a.first[tb], n = a.count[tb];
    float acc[kTile / kRows];
#pragma unroll
    for (int k = 0; k < kTile / kRows; ++k) acc[k] = 0.f;
    for (int t = 0; t < n; ++t) {
        const int o = (i0 + kHalo + a.dy[t0 + t]) * kStride + j + kHalo + a.dx[t0 + t];
#pragma unroll
        for (int k = 0; k < kTile / kRows; ++k) acc[k] = fadd(acc[k], tile[o + kRows * k * kStride]);
    }
    const float cnt = (float)n;
    if (x0 + j < W) {
#pragma unroll
        for (int k = 0; k < kTile / kRows; ++k) {
            const int y = y0 + i0 + kRows * k;
            if (y < H) out[plane + (int64_t)y * W + x0 + j] = acc[k] / cnt;
        }
    }
}

// ---- pixelate -------------------------------------------------------------------------------------------------------------
constexpr int kMaxF = 32;

// grid (3 * tiles_y * tiles_x, B); tiles of S = (32 / f) * f pixels a side, so that no block straddles two tiles
__global__ void __launch_bounds__(kTile* kRows) corrupt_pixelate_kernel(const float* __restrict__ x, float* __restrict__ out, int H,
                                                                         int W, int tiles_x, int tiles_y, int f, int S) {
    __shared__ float tile[kTile][kTile + 1];
    __shared__ float means[kTile * kTile];
    const int j = threadIdx.x, i0 = threadIdx.y;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    const int ch = b / tiles_y;
    const int y0 = ty * S, x0 = tx * S;
    const int th = min(S, H - y0), tw = min(S, W - x0);
    const int64_t plane = ((int64_t)blockIdx.y * 3 + ch) * H * W;
#pragma unroll
    for (int k = 0; k < kTile / kRows; ++k) {
        const int i = i0 + kRows * k;
        if (i < th && j < tw) tile[i][j] = x[plane + (int64_t)(y0 + i) * W + x0 + j];
    }
    __syncthreads();
    const int nb = S / f;
    for (int q = i0 * kTile + j; q < nb * nb; q += kTile * kRows) {
        const int by = q / nb, bx = q - by * nb;
        const int r0 = by * f, c0 = bx * f;
        const int r1 = min(r0 + f, th), c1 = min(c0 + f, tw);
        if (r0 < th && c0 < tw) {
            float acc = 0.f;
            for (int r = r0; r < r1; ++r)
                for (int c = c0; c < c1; ++c) acc = fadd(acc, tile[r][c]);
            means[q] = acc / (float)((r1 - r0) * (c1 - c0));
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTile / kRows; ++k) {
        const int i = i0 + kRows * k;
        if (i < th && j < tw) out[plane + (int64_t)(y0 + i) * W + x0 + j] = means[(i / f) * nb + j / f];
    }
}

// ---- JPEG -----------------------------------------------------------------------------------------------------------------
// C13[k][n] = rint(2^13 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = sqrt(2/8)
__constant__ int32_t kC13[64] = {
    2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,   //
    4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,  //
    3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,   //
    3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,  //
    2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,   //
    2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,  //
    1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,   //
    799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};

struct JpegArgs {
    uint8_t qt[2][64];  // luminance, chrominance; [vertical frequency][horizontal frequency]
};

constexpr int kJpegWaves = kThreads / 64;

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// grid ceil(blocks / 4): wave w of a workgroup owns 8 x 8 block 4 * blockIdx.x + w of B * blocks_y * blocks_x; lane = 8 r + c
__global__ void __launch_bounds__(kThreads) corrupt_jpeg_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W,
                                                                int blocks_x, int blocks_y, int64_t n_blocks, JpegArgs a) {
    __shared__ int32_t sA[kJpegWaves][3][64];
    __shared__ int32_t sB[kJpegWaves][3][64];
    __shared__ int64_t sV[kJpegWaves][3][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane >> 3, c = lane & 7;
    int64_t blk = (int64_t)blockIdx.x * kJpegWaves + wv;
    const bool live = blk < n_blocks;
    if (!live) blk = n_blocks - 1;  // an idle wave repeats the last block and stores nothing: every wave reaches the barriers
    const int bx = (int)(blk % blocks_x);
    const int by = (int)((blk / blocks_x) % blocks_y);
    const int64_t n = blk / ((int64_t)blocks_x * blocks_y);
    const int py = by * 8 + r, px = bx * 8 + c;
    const int64_t HW = (int64_t)H * W;
    const int64_t at = n * 3 * HW + (int64_t)min(py, H - 1) * W + min(px, W - 1);  // the image replicated up to multiples of 8
    int q[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) q[ch] = clamp255((int)rintf(fmul(x[at + ch * HW], 255.f)));
    const int R = q[0], G = q[1], B = q[2];
    sA[wv][0][lane] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
    sA[wv][1][lane] = ((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128;
    sA[wv][2][lane] = ((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128;
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {  // T[r][c] = sum_m C13[r][m] X[m][c]
        int32_t t = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) t += kC13[r * 8 + m] * sA[wv][ch][m * 8 + c];
        sB[wv][ch][lane] = t;
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {  // F[r][c] = sum_n T[r][n] C13[c][n], quantised and scaled back
        int64_t F = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) F += (int64_t)sB[wv][ch][r * 8 + m] * kC13[c * 8 + m];
        const int32_t t = a.qt[ch ? 1 : 0][lane];
        // (2 |F| + d) // (2 d), d = t << 26: the floor of a floor, (2 |F| + d) >> 27 first (below 2^12), then // t
        const int64_t mag = F < 0 ? -F : F;
        const int32_t qv = (int32_t)((2 * mag + ((int64_t)t << 26)) >> 27) / t;
        sA[wv][ch][lane] = (F < 0 ? -qv : qv) * t;
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {  // V[r][c] = sum_l D[r][l] C13[l][c]
        int64_t v = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) v += (int64_t)sA[wv][ch][r * 8 + m] * kC13[m * 8 + c];
        sV[wv][ch][lane] = v;
    }
    __syncthreads();
    int p[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {  // y[r][c] = sum_k C13[k][r] V[k][c]
        int64_t y = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) y += (int64_t)kC13[m * 8 + r] * sV[wv][ch][m * 8 + c];
        p[ch] = clamp255((int)((y + (1ll << 25)) >> 26) + 128);
    }
    const int Y = p[0], cb = p[1] - 128, cr = p[2] - 128;
    const int o[3] = {clamp255(Y + ((91881 * cr + 32768) >> 16)), clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)),
                      clamp255(Y + ((116130 * cb + 32768) >> 16))};
    if (live && py < H && px < W) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[at + ch * HW] = (float)o[ch] / 255.f;
    }
}

inline bool bad_image(const void* x, const void* out, int B, int H, int W) {
    return !x || !out || B < 1 || H < 1 || W < 1 || (int64_t)3 * H * W > kMax31 || (int64_t)B * 3 * H * W > kMax31 * 64;
}

}  // namespace

extern "C" int sm3_corrupt_pointwise(const float* x, int B, int H, int W, const int32_t* ids, int op, int severity, double param,
                                     uint64_t seed, int modality, float* out, void* stream) {
    if (bad_image(x, out, B, H, W) || !ids || severity < 1 || severity > 5 || (modality != 0 && modality != 1)) return SM3_EINVAL;
    if (op != kOpGaussian && op != kOpImpulse && op != kOpCast) return SM3_EINVAL;
    if (!(param >= 0.0) || param > (op == kOpImpulse ? 2147483648.0 : 1.0)) return SM3_EINVAL;  // sigma, T = int(p 2^31), c
    if (op == kOpImpulse && param != (double)(uint32_t)param) return SM3_EINVAL;
    const int64_t E = (int64_t)3 * H * W, E4c = (E + 3) / 4, total = B * E4c;
    const int vec = E % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const uint32_t c2 = (uint32_t)modality << 16 | (uint32_t)op << 8 | (uint32_t)severity;
    hipLaunchKernelGGL(corrupt_pointwise_kernel, dim3((uint32_t)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, x, out, ids, E, E4c, total, H * W, op, op == kOpImpulse ? 0.f : (float)param,
                       op == kOpImpulse ? (uint32_t)param : 0u, c2, (uint32_t)seed, (uint32_t)(seed >> 32), vec);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_corrupt_taps(const float* x, int B, int H, int W, const int16_t* tables, const int32_t* counts, int n_tables,
                                int max_taps, const int32_t* table_index, float* out, void* stream) {
    if (bad_image(x, out, B, H, W) || !tables || !counts || !table_index || n_tables < 1 || n_tables > kMaxTables || max_taps < 1 ||
        max_taps > kTapStore)
        return SM3_EINVAL;
    TapArgs a = {};
    int total = 0;
    for (int t = 0; t < n_tables; ++t) {
        if (counts[t] < 1 || counts[t] > max_taps || total + counts[t] > kTapStore) return SM3_EINVAL;
        a.first[t] = total, a.count[t] = counts[t];
        for (int k = 0; k < counts[t]; ++k) {
            const int dy = tables[((int64_t)t * max_taps + k) * 2], dx = tables[((int64_t)t * max_taps + k) * 2 + 1];
            if (dy < -kHalo || dy > kHalo || dx < -kHalo || dx > kHalo) return SM3_EINVAL;
            a.dy[total + k] = (int16_t)dy, a.dx[total + k] = (int16_t)dx;
        }
        total += counts[t];
    }
    for (int b = 0; b < B; ++b)
        if (table_index[b] < 0 || table_index[b] >= n_tables) return SM3_EINVAL;
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    if ((int64_t)3 * tiles_x * tiles_y > kMax31) return SM3_EINVAL;
    const int64_t E = (int64_t)3 * H * W;
    for (int b0 = 0; b0 < B; b0 += kCaseChunk) {
        const int nb = B - b0 < kCaseChunk ? B - b0 : kCaseChunk;
        for (int b = 0; b < nb; ++b) a.table_of[b] = (uint8_t)table_index[b0 + b];
        hipLaunchKernelGGL(corrupt_taps_kernel, dim3((uint32_t)(3 * tiles_x * tiles_y), (uint32_t)nb), dim3(kTile, kRows), 0,
                           (hipStream_t)stream, x + b0 * E, out + b0 * E, H, W, tiles_x, tiles_y, a);
        SM3_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int sm3_corrupt_pixelate(const float* x, int B, int H, int W, int f, float* out, void* stream) {
    if (bad_image(x, out, B, H, W) || f < 1 || f > kMaxF || B > 65535) return SM3_EINVAL;
    const int S = (kTile / f) * f;
    const int tiles_x = (W + S - 1) / S, tiles_y = (H + S - 1) / S;
    if ((int64_t)3 * tiles_x * tiles_y > kMax31) return SM3_EINVAL;
    hipLaunchKernelGGL(corrupt_pixelate_kernel, dim3((uint32_t)(3 * tiles_x * tiles_y), (uint32_t)B), dim3(kTile, kRows), 0,
                       (hipStream_t)stream, x, out, H, W, tiles_x, tiles_y, f, S);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_corrupt_jpeg(const float* x, int B, int H, int W, int quality, const int32_t* qt_luma, const int32_t* qt_chroma,
                                float* out, void* stream) {
    if (bad_image(x, out, B, H, W) || !qt_luma || !qt_chroma || quality < 1 || quality > 100) return SM3_EINVAL;
    JpegArgs a;
    for (int k = 0; k < 64; ++k) {
        if (qt_luma[k] < 1 || qt_luma[k] > 255 || qt_chroma[k] < 1 || qt_chroma[k] > 255) return SM3_EINVAL;
        a.qt[0][k] = (uint8_t)qt_luma[k], a.qt[1][k] = (uint8_t)qt_chroma[k];
    }
    const int blocks_x = (W + 7) / 8, blocks_y = (H + 7) / 8;
    const int64_t n_blocks = (int64_t)B * blocks_x * blocks_y;
    if ((n_blocks + kJpegWaves - 1) / kJpegWaves > kMax31) return SM3_EINVAL;
    hipLaunchKernelGGL(corrupt_jpeg_kernel, dim3((uint32_t)((n_blocks + kJpegWaves - 1) / kJpegWaves)), dim3(kThreads), 0,
                       (hipStream_t)stream, x, out, H, W, blocks_x, blocks_y, n_blocks, a);
    SM3_CHECK_LAUNCH();
    return 0;
}
