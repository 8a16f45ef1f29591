// Test-time augmentation of the predictions (sm3hip/tta.py): the two steps around the encoders' eval-mode forward.
//
//   sm3_tta_dihedral: out[r][e][ch][y][x] = x[r][ch][y'][x'] for the elements g = elements[e] of the dihedral group of the
//                     square, g = fx | fy << 1 | tr << 2: a = fy ? H - 1 - y : y, b = fx ? W - 1 - x : x, (y', x') = tr ? (b, a)
//                     : (a, b) -- torch's transpose(-1, -2) if tr, then flip(-2) if fy, then flip(-1) if fx.  A workgroup of
//                     32 x 8 threads reads one 32 x 32 source tile of one plane ONCE, rows along the lanes, into a 32 x 33 dword LDS
//                     tile and stores it once per element: lane j of a 32-lane half owns destination column j of the element's
//                     destination tile, so every global store of a half-wave is one contiguous ascending run, for the mirrored and
//                     the transposed elements alike.  LDS banks ((a / 4) % 32 for ds_write_b32 / ds_read_b32, per 32-lane half):
//                     the write and the row reads touch tile[i][0 .. 31] (33 i + j: 32 banks), the transposed reads tile[0 .. 31][i]
//                     (33 j + i: 32 banks) -- no conflict either way.  A pure copy: the bits of x, NaN payloads included.
//   sm3_tta_reduce:   one wave per case, lane v = view v.  A lane turns its view's 24 logits into the 8 labels' probabilities in
//                     fp64 (z - max, exp, the sum in ascending class order, one division) and then into Q32 integers q =
//                     rint(p * 2^32); everything that crosses the lanes is an int64 sum / min / max or an int32 count over the
//                     xor butterfly, whose result no order of the views can change.  Lanes v >= V carry the identities.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 32;          // source tile edge
constexpr int kRows = 8;           // thread rows of a workgroup: 32 x 8 threads, 4 tile rows per thread
constexpr int kCols = 24;          // logit columns of a view
constexpr int kLabels = 8;
constexpr int kMaxViews = 64;      // one wave
__constant__ int kOff[kLabels + 1] = {0, 5, 8, 10, 13, 16, 19, 22, 24};  // metrics.NUM_CLASSES, prefix sums

// grid: planes * tiles_y * tiles_x workgroups (x fastest); elements: 4 bits per element, element e at bits 4e .. 4e + 3
__global__ void __launch_bounds__(kTile* kRows) tta_dihedral_kernel(const float* __restrict__ x, float* __restrict__ out, int H,
                                                                     int W, int tiles_x, int tiles_y, uint32_t elements,
                                                                     int n_g) {
    __shared__ float tile[kTile][kTile + 1];
    const int j = threadIdx.x, i0 = threadIdx.y;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    const int plane = b / tiles_y;  // r * 3 + ch
    const int y0 = ty * kTile, x0 = tx * kTile;
    const int th = min(kTile, H - y0), tw = min(kTile, W - x0);
    const int64_t HW = (int64_t)H * W;
    const float* src = x + plane * HW;
#pragma unroll
    for (int k = 0; k < kTile / kRows; ++k) {
        const int i = i0 + kRows * k;
        if (i < th && j < tw) tile[i][j] = src[(int64_t)(y0 + i) * W + x0 + j];
    }
    __syncthreads();
    const int r = plane / 3, ch = plane - 3 * r;
    for (int e = 0; e < n_g; ++e) {
        const uint32_t g = (elements >> (4 * e)) & 7u;
        const bool fx = g & 1u, fy = g & 2u, tr = g & 4u;
        // the destination tile: nj columns from column ox, ni rows from row oy; its column j is the source tile's row (tr) or
        // column (not tr) j, counted from the far end under fx; likewise its rows under fy
        const int nj = tr ? th : tw, ni = tr ? tw : th;
        const int sx = tr ? y0 : x0, sy = tr ? x0 : y0;
        const int ox = fx ? W - sx - nj : sx, oy = fy ? H - sy - ni : sy;
        float* dst = out + (((int64_t)r * n_g + e) * 3 + ch) * HW;
        if (j < nj) {
            const int jj = fx ? nj - 1 - j : j;
#pragma unroll
            for (int k = 0; k < kTile / kRows; ++k) {
                const int i = i0 + kRows * k;
                if (i < ni) {
                    const int ii = fy ? ni - 1 - i : i;
                    dst[(int64_t)(oy + i) * W + ox + j] = tr ? tile[jj][ii] : tile[ii][jj];
                }
            }
        }
    }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (int64_t)__shfl_xor((long long)v, m, 64);
    return v;
}
__device__ __forceinline__ int64_t wave_min(int64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t o = (int64_t)__shfl_xor((long long)v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_max(int64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t o = (int64_t)__shfl_xor((long long)v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// grid B, one wave each; every lane stays to the end (the butterflies need all 64)
__global__ void __launch_bounds__(kMaxViews) tta_reduce_kernel(const float* __restrict__ logits, int V, int64_t* __restrict__ q,
                                                               int64_t* __restrict__ sum_q, int64_t* __restrict__ min_q,
                                                               int64_t* __restrict__ max_q, int32_t* __restrict__ view_class,
                                                               int32_t* __restrict__ agg_class, int32_t* __restrict__ disagree,
                                                               float* __restrict__ preds) {
    const int v = threadIdx.x;
    const int64_t n = blockIdx.x;
    const bool live = v < V;
    const int64_t row = n * V + (live ? v : 0);  // an idle lane reads view 0 and drops it
    const float* z = logits + row * kCols;
    int64_t* qv = q + row * kCols;
    const double dV = (double)V * 4294967296.0;
    for (int t = 0; t < kLabels; ++t) {
        const int c0 = kOff[t], nc = kOff[t + 1] - c0;
        double zc[5], m = (double)z[c0];
        int top = 0;
        zc[0] = m;
        for (int c = 1; c < nc; ++c) {
            zc[c] = (double)z[c0 + c];
            if (zc[c] > m) m = zc[c], top = c;  // strict: the lowest index of the maximum
        }
        double s = 0.0;
        for (int c = 0; c < nc; ++c) {
            zc[c] = exp(zc[c] - m);
            s += zc[c];
        }
        int64_t best = -1;
        int agg = 0;
        for (int c = 0; c < nc; ++c) {
            const int64_t qc = (int64_t)rint(zc[c] / s * 4294967296.0);
            if (live) qv[c0 + c] = qc;
            const int64_t sq = wave_sum(live ? qc : 0);
            const int64_t lo = wave_min(live ? qc : INT64_MAX);
            const int64_t hi = wave_max(live ? qc : INT64_MIN);
            if (sq > best) best = sq, agg = c;  // strict again; the same in every lane
            if (v == 0) {
                const int64_t o = n * kCols + c0 + c;
                sum_q[o] = sq, min_q[o] = lo, max_q[o] = hi;
                preds[o] = (float)log((double)(sq > 1 ? sq : 1) / dV);
            }
        }
        if (live) view_class[row * kLabels + t] = top;
        const int64_t d = wave_sum(live && top != agg ? 1 : 0);
        if (v == 0) agg_class[n * kLabels + t] = agg, disagree[n * kLabels + t] = (int32_t)d;
    }
}

}  // namespace

extern "C" int sm3_tta_dihedral(const float* x, int rows, int H, int W, const int* elements, int n_g, float* out, void* stream) {
    if (!x || !out || !elements || rows < 1 || H < 1 || W < 1 || n_g < 1 || n_g > 8) return SM3_EINVAL;
    uint32_t packed = 0u;
    for (int e = 0; e < n_g; ++e) {
        if (elements[e] < 0 || elements[e] > 7) return SM3_EINVAL;
        if ((elements[e] & 4) && H != W) return SM3_EINVAL;
        packed |= (uint32_t)elements[e] << (4 * e);
    }
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    const int64_t blocks = (int64_t)rows * 3 * tiles_x * tiles_y;
    if (blocks > 2147483647ll) return SM3_EINVAL;
    hipLaunchKernelGGL(tta_dihedral_kernel, dim3((uint32_t)blocks), dim3(kTile, kRows), 0, (hipStream_t)stream, x, out, H, W,
                       tiles_x, tiles_y, packed, n_g);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_tta_reduce(const float* logits, int B, int V, int64_t* q, int64_t* sum_q, int64_t* min_q, int64_t* max_q,
                              int32_t* view_class, int32_t* agg_class, int32_t* disagree, float* preds, void* stream) {
    if (!logits || !q || !sum_q || !min_q || !max_q || !view_class || !agg_class || !disagree || !preds || B < 1 || V < 1 ||
        V > kMaxViews)
        return SM3_EINVAL;
    hipLaunchKernelGGL(tta_reduce_kernel, dim3((uint32_t)B), dim3(kMaxViews), 0, (hipStream_t)stream, logits, V, q, sum_q, min_q,
                       max_q, view_class, agg_class, disagree, preds);
    SM3_CHECK_LAUNCH();
    return 0;
}
