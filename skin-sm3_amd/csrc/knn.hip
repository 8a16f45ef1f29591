// Weighted k-nearest-neighbour vote (Wu et al. 2018, sec. 3.4): the reference's KNNOnlineEvaluator.predict
// (src/models/evaluator.py:43-84) from the similarity matrix on, i.e. per query row the k largest similarities, their
// weights exp(s / T) and the per-class sums of those weights -- one set of class sums per label.
//
// One 256-thread workgroup (4 x wave64) per query row:
//   1. radix select of the k-th largest similarity on order-preserving uint32 keys of the f32 bits: 4 passes of 8 bits
//      over the row, one LDS histogram per wave, merged in wave order; the count of the selected bin narrows the next pass;
//   2. only when the k-th key is tied and not every tied element fits: 4 more passes over the bank indices of the tied
//      elements, so that the lowest indices are taken (the tie rule of the contract);
//   3. one pass collects the k winners as (key << 32 | ~index) words into LDS; their slots come from an LDS counter, but
//      the bitonic sort that follows orders them by (key descending, index ascending), a total order, so what leaves the
//      workgroup does not depend on the slot order;
//   4. one thread per label adds exp(s / T) into its own classes in rank order (rank 0 first), no atomics: two calls on
//      equal inputs give equal bits whatever the grid, and a label's sums do not depend on the other labels.
// Every pass streams the row (N floats) from L2 / HBM; at large N the kernel is bound by those 5 reads.
//
// Values (pinned by tests/test_knn_edges_gpu.py).  Similarities are ordered as floats: +inf first, -inf last, denormals by
// their value, -0 equal to +0; equal similarities go lower index first.  A +inf neighbour votes +inf, a -inf neighbour is a
// neighbour like any other (it appears in nbr_idx / nbr_sim) and votes exactly 0.  A target outside [0, C_l) casts no vote
// for label l; its row is still a neighbour.  Only the N valid columns of a row are read, whatever stands in [N, ld), and
// rows of any alignment (any ld >= N, any base) give the same bits.  NaN similarities are outside the contract: where a
// NaN ranks, and what it votes, is not defined.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 1024;
constexpr int kMaxLabels = 16;
constexpr int kMaxClasses = 256;
constexpr int kVoteChunk = 64;  // ranks whose targets are staged in LDS at a time

struct KnnLabels {
    int L;
    int off[kMaxLabels + 1];  // class offsets: label l owns scores[off[l], off[l+1])
};

// larger float -> larger key; -0 ranks with +0 (torch compares them equal)
__device__ __forceinline__ uint32_t order_key(float s) {
    uint32_t u = __float_as_uint(s);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// f(j, s) for every valid element j of the row: 16-byte loads when the row is 16-byte aligned (block-uniform test), four
// of them issued before the first is used
template <typename F>
__device__ __forceinline__ void for_row(const float* __restrict__ row, int N, F&& f) {
    constexpr int kU = 4;
    int tail = 0;
    if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0u) {
        const int n4 = N >> 2;
        const float4* r4 = reinterpret_cast<const float4*>(row);
        for (int q0 = threadIdx.x; q0 < n4; q0 += kU * kThreads) {
            float4 v[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int q = q0 + u * kThreads;
                v[u] = q < n4 ? r4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int q = q0 + u * kThreads;
                if (q < n4) {
                    f(4 * q, v[u].x);
                    f(4 * q + 1, v[u].y);
                    f(4 * q + 2, v[u].z);
                    f(4 * q + 3, v[u].w);
                }
            }
        }
        tail = n4 * 4;
    }
    for (int j = tail + (int)threadIdx.x; j < N; j += kThreads) f(j, row[j]);
}

// hist[d] += 1 for the active lanes; the lanes that share the first active lane's digit add as one (the first pass sees
// one dominant digit -- the similarities' exponent -- and 64 same-address LDS atomics per wave would serialise)
__device__ __forceinline__ void hist_add(uint32_t* hist, bool act, uint32_t d) {
    const uint64_t live = __ballot(act);
    if (live == 0) return;
    const int first = __ffsll((unsigned long long)live) - 1;
    const uint32_t d0 = __shfl(d, first, 64);
    const uint64_t same = __ballot(act && d == d0);
    if (act && d != d0) atomicAdd(&hist[d], 1u);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
}

struct SelectLds {
    uint32_t hist[kWaves][256];
    uint32_t wtot[kWaves];
    uint32_t digit, rem, count;
};

// One radix pass: among the elements `val(j, s, &v)` keeps, whose value v has `prefix` in the bits above `shift`, find the
// 8-bit digit at `shift` of the kk-th largest v.  On return prefix includes that digit, kk is the rank inside the digit's
// bin and the return value is the bin's count.  Every thread of the workgroup calls it.
template <typename V>
__device__ uint32_t radix_pass(const float* __restrict__ row, int N, int shift, uint32_t& prefix, uint32_t& kk, SelectLds& sh,
                               V&& val) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int i = t; i < kWaves * 256; i += kThreads) (&sh.hist[0][0])[i] = 0u;
    __syncthreads();
    const uint32_t hi_mask = shift >= 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
    uint32_t* h = sh.hist[w];
    for_row(row, N, [&](int j, float s) {
        uint32_t v;
        const bool keep = val(j, s, v) && (v & hi_mask) == (prefix & hi_mask);
        hist_add(h, keep, (v >> shift) & 255u);
    });
    __syncthreads();
    // bin t: its count (waves merged in a fixed order) and the count of bins >= t (suffix sum)
    const uint32_t c = ((sh.hist[0][t] + sh.hist[1][t]) + sh.hist[2][t]) + sh.hist[3][t];
    uint32_t s = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_down(s, o, 64);
        if (lane + o < 64) s += up;
    }
    if (lane == 0) sh.wtot[w] = s;
    __syncthreads();
    for (int v = w + 1; v < kWaves; ++v) s += sh.wtot[v];
    if (s >= kk && s - c < kk) {  // exactly one bin: kk <= number of kept elements
        sh.digit = (uint32_t)t;
        sh.rem = kk - (s - c);
        sh.count = c;
    }
    __syncthreads();
    prefix = (prefix & hi_mask) | (sh.digit << shift);
    kk = sh.rem;
    const uint32_t count = sh.count;
    __syncthreads();  // sh is reused by the next pass
    return count;
}

__global__ __launch_bounds__(kThreads) void knn_vote_kernel(const float* __restrict__ S, int N, int64_t ld,
                                                            const int32_t* __restrict__ targets, const KnnLabels lab, int k,
                                                            float temperature, float* __restrict__ scores, int total_classes,
                                                            int32_t* __restrict__ nbr_idx, float* __restrict__ nbr_sim) {
    __shared__ SelectLds sel;
    __shared__ uint64_t top[kMaxK];      // (key << 32) | ~index
    __shared__ float wts[kMaxK];         // exp(s / T) in rank order
    __shared__ int32_t tgt[kVoteChunk * kMaxLabels];
    __shared__ float acc[kMaxClasses];
    __shared__ uint32_t taken;

    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float* __restrict__ row = S + b * ld;

    // 1. the key of the k-th largest similarity
    uint32_t key_k = 0u, kk = (uint32_t)k, count = 0u;
    for (int shift = 24; shift >= 0; shift -= 8)
        count = radix_pass(row, N, shift, key_k, kk, sel, [](int, float s, uint32_t& v) {
            v = order_key(s);
            return true;
        });
    // 2. kk of the `count` elements equal to key_k are taken: the kk lowest indices (largest ~index)
    uint32_t last = 0u;  // ~(largest index taken among the ties); 0: every tied element is taken
    if (kk < count) {
        uint32_t kk2 = kk;
        for (int shift = 24; shift >= 0; shift -= 8)
            radix_pass(row, N, shift, last, kk2, sel, [key_k](int j, float s, uint32_t& v) {
                v = ~(uint32_t)j;
                return order_key(s) == key_k;
            });
    }

    // 3. collect the k winners, then sort them by (key desc, index asc)
    if (t == 0) taken = 0u;
    __syncthreads();
    for_row(row, N, [&](int j, float s) {
        const uint32_t key = order_key(s);
        const uint32_t nj = ~(uint32_t)j;
        const bool take = key > key_k || (key == key_k && nj >= last);
        const uint64_t m = __ballot(take);
        if (m == 0) return;
        const int lane = t & 63;
        const int first = __ffsll((unsigned long long)m) - 1;
        uint32_t base = 0u;
        if (lane == first) base = atomicAdd(&taken, (uint32_t)__popcll(m));
        base = __shfl(base, first, 64);
        if (take) {
            const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            top[base + r] = ((uint64_t)key << 32) | nj;
        }
    });
    int P = 1;
    while (P < k) P <<= 1;
    for (int i = k + t; i < P; i += kThreads) top[i] = 0ull;  // below every real word (a real ~index is >= 2^31)
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < P / 2; i += kThreads) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const uint64_t a = top[lo], c = top[hi];
                const bool desc = (lo & size) == 0;
                if (desc ? (a < c) : (a > c)) {
                    top[lo] = c;
                    top[hi] = a;
                }
            }
            __syncthreads();
        }
    }

    // 4. weights in rank order, then one thread per label adds them into its classes, rank 0 first
    for (int r = t; r < k; r += kThreads) {
        const int j = (int)~(uint32_t)top[r];
        const float s = row[j];
        wts[r] = expf(s / temperature);
        if (nbr_idx) nbr_idx[b * k + r] = j;
        if (nbr_sim) nbr_sim[b * k + r] = s;
    }
    for (int i = t; i < total_classes; i += kThreads) acc[i] = 0.f;
    const int L = lab.L;
    for (int r0 = 0; r0 < k; r0 += kVoteChunk) {
        __syncthreads();
        const int nr = min(kVoteChunk, k - r0);
        for (int e = t; e < nr * L; e += kThreads) {
            const int r = e / L, l = e - r * L;
            tgt[e] = targets[(int64_t)(int)~(uint32_t)top[r0 + r] * L + l];
        }
        __syncthreads();
        if (t < L) {
            const int c0 = lab.off[t], nc = lab.off[t + 1] - c0;
            for (int r = 0; r < nr; ++r) {
                const int c = tgt[r * L + t];
                if (c >= 0 && c < nc) acc[c0 + c] += wts[r0 + r];  // a class outside the label's range casts no vote
            }
        }
    }
    __syncthreads();
    for (int i = t; i < total_classes; i += kThreads) scores[b * total_classes + i] = acc[i];
}

}  // namespace

extern "C" int sm3_knn_vote(const float* S, int64_t B, int64_t N, int64_t ld, const int32_t* targets, int L,
                            const int32_t* class_offsets, int k, float temperature, float* scores, int32_t* nbr_idx,
                            float* nbr_sim, void* stream) {
    const int64_t kMax31 = 0x7fffffffLL;
    if (!S || !targets || !class_offsets || !scores) return SM3_EINVAL;
    if (B < 1 || N < 1 || ld < N || B > kMax31 || N > kMax31 || ld > kMax31) return SM3_EINVAL;
    if (k < 1 || k > kMaxK || k > N) return SM3_EINVAL;
    if (L < 1 || L > kMaxLabels) return SM3_EINVAL;
    if (!(temperature > 0.f) || !isfinite(temperature)) return SM3_EINVAL;
    KnnLabels lab{};
    lab.L = L;
    if (class_offsets[0] != 0) return SM3_EINVAL;
    for (int l = 0; l <= L; ++l) {
        lab.off[l] = class_offsets[l];
        if (l > 0 && lab.off[l] <= lab.off[l - 1]) return SM3_EINVAL;
    }
    if (lab.off[L] > kMaxClasses) return SM3_EINVAL;
    hipLaunchKernelGGL(knn_vote_kernel, dim3((uint32_t)B), dim3(kThreads), 0, (hipStream_t)stream, S, (int)N, ld, targets,
                       lab, k, temperature, scores, lab.off[L], nbr_idx, nbr_sim);
    SM3_CHECK_LAUNCH();
    return 0;
}
