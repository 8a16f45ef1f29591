// Significance of a paired comparison (sm3hip/significance.py): the integer counts behind the paired
// randomisation test of two sets of predictions of the same cases, and the integer placements behind DeLong's test.  Everything
// here is an integer; the divisions, the exact rationals and the p-values happen on the host.
//
// THE SWAP RULE.  Two models a, b score the same N cases.  Per column k = (label t, class c) the 2N scores are ranked jointly:
// element e = 2 * i + w is model w's score of case i (w = 0: a, w = 1: b), sorted ascending and stably ONCE, order[k][j] = the
// element at joint position j, gs[k][j] / ge[k][j] = first and one-past-last position of j's tie group (ties by == on the fp64
// scores).  Replicate r swaps case i iff bit i & 31 of swap word i >> 5 is set; swap word d is word d % 4 of Philox4x32-10
// (exact_f32.h) with key = the 64-bit seed (low word first) and counter (d / 4, r, 0, 5) -- that is counter (i >> 7, r, 0, 5),
// word (i >> 5) & 3; stream 5 is apart from SmoothGrad's 0, RISE's 1, the bootstrap's 2 and logreg's 3 and 4.  The point record
// swaps nothing.  Side A' takes element w == swap_i of every case and side B' the other, the predicted class yhat with it.  One
// swap vector serves every column of a replicate, and it is a function of (seed, r, N) alone.
//
// Per replicate, column and side, with "positive" = (y == c):
//     S[j] = the side's negative elements at joint positions < j                             (S[2N] = Q)
//     A2   = sum over the side's positive elements j of (S[gs[j]] + S[ge[j]])     = 2 * (negatives strictly below) + tied negatives
//     TP   = the side's elements with y == c & yhat == c,  FP = those with y != c & yhat == c
// P, Q and FN = P - TP do not depend on the swap and are the host's.
//
//   sm3_signif_counts: out[j][k][side] = (A2, TP, FP) int64 for replicate r = r0 + j.  One workgroup per (replicate, label), as
//                      report_counts_kernel.  The swap words are READ, not counted: ceil(N / 128) Philox calls into LDS, no
//                      atomics.  The LDS word of a case holds swap | y << 8 | yhat_a << 16 | yhat_b << 24.  Per column ONE
//                      tile_scan<uint32_t> over the 2N joint positions carries both sides' negative counts as two 16-bit
//                      halves (a side has at most N <= 8192 negatives: no carry leaves its half); TP and FP fall out of the same
//                      pass, since the joint ranking visits every element once; a second pass sums A2 of both sides.
//                      LDS: 32 KiB of case words + 64 KiB + 4 of packed S (+ 1 KiB of swap words and the reduction scratch).
//   sm3_signif_placements: DeLong's placements, times two, of ONE model's own ranking (order, gs, ge [K][N] as
//                      sm3_report_counts'), in case order: out[k][i] = u_i = 2 * (negatives below) + tied negatives for a positive
//                      case i, v_i = 2 * (positives above) + tied positives for a negative one.  One workgroup per column: one
//                      packed scan (negatives low half, positives high half), then the scatter through order.
#include "resample.h"

namespace {

constexpr int kMaxColumns = 64;
constexpr int kMaxLabels = 64;
constexpr int kMaxJoint = 2 * kMaxCases;       // joint positions of a column
constexpr int kSwapWords = kMaxCases / 32;

// grid (c, T); order, gs, ge [K][2N]; y, yhat_a, yhat_b [N][T]; colmap [K][2] = (label, class); out [c][K][2][3]
__global__ void __launch_bounds__(kThreads) signif_counts_kernel(const int* __restrict__ order, const int* __restrict__ gs,
                                                                 const int* __restrict__ ge, const int* __restrict__ y,
                                                                 const int* __restrict__ yhat_a, const int* __restrict__ yhat_b,
                                                                 const int* __restrict__ colmap, long long* __restrict__ out, int N,
                                                                 int T, int K, uint32_t key0, uint32_t key1, uint32_t r0, int point) {
    __shared__ uint32_t word[kMaxCases];       // swap | y << 8 | yhat_a << 16 | yhat_b << 24 of the workgroup's label
    __shared__ uint32_t S[kMaxJoint + 1];      // A' negatives below in the low half, B' negatives in the high half
    __shared__ uint32_t swapw[kSwapWords];
    __shared__ uint32_t wsum[2][kWaves];
    __shared__ long long red[kWaves][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = r0 + blockIdx.x;
    const int M = 2 * N;

    for (int q = tid; 128 * q < N; q += kThreads) {  // q < 64: the four words of call q are swap words 4 q .. 4 q + 3
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (!point) philox4x32_10((uint32_t)q, r, 0u, 5u, key0, key1, w);
#pragma unroll
        for (int l = 0; l < 4; ++l) swapw[4 * q + l] = w[l];
    }
    __syncthreads();

    const int t = blockIdx.y;
    for (int i = tid; i < N; i += kThreads)
        word[i] = ((swapw[i >> 5] >> (i & 31)) & 1u) | (((uint32_t)y[(int64_t)i * T + t] & 0xffu) << 8) |
                  (((uint32_t)yhat_a[(int64_t)i * T + t] & 0xffu) << 16) | (((uint32_t)yhat_b[(int64_t)i * T + t] & 0xffu) << 24);
    __syncthreads();

    for (int k = 0; k < K; ++k) {
        if (colmap[2 * k] != t) continue;      // the same for the whole workgroup
        const uint32_t cls = (uint32_t)colmap[2 * k + 1] & 0xffu;
        const int* ord = order + (int64_t)k * M;
        uint32_t carry = 0;
        int tp[2] = {0, 0}, fp[2] = {0, 0};
        for (int base = 0, it = 0; base < M; base += kTile, ++it) {
            const int j0 = base + kPer * tid;
            uint32_t v[kPer], s = 0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                v[e] = 0;
                if (j0 + e < M) {
                    const uint32_t el = min((uint32_t)ord[j0 + e], (uint32_t)(M - 1));
                    const uint32_t w = word[el >> 1], side = (el ^ w) & 1u;  // A' (0) takes the element whose model == swap
                    const bool pos = ((w >> 8) & 0xffu) == cls, hit = ((w >> (el & 1u ? 24 : 16)) & 0xffu) == cls;
                    v[e] = pos ? 0u : 1u << (16 * side);
                    tp[0] += pos && hit && !side, tp[1] += pos && hit && side;
                    fp[0] += !pos && hit && !side, fp[1] += !pos && hit && side;
                }
                s += v[e];
            }
            uint32_t run = tile_scan(s, carry, wsum, it);
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                if (j0 + e < M) S[j0 + e] = run;
                run += v[e];
            }
        }
        if (tid == 0) S[M] = carry;
        __syncthreads();

        long long a2[2] = {0, 0};
        for (int j = tid; j < M; j += kThreads) {
            const uint32_t el = min((uint32_t)ord[j], (uint32_t)(M - 1));
            const uint32_t w = word[el >> 1], side = (el ^ w) & 1u;
            if (((w >> 8) & 0xffu) == cls) {
                const uint32_t lo = min((uint32_t)gs[(int64_t)k * M + j], (uint32_t)M), hi = min((uint32_t)ge[(int64_t)k * M + j], (uint32_t)M);
                const uint32_t both = S[lo] + S[hi];   // each half at most 2 * 8192: still no carry
                a2[0] += side ? 0 : (long long)(both & 0xffffu);
                a2[1] += side ? (long long)(both >> 16) : 0;
            }
        }
        long long a[6] = {a2[0], tp[0], fp[0], a2[1], tp[1], fp[1]};
#pragma unroll
        for (int e = 0; e < 6; ++e) a[e] = wave_sum(a[e]);
        if (lane == 0)
            for (int e = 0; e < 6; ++e) red[wave][e] = a[e];
        __syncthreads();  // also: every read of S is done before the next column writes it
        if (tid == 0) {
            long long* o = out + ((int64_t)blockIdx.x * K + k) * 6;
            for (int e = 0; e < 6; ++e) {
                long long sum = 0;
                for (int w = 0; w < kWaves; ++w) sum += red[w][e];
                o[e] = sum;
            }
        }
        // red is next written after the next column's scan barriers, which thread 0 reaches only after the reads above
    }
}

// grid (K); order, gs, ge [K][N]; y [N][T]; colmap [K][2]; out [K][N] int32 in case order
__global__ void __launch_bounds__(kThreads) signif_placements_kernel(const int* __restrict__ order, const int* __restrict__ gs,
                                                                     const int* __restrict__ ge, const int* __restrict__ y,
                                                                     const int* __restrict__ colmap, int* __restrict__ out, int N,
                                                                     int T) {
    __shared__ uint32_t S[kMaxCases + 1];      // negatives below in the low half, positives below in the high half
    __shared__ uint32_t wsum[2][kWaves];
    const int tid = threadIdx.x, k = blockIdx.x;
    const int t = min(max(colmap[2 * k], 0), T - 1), cls = colmap[2 * k + 1];
    const int* ord = order + (int64_t)k * N;
    uint32_t carry = 0;
    for (int base = 0, it = 0; base < N; base += kTile, ++it) {
        const int j0 = base + kPer * tid;
        uint32_t v[kPer], s = 0;
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            v[e] = 0;
            if (j0 + e < N) {
                const int i = (int)min((uint32_t)ord[j0 + e], (uint32_t)(N - 1));
                v[e] = y[(int64_t)i * T + t] == cls ? 1u << 16 : 1u;
            }
            s += v[e];
        }
        uint32_t run = tile_scan(s, carry, wsum, it);
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            if (j0 + e < N) S[j0 + e] = run;
            run += v[e];
        }
    }
    if (tid == 0) S[N] = carry;
    __syncthreads();
    const uint32_t P = S[N] >> 16;
    for (int j = tid; j < N; j += kThreads) {
        const int i = (int)min((uint32_t)ord[j], (uint32_t)(N - 1));
        const uint32_t lo = min((uint32_t)gs[(int64_t)k * N + j], (uint32_t)N), hi = min((uint32_t)ge[(int64_t)k * N + j], (uint32_t)N);
        const uint32_t both = S[lo] + S[hi];
        const bool pos = y[(int64_t)i * T + t] == cls;
        out[(int64_t)k * N + i] = pos ? (int)(both & 0xffffu) : (int)(2u * P - (both >> 16));
    }
}

}  // namespace

extern "C" int sm3_signif_counts(const int* order, const int* gs, const int* ge, const int* targets, const int* yhat_a,
                                 const int* yhat_b, const int* colmap, int64_t* out, int N, int T, int K, uint64_t seed, int64_t r0,
                                 int c, int point, void* stream) {
    if (!order || !gs || !ge || !targets || !yhat_a || !yhat_b || !colmap || !out) return SM3_EINVAL;
    if (!resample_args_ok(N, r0, c, point) || T < 1 || T > kMaxLabels || K < 1 || K > kMaxColumns) return SM3_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 7) return SM3_EALIGN;
    hipLaunchKernelGGL(signif_counts_kernel, dim3((uint32_t)c, (uint32_t)T), dim3(kThreads), 0, (hipStream_t)stream, order, gs, ge,
                       targets, yhat_a, yhat_b, colmap, reinterpret_cast<long long*>(out), N, T, K, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_signif_placements(const int* order, const int* gs, const int* ge, const int* targets, const int* colmap,
                                     int32_t* out, int N, int T, int K, void* stream) {
    if (!order || !gs || !ge || !targets || !colmap || !out) return SM3_EINVAL;
    if (N < 1 || N > kMaxCases || T < 1 || T > kMaxLabels || K < 1 || K > kMaxColumns) return SM3_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 3) return SM3_EALIGN;
    hipLaunchKernelGGL(signif_placements_kernel, dim3((uint32_t)K), dim3(kThreads), 0, (hipStream_t)stream, order, gs, ge, targets,
                       colmap, out, N, T);
    SM3_CHECK_LAUNCH();
    return 0;
}
