// What the seven bootstrap report kernels share (report.hip, calib.hip, operating.hip, retrieval.hip, checklist.hip,
// conformal.hip, selective.hip: the *_counts_kernel of each).
//
// THE RESAMPLING RULE, stated here once for the device (sm3hip/resample.py states it for the host, DESIGN.md 8.10 in prose):
// replicate r of N cases makes N draws; draw d hits case (w * N) >> 32 in 64-bit integers, w = word d % 4 of Philox4x32-10
// (exact_f32.h) with key = the 64-bit seed (low word first) and counter (d / 4, r, 0, 2) -- the last word keeps the stream apart
// from SmoothGrad's 0 and RISE's 1.  m_r[i] = the draws that hit case i; the point estimate has m = 1 and draws nothing.  m_r is
// a function of (seed, r, N) alone, so with one seed replicate r resamples the same cases in every report: their intervals are
// joint and their comparisons paired.  conformal.hip resamples a second split, the calibration cases, by the same rule with 6 as
// the last counter word (0 to 5 are taken: sm3hip/resample.py, philox_words), so that one seed serves both splits.
#pragma once
#include "exact_f32.h"

// These names are at file scope: a file that includes this header takes its geometry from here and must not define a kThreads
// (or kWaves, kPer, kTile, kMaxCases) of its own, in an anonymous namespace or otherwise -- the name would be ambiguous.
constexpr int kThreads = 256;              // the workgroup of every *_counts_kernel
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;                    // sorted positions per thread and tile
constexpr int kTile = kThreads * kPer;     // 1024
constexpr int kMaxCases = 8192;            // sm3_report_max_cases(): m of a replicate is 32 KiB of LDS; 8192 fits 16 bits

// m[0 .. N) in LDS = m_r of the rule above, counted by integer LDS atomics (`point`: all 1).  Whole workgroup; two barriers, the
// second only when there were draws.  `also` runs before the first barrier: what it writes to LDS (retrieval.hip zeroes its
// histogram there) is visible to every thread after the call.  `word` is the last counter word: 2 for every report's own cases.
template <typename Also>
static __device__ __forceinline__ void resample_multiplicities(uint32_t* m, int N, uint32_t key0, uint32_t key1, uint32_t r,
                                                               int point, uint32_t word, Also also) {
    const int tid = threadIdx.x;
    for (int i = tid; i < N; i += kThreads) m[i] = point ? 1u : 0u;
    also();
    __syncthreads();
    if (!point) {
        for (int q = tid; 4 * q < N; q += kThreads) {
            uint32_t w[4];
            philox4x32_10((uint32_t)q, r, 0u, word, key0, key1, w);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (4 * q + l < N) atomicAdd(&m[(uint32_t)(((uint64_t)w[l] * (uint32_t)N) >> 32)], 1u);
        }
        __syncthreads();
    }
}

template <typename Also>
static __device__ __forceinline__ void resample_multiplicities(uint32_t* m, int N, uint32_t key0, uint32_t key1, uint32_t r,
                                                               int point, Also also) {
    resample_multiplicities(m, N, key0, key1, r, point, 2u, also);
}

static __device__ __forceinline__ void resample_multiplicities(uint32_t* m, int N, uint32_t key0, uint32_t key1, uint32_t r,
                                                               int point) {
    resample_multiplicities(m, N, key0, key1, r, point, 2u, [] {});
}

static __device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
static __device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One tile of a workgroup prefix scan.  s = the sum of this thread's kPer positions of tile `it`; returns the sum over every
// position before the thread's first (earlier tiles through `carry`, which advances by the tile's total).  Wave scan by
// shuffles, the wave totals through wsum[it & 1] (double-buffered: ONE barrier per tile).  T: int, or uint32_t for two packed
// 16-bit halves that cannot carry into each other.
template <typename T>
static __device__ __forceinline__ T tile_scan(T s, T& carry, T (*wsum)[kWaves], int it) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = s;  // inclusive scan of the threads' sums over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[it & 1][wave] = incl;
    __syncthreads();
    T before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T ws = wsum[it & 1][w];
        before += w < wave ? ws : 0;
        total += ws;
    }
    carry += total;
    return before + incl - s;
}

// The N / r0 / c / point part of every sm3_*_counts argument check: replicates r0 .. r0 + c - 1 fit the 32-bit counter word,
// and the point estimate is one table.
static inline bool resample_args_ok(int N, int64_t r0, int c, int point) {
    return N >= 1 && N <= kMaxCases && c >= 1 && r0 >= 0 && r0 + (int64_t)c <= ((int64_t)1 << 32) && !(point && c != 1);
}
