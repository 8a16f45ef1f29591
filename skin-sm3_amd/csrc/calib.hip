// Calibration report (sm3hip/calibration.py): the integer bin tables behind ECE, MCE and the reliability diagram, and the integer
// sums behind NLL and the Brier score, for the point estimate and for case-resampling bootstrap replicates.  Everything here is
// an integer; the divisions that turn the tables into values happen on the host.
//
// A series s is (q[s][n] int64 in Q32, ev[s][n] 0/1) over the N cases, sorted ascending by q ONCE on the host side (stable:
// order[s][j] = the case at sorted position j).  With case multiplicities m[n] >= 0, sum m = N, and M bins:
//
//     width binning: every copy of case n goes to bin min((q * M) >> 32, M - 1);
//     mass binning:  the case at sorted position j owns the copy ranks [R_j, R_j + m_j), R_j = sum of m over the positions < j;
//                    the copy at rank u goes to bin (u * M) / N -- a case whose ranks straddle a boundary is split copy by copy;
//     per bin:       n_b = copies, E_b = sum of the copies' ev, Q_b = sum of the copies' q;
//     plain sum x:   sum over n of m[n] * xq[x][n].
//
//   sm3_calib_counts: bins[j][s][b] = (n_b, E_b, Q_b), sums[j][x], int64, for replicate r = r0 + j.  One workgroup per
//                     (replicate, label): it builds m_r ONCE in LDS by resample_multiplicities (resample.h: the resampling
//                     rule, so replicate r resamples the same cases in every report), and serves every series whose label it is and
//                     every plain sum x with x % T == label: 3 to 6 series and 2 sums for derm7pt, and the point table (one
//                     replicate) still fills 8 CUs.  Both binnings walk the series in sorted order, 4 consecutive positions per
//                     thread, where the bin index never decreases: a thread adds up a run of equal bins in registers and
//                     spends two 64-bit LDS atomics per run (n_b and E_b share one word, 32 bits each), not three per case.
//                     The mass binning needs R_j: a workgroup prefix scan of m along the order (tile_scan), consumed in the
//                     same pass.
// Every sum is an integer: no order shows, no float exists.  A replicate is a function of (seed, r, N) alone.
#include "resample.h"

namespace {

constexpr int kMaxSeries = 64;
constexpr int kMaxSums = 64;
constexpr int kMaxLabels = 64;
constexpr int kMaxBins = 64;

// grid (c, T); q [S][N]; ev [S][N]; order [S][N]; slabel [S]; xq [X][N]; bins [c][S][M][3]; sums [c][X]
__global__ void __launch_bounds__(kThreads) calib_counts_kernel(const long long* __restrict__ q, const uint8_t* __restrict__ ev,
                                                                const int* __restrict__ order, const int* __restrict__ slabel,
                                                                const long long* __restrict__ xq, long long* __restrict__ bins,
                                                                long long* __restrict__ sums, int N, int S, int X, int T, int M,
                                                                int mass, uint32_t key0, uint32_t key1, uint32_t r0, int point) {
    __shared__ uint32_t mult[kMaxCases];
    __shared__ unsigned long long acc[2 * kMaxBins];  // per bin: n_b | E_b << 32 (both <= N < 2^14), then Q_b
    __shared__ int wsum[2][kWaves];
    __shared__ long long red[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = r0 + blockIdx.x;

    resample_multiplicities(mult, N, key0, key1, r, point);

    const int t = blockIdx.y;
    for (int s = 0; s < S; ++s) {
        if (slabel[s] != t) continue;  // the same for the whole workgroup
        const int* ord = order + (int64_t)s * N;
        const long long* qs = q + (int64_t)s * N;
        const uint8_t* es = ev + (int64_t)s * N;
        for (int i = tid; i < 2 * M; i += kThreads) acc[i] = 0ull;
        __syncthreads();
        int carry = 0;
        for (int base = 0, it = 0; base < N; base += kTile, ++it) {
            const int j0 = base + kPer * tid;
            int cs[kPer], mv[kPer], tot = 0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                cs[e] = 0, mv[e] = 0;
                if (j0 + e < N) {
                    cs[e] = (int)min((uint32_t)ord[j0 + e], (uint32_t)(N - 1));
                    mv[e] = (int)mult[cs[e]];
                }
                tot += mv[e];
            }
            int rank = 0;  // R of the thread's first position (mass binning)
            if (mass) rank = tile_scan(tot, carry, wsum, it);  // the same for the whole grid
            int cur = -1;  // the run of equal bins held in registers
            unsigned long long ne = 0ull, qsum = 0ull;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                const int m = mv[e];
                if (m) {
                    const unsigned long long qv = (unsigned long long)qs[cs[e]];
                    const unsigned long long one = 1ull | ((unsigned long long)(es[cs[e]] != 0) << 32);
                    // valid input keeps every bin below M; the clamps only keep foreign input inside acc
                    int b0, b1;
                    if (mass) {
                        b0 = min((int)(((int64_t)rank * M) / N), M - 1);
                        b1 = min((int)(((int64_t)(rank + m - 1) * M) / N), M - 1);
                    } else {
                        b0 = b1 = (int)min((qv * (unsigned long long)M) >> 32, (unsigned long long)(M - 1));
                    }
                    for (int b = b0; b <= b1; ++b) {
                        // bin b holds the ranks [ceil(b N / M), ceil((b + 1) N / M))
                        const int lo = b == b0 ? rank : (int)(((int64_t)b * N + M - 1) / M);
                        const int hi = b == b1 ? rank + m : (int)(((int64_t)(b + 1) * N + M - 1) / M);
                        const unsigned long long cnt = mass ? (unsigned long long)(hi - lo) : (unsigned long long)m;
                        if (b != cur) {
                            if (cur >= 0) {
                                atomicAdd(&acc[2 * cur], ne);
                                atomicAdd(&acc[2 * cur + 1], qsum);
                            }
                            cur = b, ne = 0ull, qsum = 0ull;
                        }
                        ne += cnt * one;
                        qsum += cnt * qv;
                    }
                }
                rank += m;
            }
            if (cur >= 0) {
                atomicAdd(&acc[2 * cur], ne);
                atomicAdd(&acc[2 * cur + 1], qsum);
            }
        }
        __syncthreads();
        long long* o = bins + ((int64_t)blockIdx.x * S + s) * M * 3;
        for (int b = tid; b < M; b += kThreads) {
            const unsigned long long a = acc[2 * b];
            o[3 * b] = (long long)(a & 0xffffffffull), o[3 * b + 1] = (long long)(a >> 32), o[3 * b + 2] = (long long)acc[2 * b + 1];
        }
        __syncthreads();  // every read of acc is done before the next series clears it
    }

    for (int x = t; x < X; x += T) {
        const long long* xs = xq + (int64_t)x * N;
        long long a = 0;
        for (int i = tid; i < N; i += kThreads) a += (long long)mult[i] * xs[i];
        a = wave_sum(a);
        if (lane == 0) red[wave] = a;
        __syncthreads();
        if (tid == 0) {
            long long v = 0;
            for (int w = 0; w < kWaves; ++w) v += red[w];
            sums[(int64_t)blockIdx.x * X + x] = v;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int sm3_calib_counts(const int64_t* q, const uint8_t* ev, const int* order, const int* slabel, const int64_t* xq,
                                int64_t* bins, int64_t* sums, int N, int S, int X, int T, int M, int binning, uint64_t seed,
                                int64_t r0, int c, int point, void* stream) {
    if (!q || !ev || !order || !slabel || !xq || !bins || !sums) return SM3_EINVAL;
    if (!resample_args_ok(N, r0, c, point) || S < 1 || S > kMaxSeries || X < 1 || X > kMaxSums || T < 1 || T > kMaxLabels)
        return SM3_EINVAL;
    if (M < 1 || M > kMaxBins || (binning != 0 && binning != 1)) return SM3_EINVAL;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(bins) |
         reinterpret_cast<uintptr_t>(sums)) & 7)
        return SM3_EALIGN;
    hipLaunchKernelGGL(calib_counts_kernel, dim3((uint32_t)c, (uint32_t)T), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(q), ev, order, slabel, reinterpret_cast<const long long*>(xq),
                       reinterpret_cast<long long*>(bins), reinterpret_cast<long long*>(sums), N, S, X, T, M, binning, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}
