// Conformal prediction-set report (sm3hip/conformal.py, which holds the definitions in full): split conformal thresholds from
// a calibration split, refitted in every bootstrap replicate, and the set counts of a test split under them.  Everything here
// is an integer; the divisions that turn the records into values happen on the host.
//
// Calibration: cal_a[t][n] = the true-class score of case n for label t, cal_order[t] = the cases in ascending cal_a (stable,
// sorted ONCE on the host side), cal_y[n][t] the class.  With multiplicities w on the calibration cases and a level num / den:
//
//     marginal (0): n' = sum w = N_cal;  class (1): per class c of the label, over the cases with y = c: n' = sum w [y = c];
//     k    = (n' + 1) - ((n' + 1) * num) / den                                  (int64, integer division);
//     qhat = cal_a at the first position j of the order with R_j + w_j >= k, R_j = the sum of w (of the class) before j;
//     qhat = kInf = 2^40 where k > n' (n' = 0 included).  The marginal qhat is the threshold of every class of the label.
//
// Test: with multiplicities m, the set of case n is {c : s[col(t, c)][n] <= thr[c]}; the record of a (label, level) is
//     (cov, size, single_hit, hist[0 .. 5], then per class c = 0 .. 4: n_c, cov_c, in_c)                       24 int64,
// cov = sum m [true class in set], size = sum m |set|, single_hit = sum m [|set| = 1, covered], hist[k] = sum m [|set| = k],
// n_c = sum m [y = c], cov_c = sum m [y = c][c in set], in_c = sum m [c in set]; slots of classes the label lacks are 0.
//
//   sm3_conformal_counts: one workgroup per (replicate, label).  Phase 1 (skipped with fixed thresholds): w in LDS by
//                     resample_multiplicities on stream word 6; in class mode a pass for the class totals n'; the ranks k; then
//                     ONE walk of cal_order in tiles of 1024 with tile_scan.  The marginal walk scans an int.  The class walk
//                     scans ONE packed 64-bit word, 16 bits per class 0 .. 3 (every count is at most 8192: no carry between
//                     fields), and for a label with a fifth class a second, 32-bit word: that is one label of eight, and one
//                     extra barrier per tile there, against up to five walks with one scan per class.  The position with
//                     before < k <= before + w is owned by exactly one thread, which writes its cal_a to the LDS table.
//                     Phase 2: the same LDS array holds m (stream word 2, the cases of every other report); per level a
//                     strided pass over the cases with m > 0 keeps the 24 counters in registers (each at most 5 * 8192),
//                     wave_sum, the four partials through LDS, and wave 0 stores the record and the thresholds.
// Every sum is an integer: no order shows, no float exists.  A replicate is a function of (seed, r, N_cal, N) alone.
#include "resample.h"

namespace {

constexpr int kMaxLevels = 8;
constexpr int kMaxClasses = 5;
constexpr int kRecord = 24;
constexpr int kMaxLabels = 64;
constexpr int kMaxColumns = 256;
constexpr long long kInf = 1ll << 40;  // above any score: LAC <= 2^32, APS <= the sum of a row's q, 2^32 + 5 at the most
constexpr uint32_t kCalWord = 6u;      // the calibration split's stream (resample.h)

struct Levels {
    int num[kMaxLevels], den[kMaxLevels];
};

// the 16-bit field of class c < 4 in the packed scan word
static __device__ __forceinline__ unsigned long long field(int c, uint32_t v) { return (unsigned long long)v << (16 * c); }

// grid (c, T); cal_a, cal_order [T][N_cal]; cal_y [N_cal][T]; s [K][N]; y [N][T]; colmap [K][2]; fixed_thr null or [T][A][5];
// counts [c][T][A][24]; thr [c][T][A][5]
__global__ void __launch_bounds__(kThreads)
conformal_counts_kernel(const long long* __restrict__ cal_a, const int* __restrict__ cal_order, const int* __restrict__ cal_y,
                        const long long* __restrict__ s, const int* __restrict__ y, const int* __restrict__ colmap,
                        const long long* __restrict__ fixed_thr, long long* __restrict__ counts, long long* __restrict__ thr,
                        Levels lv, int N_cal, int N, int T, int K, int A, int conditional, uint32_t key0, uint32_t key1,
                        uint32_t r0, int point) {
    __shared__ uint32_t mult[kMaxCases];
    __shared__ long long thrs[kMaxLevels * kMaxClasses];
    __shared__ int rank[kMaxLevels * kMaxClasses];  // k of (level, class); 0: no crossing is looked for
    __shared__ int total[kMaxClasses];
    __shared__ int wsum[2][kWaves];
    __shared__ unsigned long long wsum4[2][kWaves];
    __shared__ uint32_t wsum1[2][kWaves];
    __shared__ int red[2][kWaves][kRecord];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = r0 + blockIdx.x;
    const int t = blockIdx.y;

    // the label's columns: col[c] = the column of (t, c), -1 where the label has no class c.  The same for the whole workgroup.
    int col[kMaxClasses], nt = 0;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) col[c] = -1;
    for (int k = 0; k < K; ++k) {
        if (colmap[2 * k] != t) continue;
        const int cls = colmap[2 * k + 1];
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c)
            if (cls == c) col[c] = k, nt = max(nt, c + 1);
    }

    if (fixed_thr) {
        if (tid < A * kMaxClasses) thrs[tid] = fixed_thr[(int64_t)t * A * kMaxClasses + tid];
    } else {
        resample_multiplicities(mult, N_cal, key0, key1, r, point, kCalWord, [&] {
            if (tid < kMaxClasses) total[tid] = 0;
        });
        const int* ord = cal_order + (int64_t)t * N_cal;
        const long long* ca = cal_a + (int64_t)t * N_cal;
        const int cmax = max(nt - 1, 0);
        if (conditional) {  // the class totals n' come before the ranks
            int tot[kMaxClasses];
#pragma unroll
            for (int c = 0; c < kMaxClasses; ++c) tot[c] = 0;
            for (int i = tid; i < N_cal; i += kThreads) {
                const int m = (int)mult[i];
                const int yc = min(max(cal_y[(int64_t)i * T + t], 0), cmax);
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) tot[c] += yc == c ? m : 0;
            }
#pragma unroll
            for (int c = 0; c < kMaxClasses; ++c) {
                const int v = wave_sum(tot[c]);
                if (lane == 0 && v) atomicAdd(&total[c], v);
            }
            __syncthreads();
        }
        if (tid < A * kMaxClasses) {
            const int a = tid / kMaxClasses, c = tid % kMaxClasses;
            long long num = 1, den = 2;  // lv lives in scalar registers: select, do not index
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l)
                if (l == a) num = lv.num[l], den = lv.den[l];
            const long long n1 = (long long)(conditional ? total[c] : N_cal) + 1;
            const long long k = n1 - (n1 * num) / den;
            const bool live = k < n1 && (conditional ? c < nt : c == 0);
            rank[tid] = live ? (int)k : 0;
            thrs[tid] = kInf;
        }
        __syncthreads();

        int carry = 0;
        unsigned long long carry4 = 0ull;
        uint32_t carry1 = 0u;
        for (int base = 0, it = 0; base < N_cal; base += kTile, ++it) {
            const int j0 = base + kPer * tid;
            int cs[kPer], mv[kPer], yc[kPer], tot = 0;
            unsigned long long tot4 = 0ull;
            uint32_t tot1 = 0u;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                cs[e] = 0, mv[e] = 0, yc[e] = 0;
                if (j0 + e < N_cal) {
                    cs[e] = (int)min((uint32_t)ord[j0 + e], (uint32_t)(N_cal - 1));
                    mv[e] = (int)mult[cs[e]];
                    if (conditional) yc[e] = min(max(cal_y[(int64_t)cs[e] * T + t], 0), cmax);
                }
                tot += mv[e];
                if (yc[e] < 4) tot4 += field(yc[e], (uint32_t)mv[e]);
                else tot1 += (uint32_t)mv[e];
            }
            // the sums before the thread's first position: marginal, or per class (the same branch for the whole grid)
            int before = 0;
            unsigned long long before4 = 0ull;
            uint32_t before1 = 0u;
            if (!conditional) {
                before = tile_scan(tot, carry, wsum, it);
            } else {
                before4 = tile_scan(tot4, carry4, wsum4, it);
                if (nt > 4) before1 = tile_scan(tot1, carry1, wsum1, it);
            }
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                const int m = mv[e];
                if (m) {
                    const int c = yc[e];  // 0 in marginal mode
                    const int lo = !conditional ? before : c < 4 ? (int)((before4 >> (16 * c)) & 0xffffull) : (int)before1;
                    for (int a = 0; a < A; ++a) {
                        const int k = rank[a * kMaxClasses + c];
                        if (lo < k && k <= lo + m) thrs[a * kMaxClasses + c] = ca[cs[e]];  // one thread per (level, class)
                    }
                    if (!conditional) before += m;
                    else if (c < 4) before4 += field(c, (uint32_t)m);
                    else before1 += (uint32_t)m;
                }
            }
        }
    }
    __syncthreads();  // the crossings are written, and every read of mult as the calibration multiplicities is done
    if (!fixed_thr) {   // the full table: the marginal qhat for every class of the label, 0 in the slots of the classes it lacks
        long long v = 0;
        if (tid < A * kMaxClasses) {
            const int c = tid % kMaxClasses;
            v = c < nt ? thrs[conditional ? tid : tid - c] : 0;
        }
        __syncthreads();
        if (tid < A * kMaxClasses) thrs[tid] = v;
    }

    resample_multiplicities(mult, N, key0, key1, r, point);  // its first barrier also publishes thrs

    for (int a = 0; a < A; ++a) {
        long long th[kMaxClasses];
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c) th[c] = thrs[a * kMaxClasses + c];
        int rec[kRecord];
#pragma unroll
        for (int e = 0; e < kRecord; ++e) rec[e] = 0;
        for (int i = tid; i < N; i += kThreads) {
            const int m = (int)mult[i];
            if (!m) continue;
            const int yi = y[(int64_t)i * T + t];
            int size = 0, covered = 0;
#pragma unroll
            for (int c = 0; c < kMaxClasses; ++c) {
                if (col[c] < 0) continue;  // the same for the whole workgroup
                const int in = s[(int64_t)col[c] * N + i] <= th[c] ? 1 : 0;
                const int hit = yi == c ? 1 : 0;
                size += in;
                covered |= hit & in;
                rec[9 + 3 * c] += hit ? m : 0;
                rec[10 + 3 * c] += (hit & in) ? m : 0;
                rec[11 + 3 * c] += in ? m : 0;
            }
            rec[0] += covered ? m : 0;
            rec[1] += size * m;
            rec[2] += (covered && size == 1) ? m : 0;
#pragma unroll
            for (int k = 0; k <= kMaxClasses; ++k) rec[3 + k] += size == k ? m : 0;
        }
#pragma unroll
        for (int e = 0; e < kRecord; ++e) {
            const int v = wave_sum(rec[e]);
            if (lane == 0) red[a & 1][wave][e] = v;
        }
        __syncthreads();  // red is double-buffered: one barrier per level
        const int64_t o = ((int64_t)blockIdx.x * T + t) * A + a;
        if (tid < kRecord) {
            long long v = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) v += red[a & 1][w][tid];
            counts[o * kRecord + tid] = v;
        }
        if (tid < kMaxClasses) thr[o * kMaxClasses + tid] = thrs[a * kMaxClasses + tid];
    }
}

}  // namespace

extern "C" int sm3_conformal_counts(const int64_t* cal_a, const int* cal_order, const int* cal_y, const int64_t* s, const int* y,
                                    const int* colmap, const int* alpha, const int64_t* fixed_thr, int64_t* counts, int64_t* thr,
                                    int N_cal, int N, int T, int K, int A, int conditional, uint64_t seed, int64_t r0, int c,
                                    int point, void* stream) {
    if (!cal_a || !cal_order || !cal_y || !s || !y || !colmap || !alpha || !counts || !thr) return SM3_EINVAL;
    if (!resample_args_ok(N_cal, r0, c, point) || !resample_args_ok(N, r0, c, point)) return SM3_EINVAL;
    if (T < 1 || T > kMaxLabels || K < 1 || K > kMaxColumns || A < 1 || A > kMaxLevels) return SM3_EINVAL;
    if (conditional != 0 && conditional != 1) return SM3_EINVAL;
    Levels lv = {};
    for (int a = 0; a < A; ++a) {
        lv.num[a] = alpha[2 * a], lv.den[a] = alpha[2 * a + 1];
        if (lv.den[a] <= 0 || lv.num[a] <= 0 || lv.num[a] >= lv.den[a]) return SM3_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(cal_a) | reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(fixed_thr) |
         reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(thr)) & 7)
        return SM3_EALIGN;
    hipLaunchKernelGGL(conformal_counts_kernel, dim3((uint32_t)c, (uint32_t)T), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(cal_a), cal_order, cal_y, reinterpret_cast<const long long*>(s), y,
                       colmap, reinterpret_cast<const long long*>(fixed_thr), reinterpret_cast<long long*>(counts),
                       reinterpret_cast<long long*>(thr), lv, N_cal, N, T, K, A, conditional, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}
