// Evaluation report (sm3hip/report.py): the integer counts behind AUROC, Recall, Spec and Prec of every (label, class) column,
// for the point estimate and for case-resampling bootstrap replicates.  Everything here is an integer; the divisions that turn
// counts into values happen on the host.
//
// Per column k = (label t, class c), with case multiplicities m[n] >= 0, sum m = N, over a ranking sorted once (ascending,
// stable; order[k][j] = the case at sorted position j, gs[k][j] / ge[k][j] = first and one-past-last position of j's tie group):
//
//     S[j] = sum of m over the negative cases (y != c) at positions < j                       (S[N] = Q)
//     A2   = sum over positive positions j of m_j * (S[gs[j]] + S[ge[j]])    = 2 * (negatives strictly below) + tied negatives
//     P    = sum m[y == c],  Q = N - P,  TP = sum m[y == c & yhat == c],  FP = sum m[y != c & yhat == c],  FN = P - TP
//
//   sm3_report_counts: out[j][k] = (A2, P, Q, TP, FP, FN) int64 for replicate r = r0 + j.  One workgroup per (replicate, label):
//                      the columns of a label share y and yhat, and the point estimate (one replicate) still fills 8 CUs.  m_r
//                      is built in LDS by resample_multiplicities (resample.h: the resampling rule; the 8 workgroups of a
//                      replicate each count the same draws: N / 4 Philox calls beside N gathers per column).  The LDS word
//                      of a case then takes y and yhat of the label beside m (m in the low 16 bits, a byte each), so a
//                      column costs ONE LDS gather per sorted position.  Per column: a workgroup prefix scan of the
//                      negatives' multiplicities into S (tile_scan; P, TP and FP fall out of the same pass, since the
//                      ranking visits every case once), then a pass over the positives for A2.
// Every sum is an integer: no order shows, no float exists.  A replicate is a function of (seed, r, N) alone.
#include "resample.h"

namespace {

constexpr int kMaxColumns = 64;            // word and S: two int32 arrays of kMaxCases in LDS, 64 KiB + 4 of the 160 KiB
constexpr int kMaxLabels = 64;

// grid (c, T); order, gs, ge [K][N]; y, yhat [N][T]; colmap [K][2] = (label, class); out [c][K][6]
__global__ void __launch_bounds__(kThreads) report_counts_kernel(const int* __restrict__ order, const int* __restrict__ gs,
                                                                 const int* __restrict__ ge, const int* __restrict__ y,
                                                                 const int* __restrict__ yhat, const int* __restrict__ colmap,
                                                                 long long* __restrict__ out, int N, int T, int K, uint32_t key0,
                                                                 uint32_t key1, uint32_t r0, int point) {
    __shared__ uint32_t word[kMaxCases];   // m | y << 16 | yhat << 24 of the workgroup's label
    __shared__ int S[kMaxCases + 1];
    __shared__ int wsum[2][kWaves];
    __shared__ long long red[kWaves][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = r0 + blockIdx.x;

    resample_multiplicities(word, N, key0, key1, r, point);

    const int t = blockIdx.y;
    for (int i = tid; i < N; i += kThreads)
        word[i] = (word[i] & 0xffffu) | (((uint32_t)y[(int64_t)i * T + t] & 0xffu) << 16) |
                  (((uint32_t)yhat[(int64_t)i * T + t] & 0xffu) << 24);
    __syncthreads();

    for (int k = 0; k < K; ++k) {
        if (colmap[2 * k] != t) continue;  // the same for the whole workgroup
        const uint32_t cls = (uint32_t)colmap[2 * k + 1] & 0xffu;
        const int* ord = order + (int64_t)k * N;
        int carry = 0, p = 0, tp = 0, fp = 0;
        for (int base = 0, it = 0; base < N; base += kTile, ++it) {
            const int j0 = base + kPer * tid;
            int v[kPer], s = 0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                v[e] = 0;
                if (j0 + e < N) {
                    const uint32_t w = word[min((uint32_t)ord[j0 + e], (uint32_t)(N - 1))];
                    const int m = (int)(w & 0xffffu);
                    const bool pos = ((w >> 16) & 0xffu) == cls, hit = (w >> 24) == cls;
                    v[e] = pos ? 0 : m;
                    p += pos ? m : 0;
                    tp += pos && hit ? m : 0;
                    fp += !pos && hit ? m : 0;
                }
                s += v[e];
            }
            int run = tile_scan(s, carry, wsum, it);
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                if (j0 + e < N) S[j0 + e] = run;
                run += v[e];
            }
        }
        if (tid == 0) S[N] = carry;
        __syncthreads();

        long long a2 = 0;
        for (int j = tid; j < N; j += kThreads) {
            const uint32_t w = word[min((uint32_t)ord[j], (uint32_t)(N - 1))];
            const int m = (int)(w & 0xffffu);
            if (((w >> 16) & 0xffu) == cls && m) {
                const int lo = min((uint32_t)gs[(int64_t)k * N + j], (uint32_t)N), hi = min((uint32_t)ge[(int64_t)k * N + j], (uint32_t)N);
                a2 += (long long)m * (S[lo] + S[hi]);
            }
        }
        a2 = wave_sum(a2), p = wave_sum(p), tp = wave_sum(tp), fp = wave_sum(fp);
        if (lane == 0) red[wave][0] = a2, red[wave][1] = p, red[wave][2] = tp, red[wave][3] = fp;
        __syncthreads();  // also: every read of S is done before the next column writes it
        if (tid == 0) {
            long long a[4] = {0, 0, 0, 0};
            for (int w = 0; w < kWaves; ++w)
                for (int e = 0; e < 4; ++e) a[e] += red[w][e];
            long long* o = out + ((int64_t)blockIdx.x * K + k) * 6;
            o[0] = a[0], o[1] = a[1], o[2] = N - a[1], o[3] = a[2], o[4] = a[3], o[5] = a[1] - a[2];
        }
        // red is next written after the next column's scan barriers, which thread 0 reaches only after the reads above
    }
}

}  // namespace

extern "C" int sm3_report_max_cases(void) { return kMaxCases; }

extern "C" int sm3_report_counts(const int* order, const int* gs, const int* ge, const int* targets, const int* yhat,
                                 const int* colmap, int64_t* out, int N, int T, int K, uint64_t seed, int64_t r0, int c, int point,
                                 void* stream) {
    if (!order || !gs || !ge || !targets || !yhat || !colmap || !out) return SM3_EINVAL;
    if (!resample_args_ok(N, r0, c, point) || T < 1 || T > kMaxLabels || K < 1 || K > kMaxColumns) return SM3_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 7) return SM3_EALIGN;
    hipLaunchKernelGGL(report_counts_kernel, dim3((uint32_t)c, (uint32_t)T), dim3(kThreads), 0, (hipStream_t)stream, order, gs, ge, targets,
                       yhat, colmap, reinterpret_cast<long long*>(out), N, T, K, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}
