// Operating-point report (sm3hip/operating.py): the integer counts behind average precision, the Youden and F1 optima,
// sensitivity at a specificity floor, specificity at a sensitivity floor and the counts at given thresholds of every (label,
// class) column, for the point estimate and for case-resampling bootstrap replicates.  Everything here is an integer; the
// divisions that turn counts into values happen on the host.
//
// Per column k = (label t, class c), with case multiplicities m[n] >= 0, sum m = N, over the ranking of csrc/report.hip
// (ascending, stable; order[k][j] = the case at sorted position j, gs[k][j] / ge[k][j] = first and one-past-last position of
// j's tie group):
//
//     Ppre[j] / S[j] = sum of m over the positive / negative cases at positions < j      (P = Ppre[N], Q = S[N])
//     operating points: every group start a (gs[a] == a), "positive iff score >= the group's value", and the empty point a = N:
//     TP(a) = P - Ppre[a],  FP(a) = Q - S[a]
//     APN = sum over groups of dTP * precQ,  dTP = Ppre[b] - Ppre[a],  precQ = (TP * 2^32 + den / 2) / den,  den = TP + FP at a
//           (groups with dTP = 0 contribute 0 and their quotient is never formed)
//     Youden:            the maximum of (TP * Q - FP * P, a)
//     F1:                the maximum of 2 TP / (TP + FP + P) compared by cross-multiplication, then a
//     sens at spec floor sigma: among (Q - FP) * 2^32 >= sigma * Q the maximum of (TP, -FP, a)
//     spec at sens floor rho:   among TP * 2^32 >= rho * P the maximum of (-FP, TP, a)
//     fixed:             (TP(f), FP(f)) at the given positions f
//
//   sm3_operating_counts: out[j][k] = [P, Q, APN, youden (TP, FP, a), f1 (TP, FP, a), Ls x (TP, FP, a), Lr x (TP, FP, a),
//                      Lt x (TP, FP)] int64 for replicate r = r0 + j.  One workgroup per (replicate, label), as
//                      report_counts_kernel: m_r in LDS by resample_multiplicities (resample.h: the resampling rule), the
//                      label's y packed beside it.  Per column ONE workgroup prefix scan along order (tile_scan) gives both
//                      sums: S <= 8192 in the low and Ppre <= 8192 in the high half of one 32-bit word (neither half can
//                      carry), so the LDS budget is report.hip's (two 32-bit arrays of kMaxCases: 64 KiB + 4).  Then passes
//                      over the group starts: pass 0 takes APN, Youden, F1 and the first kLv levels of both floor lists, every
//                      later pass kLv more levels of each (the default of three levels each is one pass).  Every search is the
//                      maximum of a TOTAL order -- the integer searches of one packed int64 key whose lowest field is the
//                      position -- so wave shuffles and the sum across waves give the same answer in any order.
// Every value is an integer: no order shows, no float exists.  A replicate is a function of (seed, r, N) alone.
#include "resample.h"

namespace {

constexpr int kMaxColumns = 64;
constexpr int kMaxLabels = 64;
constexpr int kMaxLevels = 32;
constexpr int kLv = 4;                     // levels of each floor list per pass
constexpr int kRed = 3 + 2 * kLv;          // APN, Youden, F1, kLv spec floors, kLv sens floors
constexpr long long kOne = 1ll << 32;

// F1 candidates (TP << 32 | D << 16 | a), D = TP + FP + P <= 2 * 8192; -1 = none.  a < b in the order (2 TP / D, a): with P > 0
// every D > 0; with P = 0 every TP = 0, both products are 0 and the position decides.
__device__ __forceinline__ bool f1_less(long long a, long long b) {
    if (b < 0) return false;
    if (a < 0) return true;
    const long long l = (a >> 32) * ((b >> 16) & 0xffff), r = (b >> 32) * ((a >> 16) & 0xffff);
    return l != r ? l < r : (a & 0xffff) < (b & 0xffff);
}

__device__ __forceinline__ long long wave_max_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ long long wave_max_f1(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o, 64);
        v = f1_less(v, u) ? u : v;
    }
    return v;
}

__device__ __forceinline__ long long clamp_level(const int64_t* lv, int l) {
    const long long v = lv[l];
    return v < 0 ? 0 : v > kOne ? kOne : v;
}

// grid (c, T); order, gs, ge [K][N]; y [N][T]; colmap [K][2] = (label, class); sigma [Ls]; rho [Lr]; fixpos [K][Lt];
// out [c][K][9 + 3 Ls + 3 Lr + 2 Lt]
__global__ void __launch_bounds__(kThreads) operating_counts_kernel(const int* __restrict__ order, const int* __restrict__ gs,
                                                                    const int* __restrict__ ge, const int* __restrict__ y,
                                                                    const int* __restrict__ colmap, const int64_t* __restrict__ sigma,
                                                                    const int64_t* __restrict__ rho, const int* __restrict__ fixpos,
                                                                    long long* __restrict__ out, int N, int T, int K, int Ls, int Lr,
                                                                    int Lt, uint32_t key0, uint32_t key1, uint32_t r0, int point) {
    __shared__ uint32_t word[kMaxCases];   // m | y << 16 of the workgroup's label
    __shared__ uint32_t PS[kMaxCases + 1]; // S | Ppre << 16
    __shared__ uint32_t wsum[2][kWaves];
    __shared__ long long red[kWaves][kRed];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = r0 + blockIdx.x;
    const int rec = 9 + 3 * (Ls + Lr) + 2 * Lt;

    resample_multiplicities(word, N, key0, key1, r, point);

    const int t = blockIdx.y;
    for (int i = tid; i < N; i += kThreads) word[i] = (word[i] & 0xffffu) | (((uint32_t)y[(int64_t)i * T + t] & 0xffu) << 16);
    __syncthreads();

    for (int k = 0; k < K; ++k) {
        if (colmap[2 * k] != t) continue;  // the same for the whole workgroup
        const uint32_t cls = (uint32_t)colmap[2 * k + 1] & 0xffu;
        const int* ord = order + (int64_t)k * N;
        const int* g0 = gs + (int64_t)k * N;
        const int* g1 = ge + (int64_t)k * N;
        long long* o = out + ((int64_t)blockIdx.x * K + k) * rec;

        // ---- the scan: PS[j] = the negatives' (low half) and the positives' (high half) multiplicities at positions < j
        uint32_t carry = 0;
        for (int base = 0, it = 0; base < N; base += kTile, ++it) {
            const int j0 = base + kPer * tid;
            uint32_t v[kPer], s = 0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                v[e] = 0;
                if (j0 + e < N) {
                    const uint32_t w = word[min((uint32_t)ord[j0 + e], (uint32_t)(N - 1))];
                    const uint32_t m = w & 0xffffu;
                    v[e] = (w >> 16) == cls ? m << 16 : m;
                }
                s += v[e];
            }
            uint32_t run = tile_scan(s, carry, wsum, it);
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                if (j0 + e < N) PS[j0 + e] = run;
                run += v[e];
            }
        }
        if (tid == 0) PS[N] = carry;
        __syncthreads();
        const int P = (int)(PS[N] >> 16), Q = (int)(PS[N] & 0xffffu);

        // ---- the passes over the operating points
        const int passes = max(1, max((Ls + kLv - 1) / kLv, (Lr + kLv - 1) / kLv));
        for (int pass = 0; pass < passes; ++pass) {
            long long lvs[kLv], lvr[kLv], bs[kLv], br[kLv];
#pragma unroll
            for (int l = 0; l < kLv; ++l) {
                const int i = kLv * pass + l;
                lvs[l] = i < Ls ? clamp_level(sigma, i) * Q : -1;   // -1: no such level
                lvr[l] = i < Lr ? clamp_level(rho, i) * P : -1;
                bs[l] = br[l] = -1;
            }
            long long apn = 0, by = -1, bf = -1;
            for (int j = tid; j <= N; j += kThreads) {
                if (j < N && g0[j] != j) continue;  // not the start of a tie group
                const uint32_t a = PS[j];
                const int tp = P - (int)(a >> 16), fp = Q - (int)(a & 0xffffu), tn = Q - fp;
                if (pass == 0) {
                    if (j < N) {
                        const int b = max(j, (int)min((uint32_t)g1[j], (uint32_t)N));
                        const int dtp = (int)(PS[b] >> 16) - (int)(a >> 16);
                        if (dtp > 0) {  // then tp >= dtp > 0: the denominator is positive
                            const uint64_t den = (uint64_t)(tp + fp);
                            apn += (long long)dtp * (long long)((((uint64_t)tp << 32) + den / 2) / den);
                        }
                    }
                    const long long ky = ((long long)(tp * Q - fp * P + (1 << 27)) << 16) | j;
                    by = ky > by ? ky : by;
                    const long long kf = ((long long)tp << 32) | ((long long)(tp + fp + P) << 16) | j;
                    bf = f1_less(bf, kf) ? kf : bf;
                }
#pragma unroll
                for (int l = 0; l < kLv; ++l) {
                    if (lvs[l] >= 0 && (long long)tn * kOne >= lvs[l]) {
                        const long long key = ((long long)tp << 32) | ((long long)tn << 16) | j;
                        bs[l] = key > bs[l] ? key : bs[l];
                    }
                    if (lvr[l] >= 0 && (long long)tp * kOne >= lvr[l]) {
                        const long long key = ((long long)tn << 32) | ((long long)tp << 16) | j;
                        br[l] = key > br[l] ? key : br[l];
                    }
                }
            }
            if (pass == 0) {
                apn = wave_sum(apn), by = wave_max_i64(by), bf = wave_max_f1(bf);
                if (lane == 0) red[wave][0] = apn, red[wave][1] = by, red[wave][2] = bf;
            }
#pragma unroll
            for (int l = 0; l < kLv; ++l) {
                const long long s = wave_max_i64(bs[l]), q = wave_max_i64(br[l]);
                if (lane == 0) red[wave][3 + l] = s, red[wave][3 + kLv + l] = q;
            }
            __syncthreads();
            if (tid == 0) {
                long long a[kRed];
                for (int e = 0; e < kRed; ++e) a[e] = red[0][e];
                for (int w = 1; w < kWaves; ++w)
                    for (int e = 0; e < kRed; ++e) {
                        const long long u = red[w][e];
                        if (e == 0) a[e] += u;
                        else if (e == 2) a[e] = f1_less(a[e], u) ? u : a[e];
                        else a[e] = u > a[e] ? u : a[e];
                    }
                // the position is the lowest field of every key.  The empty point meets every spec floor and position 0 every
                // sens floor, so a search always has a point; the clamp is for rankings that are none
                auto put = [&](long long* d, long long key) {
                    const int pos = min((int)(key & 0xffff), N);
                    d[0] = P - (int)(PS[pos] >> 16), d[1] = Q - (int)(PS[pos] & 0xffffu), d[2] = pos;
                };
                if (pass == 0) {
                    o[0] = P, o[1] = Q, o[2] = a[0];
                    put(o + 3, a[1]), put(o + 6, a[2]);
                }
                for (int l = 0; l < kLv; ++l) {
                    const int i = kLv * pass + l;
                    if (i < Ls) put(o + 9 + 3 * i, a[3 + l]);
                    if (i < Lr) put(o + 9 + 3 * Ls + 3 * i, a[3 + kLv + l]);
                }
            }
            __syncthreads();  // red is read before the next pass writes it
        }

        // ---- the fixed positions
        if (tid < Lt) {
            const uint32_t a = PS[min((uint32_t)fixpos[(int64_t)k * Lt + tid], (uint32_t)N)];
            long long* d = o + 9 + 3 * (Ls + Lr) + 2 * tid;
            d[0] = P - (int)(a >> 16), d[1] = Q - (int)(a & 0xffffu);
        }
        __syncthreads();  // every read of PS is done before the next column writes it
    }
}

}  // namespace

extern "C" int sm3_operating_max_levels(void) { return kMaxLevels; }

extern "C" int sm3_operating_counts(const int* order, const int* gs, const int* ge, const int* targets, const int* colmap,
                                    const int64_t* sigma, const int64_t* rho, const int* fixpos, int64_t* out, int N, int T, int K,
                                    int Ls, int Lr, int Lt, uint64_t seed, int64_t r0, int c, int point, void* stream) {
    if (!order || !gs || !ge || !targets || !colmap || !out) return SM3_EINVAL;
    if (!resample_args_ok(N, r0, c, point) || T < 1 || T > kMaxLabels || K < 1 || K > kMaxColumns) return SM3_EINVAL;
    if (Ls < 0 || Ls > kMaxLevels || Lr < 0 || Lr > kMaxLevels || Lt < 0 || Lt > kMaxLevels) return SM3_EINVAL;
    if ((Ls && !sigma) || (Lr && !rho) || (Lt && !fixpos)) return SM3_EINVAL;
    if ((reinterpret_cast<uintptr_t>(out) & 7) || (reinterpret_cast<uintptr_t>(sigma) & 7) || (reinterpret_cast<uintptr_t>(rho) & 7))
        return SM3_EALIGN;
    hipLaunchKernelGGL(operating_counts_kernel, dim3((uint32_t)c, (uint32_t)T), dim3(kThreads), 0, (hipStream_t)stream, order, gs, ge,
                       targets, colmap, sigma, rho, fixpos, reinterpret_cast<long long*>(out), N, T, K, Ls, Lr, Lt, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}
