// Selective-prediction report (sm3hip/selective.py, which holds the definitions in full): the integer counts behind the
// risk-coverage curve of "answer the confident cases, refer the rest", for the point estimate and for case-resampling bootstrap
// replicates.  Everything here is an integer; the divisions that turn the records into values happen on the host.
//
// Per label t the host ranks the cases ONCE, most confident first: order[t][j] = the case at sorted position j.  packed[t][n]
// holds the flags of case n: err (1) = the prediction is wrong, pos (2) = the case is of the selected class, call (4) = the
// selected class is predicted, last (8) = the case's sorted position ends a tie group of the primary key.  With multiplicities
// m[n] >= 0, sum m = N, the case at position j owns the copy ranks C_j + 1 .. C_j + m_j, C_j = the copies before j; E_j, TP_j,
// FP_j, FN_j = the error / call & pos / call & !pos / !call & pos copies before j.  table[0 .. N] = PH of the harmonic tails
// (selective.harmonic_table).  The record of a (replicate, label), 3 + 4 G + 2 H + 5 Pc int64:
//
//     A = the sum over the error positions j of table[C_j + m_j] - table[C_j];  E, P = the error and the positive copies;
//     per coverage cut k (kcuts[g], 1 .. N): err, TP, FP, FN among the first k copies -- the position that straddles k gives
//         k - C_j of its copies;
//     per risk level a / b (risks[h] = (a, b), 0 <= a <= b): the largest C_{j+1} over the positions j with `last` and C_{j+1} >=
//         1 and E_{j+1} * b <= a * C_{j+1}, and the E_{j+1} there; 0, 0 where no position qualifies;
//     per position cut p (pcuts[t][i], 0 .. N): C_p, E_p, TP_p, FP_p, FN_p (p = N: the totals).
//
//   sm3_selective_counts: one workgroup per (replicate, label).  m_r in LDS by resample_multiplicities (resample.h: the resampling
//                     rule), the flags of the case beside it (m in the low 16 bits).  ONE walk of order[t] in tiles of 1024 with
//                     two tile_scans: the copies as an int, the four event prefixes as one packed 64-bit word of 16-bit fields
//                     (every sum is at most 8192: no carry between fields).  Five prefixes of 14 bits do not fit one word, so
//                     two scans is the fewest.  The walk keeps its prefixes in registers and settles everything as it passes:
//                     each error position reads its two table entries (global, 64 KiB at the most: L2), the thread that owns
//                     the position straddling a coverage cut or standing at a position cut stores that part of the record,
//                     and a flagged position that meets a risk level raises the thread's maximum of C << 16 | E (a larger C
//                     wins, and its E rides along).  Then wave_sum / a wave maximum, the four partials through LDS, and the
//                     first threads store A, E, P, the risk cuts and the position cuts at N.
// Every sum is an integer: no order shows, no float exists.  A record is a function of (inputs, seed, r, N) alone.
#include "resample.h"

namespace {

constexpr int kLabels = 8;
constexpr int kMaxCoverages = 16;
constexpr int kMaxRisks = 8;
constexpr int kMaxCuts = 8;
constexpr uint32_t kErr = 1u, kLast = 8u;

// the event fields of a case's flags: err | TP << 16 | FP << 32 | FN << 48, each 0 or 1 (times m: the case's copies)
static __device__ __forceinline__ unsigned long long events(uint32_t f) {
    const unsigned long long err = f & 1u, pos = (f >> 1) & 1u, call = (f >> 2) & 1u;
    return err | (call & pos) << 16 | (call & (pos ^ 1ull)) << 32 | (pos & (call ^ 1ull)) << 48;
}

static __device__ __forceinline__ long long field(unsigned long long v, int e) { return (long long)((v >> (16 * e)) & 0xffffull); }

static __device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// grid (c, 8); packed, order [8][N]; table [N + 1]; kcuts [G]; pcuts [8][Pc]; risks [H][2]; out [c][8][3 + 4 G + 2 H + 5 Pc]
__global__ void __launch_bounds__(kThreads)
selective_counts_kernel(const int* __restrict__ packed, const int* __restrict__ order, const long long* __restrict__ table,
                        const int* __restrict__ kcuts, const int* __restrict__ pcuts, const int* __restrict__ risks,
                        long long* __restrict__ out, int N, int G, int H, int Pc, uint32_t key0, uint32_t key1, uint32_t r0,
                        int point) {
    __shared__ uint32_t word[kMaxCases];   // m | flags << 16
    __shared__ int kc[kMaxCoverages], pc[kMaxCuts];
    __shared__ long long ra[kMaxRisks], rb[kMaxRisks];
    __shared__ int wsum[2][kWaves];
    __shared__ unsigned long long wsum4[2][kWaves];
    __shared__ long long reda[kWaves];
    __shared__ int redb[kWaves][kMaxRisks];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = r0 + blockIdx.x;
    const int t = blockIdx.y;
    const int64_t R = 3 + 4 * G + 2 * H + 5 * Pc;
    long long* o = out + ((int64_t)blockIdx.x * kLabels + t) * R;
    long long* ocov = o + 3;
    long long* orisk = ocov + 4 * G;
    long long* ocut = orisk + 2 * H;

    resample_multiplicities(word, N, key0, key1, r, point, [&] {  // the levels, clamped to their ranges
        if (tid < G) kc[tid] = min(max(kcuts[tid], 1), N);
        if (tid < Pc) pc[tid] = min(max(pcuts[t * Pc + tid], 0), N);
        if (tid < H) {
            const int b = max(risks[2 * tid + 1], 1);
            ra[tid] = min(max(risks[2 * tid], 0), b), rb[tid] = b;
        }
    });
    for (int i = tid; i < N; i += kThreads) word[i] = (word[i] & 0xffffu) | (((uint32_t)packed[(int64_t)t * N + i] & 0xfu) << 16);
    __syncthreads();

    const int* ord = order + (int64_t)t * N;
    int carry = 0;
    unsigned long long carry4 = 0ull;
    long long a = 0;
    int best[kMaxRisks];
#pragma unroll
    for (int h = 0; h < kMaxRisks; ++h) best[h] = 0;
    for (int base = 0, it = 0; base < N; base += kTile, ++it) {
        const int j0 = base + kPer * tid;
        int mv[kPer], s = 0;
        unsigned long long ev[kPer], s4 = 0ull;
        uint32_t fl[kPer];
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            mv[e] = 0, fl[e] = 0u;
            if (j0 + e < N) {
                const uint32_t w = word[min((uint32_t)ord[j0 + e], (uint32_t)(N - 1))];
                mv[e] = (int)(w & 0xffffu), fl[e] = w >> 16;
            }
            ev[e] = events(fl[e]) * (unsigned long long)mv[e];
            s += mv[e], s4 += ev[e];
        }
        const int C0 = tile_scan(s, carry, wsum, it);              // the copies before the thread's first position
        const unsigned long long E0 = tile_scan(s4, carry4, wsum4, it);  // and the four kinds of events among them

        // ---- coverage cuts: k lies in exactly one thread's range of copies, and there in one position's
        for (int g = 0; g < G; ++g) {
            const int k = kc[g];
            if (!(C0 < k && k <= C0 + s)) continue;
            int cj = C0;
            unsigned long long ej = E0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                if (cj < k && k <= cj + mv[e]) {
                    const unsigned long long v = ej + events(fl[e]) * (unsigned long long)(k - cj);
#pragma unroll
                    for (int f = 0; f < 4; ++f) ocov[4 * g + f] = field(v, f);
                }
                cj += mv[e], ej += ev[e];
            }
        }
        // ---- position cuts below N: the prefixes at the position itself
        for (int i = 0; i < Pc; ++i) {
            const int p = pc[i];
            if (p < j0 || p >= j0 + kPer || p >= N) continue;
            int cj = C0;
            unsigned long long ej = E0;
#pragma unroll
            for (int e = 0; e < kPer; ++e)
                if (j0 + e < p) cj += mv[e], ej += ev[e];
            ocut[5 * i] = cj;
#pragma unroll
            for (int f = 0; f < 4; ++f) ocut[5 * i + 1 + f] = field(ej, f);
        }
        // ---- A over the error positions, and the risk cuts at the ends of the tie groups
        int cj = C0;
        unsigned long long ej = E0;
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            if ((fl[e] & kErr) && mv[e]) a += table[min(cj + mv[e], N)] - table[min(cj, N)];  // <= N unless order repeats a case
            cj += mv[e], ej += ev[e];
            if ((fl[e] & kLast) && cj >= 1) {
                const long long E = field(ej, 0);
#pragma unroll
                for (int h = 0; h < kMaxRisks; ++h)
                    if (h < H && E * rb[h] <= ra[h] * cj) best[h] = max(best[h], cj << 16 | (int)E);
            }
        }
    }

    a = wave_sum(a);
#pragma unroll
    for (int h = 0; h < kMaxRisks; ++h) best[h] = wave_max(best[h]);
    if (lane == 0) {
        reda[wave] = a;
#pragma unroll
        for (int h = 0; h < kMaxRisks; ++h) redb[wave][h] = best[h];
    }
    __syncthreads();
    if (tid == 0) {
        long long v = 0;
        for (int w = 0; w < kWaves; ++w) v += reda[w];
        o[0] = v, o[1] = field(carry4, 0), o[2] = field(carry4, 1) + field(carry4, 3);
    }
    if (tid < H) {
        int v = 0;
        for (int w = 0; w < kWaves; ++w) v = max(v, redb[w][tid]);
        orisk[2 * tid] = v >> 16, orisk[2 * tid + 1] = v & 0xffff;
    }
    if (tid < Pc && pc[tid] == N) {  // the totals: carry and carry4 are the same in every thread
        ocut[5 * tid] = carry;
#pragma unroll
        for (int f = 0; f < 4; ++f) ocut[5 * tid + 1 + f] = field(carry4, f);
    }
}

}  // namespace

extern "C" int sm3_selective_record(int G, int H, int Pc) { return 3 + 4 * G + 2 * H + 5 * Pc; }

extern "C" int sm3_selective_counts(const int* packed, const int* order, const int64_t* table, const int* kcuts, const int* pcuts,
                                    const int* risks, int64_t* out, int N, int G, int H, int Pc, uint64_t seed, int64_t r0, int c,
                                    int point, void* stream) {
    if (!packed || !order || !table || !kcuts || !out) return SM3_EINVAL;
    if (!resample_args_ok(N, r0, c, point)) return SM3_EINVAL;
    if (G < 1 || G > kMaxCoverages || H < 0 || H > kMaxRisks || Pc < 0 || Pc > kMaxCuts) return SM3_EINVAL;
    if ((H && !risks) || (Pc && !pcuts)) return SM3_EINVAL;
    if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 7) return SM3_EALIGN;
    hipLaunchKernelGGL(selective_counts_kernel, dim3((uint32_t)c, (uint32_t)kLabels), dim3(kThreads), 0, (hipStream_t)stream, packed,
                       order, reinterpret_cast<const long long*>(table), kcuts, pcuts, risks, reinterpret_cast<long long*>(out), N, G,
                       H, Pc, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}
