// Cross-modal retrieval report (sm3hip/retrieval.py): what lies between the similarity matrix S = query . gallery^T and the
// numbers Recall@k, mean / median rank and MRR, for the point estimate and for case-resampling bootstrap replicates.
//
//   b[i][j] = 1 iff j != i and (S[i][j] > S[i][i], or S[i][j] == S[i][i] and j < i): gallery row j comes back before the
//   positive of query i (the lower index wins a tie, as in sm3_knn_vote).  Packed: bits [N][W] uint32, W = ceil(N / 32), bit
//   j & 31 of word j >> 5; the bits of j >= N are 0.  With integer case multiplicities m[n] >= 0, sum m = N, the 0-based rank is
//   rho_i = sum_j m_j b[i][j] (copies of case i are its positive, not competitors) and a replicate's record is
//       H_l = sum_i m_i [rho_i < k_l],  R = sum_i m_i rho_i,  Q = sum_i m_i floor(2^32 / (rho_i + 1)),
//       M = the least rho with 2 sum_i m_i [rho_i <= rho] >= N.
//
//   sm3_retrieval_beats:  one wave per query row.  The row is read ONCE, 64 columns a step, into LDS (N floats, sized at
//                         launch); each step's predicate goes through __ballot (64 lanes: two words of the packed row, stored
//                         by lanes 0 and 1), its popcount is the step's share of the point rank, and the row maximum rides
//                         along.  The InfoNCE term log sum_j exp(S_ij / tau) - S_ii / tau is fp64: lane l adds
//                         exp((S_ij - max) / tau) of j = l, l + 64, ... in ascending j (an order that depends on N alone),
//                         then one xor butterfly.
//   sm3_retrieval_counts: one workgroup per replicate.  m_r is built in LDS by resample_multiplicities (resample.h: the
//                         resampling rule), then split into bit-planes M_p [W] (bit j of plane p = bit p of m_j; __ballot
//                         again), P = the bits of max m, so that
//                             rho_i = sum_w sum_p 2^p popcount(bits[i][w] & M_p[w])
//                         costs W * P popcounts per row where a per-bit loop costs N multiply-adds.  A wave takes a row
//                         (lane l the words l, l + 64, ...: coalesced), rows with m_i = 0 are skipped (they weigh nothing),
//                         the lanes fold by shuffles.  This is the simplest mapping and it is UNMEASURED: for small W (the
//                         13 words of 395 cases) most lanes of the wave idle, and sub-wave groups per row may do better.
//                         H, R, Q are integer wave / workgroup sums; M comes from an integer LDS histogram of the ranks
//                         (N + 1 bins) and one workgroup scan (one shot through wred: resample.h's tile_scan would need a
//                         second row of wave totals in LDS).  No float exists in this kernel: a replicate is a function
//                         of (seed, r, N, bits) alone.
#include "resample.h"

namespace {

constexpr int kMaxWords = kMaxCases / 32;
constexpr int kMaxLevels = 8;
constexpr int kMaxPlanes = 14;   // m <= N <= 2^13

// ---- beats --------------------------------------------------------------------------------------------------------------
// grid n, one wave each; S [n][ld] (row r is query q0 + r, its positive is column q0 + r); bits [n][W], rank [n], term [n]
__global__ void __launch_bounds__(64) retrieval_beats_kernel(const float* __restrict__ S, int64_t ld, int q0, int N, double tau,
                                                             uint32_t* __restrict__ bits, int* __restrict__ rank,
                                                             double* __restrict__ term) {
    extern __shared__ float row[];  // N floats
    const int lane = threadIdx.x, r = blockIdx.x, i = q0 + r, W = (N + 31) >> 5;
    const float* s = S + (int64_t)r * ld;
    const float d = s[i];
    float mx = d;
    int rho = 0;
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        const bool in = j < N;
        const float v = in ? s[j] : d;
        if (in) row[j] = v;
        mx = fmaxf(mx, v);
        const unsigned long long mask = __ballot(in && j != i && (v > d || (v == d && j < i)));
        rho += __popcll(mask);
        const int w = (base >> 5) + lane;
        if (lane < 2 && w < W) bits[(int64_t)r * W + w] = (uint32_t)(mask >> (32 * lane));
    }
    mx = wave_max(mx);
    __syncthreads();  // one wave: orders the LDS writes before the strided reads below
    const double xm = (double)mx / tau;
    double acc = 0.0;
    for (int j = lane; j < N; j += 64) acc += exp((double)row[j] / tau - xm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) {
        rank[r] = rho;
        term[r] = (xm + log(acc)) - (double)d / tau;
    }
}

// ---- counts -------------------------------------------------------------------------------------------------------------
struct Levels {
    int k[kMaxLevels];
};

// grid c; bits [N][W]; out [c][L + 3].  One wave per row, kWaves rows in flight.
__global__ void __launch_bounds__(kThreads) retrieval_counts_kernel(const uint32_t* __restrict__ bits, long long* __restrict__ out,
                                                                    int N, Levels ks, int L, uint32_t key0, uint32_t key1,
                                                                    uint32_t r0, int point) {
    __shared__ uint32_t m[kMaxCases];
    __shared__ uint32_t plane[kMaxPlanes][kMaxWords];
    __shared__ int hist[kMaxCases + 1];
    __shared__ int wred[kWaves];
    __shared__ long long red[kWaves][kMaxLevels + 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = (N + 31) >> 5;
    const uint32_t r = r0 + blockIdx.x;

    resample_multiplicities(m, N, key0, key1, r, point, [&] {
        for (int i = tid; i <= N; i += kThreads) hist[i] = 0;
    });

    // P = the bits of max m (m <= N < 2^14), then the planes: 64 cases a wave step, one ballot per plane
    uint32_t mmax = 0;
    for (int i = tid; i < N; i += kThreads) mmax = max(mmax, m[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mmax = max(mmax, (uint32_t)__shfl_xor((int)mmax, o, 64));
    if (lane == 0) wred[wave] = (int)mmax;
    __syncthreads();
    mmax = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) mmax = max(mmax, (uint32_t)wred[w]);
    const int P = min(32 - __clz((int)mmax), kMaxPlanes);  // sum m = N >= 1: P >= 1
    for (int base = 64 * wave; base < 32 * W; base += 64 * kWaves) {
        const int j = base + lane;
        const uint32_t mj = j < N ? m[j] : 0u;
        for (int p = 0; p < P; ++p) {
            const unsigned long long mask = __ballot((mj >> p) & 1u);
            const int w = (base >> 5) + lane;
            if (lane < 2 && w < W) plane[p][w] = (uint32_t)(mask >> (32 * lane));
        }
    }
    __syncthreads();

    int h[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) h[l] = 0;
    long long R = 0, Q = 0;
    for (int i0 = 0; i0 < N; i0 += kWaves) {
        const int i = i0 + wave;
        const uint32_t mi = i < N ? m[i] : 0u;  // the same for the whole wave
        int rho = 0;
        if (mi) {
            const uint32_t* b = bits + (int64_t)i * W;
            for (int w = lane; w < W; w += 64) {
                const uint32_t x = b[w];
                for (int p = 0; p < P; ++p) rho += __popc(x & plane[p][w]) << p;
            }
        }
        rho = wave_sum(rho);
        if (mi && lane == 0) {
            rho = min(rho, N);  // planes are 0 past N, so this holds already: the bin index cannot leave hist whatever bits holds
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l) h[l] += (l < L && rho < ks.k[l]) ? (int)mi : 0;
            R += (long long)mi * rho;
            Q += (long long)mi * (long long)(0x100000000ull / (uint32_t)(rho + 1));
            atomicAdd(&hist[rho], (int)mi);
        }
    }
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) h[l] = wave_sum(h[l]);
    R = wave_sum(R), Q = wave_sum(Q);
    if (lane == 0) {
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) red[wave][l] = h[l];
        red[wave][kMaxLevels] = R, red[wave][kMaxLevels + 1] = Q;
    }
    __syncthreads();  // also: the histogram is complete
    long long* o = out + (int64_t)blockIdx.x * (L + 3);
    if (tid < L + 2) {
        const int e = tid < L ? tid : kMaxLevels + (tid - L);
        long long a = 0;
        for (int w = 0; w < kWaves; ++w) a += red[w][e];
        o[tid] = a;
    }

    // the lower weighted median: thread t owns bins [t * per, (t + 1) * per), a workgroup scan of the owners' sums finds the
    // one owner whose bins take the running count from below N / 2 to at least N / 2
    const int per = (N + kThreads) / kThreads, b0 = tid * per, b1 = min(b0 + per, N + 1);
    int own = 0;
    for (int b = b0; b < b1; ++b) own += hist[b];
    int incl = own;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int u = __shfl_up(incl, s, 64);
        if (lane >= s) incl += u;
    }
    if (lane == 63) wred[wave] = incl;  // its earlier reads (max m) lie before the planes' barrier
    __syncthreads();
    int before = incl - own;
    for (int w = 0; w < wave; ++w) before += wred[w];
    if (2 * before < N && 2 * (before + own) >= N) {
        int cum = before, b = b0;
        for (; b < b1; ++b) {
            cum += hist[b];
            if (2 * cum >= N) break;
        }
        o[L + 2] = b;
    }
}

}  // namespace

extern "C" int sm3_retrieval_beats(const float* S, int64_t ld, int n, int q0, int N, double tau, uint32_t* bits, int32_t* rank,
                                   double* term, void* stream) {
    if (!S || !bits || !rank || !term) return SM3_EINVAL;
    if (N < 1 || N > kMaxCases || n < 1 || q0 < 0 || (int64_t)q0 + n > N || ld < N) return SM3_EINVAL;
    if (!(tau > 0.0) || !(tau < __builtin_inf())) return SM3_EINVAL;
    if ((reinterpret_cast<uintptr_t>(S) & 3) || (reinterpret_cast<uintptr_t>(bits) & 3) || (reinterpret_cast<uintptr_t>(rank) & 3) ||
        (reinterpret_cast<uintptr_t>(term) & 7))
        return SM3_EALIGN;
    hipLaunchKernelGGL(retrieval_beats_kernel, dim3((uint32_t)n), dim3(64), (size_t)N * sizeof(float), (hipStream_t)stream, S, ld,
                       q0, N, tau, bits, rank, term);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_retrieval_counts(const uint32_t* bits, int N, const int32_t* ks, int L, int64_t* out, uint64_t seed, int64_t r0,
                                    int c, int point, void* stream) {
    if (!bits || !ks || !out) return SM3_EINVAL;
    if (!resample_args_ok(N, r0, c, point) || L < 1 || L > kMaxLevels) return SM3_EINVAL;
    Levels lv;
    for (int l = 0; l < kMaxLevels; ++l) {
        lv.k[l] = l < L ? ks[l] : 0;
        if (l < L && (ks[l] < 1 || ks[l] > kMaxCases)) return SM3_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(bits) & 3) || (reinterpret_cast<uintptr_t>(out) & 7)) return SM3_EALIGN;
    hipLaunchKernelGGL(retrieval_counts_kernel, dim3((uint32_t)c), dim3(kThreads), 0, (hipStream_t)stream, bits,
                       reinterpret_cast<long long*>(out), N, lv, L, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}
