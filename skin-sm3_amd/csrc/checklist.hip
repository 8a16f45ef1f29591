// Seven-point checklist report (sm3hip/checklist.py): the integer counts behind "melanoma by checklist score", for the point
// estimate and for case-resampling bootstrap replicates.  Everything here is an integer; the divisions that turn counts into
// values happen on the host.
//
// Per case n the host packs shat | sstar << 4 | mel << 8 into one int32: shat / sstar = the checklist score (0 .. 10) of the
// predicted / the annotated criteria, mel = the case is a melanoma.  With case multiplicities m[n] >= 0, sum m = N:
//
//     J[shat][sstar][mel] = sum of m over the cases with that triple                     (11 x 11 x 2 = 242 entries)
//     and for each of three continuous rankings k (ascending, stable; order[k][j] = the case at sorted position j, gs[k][j] /
//     ge[k][j] = first and one-past-last position of j's tie group), with "positive" = melanoma, as csrc/report.hip:
//     S[j] = sum of m over the negatives at positions < j,  A2 = sum over positive j of m_j * (S[gs[j]] + S[ge[j]]),
//     P = sum of m over the positives,  Q = N - P.
//
//   sm3_checklist_counts: out[j] = [J (242), 3 x (A2, P, Q)] int64 for replicate r = r0 + j.  A record has four parts: part 0
//                      the joint table, parts 1 .. 3 the rankings.  The grid is (c, 4), one workgroup per (replicate, part),
//                      while that is at most kSplitSlots workgroups, that is up to 256 replicates a launch: the point
//                      estimate and a short launch then take the time of the longest part, not of the four in turn.  Beyond
//                      it is (c, 1), one workgroup per replicate doing the four parts in turn: the chip is full either way
//                      and m_r is built once per replicate, not four times.  Both write the same integers.  m_r in LDS by
//                      resample_multiplicities (resample.h: the resampling rule), the packed word of the case beside it (m in
//                      the low 16 bits).  The table: one private 242-bin histogram per wave, filled by integer LDS atomics,
//                      merged after a barrier.  A ranking: report.hip's workgroup prefix scan (tile_scan) of the negatives'
//                      multiplicities into S, then a pass over the positives for A2.
// Every sum is an integer: no order shows, no float exists.  A replicate is a function of (seed, r, N) alone.
#include "resample.h"

namespace {

constexpr int kScores = 11;                      // score values 0 .. 10
constexpr int kBins = kScores * kScores * 2;     // 242
constexpr int kRankings = 3;
constexpr int kParts = 1 + kRankings;
constexpr int kRecord = kBins + 3 * kRankings;   // 251
// measured: (c, 4) is ahead up to c = 256, (c, 1) from c = 512.  -DSM3_CHECKLIST_SPLIT_SLOTS=0 / =1099511627776
// forces one grid for tools/checklist_bench.py --grid-sweep; the library is built without it.
#ifndef SM3_CHECKLIST_SPLIT_SLOTS
#define SM3_CHECKLIST_SPLIT_SLOTS 1024
#endif
constexpr int64_t kSplitSlots = SM3_CHECKLIST_SPLIT_SLOTS;

// grid (c, 4) or (c, 1); packed [N]; order, gs, ge [3][N]; out [c][251]
__global__ void __launch_bounds__(kThreads) checklist_counts_kernel(const int* __restrict__ packed, const int* __restrict__ order,
                                                                    const int* __restrict__ gs, const int* __restrict__ ge,
                                                                    long long* __restrict__ out, int N, uint32_t key0, uint32_t key1,
                                                                    uint32_t r0, int point) {
    __shared__ uint32_t word[kMaxCases];   // m | packed << 16
    __shared__ int S[kMaxCases + 1];
    __shared__ int hist[kWaves][kBins];
    __shared__ int wsum[2][kWaves];
    __shared__ long long red[kWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = r0 + blockIdx.x;
    long long* o = out + (int64_t)blockIdx.x * kRecord;

    resample_multiplicities(word, N, key0, key1, r, point, [&] {  // the zeroes matter to the workgroup that does part 0 alone
        for (int b = tid; b < kWaves * kBins; b += kThreads) (&hist[0][0])[b] = 0;
    });
    for (int i = tid; i < N; i += kThreads) word[i] = (word[i] & 0xffffu) | (((uint32_t)packed[i] & 0x1ffu) << 16);
    __syncthreads();

    for (int part = blockIdx.y; part < kParts; part += gridDim.y) {  // the same for the whole workgroup
        if (part == 0) {
            // ---- the joint table
            for (int i = tid; i < N; i += kThreads) {
                const uint32_t w = word[i];
                const int m = (int)(w & 0xffffu);
                const int sh = min((int)((w >> 16) & 0xfu), kScores - 1), st = min((int)((w >> 20) & 0xfu), kScores - 1);
                if (m) atomicAdd(&hist[wave][(sh * kScores + st) * 2 + (int)((w >> 24) & 1u)], m);
            }
            __syncthreads();
            for (int b = tid; b < kBins; b += kThreads) {
                long long a = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) a += hist[w][b];
                o[b] = a;
            }
            continue;
        }
        // ---- a ranking: S[j] = the negatives' multiplicities at positions < j, then A2 over the positives
        const int k = part - 1;
        const int* ord = order + (int64_t)k * N;
        int carry = 0, p = 0;
        for (int base = 0, it = 0; base < N; base += kTile, ++it) {
            const int j0 = base + kPer * tid;
            int v[kPer], s = 0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                v[e] = 0;
                if (j0 + e < N) {
                    const uint32_t w = word[min((uint32_t)ord[j0 + e], (uint32_t)(N - 1))];
                    const int m = (int)(w & 0xffffu);
                    const bool pos = (w >> 24) & 1u;
                    v[e] = pos ? 0 : m;
                    p += pos ? m : 0;
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
            if (((w >> 24) & 1u) && m) {
                const int lo = min((uint32_t)gs[(int64_t)k * N + j], (uint32_t)N), hi = min((uint32_t)ge[(int64_t)k * N + j], (uint32_t)N);
                a2 += (long long)m * (S[lo] + S[hi]);
            }
        }
        a2 = wave_sum(a2), p = wave_sum(p);
        if (lane == 0) red[wave][0] = a2, red[wave][1] = p;
        __syncthreads();  // also: every read of S is done before the next ranking writes it
        if (tid == 0) {
            long long a[2] = {0, 0};
            for (int w = 0; w < kWaves; ++w)
                for (int e = 0; e < 2; ++e) a[e] += red[w][e];
            long long* d = o + kBins + 3 * k;
            d[0] = a[0], d[1] = a[1], d[2] = N - a[1];
        }
        // red is next written after the next ranking's scan barriers, which thread 0 reaches only after the reads above
    }
}

}  // namespace

extern "C" int sm3_checklist_record(void) { return kRecord; }

extern "C" int sm3_checklist_counts(const int* packed, const int* order, const int* gs, const int* ge, int64_t* out, int N,
                                    uint64_t seed, int64_t r0, int c, int point, void* stream) {
    if (!packed || !order || !gs || !ge || !out) return SM3_EINVAL;
    if (!resample_args_ok(N, r0, c, point)) return SM3_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 7) return SM3_EALIGN;
    const uint32_t parts = (int64_t)c * kParts <= kSplitSlots ? kParts : 1;
    hipLaunchKernelGGL(checklist_counts_kernel, dim3((uint32_t)c, parts), dim3(kThreads), 0, (hipStream_t)stream, packed, order, gs, ge,
                       reinterpret_cast<long long*>(out), N, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)r0, point ? 1 : 0);
    SM3_CHECK_LAUNCH();
    return 0;
}
