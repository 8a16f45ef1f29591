// Deletion / insertion faithfulness curves of attribution maps (Petsiuk et al., RISE, BMVC 2018): the two steps around the
// encoders' eval-mode forward (sm3hip/faith.py).
//
//   sm3_faith_rank:    ranks[r][p] = #{q : map[q] > map[p]} + #{q < p : map[q] == map[p]} for `rows` independent maps of HW f32
//                      (IEEE comparisons: -0 == +0) -- descending by value, ties by ascending index, a permutation of
//                      0 .. HW - 1.  A segmented stable sort: one workgroup of 16 waves per map, a least-significant-digit radix
//                      sort of (key, index) pairs, 4 passes of 8 bits, ping-ponged through a global workspace.  key = the
//                      complement of the order-preserving uint32 of the f32 bits (knn.hip's transform) with -0 canonicalised
//                      to +0 first, so ascending keys are descending values.  In a pass every wave owns one contiguous segment
//                      of the current order: it counts its digits (integer LDS atomics: the counts do not depend on arrival
//                      order), the counts are scanned in (digit, wave) order, and the wave then walks its segment in order, 64
//                      elements at a time; a lane's slot among the lanes with its digit is the number of lower lanes in its
//                      match mask (eight ballots).  Every position is therefore a function of the input alone, and the pass is
//                      stable.  The last pass stores ranks[index] = position.
//   sm3_faith_compose: out[j][t][n][ch][p] = (ranks[n][t][p] < c_{k0 + j}) != invert ? base[n or 0][ch][p] : x[n][ch][p],
//                      c_k = (k * HW) / steps in 64-bit integers: the deletion (invert = 0) or insertion (invert = 1) inputs
//                      of curve steps k0 .. k0 + c - 1 of every label.  One thread owns 4 pixels: one 16-byte load of the
//                      ranks and of each channel of x and base, then c x 3 16-byte stores.  Pure selection: the outputs are bit
//                      copies of the inputs.
// No float arithmetic at all; no float atomics.
#include "common.h"

namespace {

constexpr int kRankThreads = 1024;
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kBatch = 4;  // loads in flight per lane in the sort's two walks
constexpr int kThreads = 256;
constexpr int64_t kMax31 = 0x7fffffffLL;

// ascending key <=> descending value; +0 and -0 share one key
__device__ __forceinline__ uint32_t rank_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}

// One pass over the 8 bits at `shift`.  kFirst: the pairs come from the map itself (index = position); kLast: the positions go
// to ranks[index] instead of the pairs to dst.  hist [kRankWaves][256] and tot [256] in LDS.
template <bool kFirst, bool kLast>
__device__ __forceinline__ void radix_pass(const float* __restrict__ map, const uint2* __restrict__ src,
                                           uint2* __restrict__ dst, int* __restrict__ ranks, int HW, int shift,
                                           uint32_t* hist, uint32_t* tot) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int seg = (HW + kRankWaves - 1) / kRankWaves;
    const int lo = min(HW, wave * seg), hi = min(HW, lo + seg);
    uint32_t* mine = hist + wave * 256;
    auto fetch = [&](int p) -> uint2 {
        if (kFirst) return make_uint2(rank_key(map[p]), (uint32_t)p);
        return src[p];
    };

    for (int i = threadIdx.x; i < kRankWaves * 256; i += kRankThreads) hist[i] = 0u;
    __syncthreads();
    // 1. this wave's digit counts
    for (int p0 = lo; p0 < hi; p0 += 64 * kBatch) {
        uint2 e[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int p = p0 + b * 64 + lane;
            if (p < hi) e[b] = fetch(p);
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b)
            if (p0 + b * 64 + lane < hi) atomicAdd(&mine[(e[b].x >> shift) & 255u], 1u);
    }
    __syncthreads();
    // 2. exclusive scan in (digit, wave) order: thread d turns the 16 counts of digit d into offsets inside the digit, thread 0
    //    scans the 256 digit totals, every entry then adds its digit's start
    if (threadIdx.x < 256) {
        uint32_t run = 0u;
        for (int w = 0; w < kRankWaves; ++w) {
            const uint32_t c = hist[w * 256 + threadIdx.x];
            hist[w * 256 + threadIdx.x] = run;
            run += c;
        }
        tot[threadIdx.x] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0u;
        for (int d = 0; d < 256; ++d) {
            const uint32_t c = tot[d];
            tot[d] = run;
            run += c;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kRankWaves * 256; i += kRankThreads) hist[i] += tot[i & 255];
    __syncthreads();
    // 3. the wave walks its segment in order; mine[d] = the next free position of digit d for this wave
    for (int p0 = lo; p0 < hi; p0 += 64 * kBatch) {
        uint2 e[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int p = p0 + b * 64 + lane;
            if (p < hi) e[b] = fetch(p);
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            if (p0 + b * 64 >= hi) break;  // wave-uniform
            const bool act = p0 + b * 64 + lane < hi;
            const uint32_t d = (e[b].x >> shift) & 255u;
            uint64_t peers = __ballot(act);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool on = (d >> bit) & 1u;
                const uint64_t m = __ballot(on);
                peers &= on ? m : ~m;
            }
            const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
            uint32_t pos = 0u;
            if (act) pos = mine[d] + below;
            __builtin_amdgcn_wave_barrier();  // every lane has read mine[d] before the group's first lane moves it on
            if (act && below == 0u) mine[d] += (uint32_t)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
            if (act && pos < (uint32_t)HW && e[b].y < (uint32_t)HW) {  // both hold by construction; a store never leaves the row
                if (kLast)
                    ranks[e[b].y] = (int)pos;
                else
                    dst[pos] = e[b];
            }
        }
    }
    // The next pass reads what this one stored.  __syncthreads() orders that at workgroup scope, which is enough while all waves
    // of a workgroup share one CU and its L1 -- the default; it would not be under threadgroup-split mode (-mtgsplit).
    __syncthreads();
}

// grid: rows; workspace: per row two buffers of HW (key, index) pairs
__global__ void __launch_bounds__(kRankThreads) faith_rank_kernel(const float* __restrict__ maps, int* __restrict__ ranks,
                                                                  uint2* __restrict__ ws, int HW) {
    __shared__ uint32_t hist[kRankWaves * 256];
    __shared__ uint32_t tot[256];
    const int64_t row = blockIdx.x;
    const float* map = maps + row * HW;
    int* out = ranks + row * HW;
    uint2* a = ws + row * 2 * (int64_t)HW;
    uint2* b = a + HW;
    radix_pass<true, false>(map, nullptr, a, nullptr, HW, 0, hist, tot);
    radix_pass<false, false>(nullptr, a, b, nullptr, HW, 8, hist, tot);
    radix_pass<false, false>(nullptr, b, a, nullptr, HW, 16, hist, tot);
    radix_pass<false, true>(nullptr, a, nullptr, out, HW, 24, hist, tot);
}

// grid (ceil(HW4 / kThreads), N * T); blockIdx.y = n * T + t
__global__ void __launch_bounds__(kThreads) faith_compose_kernel(const uint4* __restrict__ x, const uint4* __restrict__ base,
                                                                 int base_n, const int* __restrict__ ranks, int64_t stride_n,
                                                                 int64_t stride_t, uint4* __restrict__ out, int N, int T,
                                                                 int HW4, int k0, int c, int steps, int invert) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= HW4) return;
    const int n = blockIdx.y / T, t = blockIdx.y - n * T;
    const int4 r = *reinterpret_cast<const int4*>(ranks + n * stride_n + t * stride_t + 4 * (int64_t)q);
    uint4 xv[3], bv[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        xv[ch] = x[((int64_t)n * 3 + ch) * HW4 + q];
        bv[ch] = base[((int64_t)(base_n == 1 ? 0 : n) * 3 + ch) * HW4 + q];
    }
    const int64_t HW = 4 * (int64_t)HW4;
    for (int j = 0; j < c; ++j) {
        const int ck = (int)(((int64_t)(k0 + j) * HW) / steps);
        const bool s0 = (r.x < ck) != (invert != 0), s1 = (r.y < ck) != (invert != 0);
        const bool s2 = (r.z < ck) != (invert != 0), s3 = (r.w < ck) != (invert != 0);
        uint4* o = out + (((int64_t)j * T + t) * N + n) * 3 * HW4 + q;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            stg16<true>(o + (int64_t)ch * HW4, make_uint4(s0 ? bv[ch].x : xv[ch].x, s1 ? bv[ch].y : xv[ch].y,
                                                          s2 ? bv[ch].z : xv[ch].z, s3 ? bv[ch].w : xv[ch].w));
    }
}

inline bool misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}

}  // namespace

// bytes of workspace for `rows` maps of HW values (two buffers of (key, index) pairs per map); SM3_EINVAL beyond 2^31 - 1
extern "C" int sm3_faith_rank_workspace(int rows, int HW) {
    if (rows < 1 || HW < 1 || HW > (1 << 24)) return SM3_EINVAL;
    const int64_t bytes = (int64_t)rows * 2 * HW * (int64_t)sizeof(uint2);
    return bytes > kMax31 ? SM3_EINVAL : (int)bytes;
}

extern "C" int sm3_faith_rank(const float* maps, int* ranks, int rows, int HW, void* workspace, int64_t workspace_bytes,
                              void* stream) {
    if (!maps || !ranks || !workspace) return SM3_EINVAL;
    const int need = sm3_faith_rank_workspace(rows, HW);
    if (need < 0 || workspace_bytes < need) return SM3_EINVAL;
    if ((reinterpret_cast<uintptr_t>(maps) | reinterpret_cast<uintptr_t>(ranks)) & 3) return SM3_EALIGN;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return SM3_EALIGN;
    hipLaunchKernelGGL(faith_rank_kernel, dim3((uint32_t)rows), dim3(kRankThreads), 0, (hipStream_t)stream, maps, ranks,
                       reinterpret_cast<uint2*>(workspace), HW);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_faith_compose(const float* x, const float* base, int base_n, const int* ranks, int64_t rank_stride_n,
                                 int64_t rank_stride_t, float* out, int N, int T, int HW, int k0, int c, int steps, int invert,
                                 void* stream) {
    if (!x || !base || !ranks || !out || N < 1 || T < 1 || HW < 1 || c < 1 || steps < 1 || k0 < 0 ||
        (base_n != 1 && base_n != N) || (invert != 0 && invert != 1))
        return SM3_EINVAL;
    if (steps > HW || (int64_t)k0 + c > (int64_t)steps + 1 || rank_stride_n < 0 || rank_stride_t < 0) return SM3_EINVAL;
    if ((int64_t)N * T > 65535 || HW > (1 << 24)) return SM3_EINVAL;  // grid.y; every index in the kernel is 64-bit
    if (HW % 4 || rank_stride_n % 4 || rank_stride_t % 4 || misaligned(x, base, ranks, out)) return SM3_EALIGN;
    const int HW4 = HW / 4;
    const dim3 grid((uint32_t)((HW4 + kThreads - 1) / kThreads), (uint32_t)(N * T));
    hipLaunchKernelGGL(faith_compose_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(x),
                       reinterpret_cast<const uint4*>(base), base_n, ranks, rank_stride_n, rank_stride_t,
                       reinterpret_cast<uint4*>(out), N, T, HW4, k0, c, steps, invert);
    SM3_CHECK_LAUNCH();
    return 0;
}
