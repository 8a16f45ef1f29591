// Exact t-SNE of up to kMaxPoints embeddings (sm3hip/tsne.py): squared distances, conditional affinities by a
// fixed-length bisection, the symmetric P, and per iteration the pair forces and the scikit-learn update rule.  The map is a
// function of (x, settings, initial map): no float atomics, and every sum is "the fixed order" of block_fixed_sum below.
//
//   the fixed order:     thread t of a 256-thread workgroup adds the terms j = t, t + 256, ... in ascending j (fp64, from 0),
//                        then the 256 partials fold by the halving tree a[t] += a[t + h], h = 128, 64 .. 1.  A function of the
//                        terms and their number alone.
//   tsne_sqdist:         D2[i][j] = sum_k (x_ik - x_jk)^2, fp32, acc = fmaf(d, d, acc) with k ascending whatever the tiling (the
//                        zero padding of the last k tile adds fmaf(0, 0, acc) = acc); (a - b)^2 and (b - a)^2 are the same
//                        bits, so D2 is symmetric by construction; the diagonal is stored as 0.  64 x 64 outputs a workgroup.
//   tsne_affinities:     one workgroup per row, fp64.  d'_j = D2[i][j] - min_{j != i} D2[i][j]; H(beta) = log S0 + beta S1 / S0
//                        with e_j = exp(-(beta d'_j)), S0 = sum e_j, S1 = sum d'_j e_j over j != i; scikit-learn's
//                        _binary_search_perplexity from beta = 1 for exactly kSteps steps (no tolerance), then the row
//                        c_ij = e_j / S0 at the last beta.  S0 >= 1 (the nearest point has e = 1): never 0 / 0.
//   tsne_symmetrise:     P[i][j] = fp32((double(c_ij) + double(c_ji)) / (2 N)); zeros stay zeros.
//   tsne_forces:         one workgroup per point i.  Per pair in fp32: dx, dy, q = fmaf(dy, dy, fmaf(dx, dx, 1)), w = 1 / q (IEEE
//                        division) -- five roundings; then in fp64, over j != i in the fixed order: Z_i += w,
//                        A_i += (p_ij w) (dx, dy), R_i += (w w) (dx, dy).  F[i] = (Z_i, A_i.x, A_i.y, R_i.x, R_i.y).
//   tsne_update:         ONE workgroup.  Z = sum_i Z_i; g_i = 4 (e A_i - R_i / Z); gains + 0.2 where update g < 0, else x 0.8,
//                        floor 0.01; update = momentum update - lr (gains g); y += update -- all fp64 from the stored fp32
//                        state, rounded once on store.  out = (sum_i |gains g|_i^2, Z).
//   tsne_kl:             rows[i] = sum_{p_ij > 0, j != i} p_ij ((log p_ij - log w_ij) + log Z), then kl = sum_i rows[i].
//
// Floating-point contraction is off in this file: a product and a sum are two roundings unless fmaf is written, so the numpy
// restatement (tests/tsne_ref.py) states the same arithmetic.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxPoints = 16384;
constexpr int kMaxDim = 4096;
constexpr int kSteps = 100;
constexpr int kT = 256;
constexpr int kTile = 64;
constexpr int kKTile = 16;

// K sums at once in the fixed order: v[k] holds this thread's partial; the result is in every thread.  sh: K * 256 doubles.
template <int K>
__device__ __forceinline__ void block_fixed_sum(double (&v)[K], double* sh) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k * kT + t] = v[k];
    __syncthreads();
#pragma unroll
    for (int h = kT / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k * kT + t] += sh[k * kT + t + h];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[k * kT];
    __syncthreads();  // sh may be written again
}

// ---- squared distances ----------------------------------------------------------------------------------------------------
// grid (ceil(N / 64), ceil(N / 64)); thread (ty, tx) = (tid / 16, tid % 16) owns outputs (ty + 16 r, tx + 16 c), r, c < 4
__global__ void __launch_bounds__(kT) tsne_sqdist_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ d2) {
    __shared__ float xi[kTile][kKTile + 1];
    __shared__ float xj[kTile][kKTile + 1];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int k0 = 0; k0 < D; k0 += kKTile) {
        // 64 rows x 16 k = 1024 floats a side, four a thread: row e * 16 + ty, column tx
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = e * 16 + ty, k = k0 + tx;
            const bool kin = k < D;
            xi[row][tx] = (kin && i0 + row < N) ? x[(int64_t)(i0 + row) * D + k] : 0.f;
            xj[row][tx] = (kin && j0 + row < N) ? x[(int64_t)(j0 + row) * D + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kKTile; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = xi[ty + 16 * r][k];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = xj[tx + 16 * c][k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = a[r] - b[c];
                    acc[r][c] = fmaf(d, d, acc[r][c]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < N && j < N) d2[(int64_t)i * N + j] = i == j ? 0.f : acc[r][c];
        }
}

// ---- conditional affinities -----------------------------------------------------------------------------------------------
// grid N.  The row (4 N bytes, at most 64 KiB) is read again from global memory at every step: it stays in the caches, and no
// LDS is spent on it, so the occupancy is the registers'.
__global__ void __launch_bounds__(kT) tsne_affinities_kernel(const float* __restrict__ d2, int N, double log_perplexity,
                                                             float* __restrict__ cond, double* __restrict__ beta_out) {
    __shared__ double sh[2 * kT];
    const int t = threadIdx.x, i = blockIdx.x;
    const float* row = d2 + (int64_t)i * N;
    float mn = __builtin_inff();
    for (int j = t; j < N; j += kT) {
        if (j != i) mn = fminf(mn, row[j]);
    }
    // the minimum: exact in any order
    float* shf = reinterpret_cast<float*>(sh);
    shf[t] = mn;
    __syncthreads();
    for (int h = kT / 2; h > 0; h >>= 1) {
        if (t < h) shf[t] = fminf(shf[t], shf[t + h]);
        __syncthreads();
    }
    const double m = (double)shf[0];
    __syncthreads();

    double beta = 1.0, lo = -__builtin_inf(), hi = __builtin_inf();
    for (int s = 0; s <= kSteps; ++s) {  // kSteps searches, then the sums of the last beta
        double v[2] = {0.0, 0.0};
        for (int j = t; j < N; j += kT) {
            if (j == i) continue;
            const double d = (double)row[j] - m;
            const double e = exp(-(beta * d));
            v[0] += e;
            v[1] += d * e;
        }
        block_fixed_sum<2>(v, sh);
        if (s == kSteps) {
            for (int j = t; j < N; j += kT) {
                const double d = (double)row[j] - m;
                cond[(int64_t)i * N + j] = j == i ? 0.f : (float)(exp(-(beta * d)) / v[0]);
            }
            if (t == 0) beta_out[i] = beta;
            break;
        }
        const double H = log(v[0]) + beta * v[1] / v[0];
        if (H > log_perplexity) {
            lo = beta;
            beta = hi == __builtin_inf() ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -__builtin_inf() ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
}

// ---- symmetrise -----------------------------------------------------------------------------------------------------------
// grid (ceil(N / 64), ceil(N / 64)); the transposed tile goes through LDS so that both reads are row-wise
__global__ void __launch_bounds__(kT) tsne_symmetrise_kernel(const float* __restrict__ cond, int N, float* __restrict__ P) {
    __shared__ float tr[kTile][kTile + 1];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    for (int r = ty; r < kTile; r += 4) {  // tr[r][c] = cond[j0 + r][i0 + c]
        const int jj = j0 + r, ii = i0 + tx;
        tr[r][tx] = (jj < N && ii < N) ? cond[(int64_t)jj * N + ii] : 0.f;
    }
    __syncthreads();
    const double scale = (double)(2 * N);
    for (int r = ty; r < kTile; r += 4) {
        const int i = i0 + r, j = j0 + tx;
        if (i < N && j < N) P[(int64_t)i * N + j] = (float)(((double)cond[(int64_t)i * N + j] + (double)tr[tx][r]) / scale);
    }
}

// ---- forces ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pair_weight(float2 yi, float2 yj, float& dx, float& dy) {
    dx = yi.x - yj.x;
    dy = yi.y - yj.y;
    const float q = fmaf(dy, dy, fmaf(dx, dx, 1.0f));
    return __fdiv_rn(1.0f, q);
}

// grid N
__global__ void __launch_bounds__(kT) tsne_forces_kernel(const float* __restrict__ P, const float2* __restrict__ y, int N,
                                                         double* __restrict__ F) {
    __shared__ double sh[5 * kT];
    const int t = threadIdx.x, i = blockIdx.x;
    const float* p = P + (int64_t)i * N;
    const float2 yi = y[i];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = t; j < N; j += kT) {
        if (j == i) continue;
        float dx, dy;
        const double w = (double)pair_weight(yi, y[j], dx, dy);
        const double pw = (double)p[j] * w, ww = w * w;
        v[0] += w;
        v[1] += pw * (double)dx;
        v[2] += pw * (double)dy;
        v[3] += ww * (double)dx;
        v[4] += ww * (double)dy;
    }
    block_fixed_sum<5>(v, sh);
    if (t < 5) F[(int64_t)i * 5 + t] = v[t];
}

// ---- update ---------------------------------------------------------------------------------------------------------------
// sum_i F[i][0] in the fixed order
__device__ __forceinline__ double z_total(const double* __restrict__ F, int N, double* sh) {
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < N; i += kT) v[0] += F[(int64_t)i * 5];
    block_fixed_sum<1>(v, sh);
    return v[0];
}

// grid 1
__global__ void __launch_bounds__(kT) tsne_update_kernel(const double* __restrict__ F, int N, double exaggeration, double momentum,
                                                         double lr, float* __restrict__ y, float* __restrict__ upd,
                                                         float* __restrict__ gains, double* __restrict__ out) {
    __shared__ double sh[kT];
    const double Z = z_total(F, N, sh);
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < N; i += kT) {
        double sq[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int64_t e = (int64_t)i * 2 + d;
            const double g = 4.0 * (exaggeration * F[(int64_t)i * 5 + 1 + d] - F[(int64_t)i * 5 + 3 + d] / Z);
            double u = (double)upd[e], ga = (double)gains[e];
            ga = u * g < 0.0 ? ga + 0.2 : ga * 0.8;
            ga = ga < 0.01 ? 0.01 : ga;
            const double gg = ga * g;
            u = momentum * u - lr * gg;
            gains[e] = (float)ga;
            upd[e] = (float)u;
            y[e] = (float)((double)y[e] + u);
            sq[d] = gg * gg;
        }
        v[0] += sq[0] + sq[1];
    }
    block_fixed_sum<1>(v, sh);
    if (threadIdx.x == 0) {
        out[0] = v[0];
        out[1] = Z;
    }
}

// ---- KL -------------------------------------------------------------------------------------------------------------------
// grid 1: out[1] = Z
__global__ void __launch_bounds__(kT) tsne_ztotal_kernel(const double* __restrict__ F, int N, double* __restrict__ out) {
    __shared__ double sh[kT];
    const double Z = z_total(F, N, sh);
    if (threadIdx.x == 0) out[1] = Z;
}

// grid N
__global__ void __launch_bounds__(kT) tsne_kl_rows_kernel(const float* __restrict__ P, const float2* __restrict__ y, int N,
                                                          const double* __restrict__ out, double* __restrict__ rows) {
    __shared__ double sh[kT];
    const int t = threadIdx.x, i = blockIdx.x;
    const float* p = P + (int64_t)i * N;
    const float2 yi = y[i];
    const double logZ = log(out[1]);
    double v[1] = {0.0};
    for (int j = t; j < N; j += kT) {
        const float pj = p[j];
        if (j == i || !(pj > 0.f)) continue;
        float dx, dy;
        const double w = (double)pair_weight(yi, y[j], dx, dy);
        v[0] += (double)pj * ((log((double)pj) - log(w)) + logZ);
    }
    block_fixed_sum<1>(v, sh);
    if (t == 0) rows[i] = v[0];
}

// grid 1: out[0] = sum_i rows[i]
__global__ void __launch_bounds__(kT) tsne_kl_total_kernel(const double* __restrict__ rows, int N, double* __restrict__ out) {
    __shared__ double sh[kT];
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < N; i += kT) v[0] += rows[i];
    block_fixed_sum<1>(v, sh);
    if (threadIdx.x == 0) out[0] = v[0];
}

inline bool n_ok(int N) { return N >= 4 && N <= kMaxPoints; }
inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline bool finite_d(double v) { return v > -__builtin_inf() && v < __builtin_inf(); }

}  // namespace

extern "C" int sm3_tsne_max_points(void) { return kMaxPoints; }

extern "C" int sm3_tsne_sqdist(const float* x, int N, int D, float* d2, void* stream) {
    if (!x || !d2) return SM3_EINVAL;
    if (!n_ok(N) || D < 1 || D > kMaxDim) return SM3_EINVAL;
    if (misaligned(x, 3) || misaligned(d2, 3)) return SM3_EALIGN;
    const uint32_t tiles = (uint32_t)((N + kTile - 1) / kTile);
    hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(tiles, tiles), dim3(kT), 0, (hipStream_t)stream, x, N, D, d2);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_tsne_affinities(const float* d2, int N, double perplexity, float* cond, double* beta, void* stream) {
    if (!d2 || !cond || !beta || d2 == cond) return SM3_EINVAL;
    if (!n_ok(N) || !(perplexity >= 1.0) || !(perplexity <= (double)(N - 1))) return SM3_EINVAL;
    if (misaligned(d2, 3) || misaligned(cond, 3) || misaligned(beta, 7)) return SM3_EALIGN;
    hipLaunchKernelGGL(tsne_affinities_kernel, dim3((uint32_t)N), dim3(kT), 0, (hipStream_t)stream, d2, N,
                       __builtin_log(perplexity), cond, beta);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_tsne_symmetrise(const float* cond, int N, float* P, void* stream) {
    if (!cond || !P || cond == P) return SM3_EINVAL;
    if (!n_ok(N)) return SM3_EINVAL;
    if (misaligned(cond, 3) || misaligned(P, 3)) return SM3_EALIGN;
    const uint32_t tiles = (uint32_t)((N + kTile - 1) / kTile);
    hipLaunchKernelGGL(tsne_symmetrise_kernel, dim3(tiles, tiles), dim3(kT), 0, (hipStream_t)stream, cond, N, P);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_tsne_forces(const float* P, const float* y, int N, double* F, void* stream) {
    if (!P || !y || !F) return SM3_EINVAL;
    if (!n_ok(N)) return SM3_EINVAL;
    if (misaligned(P, 3) || misaligned(y, 7) || misaligned(F, 7)) return SM3_EALIGN;
    hipLaunchKernelGGL(tsne_forces_kernel, dim3((uint32_t)N), dim3(kT), 0, (hipStream_t)stream, P,
                       reinterpret_cast<const float2*>(y), N, F);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_tsne_update(const double* F, int N, double exaggeration, double momentum, double lr, float* y, float* update,
                               float* gains, double* out, void* stream) {
    if (!F || !y || !update || !gains || !out) return SM3_EINVAL;
    if (!n_ok(N) || !finite_d(exaggeration) || !finite_d(momentum) || !finite_d(lr)) return SM3_EINVAL;
    if (misaligned(F, 7) || misaligned(y, 3) || misaligned(update, 3) || misaligned(gains, 3) || misaligned(out, 7)) return SM3_EALIGN;
    hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, F, N, exaggeration, momentum, lr, y, update,
                       gains, out);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_tsne_kl(const float* P, const float* y, const double* F, int N, double* rows, double* out, void* stream) {
    if (!P || !y || !F || !rows || !out) return SM3_EINVAL;
    if (!n_ok(N)) return SM3_EINVAL;
    if (misaligned(P, 3) || misaligned(y, 7) || misaligned(F, 7) || misaligned(rows, 7) || misaligned(out, 7)) return SM3_EALIGN;
    hipLaunchKernelGGL(tsne_ztotal_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, F, N, out);
    SM3_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsne_kl_rows_kernel, dim3((uint32_t)N), dim3(kT), 0, (hipStream_t)stream, P,
                       reinterpret_cast<const float2*>(y), N, out, rows);
    SM3_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsne_kl_total_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, rows, N, out);
    SM3_CHECK_LAUNCH();
    return 0;
}
