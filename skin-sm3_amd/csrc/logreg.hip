// L2-regularised multinomial logistic regression on cached encoder features (sm3hip/logreg.py): value and
// gradient of P problems, an L-BFGS fit of P problems, and the logits of query rows under P fitted problems.
//
//   the problem:   p = (label t, C, weight row s).  With S = sum_i s_i and lambda = 1 / (C S),
//                  F(W, b) = (1 / S) sum_i s_i CE(softmax(W x_i + b), y_it) + (lambda / 2) |W|^2; b is not penalised.  A class
//                  of zero total weight leaves the softmax: its coefficient row is 0, its intercept -inf.
//   one workgroup  of 256 threads owns one problem from the first pass to the last: no problem reads what another writes, so
//   per problem:   the result of a problem is a function of (X, y_t, s, C, settings) alone -- not of the batch, of its place in
//                  it, of the chunk or of the launch.  The P workgroups of a launch read the same X, which stays in the caches.
//   arithmetic:    X is fp32 in memory and widened on load; logits, softmax, residuals, sums and all solver state are fp64.
//                  No atomics.  Every sum has one order:
//     over features (logits):   lane l of a wave adds k = l, l + 64, ... ascending (fma), the 64 lanes fold by the xor butterfly;
//     over rows (gradient):     i ascending (fma) -- a row of weight 0 has residual 0 and is skipped, which changes no bit;
//     everything else:          "the fixed order" of csrc/tsne.hip: thread t adds terms t, t + 256, ..., then the halving tree.
//   the solver:    L-BFGS, history 10, from W = 0, b = 0.  Logits are linear in the parameters: Z(theta + a d) = Z + a ZD with
//                  ZD = X d one pass over X, so a line-search trial costs O(N n_t); the gradient at the accepted point is the
//                  second pass.  The line search brackets on the slope (phi' is monotone: phi is convex) and accepts
//                  |phi'(a)| <= 0.9 |phi'(0)| together with a decrease (Armijo, or phi' <= 0, or phi within rounding of phi(0)).
//                  Before a problem is declared converged its logits are formed afresh from X and theta, so the reported
//                  gradient norm is that of the returned point and not of the running sum Z += a ZD.
//   launches:      a launch runs at most `iters` iterations of every problem and saves the solver state (kState doubles) in the
//                  workspace; the next launch (resume) goes on from it, with the same arithmetic, so the result does not depend
//                  on where the launches are cut.  The host reads the statuses between launches: a launch is bounded in time.
//   status:        0 converged (|grad|_inf <= gtol), 1 max_iter reached, 2 the line search found no step, 3 fewer than two
//                  classes of positive weight (nothing fitted), 4 a table entry out of range (nothing read).
//   Every loop is bounded (max_iter, kTrials); every branch around a barrier is taken on a value all 256 threads hold alike.
#include "common.h"

namespace {

constexpr int kMaxRows = 16384;
constexpr int kMaxDim = 4096;
constexpr int kC = 8;        // classes a problem has room for (NUM_CLASSES <= 5); the stride of every per-class array
constexpr int kLabels = 8;   // labels of a case: the row length of targets [N][kLabels]
constexpr int kT = 256;
constexpr int kState = 16;   // doubles of a problem's saved solver state: phase, iter, count, gamma, F, |g|, rho[kHist]
constexpr int kRunning = 5;  // info status of a problem whose launch ran out of its iterations: the next launch goes on
constexpr int kHist = 10;
constexpr int kTrials = 60;
constexpr int kRows = 4;     // rows a wave carries through one sweep of the features
constexpr int kCols = 4;     // features a thread carries through one sweep of the rows

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
    __syncthreads();
}

__device__ __forceinline__ double block_max(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int h = kT / 2; h > 0; h >>= 1) {
        if (t < h) sh[t] = fmax(sh[t], sh[t + h]);  // a NaN loses against a number: callers test the inputs' sums as well
        __syncthreads();
    }
    const double m = sh[0];
    __syncthreads();
    return m;
}

// A parameter vector: W [kC][D] then b [kC], kC * D + kC doubles.  Its live entries: c < nt.
struct Vec {
    int D, nt;
    __device__ __forceinline__ int live() const { return nt * D + nt; }
    __device__ __forceinline__ int at(int j) const { return j < nt * D ? j : kC * D + (j - nt * D); }
};

// out[(i - r0) * kC + c] = sum_k X[i][k] W[c][k] + b[c] for r0 <= i < r1, c < nt (0 for c >= nt).  s: the weight row, or null;
// a group of kRows rows whose weights are all 0 is left out (its logits are never read).
__device__ void pass_logits(const float* __restrict__ X, int r0, int r1, int D, int nt, const double* W, const double* b,
                            const double* s, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i0 = r0 + wave * kRows; i0 < r1; i0 += (kT / 64) * kRows) {
        if (s) {
            bool any = false;
#pragma unroll
            for (int r = 0; r < kRows; ++r) any = any || (i0 + r < r1 && s[i0 + r] != 0.0);
            if (!any) continue;
        }
        double acc[kRows][kC];
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int c = 0; c < kC; ++c) acc[r][c] = 0.0;
        for (int k = lane; k < D; k += 64) {
            double x[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) x[r] = i0 + r < r1 ? (double)X[(int64_t)(i0 + r) * D + k] : 0.0;
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                if (c < nt) {
                    const double w = W[(int64_t)c * D + k];
#pragma unroll
                    for (int r = 0; r < kRows; ++r) acc[r][c] = fma(x[r], w, acc[r][c]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                double v = acc[r][c];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0 && i0 + r < r1) out[(int64_t)(i0 + r - r0) * kC + c] = c < nt ? v + b[c] : 0.0;
            }
    }
}

// Over the rows of positive weight, with z_i = Z_i + alpha ZD_i (ZD may be null) and the softmax over the classes of `present`:
// loss = (1 / S) sum_i s_i (lse(z_i) - z_iy), slope = (1 / S) sum_i s_i sum_c (p_ic - [c = y_i]) ZD_ic, and, if Rout is given,
// Rout[i][c] = s_i (p_ic - [c = y_i]) / S (0 for a row of weight 0 and for a class that is not present).
__device__ void eval_rows(int N, unsigned present, const int32_t* __restrict__ y, const double* __restrict__ s, double invS,
                          const double* Z, const double* ZD, double alpha, double* Rout, double& loss, double& slope, double* sh) {
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < N; i += kT) {
        const double si = s[i];
        if (si == 0.0) {
            if (Rout) {
#pragma unroll
                for (int c = 0; c < kC; ++c) Rout[(int64_t)i * kC + c] = 0.0;
            }
            continue;
        }
        const int yi = y[(int64_t)i * kLabels];
        double z[kC], zd[kC], m = -__builtin_inf(), zy = 0.0;
#pragma unroll
        for (int c = 0; c < kC; ++c) {
            z[c] = 0.0;
            zd[c] = 0.0;
            if ((present >> c) & 1u) {
                z[c] = Z[(int64_t)i * kC + c];
                if (ZD) {
                    zd[c] = ZD[(int64_t)i * kC + c];
                    z[c] = fma(alpha, zd[c], z[c]);
                }
                m = fmax(m, z[c]);
                if (c == yi) zy = z[c];
            }
        }
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < kC; ++c) {
            if ((present >> c) & 1u) {
                z[c] = exp(z[c] - m);
                sum += z[c];
            }
        }
        v[0] += si * ((m + log(sum)) - zy);
        double sl = 0.0;
#pragma unroll
        for (int c = 0; c < kC; ++c) {
            double r = 0.0;
            if ((present >> c) & 1u) {
                r = si * (z[c] / sum - (c == yi ? 1.0 : 0.0));
                sl = fma(r, zd[c], sl);
            }
            if (Rout) Rout[(int64_t)i * kC + c] = r * invS;
        }
        v[1] += sl;
    }
    block_fixed_sum<2>(v, sh);
    loss = v[0] * invS;
    slope = v[1] * invS;
}

// gW[c][k] = sum_i R[i][c] X[i][k] + lambda W[c][k] (i ascending), gb[c] = sum_i R[i][c] (the fixed order); 0 for c >= nt.
__device__ void pass_grad(const float* __restrict__ X, int N, int D, int nt, const double* __restrict__ s, const double* R,
                          const double* W, double lambda, double* gW, double* gb, double* sh) {
    for (int k0 = 0; k0 < D; k0 += kCols * kT) {
        double acc[kCols][kC];
#pragma unroll
        for (int q = 0; q < kCols; ++q)
#pragma unroll
            for (int c = 0; c < kC; ++c) acc[q][c] = 0.0;
        int k[kCols];
#pragma unroll
        for (int q = 0; q < kCols; ++q) k[q] = k0 + q * kT + threadIdx.x;
        for (int i = 0; i < N; ++i) {
            if (s[i] == 0.0) continue;
            double x[kCols];
#pragma unroll
            for (int q = 0; q < kCols; ++q) x[q] = k[q] < D ? (double)X[(int64_t)i * D + k[q]] : 0.0;
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                if (c < nt) {
                    const double r = R[(int64_t)i * kC + c];
#pragma unroll
                    for (int q = 0; q < kCols; ++q) acc[q][c] = fma(r, x[q], acc[q][c]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kCols; ++q)
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                if (k[q] < D) {
                    const int64_t o = (int64_t)c * D + k[q];
                    gW[o] = c < nt ? fma(lambda, W[o], acc[q][c]) : 0.0;
                }
            }
    }
    double v[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) v[c] = 0.0;
    for (int i = threadIdx.x; i < N; i += kT) {
        if (s[i] == 0.0) continue;
#pragma unroll
        for (int c = 0; c < kC; ++c) v[c] += R[(int64_t)i * kC + c];
    }
    block_fixed_sum<kC>(v, sh);
#pragma unroll
    for (int c = 0; c < kC; ++c)
        if (threadIdx.x == c) gb[c] = c < nt ? v[c] : 0.0;
}

__device__ __forceinline__ double vdot(const Vec& V, const double* a, const double* b, double* sh) {
    double v[1] = {0.0};
    for (int j = threadIdx.x; j < V.live(); j += kT) {
        const int o = V.at(j);
        v[0] = fma(a[o], b[o], v[0]);
    }
    block_fixed_sum<1>(v, sh);
    return v[0];
}

// (a.a, a.b, b.b) over the W part alone: what the penalty needs
__device__ __forceinline__ void wdots(const Vec& V, const double* a, const double* b, double (&v)[3], double* sh) {
    v[0] = v[1] = v[2] = 0.0;
    for (int j = threadIdx.x; j < V.nt * V.D; j += kT) {
        v[0] = fma(a[j], a[j], v[0]);
        v[1] = fma(a[j], b[j], v[1]);
        v[2] = fma(b[j], b[j], v[2]);
    }
    block_fixed_sum<3>(v, sh);
}

__device__ __forceinline__ double vmaxabs(const Vec& V, const double* a, double* sh) {
    double m = 0.0;
    for (int j = threadIdx.x; j < V.live(); j += kT) {
        const double x = fabs(a[V.at(j)]);
        m = x > m || x != x ? x : m;  // a NaN stays
    }
    double nan[1] = {m != m ? 1.0 : 0.0};
    const double r = block_max(m != m ? 0.0 : m, sh);
    block_fixed_sum<1>(nan, sh);
    return nan[0] > 0.0 ? __builtin_nan("") : r;
}

struct Problem {
    int label, row, nt;
    double C, S, invS, lambda;
    unsigned present;
    int npresent;
    const int32_t* y;
    const double* s;
};

// Reads entry p of the table; false (all threads alike) when it is out of range.  Then the class weights, S and `present`.
__device__ bool read_problem(const int32_t* __restrict__ targets, const double* __restrict__ weights,
                             const int32_t* __restrict__ table, const double* __restrict__ Cs, int N, int R, int p, Problem& q,
                             double* sh) {
    q.label = table[(int64_t)p * 4];
    q.row = table[(int64_t)p * 4 + 1];
    q.nt = table[(int64_t)p * 4 + 2];
    q.C = Cs[p];
    if (q.label < 0 || q.label >= kLabels || q.row < 0 || q.row >= R || q.nt < 2 || q.nt > kC || !(q.C > 0.0) ||
        !(q.C < __builtin_inf()))
        return false;
    q.y = targets + q.label;
    q.s = weights + (int64_t)q.row * N;
    double cw[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) cw[c] = 0.0;
    for (int i = threadIdx.x; i < N; i += kT) {
        const double si = q.s[i];
        const int yi = q.y[(int64_t)i * kLabels];
#pragma unroll
        for (int c = 0; c < kC; ++c) cw[c] += yi == c ? si : 0.0;
    }
    block_fixed_sum<kC>(cw, sh);
    q.S = 0.0;
    q.present = 0u;
    q.npresent = 0;
#pragma unroll
    for (int c = 0; c < kC; ++c) {
        if (c < q.nt && cw[c] > 0.0) {
            q.S += cw[c];
            q.present |= 1u << c;
            ++q.npresent;
        }
    }
    q.invS = q.S > 0.0 ? 1.0 / q.S : 0.0;
    q.lambda = q.S > 0.0 ? 1.0 / (q.C * q.S) : 0.0;
    return true;
}

// ---- value and gradient ---------------------------------------------------------------------------------------------------
// grid P.  ws per problem: Z [N][kC], R [N][kC].
__global__ void __launch_bounds__(kT) logreg_value_grad_kernel(const float* __restrict__ X, const int32_t* __restrict__ targets,
                                                               const double* __restrict__ weights,
                                                               const int32_t* __restrict__ table, const double* __restrict__ Cs,
                                                               const double* __restrict__ W, const double* __restrict__ b, int N,
                                                               int D, int R, double* ws, int64_t stride, double* F, double* gW,
                                                               double* gb) {
    __shared__ double sh[kC * kT];
    const int p = blockIdx.x, t = threadIdx.x;
    Problem q;
    const bool ok = read_problem(targets, weights, table, Cs, N, R, p, q, sh);
    double* gWp = gW + (int64_t)p * kC * D;
    if (!ok || q.npresent == 0) {  // nothing to differentiate: zeros
        for (int j = t; j < kC * D; j += kT) gWp[j] = 0.0;
        if (t < kC) gb[(int64_t)p * kC + t] = 0.0;
        if (t == 0) F[p] = ok ? 0.0 : __builtin_nan("");
        return;
    }
    double* Z = ws + (int64_t)p * stride;
    double* Rr = Z + (int64_t)N * kC;
    const double* Wp = W + (int64_t)p * kC * D;
    // the intercept of a class that is not present may be -inf: it is not read
    __shared__ double bs[kC];
    if (t < kC) {
        const double bv = b[(int64_t)p * kC + t];
        bs[t] = ((q.present >> t) & 1u) ? bv : 0.0;
    }
    __syncthreads();
    pass_logits(X, 0, N, D, q.nt, Wp, bs, q.s, Z);
    __syncthreads();
    double loss, slope;
    eval_rows(N, q.present, q.y, q.s, q.invS, Z, nullptr, 0.0, Rr, loss, slope, sh);
    __syncthreads();
    pass_grad(X, N, D, q.nt, q.s, Rr, Wp, q.lambda, gWp, gb + (int64_t)p * kC, sh);
    const Vec V{D, q.nt};
    double ww[3];
    wdots(V, Wp, Wp, ww, sh);
    if (t == 0) F[p] = loss + 0.5 * q.lambda * ww[0];
}

// ---- the fit --------------------------------------------------------------------------------------------------------------
// grid P.  ws per problem: theta, g, d, S[kHist], Y[kHist] (vectors of kC D + kC), then Z, ZD, R [N][kC] each, then kState.
__global__ void __launch_bounds__(kT) logreg_fit_kernel(const float* __restrict__ X, const int32_t* __restrict__ targets,
                                                        const double* __restrict__ weights, const int32_t* __restrict__ table,
                                                        const double* __restrict__ Cs, int N, int D, int R, double gtol,
                                                        int max_iter, int resume, int iters, double* ws, int64_t stride, double* coef, double* intercept,
                                                        int32_t* info, double* res) {
    __shared__ double sh[kC * kT];
    __shared__ double rho[kHist];
    const int p = blockIdx.x, t = threadIdx.x;
    const int64_t nvec = (int64_t)kC * D + kC;
    double* th = ws + (int64_t)p * stride;
    double* g = th + nvec;
    double* d = g + nvec;
    double* Sh = d + nvec;
    double* Yh = Sh + kHist * nvec;
    double* Z = Yh + kHist * nvec;
    double* ZD = Z + (int64_t)N * kC;
    double* Rr = ZD + (int64_t)N * kC;
    double* st = Rr + (int64_t)N * kC;
    if (resume && st[0] == 2.0) return;  // finished in an earlier launch: its outputs stand
    double* outW = coef + (int64_t)p * kC * D;
    double* outb = intercept + (int64_t)p * kC;
    for (int j = t; j < kC * D; j += kT) outW[j] = 0.0;
    if (t < kC) outb[t] = 0.0;
    Problem q;
    const bool ok = read_problem(targets, weights, table, Cs, N, R, p, q, sh);
    if (!ok || q.npresent < 2) {
        if (ok && t < q.nt) outb[t] = ((q.present >> t) & 1u) ? 0.0 : -__builtin_inf();
        if (t == 0) {
            info[(int64_t)p * 2] = ok ? 3 : 4;
            info[(int64_t)p * 2 + 1] = 0;
            res[(int64_t)p * 2] = 0.0;
            res[(int64_t)p * 2 + 1] = 0.0;
            st[0] = 2.0;
        }
        return;
    }
    const Vec V{D, q.nt};

    double F = 0.0, gn = 0.0;
    // F, g and |g|_inf at theta; fresh: the logits from X and theta, else from the running Z
    auto full_eval = [&](bool fresh) {
        if (fresh) {
            pass_logits(X, 0, N, D, q.nt, th, th + (int64_t)kC * D, q.s, Z);
            __syncthreads();
        }
        double loss, slope;
        eval_rows(N, q.present, q.y, q.s, q.invS, Z, nullptr, 0.0, Rr, loss, slope, sh);
        __syncthreads();
        pass_grad(X, N, D, q.nt, q.s, Rr, th, q.lambda, g, g + (int64_t)kC * D, sh);
        __syncthreads();
        double ww[3];
        wdots(V, th, th, ww, sh);
        F = loss + 0.5 * q.lambda * ww[0];
        gn = vmaxabs(V, g, sh);
    };

    int status = 1, iter = 0, count = 0;
    double gamma = 1.0;
    if (!resume) {
        for (int64_t j = t; j < nvec; j += kT) {
            th[j] = 0.0;
            g[j] = 0.0;
            d[j] = 0.0;
        }
        __syncthreads();
        full_eval(true);
        if (gn <= gtol) status = 0;
    } else {  // the state the last launch saved: every thread reads the same words
        iter = (int)st[1];
        count = (int)st[2];
        gamma = st[3];
        F = st[4];
        gn = st[5];
        if (t < kHist) rho[t] = st[6 + t];
        __syncthreads();
    }
    int budget = iters;
    while (status == 1 && iter < max_iter && budget-- > 0) {
        // ---- direction: d = -H g by the two-loop recursion over the last min(count, kHist) pairs
        const int hn = count < kHist ? count : kHist;
        for (int j = t; j < V.live(); j += kT) {
            const int o = V.at(j);
            d[o] = g[o];
        }
        double a[kHist];
#pragma unroll
        for (int h = 0; h < kHist; ++h) {
            a[h] = 0.0;
            if (h < hn) {
                const int slot = (count - 1 - h) % kHist;
                const double* Sv = Sh + slot * nvec;
                const double* Yv = Yh + slot * nvec;
                a[h] = rho[slot] * vdot(V, Sv, d, sh);
                for (int j = t; j < V.live(); j += kT) {
                    const int o = V.at(j);
                    d[o] = fma(-a[h], Yv[o], d[o]);
                }
            }
        }
        for (int j = t; j < V.live(); j += kT) {
            const int o = V.at(j);
            d[o] *= gamma;
        }
#pragma unroll
        for (int h = kHist - 1; h >= 0; --h) {
            if (h < hn) {
                const int slot = (count - 1 - h) % kHist;
                const double* Sv = Sh + slot * nvec;
                const double* Yv = Yh + slot * nvec;
                const double beta = rho[slot] * vdot(V, Yv, d, sh);
                for (int j = t; j < V.live(); j += kT) {
                    const int o = V.at(j);
                    d[o] = fma(a[h] - beta, Sv[o], d[o]);
                }
            }
        }
        for (int j = t; j < V.live(); j += kT) {
            const int o = V.at(j);
            d[o] = -d[o];
        }
        double gd = vdot(V, g, d, sh);
        if (!(gd < 0.0)) {  // not a descent direction (rounding, or a NaN): forget the history, steepest descent
            count = 0;
            gamma = 1.0;
            for (int j = t; j < V.live(); j += kT) {
                const int o = V.at(j);
                d[o] = -g[o];
            }
            gd = vdot(V, g, d, sh);
            if (!(gd < 0.0)) {
                status = 2;
                break;
            }
        }
        __syncthreads();
        pass_logits(X, 0, N, D, q.nt, d, d + (int64_t)kC * D, q.s, ZD);
        __syncthreads();

        // ---- line search on phi(alpha) = F(theta + alpha d)
        double w3[3];
        wdots(V, th, d, w3, sh);  // (W.W, W.dW, dW.dW)
        double loss0, slope0;
        eval_rows(N, q.present, q.y, q.s, q.invS, Z, ZD, 0.0, nullptr, loss0, slope0, sh);
        const double phi0 = loss0 + 0.5 * q.lambda * w3[0];
        const double dphi0 = slope0 + q.lambda * w3[1];
        if (!(dphi0 < 0.0)) {
            status = 2;
            break;
        }
        double alpha = count == 0 ? fmin(1.0, 1.0 / sqrt(-gd)) : 1.0;
        double lo = 0.0, dlo = dphi0, hi = __builtin_inf(), dhi = 0.0;
        const double noise = 64.0 * 2.220446049250313e-16 * fabs(phi0);
        bool found = false;
        for (int trial = 0; trial < kTrials; ++trial) {
            double loss, slope;
            eval_rows(N, q.present, q.y, q.s, q.invS, Z, ZD, alpha, nullptr, loss, slope, sh);
            const double phi = loss + 0.5 * q.lambda * (w3[0] + alpha * (2.0 * w3[1] + alpha * w3[2]));
            const double dphi = slope + q.lambda * (w3[1] + alpha * w3[2]);
            const bool finite = phi < __builtin_inf() && phi > -__builtin_inf() && dphi == dphi;
            const bool decrease = finite && (phi <= phi0 + 1e-4 * alpha * dphi0 || dphi <= 0.0 || phi <= phi0 + noise);
            if (decrease && fabs(dphi) <= 0.9 * fabs(dphi0)) {
                found = true;
                break;
            }
            if (!finite || !decrease || dphi > 0.0) {
                hi = alpha;
                dhi = finite ? dphi : 0.0;
            } else {
                lo = alpha;
                dlo = dphi;
            }
            if (hi == __builtin_inf()) {
                alpha *= 4.0;
            } else {
                const double wdt = hi - lo;
                double next = 0.5 * (lo + hi);
                if (dhi > 0.0 && dlo < 0.0) {  // the zero of the secant of phi', kept inside the bracket
                    next = lo - dlo * wdt / (dhi - dlo);
                    next = fmin(fmax(next, lo + 0.1 * wdt), hi - 0.1 * wdt);
                }
                if (!(next > lo && next < hi)) break;  // the bracket has closed
                alpha = next;
            }
        }
        if (!found) {
            status = 2;
            break;
        }

        // ---- the step: theta += alpha d, Z += alpha ZD, the new pair (s, y)
        const int slot = count % kHist;
        double* Sv = Sh + slot * nvec;
        double* Yv = Yh + slot * nvec;
        for (int j = t; j < V.live(); j += kT) {
            const int o = V.at(j);
            const double sv = alpha * d[o];
            Sv[o] = sv;
            th[o] += sv;
            Yv[o] = -g[o];
        }
        for (int64_t e = t; e < (int64_t)N * kC; e += kT) {
            if (q.s[e / kC] != 0.0) Z[e] = fma(alpha, ZD[e], Z[e]);
        }
        __syncthreads();
        full_eval(false);
        for (int j = t; j < V.live(); j += kT) {
            const int o = V.at(j);
            Yv[o] += g[o];
        }
        const double ys = vdot(V, Sv, Yv, sh);
        const double yy = vdot(V, Yv, Yv, sh);
        if (ys > 0.0 && yy > 0.0 && ys < __builtin_inf() && yy < __builtin_inf()) {
            if (t == 0) rho[slot] = 1.0 / ys;
            gamma = ys / yy;
            ++count;
        } else {  // the pair is not usable and its slot has been overwritten: forget the history
            count = 0;
            gamma = 1.0;
        }
        __syncthreads();
        ++iter;
        if (gn <= gtol) {
            full_eval(true);  // the gradient of the returned point, not of the running sum
            if (gn <= gtol) status = 0;
        }
        if (!(gn == gn)) {
            status = 2;
            break;
        }
    }

    for (int j = t; j < q.nt * D; j += kT) outW[j] = th[j];
    if (t < q.nt) outb[t] = ((q.present >> t) & 1u) ? th[(int64_t)kC * D + t] : -__builtin_inf();
    const bool finished = status != 1 || iter >= max_iter;
    __syncthreads();
    if (t == 0) {
        info[(int64_t)p * 2] = finished ? status : kRunning;
        info[(int64_t)p * 2 + 1] = iter;
        res[(int64_t)p * 2] = F;
        res[(int64_t)p * 2 + 1] = gn;
        st[0] = finished ? 2.0 : 1.0;
        st[1] = (double)iter;
        st[2] = (double)count;
        st[3] = gamma;
        st[4] = F;
        st[5] = gn;
        for (int h = 0; h < kHist; ++h) st[6 + h] = rho[h];
    }
}

// ---- prediction -----------------------------------------------------------------------------------------------------------
// grid (ceil(Q / 16), P): logits [P][Q][kC]; nts [P] = the classes of each problem's label
__global__ void __launch_bounds__(kT) logreg_predict_kernel(const float* __restrict__ Xq, const double* __restrict__ coef,
                                                            const double* __restrict__ intercept, const int32_t* __restrict__ nts,
                                                            int Q, int D, double* logits) {
    const int p = blockIdx.y;
    const int r0 = blockIdx.x * (kT / 64) * kRows;
    const int r1 = min(Q, r0 + (kT / 64) * kRows);
    int nt = nts[p];
    nt = nt < 0 ? 0 : (nt > kC ? kC : nt);
    pass_logits(Xq, r0, r1, D, nt, coef + (int64_t)p * kC * D, intercept + (int64_t)p * kC, nullptr,
                logits + ((int64_t)p * Q + r0) * kC);
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline bool shape_ok(int N, int D, int P) { return N >= 1 && N <= kMaxRows && D >= 1 && D <= kMaxDim && P >= 1; }
inline int64_t fit_doubles(int N, int D) {
    return (int64_t)(3 + 2 * kHist) * ((int64_t)kC * D + kC) + 3 * (int64_t)N * kC + kState;
}
inline int64_t value_grad_doubles(int N) { return 2 * (int64_t)N * kC; }

}  // namespace

extern "C" int sm3_logreg_max_rows(void) { return kMaxRows; }

extern "C" int sm3_logreg_workspace(int N, int D, int fit, int64_t* doubles_per_problem) {
    if (!doubles_per_problem || !shape_ok(N, D, 1)) return SM3_EINVAL;
    *doubles_per_problem = fit ? fit_doubles(N, D) : value_grad_doubles(N);
    return 0;
}

extern "C" int sm3_logreg_check_host(const int32_t* targets, const double* weights, const int32_t* table, const double* Cs,
                                     const int32_t* n_classes, int N, int R, int P) {
    if (!targets || !weights || !table || !Cs || !n_classes) return SM3_EINVAL;
    if (N < 1 || N > kMaxRows || R < 1 || P < 1) return SM3_EINVAL;
    for (int t = 0; t < kLabels; ++t)
        if (n_classes[t] < 2 || n_classes[t] > kC) return SM3_EINVAL;
    bool used[kLabels] = {false, false, false, false, false, false, false, false};
    for (int p = 0; p < P; ++p) {
        const int32_t* e = table + (int64_t)p * 4;
        if (e[0] < 0 || e[0] >= kLabels || e[1] < 0 || e[1] >= R || e[2] != n_classes[e[0]]) return SM3_EINVAL;
        if (!(Cs[p] > 0.0) || !(Cs[p] < __builtin_inf())) return SM3_EINVAL;
        used[e[0]] = true;
    }
    for (int64_t i = 0; i < (int64_t)N; ++i)
        for (int t = 0; t < kLabels; ++t)
            if (used[t] && (targets[i * kLabels + t] < 0 || targets[i * kLabels + t] >= n_classes[t])) return SM3_EINVAL;
    for (int64_t j = 0; j < (int64_t)R * N; ++j)
        if (!(weights[j] >= 0.0) || !(weights[j] < __builtin_inf())) return SM3_EINVAL;
    return 0;
}

extern "C" int sm3_logreg_value_grad(const float* X, const int32_t* targets, const double* weights, const int32_t* table,
                                     const double* Cs, const double* W, const double* b, int N, int D, int R, int P, double* ws,
                                     int64_t ws_doubles, double* F, double* gW, double* gb, void* stream) {
    if (!X || !targets || !weights || !table || !Cs || !W || !b || !ws || !F || !gW || !gb) return SM3_EINVAL;
    if (!shape_ok(N, D, P) || R < 1 || ws_doubles < (int64_t)P * value_grad_doubles(N)) return SM3_EINVAL;
    if (misaligned(X, 3) || misaligned(targets, 3) || misaligned(table, 3) || misaligned(weights, 7) || misaligned(Cs, 7) ||
        misaligned(W, 7) || misaligned(b, 7) || misaligned(ws, 7) || misaligned(F, 7) || misaligned(gW, 7) || misaligned(gb, 7))
        return SM3_EALIGN;
    hipLaunchKernelGGL(logreg_value_grad_kernel, dim3((uint32_t)P), dim3(kT), 0, (hipStream_t)stream, X, targets, weights, table,
                       Cs, W, b, N, D, R, ws, value_grad_doubles(N), F, gW, gb);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_logreg_fit(const float* X, const int32_t* targets, const double* weights, const int32_t* table,
                              const double* Cs, int N, int D, int R, int P, double gtol, int max_iter, int resume, int iters,
                              double* ws, int64_t ws_doubles, double* coef, double* intercept, int32_t* info, double* res, void* stream) {
    if (!X || !targets || !weights || !table || !Cs || !ws || !coef || !intercept || !info || !res) return SM3_EINVAL;
    if (!shape_ok(N, D, P) || R < 1 || ws_doubles < (int64_t)P * fit_doubles(N, D)) return SM3_EINVAL;
    if (!(gtol >= 0.0) || !(gtol < __builtin_inf()) || max_iter < 0 || iters < 1 || (resume != 0 && resume != 1)) return SM3_EINVAL;
    if (misaligned(X, 3) || misaligned(targets, 3) || misaligned(table, 3) || misaligned(info, 3) || misaligned(weights, 7) ||
        misaligned(Cs, 7) || misaligned(ws, 7) || misaligned(coef, 7) || misaligned(intercept, 7) || misaligned(res, 7))
        return SM3_EALIGN;
    hipLaunchKernelGGL(logreg_fit_kernel, dim3((uint32_t)P), dim3(kT), 0, (hipStream_t)stream, X, targets, weights, table, Cs, N,
                       D, R, gtol, max_iter, resume, iters, ws, fit_doubles(N, D), coef, intercept, info, res);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_logreg_predict(const float* Xq, const double* coef, const double* intercept, const int32_t* nts, int Q, int D,
                                  int P, double* logits, void* stream) {
    if (!Xq || !coef || !intercept || !nts || !logits) return SM3_EINVAL;
    if (Q < 1 || Q > (1 << 24) || D < 1 || D > kMaxDim || P < 1 || P > 65535) return SM3_EINVAL;
    if (misaligned(Xq, 3) || misaligned(nts, 3) || misaligned(coef, 7) || misaligned(intercept, 7) || misaligned(logits, 7))
        return SM3_EALIGN;
    const uint32_t groups = (uint32_t)((Q + (kT / 64) * kRows - 1) / ((kT / 64) * kRows));
    hipLaunchKernelGGL(logreg_predict_kernel, dim3(groups, (uint32_t)P), dim3(kT), 0, (hipStream_t)stream, Xq, coef, intercept,
                       nts, Q, D, logits);
    SM3_CHECK_LAUNCH();
    return 0;
}
