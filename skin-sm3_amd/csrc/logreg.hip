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
//   the lockstep   a second solver of the same problems by the same rules (further down): the problems of a call go through every
//   solver:        iteration side by side, the two passes over X as two products on the f64 MFMA that all problems share, the
//                  per-problem steps as kernels between them.  Its two big sums run in orders of their own, stated there.
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

// ---- the solver's steps: what the workgroup fit and the lockstep fit both run, one workgroup a problem ---------------------
// d = -H g by the two-loop recursion over the last min(count, kHist) pairs, gd = g . d.  Where that is no descent direction
// (rounding, or a NaN) the history is forgotten and d = -g; false when that is none either.
__device__ bool lbfgs_direction(const Vec& V, int64_t nvec, const double* g, double* d, const double* Sh, const double* Yh,
                                const double* rho, int& count, double& gamma, double& gd, double* sh) {
    const int t = threadIdx.x;
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
    gd = vdot(V, g, d, sh);
    if (!(gd < 0.0)) {
        count = 0;
        gamma = 1.0;
        for (int j = t; j < V.live(); j += kT) {
            const int o = V.at(j);
            d[o] = -g[o];
        }
        gd = vdot(V, g, d, sh);
        if (!(gd < 0.0)) return false;
    }
    return true;
}

// The line search on phi(alpha) = F(theta + alpha d) from the logits Z + alpha ZD; false when it finds no step.
__device__ bool line_search(const Problem& q, int N, const Vec& V, const double* th, const double* d, const double* Z,
                            const double* ZD, int count, double gd, double& alpha, double* sh) {
    double w3[3];
    wdots(V, th, d, w3, sh);  // (W.W, W.dW, dW.dW)
    double loss0, slope0;
    eval_rows(N, q.present, q.y, q.s, q.invS, Z, ZD, 0.0, nullptr, loss0, slope0, sh);
    const double phi0 = loss0 + 0.5 * q.lambda * w3[0];
    const double dphi0 = slope0 + q.lambda * w3[1];
    if (!(dphi0 < 0.0)) return false;
    alpha = count == 0 ? fmin(1.0, 1.0 / sqrt(-gd)) : 1.0;
    double lo = 0.0, dlo = dphi0, hi = __builtin_inf(), dhi = 0.0;
    const double noise = 64.0 * 2.220446049250313e-16 * fabs(phi0);
    for (int trial = 0; trial < kTrials; ++trial) {
        double loss, slope;
        eval_rows(N, q.present, q.y, q.s, q.invS, Z, ZD, alpha, nullptr, loss, slope, sh);
        const double phi = loss + 0.5 * q.lambda * (w3[0] + alpha * (2.0 * w3[1] + alpha * w3[2]));
        const double dphi = slope + q.lambda * (w3[1] + alpha * w3[2]);
        const bool finite = phi < __builtin_inf() && phi > -__builtin_inf() && dphi == dphi;
        const bool decrease = finite && (phi <= phi0 + 1e-4 * alpha * dphi0 || dphi <= 0.0 || phi <= phi0 + noise);
        if (decrease && fabs(dphi) <= 0.9 * fabs(dphi0)) return true;
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
    return false;
}

// The step: theta += alpha d, Z += alpha ZD, and the new pair's halves s = alpha d, y = -g (update_pair adds the new g).
__device__ void take_step(const Vec& V, int N, const double* __restrict__ s, double alpha, const double* d, const double* g,
                          double* th, double* Sv, double* Yv, double* Z, const double* ZD) {
    const int t = threadIdx.x;
    for (int j = t; j < V.live(); j += kT) {
        const int o = V.at(j);
        const double sv = alpha * d[o];
        Sv[o] = sv;
        th[o] += sv;
        Yv[o] = -g[o];
    }
    for (int64_t e = t; e < (int64_t)N * kC; e += kT) {
        if (s[e / kC] != 0.0) Z[e] = fma(alpha, ZD[e], Z[e]);
    }
}

// y += g at the new point; the pair enters the history if s . y > 0, else the history is forgotten (its slot is overwritten).
__device__ void update_pair(const Vec& V, const double* g, const double* Sv, double* Yv, double* rho_slot, int& count,
                            double& gamma, double* sh) {
    const int t = threadIdx.x;
    for (int j = t; j < V.live(); j += kT) {
        const int o = V.at(j);
        Yv[o] += g[o];
    }
    const double ys = vdot(V, Sv, Yv, sh);
    const double yy = vdot(V, Yv, Yv, sh);
    if (ys > 0.0 && yy > 0.0 && ys < __builtin_inf() && yy < __builtin_inf()) {
        if (t == 0) *rho_slot = 1.0 / ys;
        gamma = ys / yy;
        ++count;
    } else {
        count = 0;
        gamma = 1.0;
    }
    __syncthreads();
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
        double gd;
        if (!lbfgs_direction(V, nvec, g, d, Sh, Yh, rho, count, gamma, gd, sh)) {
            status = 2;
            break;
        }
        __syncthreads();
        pass_logits(X, 0, N, D, q.nt, d, d + (int64_t)kC * D, q.s, ZD);
        __syncthreads();

        double alpha;
        if (!line_search(q, N, V, th, d, Z, ZD, count, gd, alpha, sh)) {
            status = 2;
            break;
        }

        const int slot = count % kHist;
        double* Sv = Sh + slot * nvec;
        double* Yv = Yh + slot * nvec;
        take_step(V, N, q.s, alpha, d, g, th, Sv, Yv, Z, ZD);
        __syncthreads();

        full_eval(false);
        update_pair(V, g, Sv, Yv, rho + slot, count, gamma, sh);
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

// ---- the batched products (the lockstep solver) ------------------------------------------------------------
// The problems of a launch lie side by side as COLUMNS: column j is one (problem, class) pair, cols[j] = 8 p + c, only the
// classes c < n_t of every problem (the host builds the table).  modes [P]: 0 = the problem is not touched (none of its
// outputs is written), 1 / 2 = live, reading the first / the second operand set.  Both products run on
// v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], and of the result the four
// words reg = 0 .. 3 at [row (l >> 4) + 4 reg][col l & 15] -- not the f32 instructions' map.  A column of the instruction is
// a dot product of its own: what shares its tile, and whether a neighbour is live, changes none of its bits.  A lane loads
// four consecutive k at once (k0 + 4 (l >> 4) + j, j = 0 .. 3) and instruction j of a group takes word j, so
//   one sum runs over groups of 16 ascending and in a group over j = 0 .. 3, instruction j adding k0 + j, + 4, + 8, + 12;
// k is the feature in the logits product and the row in the gradient product.  Tails are zero operands.
//   logits:    Z[p][i][c] = sum_k X[i][k] V[p][c][k] + vb[p][c], the sum first, then the intercept.  A wave holds kLR x kLC
//              tiles (32 rows x 64 columns), a workgroup 128 rows: X is read once per 64 columns, not once per problem.
//   gradient:  G[p][c][k] = sum_i R[p][i][c] X[i][k], the rows in slabs of kSlab: slab s covers i in [s kSlab, (s + 1)
//              kSlab), its partial sums are stored plainly [slab][column][D] and a second kernel adds them in slab order
//              from slab 0.  gb[p][c] = sum_i R[p][i][c] in the fixed order.  A wave holds kGC x kGF tiles (64 columns x 32
//              features), a workgroup 128 features: X is read once per 64 columns.
typedef double double4v __attribute__((ext_vector_type(4)));
constexpr int kSlab = 2048;
constexpr int kLR = 2, kLC = 4;
constexpr int kGC = 4, kGF = 2;
constexpr int kMaxProblems = 65535;  // of one lockstep call

// The mode of column j's problem (0: beyond the table, an entry out of range, or a problem that is not live), and (p, c).
__device__ __forceinline__ int column_of(const int32_t* __restrict__ cols, int ncols, const int32_t* __restrict__ modes, int P,
                                         int j, int& p, int& c) {
    if (j >= ncols) return 0;
    const int e = cols[j];
    if (e < 0 || e >= P * kC) return 0;
    p = e >> 3;
    c = e & 7;
    return modes[p];
}

// grid (ceil(N / 128), ceil(ncols / 64)).  Operand set m (1, 2): V = Wm + p wstride + c D, vb = bm[p bstride + c] (bm may be
// null), out = Zm + p zstride + i kC + c.
__global__ void __launch_bounds__(kT) batch_logits_kernel(const float* __restrict__ X, int N, int D, const int32_t* __restrict__ cols,
                                                          int ncols, const int32_t* __restrict__ modes, int P, const double* W1,
                                                          const double* b1, double* Z1, const double* W2, const double* b2,
                                                          double* Z2, int64_t wstride, int64_t bstride, int64_t zstride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lg = lane >> 4;
    const int row0 = (blockIdx.x * (kT / 64) + wave) * 16 * kLR;
    const int col0 = blockIdx.y * 16 * kLC;
    if (row0 >= N) return;  // no barrier in this kernel
    const double* v[kLC];
    double* out[kLC];
    double bias[kLC];
    bool live[kLC], any = false;
#pragma unroll
    for (int ct = 0; ct < kLC; ++ct) {
        int p = 0, c = 0;
        const int m = column_of(cols, ncols, modes, P, col0 + ct * 16 + lc, p, c);
        v[ct] = nullptr;
        out[ct] = nullptr;
        bias[ct] = 0.0;
        if (m != 0) {
            const double* b = m == 2 ? b2 : b1;
            v[ct] = (m == 2 ? W2 : W1) + (int64_t)p * wstride + (int64_t)c * D;
            out[ct] = (m == 2 ? Z2 : Z1) + (int64_t)p * zstride + c;
            if (b) bias[ct] = b[(int64_t)p * bstride + c];
        }
        live[ct] = __ballot(m != 0) != 0;  // a tile whose problems are all done is skipped
        any = any || live[ct];
    }
    if (!any) return;
    const float* x[kLR];
#pragma unroll
    for (int rt = 0; rt < kLR; ++rt) {
        const int i = row0 + rt * 16 + lc;
        x[rt] = i < N ? X + (int64_t)i * D : nullptr;
    }
    double4v acc[kLR][kLC];
#pragma unroll
    for (int rt = 0; rt < kLR; ++rt)
#pragma unroll
        for (int ct = 0; ct < kLC; ++ct) acc[rt][ct] = double4v{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += 16) {
        const int kb = k0 + 4 * lg;
        double a[kLR][4];
#pragma unroll
        for (int rt = 0; rt < kLR; ++rt)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[rt][j] = x[rt] && kb + j < D ? (double)x[rt][kb + j] : 0.0;
#pragma unroll
        for (int ct = 0; ct < kLC; ++ct) {
            if (!live[ct]) continue;
            double b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = v[ct] && kb + j < D ? v[ct][kb + j] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < kLR; ++rt)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt][j], b[j], acc[rt][ct], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ct = 0; ct < kLC; ++ct) {
        if (!out[ct]) continue;
#pragma unroll
        for (int rt = 0; rt < kLR; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = row0 + rt * 16 + lg + 4 * r;
                if (i < N) out[ct][(int64_t)i * kC] = acc[rt][ct][r] + bias[ct];
            }
    }
}

// grid (ceil(D / 128), ceil(ncols / 64), slabs).  R^T is the A operand (R[p][i][c] at Rb + p rstride + i kC + c), X the B
// operand; part [slab][column][D].
__global__ void __launch_bounds__(kT) batch_grad_kernel(const float* __restrict__ X, int N, int D, const int32_t* __restrict__ cols,
                                                        int ncols, const int32_t* __restrict__ modes, int P, const double* Rb,
                                                        int64_t rstride, double* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lg = lane >> 4;
    const int f0 = (blockIdx.x * (kT / 64) + wave) * 16 * kGF;
    const int col0 = blockIdx.y * 16 * kGC;
    const int i_begin = blockIdx.z * kSlab, i_end = min(N, i_begin + kSlab);
    if (f0 >= D) return;  // no barrier in this kernel
    const double* r[kGC];
    bool live[kGC], any = false;
#pragma unroll
    for (int ct = 0; ct < kGC; ++ct) {
        int p = 0, c = 0;
        const int m = column_of(cols, ncols, modes, P, col0 + ct * 16 + lc, p, c);
        r[ct] = m != 0 ? Rb + (int64_t)p * rstride + c : nullptr;
        live[ct] = __ballot(m != 0) != 0;
        any = any || live[ct];
    }
    if (!any) return;
    double4v acc[kGC][kGF];
#pragma unroll
    for (int ct = 0; ct < kGC; ++ct)
#pragma unroll
        for (int ft = 0; ft < kGF; ++ft) acc[ct][ft] = double4v{0.0, 0.0, 0.0, 0.0};
    for (int i0 = i_begin; i0 < i_end; i0 += 16) {
        const int ib = i0 + 4 * lg;
        double b[kGF][4];
#pragma unroll
        for (int ft = 0; ft < kGF; ++ft) {
            const int f = f0 + ft * 16 + lc;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[ft][j] = f < D && ib + j < i_end ? (double)X[(int64_t)(ib + j) * D + f] : 0.0;
        }
#pragma unroll
        for (int ct = 0; ct < kGC; ++ct) {
            if (!live[ct]) continue;
            double a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = r[ct] && ib + j < i_end ? r[ct][(int64_t)(ib + j) * kC] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ft = 0; ft < kGF; ++ft)
                    acc[ct][ft] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], b[ft][j], acc[ct][ft], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ct = 0; ct < kGC; ++ct) {
        if (!live[ct]) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // the result's rows are columns of the table: lg + 4 q of this tile
            const int j = col0 + ct * 16 + lg + 4 * q;
            int p = 0, c = 0;
            if (column_of(cols, ncols, modes, P, j, p, c) == 0) continue;
#pragma unroll
            for (int ft = 0; ft < kGF; ++ft) {
                const int f = f0 + ft * 16 + lc;
                if (f < D) part[((int64_t)blockIdx.z * ncols + j) * D + f] = acc[ct][ft][q];
            }
        }
    }
}

// grid ncols: G[p][c][k] = part[0][j][k] + part[1][j][k] + ... at Gb + p gstride + c D + k, gb at gbb + p gbstride + c.
__global__ void __launch_bounds__(kT) batch_grad_reduce_kernel(const double* __restrict__ part, int nslab, int N, int D,
                                                               const int32_t* __restrict__ cols, int ncols,
                                                               const int32_t* __restrict__ modes, int P, const double* Rb,
                                                               int64_t rstride, double* Gb, int64_t gstride, double* gbb,
                                                               int64_t gbstride) {
    __shared__ double sh[kT];
    const int j = blockIdx.x, t = threadIdx.x;
    int p = 0, c = 0;
    if (column_of(cols, ncols, modes, P, j, p, c) == 0) return;  // the whole workgroup alike
    double* G = Gb + (int64_t)p * gstride + (int64_t)c * D;
    for (int k = t; k < D; k += kT) {
        double s = part[(int64_t)j * D + k];
        for (int sl = 1; sl < nslab; ++sl) s += part[((int64_t)sl * ncols + j) * D + k];
        G[k] = s;
    }
    const double* r = Rb + (int64_t)p * rstride + c;
    double v[1] = {0.0};
    for (int i = t; i < N; i += kT) v[0] += r[(int64_t)i * kC];
    block_fixed_sum<1>(v, sh);
    if (t == 0) gbb[(int64_t)p * gbstride + c] = v[0];
}

// ---- the lockstep fit -------------------------------------------------------------------------------------------------------
// The workgroup fit cut at its two passes over X: an iteration is four launches, and the problems of a chunk go through them
// side by side.  (1) lockstep_direction_kernel, a workgroup a problem: takes in the gradient the last iteration left (adds the
// penalty's part, F, |g|, the pair update, the convergence test), then either finishes the problem, asks for the fresh logits
// of its certificate (mode 2) or forms the next direction (mode 1).  (2) the logits product: ZD = X d (mode 1) or Z = X theta
// (mode 2).  (3) lockstep_search_kernel, a workgroup a problem: the line search and the step (mode 1), then the residuals R at
// the new Z.  (4) the gradient product and its slab sum: g = sum_i R x.  Everything a problem knows lies in its workspace
// between two launches, so the result does not depend on where the host calls are cut; a finished problem (st[0] = 2, mode 0)
// is not touched again.  The scalar rules are the functions above, the ones the workgroup fit runs.
// ws per problem: as the workgroup fit's (theta, g, d, S, Y, Z, ZD, R) and kLockState doubles of state: [0 .. 15] as kState,
// [16] what the direction kernel takes in next, [17] the loss at Z, [18] 1 if the line search found no step, [19] g . d.
constexpr int kLockState = 24;
constexpr int kMaxLockIters = 1024;  // iterations one host call may enqueue
enum { kTakeInit = 0, kTakeStep = 1, kTakeCertificate = 2 };

struct LockWs {
    double *th, *g, *d, *Sh, *Yh, *Z, *ZD, *Rr, *st;
};
__host__ __device__ inline int64_t lock_vec(int D) { return (int64_t)kC * D + kC; }
__host__ __device__ inline int64_t lock_doubles(int N, int D) {
    return (int64_t)(3 + 2 * kHist) * lock_vec(D) + 3 * (int64_t)N * kC + kLockState;
}
__device__ __forceinline__ LockWs lock_ws(double* ws, int64_t stride, int p, int N, int D) {
    const int64_t nvec = lock_vec(D);
    LockWs w;
    w.th = ws + (int64_t)p * stride;
    w.g = w.th + nvec;
    w.d = w.g + nvec;
    w.Sh = w.d + nvec;
    w.Yh = w.Sh + kHist * nvec;
    w.Z = w.Yh + kHist * nvec;
    w.ZD = w.Z + (int64_t)N * kC;
    w.Rr = w.ZD + (int64_t)N * kC;
    w.st = w.Rr + (int64_t)N * kC;
    return w;
}

__global__ void __launch_bounds__(kT) lockstep_direction_kernel(const int32_t* __restrict__ targets, const double* __restrict__ weights,
                                                                const int32_t* __restrict__ table, const double* __restrict__ Cs,
                                                                int N, int D, int R, double gtol, int max_iter, int fresh,
                                                                double* ws, int64_t stride, int32_t* modes, double* coef,
                                                                double* intercept, int32_t* info, double* res) {
    __shared__ double sh[kC * kT];
    __shared__ double rho[kHist];
    const int p = blockIdx.x, t = threadIdx.x;
    const int64_t nvec = lock_vec(D);
    const LockWs w = lock_ws(ws, stride, p, N, D);
    double* st = w.st;
    if (!fresh && st[0] == 2.0) return;  // finished: its outputs stand
    double* outW = coef + (int64_t)p * kC * D;
    double* outb = intercept + (int64_t)p * kC;
    Problem q;
    const bool ok = read_problem(targets, weights, table, Cs, N, R, p, q, sh);
    if (fresh) {
        for (int j = t; j < kC * D; j += kT) outW[j] = 0.0;
        if (t < kC) outb[t] = 0.0;
        const bool fit = ok && q.npresent >= 2;
        if (!fit && ok && t < q.nt) outb[t] = ((q.present >> t) & 1u) ? 0.0 : -__builtin_inf();
        if (fit) {
            for (int64_t j = t; j < nvec; j += kT) {
                w.th[j] = 0.0;
                w.g[j] = 0.0;
                w.d[j] = 0.0;
            }
        }
        if (t == 0) {
            info[(int64_t)p * 2] = fit ? kRunning : (ok ? 3 : 4);
            info[(int64_t)p * 2 + 1] = 0;
            res[(int64_t)p * 2] = 0.0;
            res[(int64_t)p * 2 + 1] = 0.0;
            for (int k = 0; k < kLockState; ++k) st[k] = 0.0;
            st[0] = fit ? 1.0 : 2.0;
            st[3] = 1.0;
            st[16] = (double)kTakeInit;
            modes[p] = fit ? 2 : 0;  // the first logits are those of theta = 0, formed as any fresh logits are
        }
        return;
    }
    int iter = (int)st[1], count = (int)st[2];
    double gamma = st[3], F = st[4], gn = st[5], gd = 0.0;
    const int take = (int)st[16];
    const double loss = st[17];
    const bool no_step = st[18] != 0.0;
    if (t < kHist) rho[t] = st[6 + t];
    __syncthreads();
    int status = 1;
    bool finished = false, certify = false;
    if (!ok) {  // the table changed under a running fit: nothing is followed
        status = 4;
        finished = true;
    } else if (no_step) {
        status = 2;
        finished = true;
    } else {
        const Vec V{D, q.nt};
        for (int j = t; j < q.nt * D; j += kT) w.g[j] = fma(q.lambda, w.th[j], w.g[j]);
        __syncthreads();
        double ww[3];
        wdots(V, w.th, w.th, ww, sh);
        F = loss + 0.5 * q.lambda * ww[0];
        gn = vmaxabs(V, w.g, sh);
        if (take == kTakeStep) {
            const int slot = count % kHist;
            update_pair(V, w.g, w.Sh + slot * nvec, w.Yh + slot * nvec, rho + slot, count, gamma, sh);
            ++iter;
            if (gn <= gtol) {
                certify = true;  // the gradient of the returned point, not of the running sum: fresh logits first
            } else if (!(gn == gn)) {
                status = 2;
                finished = true;
            }
        } else if (gn <= gtol) {
            status = 0;
            finished = true;
        } else if (take == kTakeCertificate && !(gn == gn)) {
            status = 2;
            finished = true;
        }
        if (!finished && !certify && iter >= max_iter) finished = true;
        if (!finished && !certify && !lbfgs_direction(V, nvec, w.g, w.d, w.Sh, w.Yh, rho, count, gamma, gd, sh)) {
            status = 2;
            finished = true;
        }
    }
    __syncthreads();
    if (finished && ok) {  // whatever the status: the last point, as the workgroup fit returns it
        for (int j = t; j < q.nt * D; j += kT) outW[j] = w.th[j];
        if (t < q.nt) outb[t] = ((q.present >> t) & 1u) ? w.th[(int64_t)kC * D + t] : -__builtin_inf();
    }
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
        st[16] = (double)(certify ? kTakeCertificate : kTakeStep);
        st[19] = gd;
        modes[p] = finished ? 0 : (certify ? 2 : 1);
    }
}

__global__ void __launch_bounds__(kT) lockstep_search_kernel(const int32_t* __restrict__ targets, const double* __restrict__ weights,
                                                             const int32_t* __restrict__ table, const double* __restrict__ Cs,
                                                             int N, int D, int R, double* ws, int64_t stride, int32_t* modes) {
    __shared__ double sh[kC * kT];
    const int p = blockIdx.x, t = threadIdx.x;
    const int m = modes[p];
    if (m == 0) return;
    Problem q;
    const bool ok = read_problem(targets, weights, table, Cs, N, R, p, q, sh);  // its barriers order the read of modes[p]
    if (!ok) return;  // the direction kernel finishes such a problem
    const LockWs w = lock_ws(ws, stride, p, N, D);
    if (m == 1) {
        const Vec V{D, q.nt};
        const int64_t nvec = lock_vec(D);
        const int count = (int)w.st[2];
        const double gd = w.st[19];
        double alpha;
        if (!line_search(q, N, V, w.th, w.d, w.Z, w.ZD, count, gd, alpha, sh)) {
            if (t == 0) {
                w.st[18] = 1.0;
                modes[p] = 0;  // no gradient of this point is wanted: the direction kernel reports status 2
            }
            return;
        }
        const int slot = count % kHist;
        take_step(V, N, q.s, alpha, w.d, w.g, w.th, w.Sh + slot * nvec, w.Yh + slot * nvec, w.Z, w.ZD);
        __syncthreads();
    }
    double loss, slope;
    eval_rows(N, q.present, q.y, q.s, q.invS, w.Z, nullptr, 0.0, w.Rr, loss, slope, sh);
    if (t == 0) w.st[17] = loss;
}

// ---- value and gradient through the two products ------------------------------------------------------------------------------
// ws per problem: Z [N][kC], R [N][kC], then the loss (2 doubles).  gW, gb are the products' outputs; the last kernel adds
// lambda W and forms F.
__host__ __device__ inline int64_t lock_vg_doubles(int N) { return 2 * (int64_t)N * kC + 2; }

__global__ void __launch_bounds__(kT) lockstep_vg_prepare_kernel(const int32_t* __restrict__ targets, const double* __restrict__ weights,
                                                                 const int32_t* __restrict__ table, const double* __restrict__ Cs,
                                                                 int N, int D, int R, int32_t* modes, double* F, double* gW,
                                                                 double* gb) {
    __shared__ double sh[kC * kT];
    const int p = blockIdx.x, t = threadIdx.x;
    Problem q;
    const bool ok = read_problem(targets, weights, table, Cs, N, R, p, q, sh);
    const bool go = ok && q.npresent > 0;
    const int nt = go ? q.nt : 0;  // the rows behind the classes, or all of them: zeros
    double* gWp = gW + (int64_t)p * kC * D;
    for (int j = nt * D + t; j < kC * D; j += kT) gWp[j] = 0.0;
    if (t >= nt && t < kC) gb[(int64_t)p * kC + t] = 0.0;
    if (t == 0) {
        modes[p] = go ? 1 : 0;
        if (!go) F[p] = ok ? 0.0 : __builtin_nan("");
    }
}

__global__ void __launch_bounds__(kT) lockstep_vg_rows_kernel(const int32_t* __restrict__ targets, const double* __restrict__ weights,
                                                              const int32_t* __restrict__ table, const double* __restrict__ Cs,
                                                              int N, int R, double* ws, int64_t stride, const int32_t* modes) {
    __shared__ double sh[kC * kT];
    const int p = blockIdx.x;
    if (modes[p] == 0) return;
    Problem q;
    if (!read_problem(targets, weights, table, Cs, N, R, p, q, sh)) return;
    double* Z = ws + (int64_t)p * stride;
    double* Rr = Z + (int64_t)N * kC;
    double loss, slope;
    eval_rows(N, q.present, q.y, q.s, q.invS, Z, nullptr, 0.0, Rr, loss, slope, sh);
    if (threadIdx.x == 0) Rr[(int64_t)N * kC] = loss;
}

__global__ void __launch_bounds__(kT) lockstep_vg_finish_kernel(const int32_t* __restrict__ targets, const double* __restrict__ weights,
                                                                const int32_t* __restrict__ table, const double* __restrict__ Cs,
                                                                const double* __restrict__ W, int N, int D, int R, const double* ws,
                                                                int64_t stride, const int32_t* modes, double* F, double* gW) {
    __shared__ double sh[kC * kT];
    const int p = blockIdx.x, t = threadIdx.x;
    if (modes[p] == 0) return;
    Problem q;
    if (!read_problem(targets, weights, table, Cs, N, R, p, q, sh)) return;
    const double* Wp = W + (int64_t)p * kC * D;
    double* gWp = gW + (int64_t)p * kC * D;
    for (int j = t; j < q.nt * D; j += kT) gWp[j] = fma(q.lambda, Wp[j], gWp[j]);
    const Vec V{D, q.nt};
    double ww[3];
    wdots(V, Wp, Wp, ww, sh);
    if (t == 0) F[p] = ws[(int64_t)p * stride + 2 * (int64_t)N * kC] + 0.5 * q.lambda * ww[0];
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

// ---- the lockstep solver's entry points -------------------------------------------------------------------------------------
namespace {

inline int slabs_of(int N) { return (N + kSlab - 1) / kSlab; }
inline bool batch_ok(int N, int D, int P, int ncols) {
    return shape_ok(N, D, P) && P <= kMaxProblems && ncols >= 1 && ncols <= P * kC;
}
inline int64_t part_doubles(int N, int D, int ncols) { return (int64_t)slabs_of(N) * ncols * D; }
inline int64_t lock_total(int N, int D, int P, int ncols, bool fit) {
    return (int64_t)P * (fit ? lock_doubles(N, D) : lock_vg_doubles(N)) + part_doubles(N, D, ncols) + (P + 1) / 2;
}

void launch_logits(const float* X, int N, int D, const int32_t* cols, int ncols, const int32_t* modes, int P, const double* W1,
                   const double* b1, double* Z1, const double* W2, const double* b2, double* Z2, int64_t wstride, int64_t bstride,
                   int64_t zstride, hipStream_t stream) {
    const dim3 grid((uint32_t)((N + 16 * kLR * (kT / 64) - 1) / (16 * kLR * (kT / 64))), (uint32_t)((ncols + 16 * kLC - 1) / (16 * kLC)));
    hipLaunchKernelGGL(batch_logits_kernel, grid, dim3(kT), 0, stream, X, N, D, cols, ncols, modes, P, W1, b1, Z1, W2, b2, Z2,
                       wstride, bstride, zstride);
}

void launch_grad(const float* X, int N, int D, const int32_t* cols, int ncols, const int32_t* modes, int P, const double* Rb,
                 int64_t rstride, double* part, double* Gb, int64_t gstride, double* gbb, int64_t gbstride, hipStream_t stream) {
    const dim3 grid((uint32_t)((D + 16 * kGF * (kT / 64) - 1) / (16 * kGF * (kT / 64))), (uint32_t)((ncols + 16 * kGC - 1) / (16 * kGC)),
                    (uint32_t)slabs_of(N));
    hipLaunchKernelGGL(batch_grad_kernel, grid, dim3(kT), 0, stream, X, N, D, cols, ncols, modes, P, Rb, rstride, part);
    hipLaunchKernelGGL(batch_grad_reduce_kernel, dim3((uint32_t)ncols), dim3(kT), 0, stream, part, slabs_of(N), N, D, cols, ncols,
                       modes, P, Rb, rstride, Gb, gstride, gbb, gbstride);
}

}  // namespace

extern "C" int sm3_logreg_lockstep_slab(void) { return kSlab; }

extern "C" int sm3_logreg_lockstep_workspace(int N, int D, int P, int ncols, int fit, int64_t* doubles) {
    if (!doubles || !batch_ok(N, D, P, ncols)) return SM3_EINVAL;
    *doubles = lock_total(N, D, P, ncols, fit != 0);
    return 0;
}

extern "C" int sm3_logreg_batch_logits(const float* X, const double* V, const double* vb, const int32_t* cols,
                                       const int32_t* active, int N, int D, int P, int ncols, double* Z, void* stream) {
    if (!X || !V || !cols || !active || !Z || !batch_ok(N, D, P, ncols)) return SM3_EINVAL;
    if (misaligned(X, 3) || misaligned(cols, 3) || misaligned(active, 3) || misaligned(V, 7) || misaligned(vb, 7) || misaligned(Z, 7))
        return SM3_EALIGN;
    launch_logits(X, N, D, cols, ncols, active, P, V, vb, Z, V, vb, Z, (int64_t)kC * D, kC, (int64_t)N * kC, (hipStream_t)stream);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_logreg_batch_grad(const float* X, const double* Rm, const int32_t* cols, const int32_t* active, int N, int D,
                                     int P, int ncols, double* ws, int64_t ws_doubles, double* G, double* gb, void* stream) {
    if (!X || !Rm || !cols || !active || !ws || !G || !gb || !batch_ok(N, D, P, ncols)) return SM3_EINVAL;
    if (ws_doubles < part_doubles(N, D, ncols)) return SM3_EINVAL;
    if (misaligned(X, 3) || misaligned(cols, 3) || misaligned(active, 3) || misaligned(Rm, 7) || misaligned(ws, 7) ||
        misaligned(G, 7) || misaligned(gb, 7))
        return SM3_EALIGN;
    launch_grad(X, N, D, cols, ncols, active, P, Rm, (int64_t)N * kC, ws, G, (int64_t)kC * D, gb, kC, (hipStream_t)stream);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_logreg_value_grad_lockstep(const float* X, const int32_t* targets, const double* weights, const int32_t* table,
                                              const double* Cs, const int32_t* cols, const double* W, const double* b, int N, int D,
                                              int R, int P, int ncols, double* ws, int64_t ws_doubles, double* F, double* gW,
                                              double* gb, void* stream) {
    if (!X || !targets || !weights || !table || !Cs || !cols || !W || !b || !ws || !F || !gW || !gb) return SM3_EINVAL;
    if (!batch_ok(N, D, P, ncols) || R < 1 || ws_doubles < lock_total(N, D, P, ncols, false)) return SM3_EINVAL;
    if (misaligned(X, 3) || misaligned(targets, 3) || misaligned(table, 3) || misaligned(cols, 3) || misaligned(weights, 7) ||
        misaligned(Cs, 7) || misaligned(W, 7) || misaligned(b, 7) || misaligned(ws, 7) || misaligned(F, 7) || misaligned(gW, 7) ||
        misaligned(gb, 7))
        return SM3_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t stride = lock_vg_doubles(N);
    double* part = ws + (int64_t)P * stride;
    int32_t* modes = reinterpret_cast<int32_t*>(part + part_doubles(N, D, ncols));
    hipLaunchKernelGGL(lockstep_vg_prepare_kernel, dim3((uint32_t)P), dim3(kT), 0, s, targets, weights, table, Cs, N, D, R, modes, F,
                       gW, gb);
    launch_logits(X, N, D, cols, ncols, modes, P, W, b, ws, W, b, ws, (int64_t)kC * D, kC, stride, s);
    hipLaunchKernelGGL(lockstep_vg_rows_kernel, dim3((uint32_t)P), dim3(kT), 0, s, targets, weights, table, Cs, N, R, ws, stride,
                       modes);
    launch_grad(X, N, D, cols, ncols, modes, P, ws + (int64_t)N * kC, stride, part, gW, (int64_t)kC * D, gb, kC, s);
    hipLaunchKernelGGL(lockstep_vg_finish_kernel, dim3((uint32_t)P), dim3(kT), 0, s, targets, weights, table, Cs, W, N, D, R, ws,
                       stride, modes, F, gW);
    SM3_CHECK_LAUNCH();
    return 0;
}

extern "C" int sm3_logreg_fit_lockstep(const float* X, const int32_t* targets, const double* weights, const int32_t* table,
                                       const double* Cs, const int32_t* cols, int N, int D, int R, int P, int ncols, double gtol,
                                       int max_iter, int resume, int iters, double* ws, int64_t ws_doubles, double* coef,
                                       double* intercept, int32_t* info, double* res, void* stream) {
    if (!X || !targets || !weights || !table || !Cs || !cols || !ws || !coef || !intercept || !info || !res) return SM3_EINVAL;
    if (!batch_ok(N, D, P, ncols) || R < 1 || ws_doubles < lock_total(N, D, P, ncols, true)) return SM3_EINVAL;
    if (!(gtol >= 0.0) || !(gtol < __builtin_inf()) || max_iter < 0 || iters < 1 || iters > kMaxLockIters ||
        (resume != 0 && resume != 1))
        return SM3_EINVAL;
    if (misaligned(X, 3) || misaligned(targets, 3) || misaligned(table, 3) || misaligned(cols, 3) || misaligned(info, 3) ||
        misaligned(weights, 7) || misaligned(Cs, 7) || misaligned(ws, 7) || misaligned(coef, 7) || misaligned(intercept, 7) ||
        misaligned(res, 7))
        return SM3_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t stride = lock_doubles(N, D), nvec = lock_vec(D), rows = (int64_t)N * kC;
    double* th = ws;
    double* g = th + nvec;
    double* d = g + nvec;
    double* Z = d + nvec + 2 * kHist * nvec;
    double* ZD = Z + rows;
    double* Rr = ZD + rows;
    double* part = ws + (int64_t)P * stride;
    int32_t* modes = reinterpret_cast<int32_t*>(part + part_doubles(N, D, ncols));
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(lockstep_direction_kernel, dim3((uint32_t)P), dim3(kT), 0, s, targets, weights, table, Cs, N, D, R, gtol,
                           max_iter, it == 0 && !resume ? 1 : 0, ws, stride, modes, coef, intercept, info, res);
        launch_logits(X, N, D, cols, ncols, modes, P, d, d + (int64_t)kC * D, ZD, th, th + (int64_t)kC * D, Z, stride, stride, stride, s);
        hipLaunchKernelGGL(lockstep_search_kernel, dim3((uint32_t)P), dim3(kT), 0, s, targets, weights, table, Cs, N, D, R, ws, stride,
                           modes);
        launch_grad(X, N, D, cols, ncols, modes, P, Rr, stride, part, g, stride, g + (int64_t)kC * D, stride, s);
    }
    SM3_CHECK_LAUNCH();
    return 0;
}
