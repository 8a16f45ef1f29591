/*
 * sm3_hip.h -- C ABI of libsm3hip.so: the MI355X (gfx950) kernels of the SM3 pre-training hot path.
 *
 * The reference (Dylan-H-Wang/skin-sm3) is pure Python and has no FFI of its own: every entry point
 * below replaces the ATen/cuDNN/cuBLAS work behind one call site of the reference, cited as
 * file:line under /root/reference.  The library has no PyTorch types in its signatures: device
 * pointers, sizes, a hipStream_t passed as void*.  All tensors are dense; activations are NHWC
 * ("rows x channels", channels contiguous), weights are [Cout][taps][Cin] (= the memory order of a
 * torch channels_last OIHW tensor).  `dtype` selects the storage/MFMA type of activations and
 * weight copies: SM3_F32 (exact-f32 MFMA, parity mode), SM3_BF16 or SM3_F16 (16-bit MFMA, fp32 accumulate; SM3_F16
 * needs the caller's loss scaling: sm3_loss_scale_update).
 * Statistics, master weights, gradients of weights and optimizer state are always fp32 (BN sums fp64).
 *
 * Every function returns 0 on success, a positive hipError_t on a runtime failure, or a negative
 * SM3_E* code on a rejected argument; nothing is launched when an argument is rejected.
 * Nothing here allocates, frees or synchronises: safe to capture into a hipGraph.
 */
#ifndef SM3_HIP_H
#define SM3_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SM3_F32 0
#define SM3_BF16 1
#define SM3_F16 2   /* IEEE half storage + f16 MFMA, fp32 accumulate: the reference's AMP type (backbone_train.py:27,98) */

#define SM3_EINVAL (-1)   /* bad size / null pointer */
#define SM3_EALIGN (-2)   /* channel count not a multiple of the kernel's K chunk */
#define SM3_EDTYPE (-3)

#define SM3_MAX_TAPS 9

/* ABI version, bumped on any signature change. */
int sm3_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Gather-GEMM convolution: forward conv, data-gradient of a conv, and bias-free Linear.
 *   replaces nn.Conv2d forward/backward-data  (src/models/resnet.py:49-67 conv3x3/conv1x1, used at
 *   :144-148,:260; the 7x7 stem :208-210 runs on sm3_stem_conv_fwd straight from the images in all three arithmetic
 *   modes) and nn.Linear(bias=False)
 *   (src/models/simclr.py:17-27).
 *
 *   y[n, oy*osy+ooy, ox*osx+oox, co] = sum_t sum_ci x[n, oy*sy+dy[t], ox*sx+dx[t], ci]
 *                                                 * w[co*w_row_stride + wtap[t]*Ci + ci]   (+ addend)
 *   for (n,oy,ox) in N x Ho x Wo; out-of-range x reads are zero.  Ci must be a multiple of
 *   128 bytes / sizeof(T) (64 bf16 / 32 f32).
 * ------------------------------------------------------------------------------------------ */
typedef struct sm3_conv_desc {
    int32_t dtype;
    int32_t N, Hi, Wi, Ci;          /* x: [N,Hi,Wi,Ci] */
    int32_t Ho, Wo, Co;             /* iteration space and GEMM-N */
    int32_t sy, sx;
    int32_t ntaps;
    int32_t dy[SM3_MAX_TAPS], dx[SM3_MAX_TAPS], wtap[SM3_MAX_TAPS];
    int32_t w_row_stride;           /* elements between rows (co) of w */
    int32_t Hout, Wout;             /* y: [N,Hout,Wout,Co] */
    int32_t osy, osx, ooy, oox;
} sm3_conv_desc;

/* number of [2][Co] fp32 partial-statistics rows sm3_conv_gather_gemm writes for this desc */
int sm3_conv_partial_rows(const sm3_conv_desc* d);

/* stat_partials (nullable): [partial_rows][2][Co] fp32 -- per-row-block sum and sum of squares of
 * the stored (rounded) outputs, for train-mode BatchNorm (resnet.py:145-149,211,261).
 * addend (nullable): same indexing as y, added in the epilogue (may alias y). */
int sm3_conv_gather_gemm(const sm3_conv_desc* d, const void* x, const void* w, void* y,
                         const void* addend, float* stat_partials, void* stream);

/* Data-gradient launch with the FIRST phase of the next BatchNorm backward fused into its epilogue.  The
 * gather-GEMM result (+addend) is dy of a BatchNorm output y = relu?(bn(x)); instead of storing dy this stores
 * dz = dy * (y > 0) (relu_mask NULL: no ReLU) and writes per-row-block partial sums of (dz, dz * xhat) for the
 * channels of y -- exactly what sm3_bn_bwd_reduce would produce from a second pass over dy, y and x.
 * partials: [partial_row_offset + sm3_conv_partial_rows(d)][2][Co]; parity launches of a stride-2 gradient use
 * consecutive row offsets.  x / relu_mask are indexed like dz_out. */
typedef struct sm3_bn_bwd_fuse {
    const uint8_t* relu_mask;
    const void* x;
    const float* mean;           /* [views][Co] */
    const float* invstd;         /* [views][Co] */
    float* partials;
    int32_t partial_row_offset;  /* first partial row of view 0's tiles */
    int32_t views;               /* 0 or 1: one BatchNorm batch.  2: the launch covers two views back to back (rows
                                  * [0, M/2) and [M/2, M), M/2 a multiple of 128), each with its own mean / invstd ... */
    int32_t partial_row_offset_view1; /* ... and view 1's tiles write their partial rows from here */
    int32_t addend_sp_h, addend_sp_w; /* > 0: `addend` is a COMPACT [N, addend_sp_h, addend_sp_w, Co] tensor holding values for
                                  * the even (y, x) output positions only (= (Ho+1)/2 x (Wo+1)/2) and zero elsewhere: the data
                                  * gradient of a Bottleneck's stride-2 1x1 downsample convolution (resnet.py:260), joined with
                                  * conv1's data gradient here instead of by a second pass over the block-input gradient */
} sm3_bn_bwd_fuse;
int sm3_conv_dgrad_bnfuse(const sm3_conv_desc* d, const void* dy_in, const void* w_dgrad, void* dz_out,
                          const void* addend, const sm3_bn_bwd_fuse* fuse, void* stream);
/* fuse->x == NULL (with mean / invstd then unused): the epilogue applies the ReLU mask and sums dz only -- the
 * sum(dz * xhat) slot of every partial row is written as 0.  For a producer BatchNorm whose backward goes through
 * sm3_linbn_stats, which derives that sum from the weight-gradient product instead of a read of x. */

/* The same launch over TWO K segments: dz_out = mask( x0 w0^T + x1 w1^T + col_bias (+ addend) ), for a 1x1 / stride-1
 * descriptor d (x0: [pixels][d->Ci], w0: [d->Co][d->w_row_stride]) and a second operand pair over the same pixels.
 * With x0 = dz of an expanding conv's BatchNorm, w0 = diag(a) W, x1 = that conv's input, w1 = -H, col_bias = const
 * (sm3_linbn_coeffs, sm3_conv_gather_gemm) this is the data gradient of conv -> BatchNorm with the BatchNorm-backward
 * apply pass folded into the GEMM by linearity (see "BatchNorm backward by linearity" below).  16-bit dtypes only.
 * Two views in one launch (fuse->views == 2): view 1's tiles read w0 + w_view_stride, w1 + w1_view_stride (elements)
 * and col_bias + Co. */
typedef struct sm3_conv_seg {
    const void* x1;            /* [pixels][Ci1] */
    const void* w1;            /* [views][Co][Ci1] */
    int32_t Ci1;               /* multiple of 64 */
    int64_t w_view_stride;     /* elements between the views' w0 banks (0: shared) */
    int64_t w1_view_stride;
    const float* col_bias;     /* [views][Co], nullable */
    int32_t views;             /* sm3_conv_gather_gemm_seg only (0 / 1: one view; 2: two views back to back, each a multiple
                                * of 128 rows); sm3_conv_dgrad_seg_bnfuse takes the views from its fuse argument */
} sm3_conv_seg;
int sm3_conv_dgrad_seg_bnfuse(const sm3_conv_desc* d, const void* x0, const void* w0, const sm3_conv_seg* seg,
                              void* dz_out, const void* addend, const sm3_bn_bwd_fuse* fuse, void* stream);
/* The two-segment product alone, y = x0 w0^T + x1 w1^T + col_bias (+ addend): the data gradient of an expanding conv ->
 * BatchNorm pair whose result has no producer BatchNorm to prepare (a Bottleneck's downsample branch: the compact
 * gradient that the block's conv1 data gradient then takes as its sparse addend). */
int sm3_conv_gather_gemm_seg(const sm3_conv_desc* d, const void* x0, const void* w0, const sm3_conv_seg* seg, void* y,
                             const void* addend, void* stream);
/* ... and with a ReLU (+ its bits) on the sum: y = relu?(x0 w0^T + x1 w1^T + col_bias).  With the two BatchNorm scales
 * folded into the banks and the shifts into col_bias (sm3_linbn_scale_banks) this is the WHOLE join of a Bottleneck that has
 * a downsample branch -- conv3, bn3, the 1x1 downsample convolution, its BatchNorm, the add and the ReLU
 * (resnet.py:162-172) -- in one launch, neither pre-BatchNorm tensor stored. */
int sm3_conv_seg_act(const sm3_conv_desc* d, const void* x0, const void* w0, const sm3_conv_seg* seg, int relu, void* y,
                     uint8_t* relu_mask, void* stream);

/* Inference: conv + eval-mode BatchNorm (+ residual) (+ ReLU) in one launch,
 *   y = relu?( conv(x, w) * scale[co] + shift[co] (+ residual) ),
 * scale/shift from sm3_bn_eval_scale_shift.  Replaces the conv->bn->(add)->relu chains of Bottleneck.forward
 * (src/models/resnet.py:154-174) under model.eval(): frozen-encoder feature extraction (simclr.py:393-396,
 * tools/backbone_eval.py --finetune fc, inference.py) never writes or re-reads a pre-BN tensor. */
int sm3_conv_bn_act_eval(const sm3_conv_desc* d, const void* x, const void* w, const float* scale,
                         const float* shift, const void* residual, int relu, void* y, void* stream);
/* The train-mode form: scale / shift are [views][Co] (a launch over two views back to back, each a multiple of 128 rows,
 * uses view v's vectors for view v's rows) and relu_mask (nullable, with relu) receives the ReLU bits of y as sm3_bn_act
 * writes them.  With scale / shift from sm3_linbn_fwd_stats + sm3_bn_finalize this is conv3 -> bn3 -> (+identity) -> ReLU
 * of a Bottleneck (resnet.py:162-172) in ONE launch: the pre-BatchNorm tensor is never written.  Dense outputs only. */
int sm3_conv_bn_act_fused(const sm3_conv_desc* d, const void* x, const void* w, const float* scale, const float* shift,
                          const void* residual, int relu, void* y, uint8_t* relu_mask, int views, void* stream);
/* Same launch with scale/shift derived in the epilogue from the BatchNorm's own tensors,
 *   scale = gamma / sqrt(running_var + eps),  shift = beta - running_mean * scale      (gamma/beta NULL: 1 / 0),
 * bit-identical to sm3_bn_eval_scale_shift followed by sm3_conv_bn_act_eval, without the 53 small launches per encoder
 * pass that computing the vectors first costs (nn.BatchNorm2d.forward in eval mode, src/models/resnet.py:156-169). */
int sm3_conv_bn_eval(const sm3_conv_desc* d, const void* x, const void* w, const float* gamma, const float* beta,
                     const float* running_mean, const float* running_var, float eps, const void* residual, int relu,
                     void* y, void* stream);

/* Weight gradient of the forward conv described by d (autograd of the same call sites):
 *   dw[co*w_row_stride + wtap[t]*Ci + ci] += sum_{n,oy,ox} dy[(n,oy,ox), co] * x[n, oy*sy+dy[t], ox*sx+dx[t], ci]
 * dy is dense [N*Ho*Wo, Co]; dw is fp32 and is accumulated into (float atomics, split over pixels: run-to-run
 * differences of 1 ulp; sm3_conv_wgrad_det below is the fixed-order form).
 * Columns wtap[t]*Ci+ci >= w_row_stride are dropped (a zero-padded K tail). */
int sm3_conv_wgrad(const sm3_conv_desc* d, const void* x, const void* dy, float* dw, void* stream);
/* The same product over `views` equal pixel ranges that accumulate into dw + v * dw_view_stride (per-view weight-gradient
 * products: P_v = dz_v^T x_v, or with dy = x the Gram matrix G_v = x_v^T x_v), and optionally with dY the channel
 * concatenation [dy (d->Co) | dy1 (Co1)] of two tensors over the same pixels (rows of the second part accumulate into
 * dw1 + v * dw1_view_stride; d->Co then a multiple of 128).  Co1 = 0: dy1 / dw1 unused. */
int sm3_conv_wgrad_cat(const sm3_conv_desc* d, const void* x, const void* dy, float* dw, const void* dy1, int Co1,
                       float* dw1, int views, int64_t dw_view_stride, int64_t dw1_view_stride, void* stream);
/* The same product WITHOUT atomics (plain-store split-K): slice j of view v of the pixel axis stores its whole
 * [Co][taps * Ci] partial product into slabs + (v * *slabs_used + j) * Co * taps * Ci; the caller adds the slabs up in a
 * fixed order (sm3_linbn_moments, sm3_linbn_stats / sm3_linbn_post): deterministic, and at these sizes faster than
 * ~1.3 TB/s of float atomics.  *slabs_used <= slab_capacity slabs per view (host int, written before return); a view is cut
 * the same way whether the launch holds one view or two. */
int sm3_conv_wgrad_slabs(const sm3_conv_desc* d, const void* x, const void* dy, float* slabs, int slab_capacity, int views,
                         int* slabs_used, void* stream);
/* out[e] = (accumulate ? out[e] : 0) + sum_j slabs[j * n + e], j ascending on a fixed tree that depends on (nslabs, e)
 * only; n a multiple of 4, both pointers 16-byte aligned.  The fixed-order sum behind every split-K product of the
 * training step (ABI 8). */
int sm3_slab_reduce(const float* slabs, int nslabs, int64_t n, float* out, int accumulate, void* stream);
/* sm3_conv_wgrad as a FUNCTION OF ITS INPUTS (ABI 8; what the training step uses): the pixel slices store plain slabs
 * into `slabs` (room for slab_capacity matrices [Co][taps * Ci] fp32; d->w_row_stride == taps * Ci) and one
 * sm3_slab_reduce adds them to dw.  The partition depends on the geometry and the device only, so two runs of the same
 * step produce the same bits -- the autograd backward of nn.Conv2d / nn.Linear it replaces (tools/backbone_train.py:125)
 * is a fixed-order reduction too.  A launch that needs a single slice adds its tiles to dw directly (no slab). */
int sm3_conv_wgrad_det(const sm3_conv_desc* d, const void* x, const void* dy, float* dw, float* slabs, int slab_capacity,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm (2d and 1d: rows x C), train and eval.  replaces nn.BatchNorm2d/1d (+SyncBatchNorm,
 * tools/backbone_train.py:510) at resnet.py:145-149,211,261 and simclr.py:20-26.
 * ------------------------------------------------------------------------------------------ */
/* sums[0..C) = sum over partial rows of p[r][0][c]; sums[C..2C) likewise of p[r][1][c]  (fp64, deterministic
 * two-stage reduction).  workspace: SM3_BN_REDUCE_GROUPS * 2C doubles. */
#define SM3_BN_REDUCE_GROUPS 64
/* number of fp64 [2C] rows stage A leaves in workspace for `rows` partial rows */
int sm3_bn_reduce_groups(int rows);
/* "views": the two views of a branch go through the convolutions as ONE batch (view 0's rows, then view 1's) but
 * keep separate BatchNorm statistics (simclr.py:58-59).  Every BatchNorm entry point takes `views` >= 1 and treats
 * its tensors as `views` equal row ranges laid out back to back, with per-view parameter vectors [views][C] /
 * [views][2C]; `rows` is always the row count of ONE view.
 * sums == NULL: only stage A runs; pass (workspace, sm3_bn_reduce_groups(rows)) to sm3_bn_finalize.
 * partials: [views][rows][2][C]; sums: [views][2C]; workspace: views * SM3_BN_REDUCE_GROUPS * 2C doubles. */
int sm3_bn_stats_reduce(const float* partials, int rows, int C, double* sums, double* workspace, int views,
                        void* stream);
/* From (possibly all-reduced) sums and the global element count per channel: mean, biased var ->
 * scale = gamma*invstd, shift = beta - mean*scale; running stats momentum update with the unbiased
 * variance; saves mean / invstd for backward.  gamma/beta NULL => affine=False. */
int sm3_bn_finalize(const double* sums, int groups /* sums is [views][groups][2C], groups summed here */, int views,
                    double count /* per view */, int C, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked /* += views */, float* scale, float* shift, float* save_mean,
                    float* save_invstd /* all four [views][C]; running statistics updated view by view */, void* stream);
/* eval mode: scale/shift from the running statistics */
int sm3_bn_eval_scale_shift(const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, int C, float* scale, float* shift,
                            void* stream);
/* y = [relu]( x*scale + shift [+ residual] ), x,residual,y: [rows, C] of dtype; out_f32 != 0 stores y as fp32.
 * relu_mask (nullable, with relu): one byte per 16-byte vector of y, bit e = (y[e] > 0) -- all that the backward
 * pass needs of y, at 1/16 of its bytes.
 * replaces the bn->relu / bn->add->relu chains of Bottleneck.forward (resnet.py:154-174). */
int sm3_bn_act(int dtype, const void* x, const float* scale, const float* shift, const void* residual,
               int relu, int out_f32, void* y, uint8_t* relu_mask, int64_t rows, int C, int views, void* stream);
/* sm3_bn_act (storage dtype output) that also leaves per-block column sums of the STORED outputs:
 * colsum_partials [views][sm3_bn_act_colsum_rows(rows, C, dtype)][C] fp32 -- the first moment of a convolution input, for
 * the BatchNorm by linearity below (sm3_linbn_moments sums the rows in a fixed order).  A view's rows are cut the same way
 * whether the launch holds one view or two, so its sums do not depend on that. */
int sm3_bn_act_colsum_rows(int64_t rows, int C, int dtype);
int sm3_bn_act_colsum(int dtype, const void* x, const float* scale, const float* shift, const void* residual, int relu,
                      void* y, uint8_t* relu_mask, float* colsum_partials, int64_t rows, int C, int views, void* stream);
/* Column sums of x [N, H, W, C] at the pixels (y % stride == 0, x % stride == 0) as partial rows
 * [views][sm3_subsample_colsum_rows(N / views * Hs * Ws, C, dtype)][C] fp32 (summed by sm3_linbn_moments), and -- y given --
 * those pixels as a compact tensor y [N, Hs, Ws, C], Hs = (H - 1) / stride + 1: the input of a strided 1x1 convolution
 * (a Bottleneck's downsample branch, resnet.py:260) as the dense operand that BatchNorm by linearity needs. */
int sm3_subsample_colsum_rows(int64_t rows, int C, int dtype);
int sm3_subsample_colsum(int dtype, const void* x, void* y, float* colsum_partials, int N, int H, int W, int C, int stride,
                         int views, void* stream);
/* The join of a Bottleneck with a downsample branch in ONE pass (resnet.py:164-172: out = bn3(conv3); identity =
 * downsample(x) [conv + BatchNorm]; out += identity; relu):  y = [relu]( x*scale + shift + x2*scale2 + shift2 ),
 * x2 the pre-BatchNorm output of the downsample convolution, scale2/shift2 [views][C] from its sm3_bn_finalize.
 * The downsample BatchNorm's own apply pass (one read + one write of a block-output-sized tensor) disappears. */
int sm3_bn_add_bn_act(int dtype, const void* x, const float* scale, const float* shift, const void* x2,
                      const float* scale2, const float* shift2, int relu, void* y, uint8_t* relu_mask,
                      int64_t rows, int C, int views, void* stream);
/* Backward, phase 1: dz = dy * (y > 0), the mask taken from relu_mask if given, else from y if given, else all
 * ones; writes dz (may alias dy; NULL to skip) and
 * per-block partial sums [bwd_partial_rows][2][C] of (dz, dz * xhat), xhat = (x-mean)*invstd.  x == NULL (mean / invstd
 * then unused): mask and sum(dz) only, the second slot is written as 0 (BatchNorm by linearity, below). */
int sm3_bn_bwd_partial_rows(int64_t rows, int C);
int sm3_bn_bwd_reduce(int dtype, const void* dy, const void* y, const uint8_t* relu_mask, const void* x,
                      const float* mean, const float* invstd, void* dz, int64_t rows, int C,
                      float* partials /* [views][bwd_partial_rows][2][C] */, int views, void* stream);
/* Backward, phase 2: dx = gamma*invstd*(dz - sum_dz/count - xhat*sum_dz_xhat/count) with the
 * (all-reduced) global sums; dgamma += local sum(dz*xhat), dbeta += local sum(dz) (NULL to skip). */
int sm3_bn_bwd_apply(int dtype, const void* dz, const void* x, const float* mean, const float* invstd,
                     const float* gamma, const double* global_sums, double count,
                     const double* local_sums, float* dgamma, float* dbeta, void* dx, int64_t rows,
                     int C, int views, void* stream);

/* Phase 2 for the TWO BatchNorms of such a join, which receive the same dz: reads dz once, writes both input
 * gradients (arithmetic of each side = sm3_bn_bwd_apply). */
typedef struct sm3_bn_apply_side {
    const void* x;                 /* pre-BatchNorm tensor, [views][rows][C] */
    const float* mean;             /* [views][C] */
    const float* invstd;
    const float* gamma;            /* [C], nullable */
    const double* global_sums;     /* [views][2C] */
    const double* local_sums;      /* [views][2C], nullable with dgamma/dbeta */
    float* dgamma;
    float* dbeta;
    void* dx;
} sm3_bn_apply_side;
int sm3_bn_bwd_apply2(int dtype, const void* dz, double count, const sm3_bn_apply_side* a,
                      const sm3_bn_apply_side* b, int64_t rows, int C, int views, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm BY LINEARITY, for an expanding 1x1 convolution followed by train-mode BatchNorm (Bottleneck conv3 -> bn3:
 * resnet.py:162-163 and their autograd backward; 16-bit dtypes).  With x = y W^T (y: [M, p] conv input, W: [C, p]),
 * s = sum_m y (sm3_bn_act_colsum) and G = y^T y (sm3_conv_wgrad_cat on y alone):
 *   forward   sum_m x = W s,  sum_m x^2 = rowdot(W G, W)  -> sm3_bn_finalize -> sm3_conv_bn_act_fused: x is never stored
 *   backward  dx = a (dz - m1) - b (x - mu)   [a = gamma invstd, b = a invstd mean(dz xhat), m1 = mean(dz)], so with
 *             P = dz^T y (sm3_conv_wgrad_cat):
 *               sum_m dz xhat = invstd (rowdot(W, P) - mu sum_m dz)                                (sm3_linbn_stats)
 *               dy = dz (diag(a) W) - y H + const,  H = W^T diag(b) W   (sm3_linbn_banks, sm3_linbn_post for H,
 *                                                                        sm3_conv_dgrad_seg_bnfuse)
 *               dW += diag(a)(P - m1 s^T) - diag(b)(W G - mu s^T)                                  (sm3_linbn_post)
 * so neither sm3_bn_bwd_apply's pass over dz / x / dx nor any other read of x is made.  All per-channel vectors are
 * [views][C]; coef is [views][C][4] fp32 = (a, b, m1, mu).
 * ------------------------------------------------------------------------------------------ */
/* out [views][n] fp32 = the sum of the nslabs slabs per view sm3_conv_wgrad_slabs left (n = p * p for G = y^T y, C * p for
 * P = dz^T y), and -- colsum_partials given -- s_out [views][p] fp64 = the sum of the colsum_rows partial rows of
 * sm3_bn_act_colsum; both in a fixed order. */
int sm3_linbn_moments(const float* slabs, int nslabs, int64_t n, float* out, const float* colsum_partials, int colsum_rows,
                      double* s_out, int p, int views, void* stream);
/* Tm [views][C][p] fp32 = W G_v (exact-f32 MFMA), and the batch sums of x as sums_ws [views][p/32][2C] fp64 -- pass it to
 * sm3_bn_finalize with groups = p/32 (data parallel: all-reduce it first).  G: [views][p][p] fp32; s: [views][p] fp64;
 * w_dgrad: dtype [p][C]; w_fwd: dtype [C][p].  C, p multiples of 32. */
int sm3_linbn_fwd_stats(int dtype, const float* G, const void* w_dgrad, const void* w_fwd, const double* s, float* Tm,
                        double* sums_ws, int C, int p, int views, void* stream);
/* reduce_ws / groups: what sm3_bn_stats_reduce(partials of (dz, .), sums = NULL) left -- its stage B runs here.
 * reduce_ws is [views][groups][2C] fp64 and only the first C entries of a row (the sums of dz) are read: the second
 * half may hold anything.  No alignment of C or p is required.
 * lsums: [views][2C] fp64, both halves written (sum dz | sum dz xhat); dgamma += sum dz xhat, dbeta += sum dz (NULL to
 * skip).  count > 0 (single rank: the local sums are the global ones): coef is written too; count <= 0: the caller
 * all-reduces lsums and calls sm3_linbn_coef.  P: [views][C][p] fp32; w_fwd: dtype [C][p]. */
int sm3_linbn_stats(int dtype, const float* P, const void* w_fwd, const float* mean, const float* invstd, const float* gamma,
                    const double* reduce_ws, int groups, double* lsums, float* dgamma, float* dbeta, double count,
                    float* coef, int C, int p, int views, void* stream);
int sm3_linbn_coef(const double* global_sums, double count, const float* gamma, const float* mean, const float* invstd,
                   float* coef, int C, int views, void* stream);
/* wa = diag(a) W and wbn = -diag(b) W in data-gradient order (dtype [views][p][C], from w_dgrad [p][C]);
 * col_const [views][p] = (b mu - a m1) W, summed over the rounded products.  C a multiple of 8; any p. */
int sm3_linbn_banks(int dtype, const void* w_dgrad, const float* coef, void* wa, void* wbn, float* col_const, int C, int p,
                    int views, void* stream);
/* out[v][e] = sum over the `groups` partial rows of sums_ws [views][groups][n] (n = 2C), fixed order: what a data-parallel
 * run exchanges between ranks (then sm3_bn_finalize with groups = 1). */
int sm3_linbn_fold(const double* sums_ws, int groups, int n, int views, double* out, void* stream);
/* out3[v][c][:] = scale3[v][c] w3[c][:] ([C][K3] banks), outd[v][c][:] = scaled[v][c] wd[c][:] ([C][Kd]), and
 * bias[v][c] = shift3[v][c] + shiftd[v][c]: what sm3_conv_seg_act needs to run conv3 + bn3 + downsample conv + its BatchNorm
 * + add + ReLU as one two-segment GEMM.  K3, Kd multiples of 8; any C.  Both banks are rounded once from the fp32 product. */
int sm3_linbn_scale_banks(int dtype, const void* w3, int K3, const float* scale3, const float* shift3, void* out3,
                          const void* wd, int Kd, const float* scaled, const float* shiftd, void* outd, float* bias, int C,
                          int views, void* stream);
/* One launch of 32 x 32 MFMA tiles:  hn [views][p][p] (dtype) = wbn_v w_dgrad^T = -H_v, and
 * dw[C][p] += sum_v diag(a_v)(P_v - m1_v s_v^T) - diag(b_v)(W G_v - mu_v s_v^T), W G_v from Tm (sm3_linbn_fwd_stats) or,
 * Tm NULL, recomputed from G.  C % 128 == 0, p % 32 == 0. */
int sm3_linbn_post(int dtype, const void* wbn, const void* w_dgrad, void* hn, const float* P, const float* G,
                   const float* Tm, const double* s, const float* coef, float* dw, int C, int p, int views, void* stream);
/* sm3_linbn_banks + sm3_linbn_post as ONE launch (the links of the chain between a unit's backward GEMMs are launch
 * latency): wa, col_const, hn and dw as those two produce them, bit for bit; the -diag(b) W bank is formed in registers
 * (same product, same rounding) and never stored. */
int sm3_linbn_banks_post(int dtype, const void* w_dgrad, const float* coef, void* wa, float* col_const, void* hn,
                         const float* P, const float* G, const float* Tm, const double* s, float* dw, int C, int p, int views,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Stem, pooling.  replaces resnet.py:208-213,224,294-305.
 * ------------------------------------------------------------------------------------------ */
/* Direct stem (bf16 / fp16 on the 16-bit MFMA; SM3_F32 on v_mfma_f32_32x32x2_f32, fp32 patch fragments and filter bank):
 * the 7x7/2 pad-3 convolution straight from the NCHW fp32 images, no im2col matrix in HBM.
 *   w_stem: dtype [64][176] from sm3_stem_weight_prep (K order (kh, c, kw padded to 8); master is [64][kh][kw][c]);
 *   y: [N*Ho*Wo, 64] dtype; stat_partials (nullable): [sm3_stem_partial_rows][2][64], one row per tile of <= 128
 *   output pixels of one output row -- tiles are image-major, so a view's rows are contiguous. */
int sm3_stem_partial_rows(int N, int H, int W);
int sm3_stem_weight_prep(int dtype, const float* w_master, void* w_stem, void* stream);
int sm3_stem_weight_prep_if(int dtype, const float* w_master, void* w_stem, const int* only_if, void* stream);
int sm3_stem_conv_fwd(int dtype, const float* x_nchw, const void* w_stem, void* y, float* stat_partials, int N, int H,
                      int W, void* stream);
/* Stem weight gradient with phase 2 of bn1's backward fused into its operand load:
 *   dxo = gamma*invstd*(dz - sum_dz/count - xhat*sum_dz_xhat/count)   (never written to HBM: the stem has no data
 *   gradient, so this tensor has no other consumer),  dw[64][147] += dxo^T * im2col(x),
 *   dgamma += local sum(dz*xhat), dbeta += local sum(dz).  Arguments as sm3_bn_bwd_apply; dz, xo: [N*Ho*Wo, 64].
 *   dw_slabs (ABI 8; nullable): room for SM3_STEM_WGRAD_SLABS matrices [64][147] fp32 -- every workgroup of the persistent
 *   grid stores its partial product there and one sm3_slab_reduce adds them to dw in a fixed order (what the training step
 *   uses); NULL: float atomics straight into dw. */
#define SM3_STEM_WGRAD_SLABS 768
int sm3_stem_wgrad_bn(int dtype, const float* x_nchw, const void* dz, const void* xo, const float* mean,
                      const float* invstd, const float* gamma, const double* global_sums, double count,
                      const double* local_sums, float* dgamma, float* dbeta, float* dw, float* dw_slabs, int N, int H, int W,
                      int views, void* stream);
/* The same two kernels on images rounded to the 16-bit type ONCE per step (ABI 8; what the training step uses in the
 * 16-bit modes; every output bit equals sm3_stem_conv_fwd / sm3_stem_wgrad_bn on the fp32 images -- the rounding is the
 * same, it only happens once instead of per staged tile, forward and again in the weight gradient):
 *   sm3_stem_image_prep: ximg [views * n_per_view][3][H][Wp] dtype, Wp = sm3_stem_image_cols(W) = round_up(W + 6, 8),
 *     ximg[.., q] = x[.., q - 3] for 3 <= q < W + 3, else 0 (the convolution's zero padding materialised); the views of a
 *     branch come from two NCHW fp32 tensors (x_view1 NULL with views = 1) -- no concatenated copy of the images is made.
 *   sm3_stem_conv_fwd16 / sm3_stem_wgrad_bn16: arguments as the fp32-image forms with ximg in place of x_nchw; the staged
 *     rows are aligned 16-byte chunks of ximg moved by LDS-DMA one tile ahead.  resnet.py:208-213,294-295. */
int sm3_stem_image_cols(int W);
int sm3_stem_image_prep(int dtype, const float* x_view0, const float* x_view1, void* ximg, int n_per_view, int views, int H,
                        int W, void* stream);
int sm3_stem_conv_fwd16(int dtype, const void* ximg, const void* w_stem, void* y, float* stat_partials, int N, int H, int W,
                        void* stream);
int sm3_stem_wgrad_bn16(int dtype, const void* ximg, const void* dz, const void* xo, const float* mean, const float* invstd,
                        const float* gamma, const double* global_sums, double count, const double* local_sums,
                        float* dgamma, float* dbeta, float* dw, float* dw_slabs, int N, int H, int W, int views,
                        void* stream);
/* Stem data gradient (ABI 9, additive): the gradient of the fp32 NCHW image batch,
 *   dx[n, c, iy, ix] = sum over the taps of (iy, ix) of dxo[n, oy, ox, co] * w[co][kh][kw][c],   dx: [N][3][H][W] fp32,
 * with dxo the stem BatchNorm's input gradient computed on the fly from dz, xo, mean, invstd, gamma, global_sums and count
 * exactly as sm3_stem_wgrad_bn computes it (all-zero global_sums: frozen statistics, dxo = gamma*invstd*dz); dxo is not
 * written to HBM.  w_master: the fp32 [64][7][7][3] weight (rounded to dtype in LDS as sm3_stem_weight_prep rounds it);
 * dz, xo: [N*Ho*Wo, 64] dtype, 16-byte aligned.  Gather form: every element of dx is written once, in a fixed summation
 * order (no atomics: the result is a function of the inputs).  Any geometry sm3_stem_conv_fwd accepts; views as
 * sm3_stem_wgrad_bn.  The same kernel serves both image paths: the image gradient passes straight through the 16-bit
 * rounding of sm3_stem_image_prep. */
int sm3_stem_dgrad_bn(int dtype, const void* dz, const void* xo, const float* mean, const float* invstd, const float* gamma,
                      const double* global_sums, double count, const float* w_master, float* dx, int N, int H, int W,
                      int views, void* stream);
/* argmax (nullable): [N,Ho,Wo,C] bytes, window position kh*3+kw of the first maximum in scan order (ATen's tie rule) */
int sm3_maxpool3x3s2_fwd(int dtype, const void* x, void* y, uint8_t* argmax, int N, int H, int W, int C, void* stream);
/* dx[n,iy,ix,c] = sum of dy over the windows whose recorded argmax is (iy,ix); gather form, no atomics */
int sm3_maxpool3x3s2_bwd(int dtype, const uint8_t* argmax, const void* dy, void* dx, int N, int H, int W, int C,
                         void* stream);
/* Stem chain bn1 -> relu -> maxpool (resnet.py:295-297) in ONE pass over the pre-BatchNorm stem output x [N,H,W,C]:
 * y[N,Ho,Wo,C] = maxpool3x3s2(relu(x*scale + shift)), argmax as above; scale/shift [views][C] (images [0,N/views) are
 * view 0).  Bit-identical to sm3_bn_act followed by sm3_maxpool3x3s2_fwd; the post-ReLU map is never stored. */
int sm3_bn_relu_maxpool_fwd(int dtype, const void* x, const float* scale, const float* shift, void* y,
                            uint8_t* argmax, int N, int H, int W, int C, int views, void* stream);
/* ... and its backward up to BatchNorm-backward phase 1: dz[N,H,W,C] = (x*scale+shift > 0) * maxpool_bwd(dy), plus
 * partial sums [views][sm3_maxpool_bn_bwd_partial_rows][2][C] of (dz, dz*xhat) as sm3_bn_bwd_reduce writes them. */
int sm3_maxpool_bn_bwd_partial_rows(int N, int H, int W, int views);
int sm3_maxpool_bn_bwd(int dtype, const uint8_t* argmax, const void* dy, const void* x, const float* scale,
                       const float* shift, const float* mean, const float* invstd, void* dz, float* partials,
                       int N, int H, int W, int C, int views, void* stream);
/* feat[n,c] = mean over HW; feat_f32 and feat_t (dtype copy for the projector GEMM) both optional */
int sm3_avgpool_fwd(int dtype, const void* x, float* feat_f32, void* feat_t, int N, int HW, int C, void* stream);
int sm3_avgpool_bwd(int dtype, const void* dfeat, void* dx, int N, int HW, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight layout preparation (per optimizer step).  w: fp32 master [Co][taps][Ci].
 *   w_fwd   (nullable): dtype [Co][ld_fwd]  (ld_fwd >= taps*Ci, tail zero-filled)
 *   w_dgrad (nullable): dtype [Ci][taps][Co]   (the transposed filter bank used by the data gradient)
 * ------------------------------------------------------------------------------------------ */
int sm3_weight_prep(int dtype, const float* w, int Co, int taps, int Ci, void* w_fwd, int ld_fwd,
                    void* w_dgrad, void* stream);
/* the same for n filter banks in ONE launch; items_device: device array of n descriptors */
typedef struct sm3_wprep_item {
    const float* w;
    void* w_fwd;
    void* w_dgrad;
    int32_t Co, taps, Ci, ld_fwd;
} sm3_wprep_item;
int sm3_weight_prep_batch(int dtype, const sm3_wprep_item* items_device, int n, void* stream);
/* Frozen weights keep their banks (frozen-encoder loops: tools/backbone_eval.py --finetune fc, tools/mlc_train.py,
 * inference.py) without the host ever reading device memory or trusting a framework's dirty bits:
 *   sm3_weights_changed: position-weighted 64-bit hash of the n fp32 words at `flat`; *changed = (hash != state[1]);
 *                        state[1] = hash.  state: 2 x uint64 on the device, zero-initialised by the caller once.
 *   sm3_weight_prep_batch_if / sm3_stem_weight_prep_if: the launches above, whose workgroups return at once when
 *                        *only_if == 0 (only_if NULL = unconditional).  Two launches + early-exit kernels: ~0.03 ms
 *                        instead of the 0.2 ms re-layout of 47 M weights. */
int sm3_weights_changed(const float* flat, int64_t n, uint64_t* state, int* changed, void* stream);
int sm3_weight_prep_batch_if(int dtype, const sm3_wprep_item* items_device, int n, const int* only_if, void* stream);
/* elementwise cast fp32 -> dtype */
int sm3_cast_from_f32(int dtype, const float* src, void* dst, int64_t n, void* stream);
int sm3_cast_to_f32(int dtype, const void* src, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * NT-Xent.  replaces F.normalize + matmul + mask/select + /T (simclr.py:62-88, 294-320) and
 * nn.CrossEntropyLoss (tools/backbone_train.py:531, applied :101-102,119-120).
 * R = 2B rows, D = proj_dim.
 * ------------------------------------------------------------------------------------------ */
/* zn = z / max(|z|,1e-12); logits[i][0] = S[i][p]/T, logits[i][1..] = S[i][j != i,p]/T ascending j, p=(i+R/2)%R */
int sm3_ntxent_logits(const float* z, int R, int D, float temperature, float* zn, float* inv_norm,
                      float* logits, void* stream);
/* d(loss)/dz from d(loss)/dlogits (reference layout), written as dtype */
int sm3_ntxent_logits_bwd(int dtype, const float* dlogits, const float* zn, const float* inv_norm, int R,
                          int D, float temperature, void* dz, void* stream);
/* Every loss entry point below adds ONE value per call to loss[0]: the per-row terms are written to a buffer and summed
 * in a fixed order (fp64, one workgroup) -- like the reference's single CrossEntropyLoss reduction over a materialised
 * logits tensor (tools/backbone_train.py:531), the loss is a function of its inputs bit for bit (no float atomics).
 * The calls that accumulate into the same loss[0] must be enqueued on one stream. */
/* mean cross-entropy against label 0 of logits [R][Cc]; loss[0] += weight*CE; dlogits = weight*grad.
 * row_terms: R floats of scratch (required when loss is given). */
int sm3_ce_label0(const float* logits, int R, int Cc, float weight, float* row_terms, float* loss, float* dlogits,
                  void* stream);
/* fused: loss[0] += weight * NTXent(z); dz = weight * dNTXent/dz (dtype); never materialises logits.
 * workspace: R*D + 3*R floats (normalised rows, inverse norms, per-row logsumexp, per-row loss terms). */
int sm3_ntxent_fused(int dtype, const float* z, int R, int D, float temperature, float weight,
                     float* workspace, float* loss, void* dz, void* stream);

/* the same with dz additionally multiplied by the device scalar dz_scale[0] (loss scaling of the fp16 mode; the loss itself
 * stays unscaled) */
int sm3_ntxent_fused_scaled(int dtype, const float* z, int R, int D, float temperature, float weight,
                            const float* dz_scale, float* workspace, float* loss, void* dz, void* stream);

/* n <= 4 NT-Xent terms of EQUAL shape in three launches instead of 3 n (round 6; ABI 8 addition): the four loss terms of a
 * step -- derm, clinic and the two cross-modal ones (tools/backbone_train.py:99-102,119-121) -- sit on the main stream between
 * the lanes' forward and backward, where nothing else runs.  z, dz: host arrays of n device pointers; weights: host array of n;
 * dz_scale: NULL or the device scalar of sm3_ntxent_fused_scaled; workspace: n * round_up(R*D + 3*R, 4) floats, 16-byte aligned.  Every
 * dz[t] and the loss are bit-identical to n calls of sm3_ntxent_fused(_scaled) in term order.  D % 4 == 0, D <= 128
 * (SM3_EINVAL otherwise: the caller keeps the per-term calls). */
int sm3_ntxent_fused_batch(int dtype, int nterms, const float* const* z, int R, int D, float temperature, const float* weights,
                           const float* dz_scale, float* workspace, float* loss, void* const* dz, void* stream);

/* Global negatives under data parallelism (BASELINE.json north_star: all-gather of the projection embeddings; NOT the
 * reference's behaviour -- its negatives are the local batch, SURVEY.md section 0 -- hence an opt-in mode of the trainer):
 *   zn = normalise(z) (sm3_normalize_rows), all-gathered over RCCL to zg [Rg = world*Rl][D];
 *   S = zn zg^T (sm3_conv_gather_gemm, exact-f32);  sm3_ntxent_rect: loss += weight * mean_i(-S_ip/T + log sum_{j != self}
 *   exp(S_ij/T)) over the Rl local rows (self = column self_offset + i, positive = self_offset + (i + Rl/2) % Rl) and
 *   S <- d(loss)/dS in place (x dz_scale[0] if given);  d(zn) = dS zg (anchor role, sm3_conv_gather_gemm) + the local
 *   rows of all_reduce(dS^T zn) (candidate role, sm3_conv_wgrad);  sm3_normalize_rows_bwd: dz = inv_norm * (v - zn (zn.v)),
 *   v = dzn_a + dzn_b (dzn_b nullable). */
int sm3_normalize_rows(const float* z, int R, int D, float* zn, float* inv_norm, void* stream);
int sm3_ntxent_rect(float* S, int Rl, int Rg, int self_offset, float temperature, float weight, const float* dz_scale,
                    float* row_terms /* Rl floats of scratch */, float* loss, void* stream);
int sm3_normalize_rows_bwd(int dtype, const float* dzn_a, const float* dzn_b, const float* zn, const float* inv_norm,
                           int R, int D, void* dz, void* stream);

/* ------------------------------------------------------------------------------------------
 * AdamW over a flat fp32 buffer.  replaces torch.optim.AdamW(eps=1e-5, wd) + GradScaler unscale
 * (tools/backbone_train.py:124-127, 525-527).  g is multiplied by grad_scale first.
 * found_inf (nullable): if *found_inf != 0 the step is skipped (GradScaler semantics).
 * ------------------------------------------------------------------------------------------ */
int sm3_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
              float eps, float weight_decay, int step, float grad_scale, const int32_t* found_inf,
              void* stream);
/* The fp16 mode's dynamic loss scaling (torch.cuda.amp.GradScaler, backbone_train.py:125-127,480) with the scaler's state
 * on the DEVICE, so that a step needs no host synchronisation: loss_scale[1] (the factor sm3_ntxent_fused_scaled applied to
 * dz), steps_taken[1] (optimizer steps actually taken: a skipped step does not advance Adam's bias correction).
 * sm3_adamw_dynamic: as sm3_adamw with g multiplied by grad_scale / loss_scale[0] and step = steps_taken[0] + 1; skipped when
 * found_inf[0] != 0.  sm3_loss_scale_update: GradScaler.update() -- on overflow scale *= backoff and the growth tracker
 * restarts, else steps_taken += 1 and after growth_interval clean steps scale *= growth; clears found_inf. */
int sm3_adamw_dynamic(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float grad_scale, const float* loss_scale,
                      const int32_t* steps_taken, const int32_t* found_inf, void* stream);
int sm3_loss_scale_update(float* loss_scale, int32_t* found_inf, int32_t* growth_tracker, int32_t* steps_taken,
                          float growth_factor, float backoff_factor, int growth_interval, void* stream);
/* Momentum ("target") encoder of BASELINE.json's north_star -- an extension: the reference has no target network
 * (SURVEY.md section 0).  target = momentum * target + (1 - momentum) * online over the flat fp32 parameter buffer. */
int sm3_ema_update(float* target, const float* online, int64_t n, float momentum, void* stream);
/* found_inf[0] |= any(!isfinite(g)) */
int sm3_check_finite(const float* g, int64_t n, int32_t* found_inf, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input pipeline on the GPU: the SimCLR augmentation chain of tools/backbone_train.py:448-466 (torchvision 0.13
 * transforms on PIL images in DataLoader workers there) over a batch of decoded RGB images resident in HBM.
 * Random parameters are drawn by the host (sm3hip/augment.py, torchvision's sampling rules) and passed per sample.
 * ------------------------------------------------------------------------------------------ */
/* RandomResizedCrop + RandomHorizontalFlip + ToTensor: crop box[b] = (top, left, height, width) of src [B,Hs,Ws,3] uint8,
 * antialiased bilinear resample (PIL's triangle filter, support max(scale,1)) to [H,W], mirrored when flip[b] != 0;
 * out [B,3,H,W] fp32 in [0,1]. */
int sm3_aug_resized_crop(const uint8_t* src, int B, int Hs, int Ws, const int32_t* box, const uint8_t* flip, float* out,
                         int H, int W, void* stream);
/* The same resample over images of DIFFERENT sizes (ABI 8 addition): the images lie HWC uint8, one after another, in
 * `arena` (arena_bytes long, device memory); image k starts at byte offset[k] and is img_h[k] x img_w[k].  Sample b reads
 * image index[b] (0 <= index[b] < n_images) with crop box[b] = (top, left, height, width) inside that image and flip[b];
 * out [B,3,H,W] fp32 in [0,1].  offset / img_h / img_w / index / box / flip are HOST arrays: every box and image is checked
 * against its own image and the arena (SM3_EINVAL) before anything is launched, and the per-sample geometry travels in the
 * kernel arguments.  Arithmetic identical to sm3_aug_resized_crop: on an equal-sized batch the two agree bit for bit. */
int sm3_aug_resized_crop_ragged(const uint8_t* arena, int64_t arena_bytes, const int64_t* offset, const int32_t* img_h,
                                const int32_t* img_w, int n_images, const int32_t* index, const int32_t* box,
                                const uint8_t* flip, int B, float* out, int H, int W, void* stream);
/* One position of ColorJitter's randomly ordered chain, in place on img [B,3,H,W]: op[b] = 0 none, 1 brightness, 2 contrast,
 * 3 saturation, 4 hue, with factor[b] (torchvision functional_tensor: _blend / rgb_to_grayscale / _rgb2hsv / _hsv2rgb).
 * gray_mean: [B] scratch (the per-image grayscale mean the contrast blend needs, recomputed by every call). */
int sm3_aug_color_op(float* img, int B, int H, int W, const int32_t* op, const float* factor, float* gray_mean, void* stream);
/* RandomGrayscale (gray[b] != 0: 3-channel grayscale) -> GaussianBlur 3x3 with reflect padding (sigma[b] > 0, else none) ->
 * Normalize: out = (x - mean3[c]) / std3[c].  mean3 / std3 are HOST arrays of 3 floats. */
int sm3_aug_finish(const float* img, int B, int H, int W, const uint8_t* gray, const float* sigma, const float* mean3,
                   const float* std3, float* out, void* stream);

/* ---- multi-label heads of the inference model (reference inference.py:53-96; eval mode) -------------------
 * The Linear layers of that model run as sm3_conv_gather_gemm (1x1, bias-free) + sm3_bn_act(scale=1, shift=bias).
 * qkv: [B*S, 3*D] rows b*S+s, columns [q|k|v] (nn.MultiheadAttention's in_proj layout); out: [B*S, D]:
 * softmax(q k^T / sqrt(D/nhead)) v over the S <= 8 label tokens of each sample, per head. */
int sm3_token_attention(int dtype, const void* qkv, void* out, int B, int S, int D, int nhead, void* stream);
/* out = LayerNorm(a + b) * gamma + beta over the last axis (b nullable); rows x D of dtype, D <= 1024
 * (the post-norm residual joins of nn.TransformerEncoderLayer, inference.py:58-60). */
int sm3_add_layernorm(int dtype, const void* a, const void* b, const float* gamma, const float* beta, float eps,
                      void* out, int64_t rows, int D, void* stream);
/* out[b, t] = <x[b, token_of[t], :], W[t, :]> + bias[t], x: [B, S, D] of dtype (each token L2-normalised first when
 * l2_norm != 0), W: [T, D] fp32 = the prototype Linears concatenated (inference.py:62-71,90-94). */
int sm3_token_heads(int dtype, const void* x, const float* W, const float* bias, const int* token_of, int l2_norm,
                    float* out, int B, int S, int D, int T, void* stream);

/* ---- TRAINING of those heads (reference tools/mlc_train.py:58-90,241-283; tools/mlc_eval.py), all fp32 ------------------
 * The Linear layers (label projectors, attention in/out projections, feed-forward) are sm3_conv_gather_gemm / sm3_conv_wgrad
 * in SM3_F32; these entry points are everything else of one train-mode nn.TransformerEncoderLayer (post-norm, ReLU) over the
 * S <= 8 label tokens, the prototype heads, the pseudo-label cross-entropy and the spherical k-means behind the pseudo-labels.
 * Dropout keeps no mask: element e of stream `seed` is kept iff hash(seed, e) >= p; backward recomputes it. */
/* Token rows: label_major = 0: row(b, s) = b*S + s (the inference path's layout); 1: row(b, s) = s*B + b, the reference's
 * [S, B, D] stacking (mlc_train.py:79).
 * out[rows, D] = softmax(QK^T/sqrt(hd)) (dropout p on the probabilities) V, qkv [rows, 3D]; and its backward */
int sm3_mlc_attention_fwd(const float* qkv, float* out, int B, int S, int D, int nhead, float p, uint32_t seed,
                          int label_major, void* stream);
int sm3_mlc_attention_bwd(const float* qkv, const float* dout, float* dqkv, int B, int S, int D, int nhead, float p,
                          uint32_t seed, int label_major, void* stream);
/* out = LayerNorm(a + dropout_p(b)) * gamma + beta; stats[rows][2] = (mean, rstd).  Backward: da = d(sum), db = mask/(1-p) *
 * d(sum), dgamma / dbeta accumulated (atomics).  D <= 4096 (--mlc-proj v0 runs the layer at d_model = in_dim); the row sums
 * have a fixed order. */
int sm3_mlc_add_ln_fwd(const float* a, const float* b, const float* gamma, const float* beta, float eps, float p,
                       uint32_t seed, float* out, float* stats, int64_t rows, int D, void* stream);
int sm3_mlc_add_ln_bwd(const float* dout, const float* a, const float* b, const float* stats, const float* gamma, float p,
                       uint32_t seed, float* da, float* db, float* dgamma, float* dbeta, int64_t rows, int D, void* stream);
/* h = relu(y + bias) [rows, N], hd = dropout_p(h); backward dh = dhd * mask/(1-p) * (h > 0), dbias += column sums (atomics;
 * dbias nullable: dh only, the bias gradient then being sm3_mlc_colsum_det of dh) */
int sm3_mlc_bias_relu_drop_fwd(const float* y, const float* bias, float p, uint32_t seed, float* h, float* hd, int64_t rows,
                               int N, void* stream);
int sm3_mlc_relu_drop_bwd(const float* dhd, const float* h, float p, uint32_t seed, float* dh, float* dbias, int64_t rows,
                          int N, void* stream);
/* db[c] += sum_r dy[r][c]: the bias gradient of a Linear */
int sm3_mlc_colsum(const float* dy, float* db, int64_t rows, int N, void* stream);
/* loss[0] += mean_h mean_b CE(logits[b, off[h]:off[h+1]] / T, targets[h][b]); dlogits written (mlc_train.py:252-261).
 * ONE workgroup adds the B * H terms in a fixed fp64 order and does a plain (non-atomic) `loss[0] +=`: the caller zeroes
 * loss[0] before the first term of a step and issues every launch that adds to it on ONE stream (sm3hip/mlc.py does).
 * Launch time is linear in B * H on one CU (4 096 pairs at config 4's size: ~20 us); a caller with far larger B * H
 * should split the batch over calls. */
int sm3_mlc_ce(const float* logits, const int64_t* targets, const int* head_offsets, int H, int B, int Tn, float temperature,
               float* loss, float* dlogits, void* stream);
/* prototype heads in fp32 with either row layout (bias nullable: mlc_train.py's prototypes have none), and the backward:
 * dx written, dW [Tn,D] and dbias [Tn] (nullable) accumulated */
int sm3_mlc_heads_fwd(const float* x, const float* W, const float* bias, const int* token_of, int l2_norm, float* out, int B,
                      int S, int D, int Tn, int label_major, void* stream);
int sm3_mlc_heads_bwd(const float* dlogits, const float* x, const float* W, const int* token_of, int l2_norm, float* dx,
                      float* dW, float* dbias, int B, int S, int D, int Tn, int label_major, void* stream);
/* spherical k-means (mlc_train.py:146-177): E step assign[n] = argmax_k <emb[n], centroids[k]> (+ sums / counts of the M
 * step when given); M step centroid = normalise(sum / count) for non-empty clusters, every centroid L2-normalised */
int sm3_mlc_kmeans_assign(const float* emb, const float* centroids, int64_t* assign, float* sums, int* counts, int N, int D,
                          int K, void* stream);
int sm3_mlc_kmeans_update(float* centroids, const float* sums, const int* counts, int K, int D, void* stream);

/* ---- the same sums as functions of their inputs: no float atomics (what sm3hip/mlc.py runs unless SM3_WGRAD_DET=0) -----
 * Every float sum over rows below has ONE order, which depends on the shapes alone: the rows are cut into slabs of
 * SM3_MLC_SLAB_ROWS consecutive rows; within slab j four partial sums start at 0 and add the rows j*256 + t, + 4, + 8, ...
 * (t = 0..3) in ascending order, the slab's value being (p0 + p1) + (p2 + p3); then out = out + (((q0 + q1) + q2) + ... + q_{m-1})
 * over the m = ceil(rows / 256) slabs in index order.  With m > 1 the slab values are stored plainly into `slabs` (room for
 * m * W floats, W the number of output elements named at each entry point) and a second launch adds them; with m = 1 slabs may
 * be null.  Outputs are accumulated into (+=), as by the atomic forms.  Arguments are checked before anything is launched. */
#define SM3_MLC_SLAB_ROWS 256
/* db[g*N + c] += sum_{r < rows} dy[g*rows + r][c] for g < groups (W = groups * N): the bias gradient of a Linear, or of
 * `groups` Linears over consecutive row blocks of one dy (the v4 label projectors) */
int sm3_mlc_colsum_det(const float* dy, float* db, float* slabs, int64_t rows, int N, int groups, void* stream);
/* sm3_mlc_add_ln_bwd with dgamma[d] += sum_r dout[r][d] * xhat[r][d] and dbeta[d] += sum_r dout[r][d] in the order above
 * (W = 2 * D; slab j holds dgamma's D values, then dbeta's).  da / db are those of sm3_mlc_add_ln_bwd, bit for bit. */
int sm3_mlc_add_ln_bwd_det(const float* dout, const float* a, const float* b, const float* stats, const float* gamma, float p,
                           uint32_t seed, float* da, float* db, float* dgamma, float* dbeta, float* slabs, int64_t rows, int D,
                           void* stream);
/* sm3_mlc_heads_bwd with the sums over the batch in the order above, the rows being the B samples:
 * dW[t][d] += dlogits[b][t] * x[b, tok t][d] * inv[b][tok t] (inv = 1 / |x[b, s]| when l2_norm, else the factor is absent)
 * and dbias[t] += dlogits[b][t] (dbias nullable).  dx is that of sm3_mlc_heads_bwd, bit for bit.  work: room for
 * B * S + m * W floats, W = Tn * D + (dbias ? Tn : 0) -- the per-token 1/|x| first, then the slabs (never null). */
int sm3_mlc_heads_bwd_det(const float* dlogits, const float* x, const float* W, const int* token_of, int l2_norm, float* dx,
                          float* dW, float* dbias, float* work, int B, int S, int D, int Tn, int label_major, void* stream);
/* sm3_mlc_kmeans_assign with the M-step sums in the order above over the N embeddings: sums[k][d] += emb[n][d] for the n with
 * assign[n] = k, ascending n within each lane of a slab (W = K * D); assign (first maximum) and the integer counts as there.
 * sums and counts required; sm3_mlc_kmeans_update then runs on them unchanged. */
int sm3_mlc_kmeans_assign_det(const float* emb, const float* centroids, int64_t* assign, float* sums, int* counts, float* slabs,
                              int N, int D, int K, void* stream);

/* ---- grouped 1x1 GEMM: the per-label layers of the BN-MLP label projectors (reference src/models/projector.py:5-62, built by
 * tools/mlc_train.py:352-361 and tools/mlc_eval.py:344-353 for --mlc-proj v1 / v2 / v3), exact f32 (SM3_F32 only) ------------
 * G groups over one batch of `rows`: group g reads columns [g*K, (g+1)*K) of x [rows][G*K] and writes columns [g*N, (g+1)*N)
 * of y [rows][G*N] -- the label-major layout in which the BatchNorm1d of one layer for all labels is ONE BatchNorm over G*N
 * channels.  Within a group every sum has the order of a single-group sm3_conv_gather_gemm / sm3_conv_wgrad_det on compact
 * operands, so a grouped launch equals G per-group launches bit for bit.
 * Forward: y = per-group x_g w[g]^T, w: [G][N][K]; stat_partials (nullable): [ceil(rows / 128)][2][G*N] per-row-block sums and
 * sums of squares of y for train-mode BatchNorm (sm3_bn_stats_reduce / sm3_bn_finalize over G*N channels).
 * Data gradient: the same entry with the transposed banks w_t [G][K][N] (dx_g = dy_g w[g]; K and N swap roles). */
int sm3_grouped_gemm(int dtype, const void* x, const void* w, void* y, float* stat_partials, int rows, int groups, int K, int N,
                     void* stream);
/* Weight gradient, a function of its inputs (no float atomics): dw[g] += dy_g^T x_g, dw: [G][N][K] fp32; x: [rows][G*K], dy:
 * [rows][G*N].  slabs: room for slab_capacity banks of G*N*K floats; the pixel slices of each group are those of
 * sm3_conv_wgrad_det on one group with the same capacity, and one sm3_slab_reduce adds them up. */
int sm3_grouped_wgrad_det(int dtype, const void* x, const void* dy, float* dw, float* slabs, int slab_capacity, int rows,
                          int groups, int K, int N, void* stream);

/* ---- grouped 3x3 convolution: ResNeXt's conv2 (reference src/models/resnet.py:142-146, conv3x3(width, width, stride, groups)),
 * csrc/gconv.hip ---------------------------------------------------------------------------------------------------------------
 * NHWC activations [N][H][W][C] (rows = pixels), pad 1, stride 1 or 2, `groups` groups of cg = C / groups channels with cg in
 * {4, 8, 16, 32, 64} and C a multiple of 64; all three dtypes (f32 accumulation).  Sizes and dtypes are checked on the host
 * (SM3_EINVAL / SM3_EALIGN / SM3_EDTYPE) before anything is launched; every pointer must be 16-byte aligned.
 * Weight prep: master [C][3][3][cg] fp32 (OHWI) -> w_fwd [9][cg][C] (w_fwd[t][k][co] = w[co][t][k]) and w_dgrad [9][cg][C]
 * (w_dgrad[t][j][g*cg + k] = w[g*cg + j][t][k]), `dtype`; only_if (nullable device int): skip when *only_if == 0.
 * Forward: y [N][Ho][Wo][C], Ho = (H - 1) / stride + 1; stat_partials (nullable): the BatchNorm partial rows of
 * sm3_conv_gather_gemm ([ceil(N*Ho*Wo / 128)][2][C] sums and sums of squares of the rounded outputs), for the unchanged
 * sm3_bn_stats_reduce / sm3_bn_finalize path.
 * Data gradient: dx [N][H][W][C] from dy [N][Ho][Wo][C] (H, W: the forward input's map).
 * Weight gradient, a function of its inputs: dw [C][3][3][cg] += dy^T x, as sm3_gconv_wgrad_slabs(N, H, W, stride, capacity)
 * plain-store slabs of C*9*cg floats (the pixel partition depends on the geometry and the capacity only) and one
 * sm3_slab_reduce; no float atomics. */
int sm3_gconv_weight_prep(int dtype, const float* master, void* w_fwd, void* w_dgrad, int C, int groups, const int* only_if,
                          void* stream);
int sm3_gconv_fwd(int dtype, const void* x, const void* w_fwd, void* y, float* stat_partials, int N, int H, int W, int C,
                  int groups, int stride, void* stream);
int sm3_gconv_dgrad(int dtype, const void* dy, const void* w_dgrad, void* dx, int N, int H, int W, int C, int groups, int stride,
                    void* stream);
int sm3_gconv_wgrad_slabs(int N, int H, int W, int stride, int slab_capacity);
int sm3_gconv_wgrad_det(int dtype, const void* x, const void* dy, float* dw, float* slabs, int slab_capacity, int N, int H,
                        int W, int C, int groups, int stride, void* stream);

/* ---- peer-to-peer SyncBatchNorm statistics exchange on one node (csrc/p2p.hip; opt-in, RCCL is the default) ----------------
 * Replaces the all-reduce torch.nn.SyncBatchNorm performs per BatchNorm and direction (tools/backbone_train.py:510) for the
 * fp64 [views][2C] sums of sm3_bn_stats_reduce / sm3_linbn_fold / sm3_linbn_stats.
 * sm3_p2p_alloc: a zeroed mailbox of sm3_p2p_mailbox_bytes() in device memory + its 64-byte hipIpc handle (to be sent to the
 * peers by any means); sm3_p2p_open / _close: map / unmap a peer's mailbox; sm3_p2p_free: release one's own.
 * sm3_p2p_allreduce_f64: buf[0..n) += the same range of every other rank, in place, ONE launch on `stream`, result
 * bit-identical on all ranks (contributions added in rank order).  mailboxes: host array of `world` device pointers indexed by
 * rank (one's own included); seq: 1, 2, 3, ... -- the same value on every rank for the same exchange, per mailbox set;
 * n <= sm3_p2p_max_elems(); err_flag (device int): set to 1 when a peer's contribution did not arrive within timeout_s --
 * that exchange and EVERY later one with the same err_flag then writes NaN into buf and returns at once (no further waits),
 * so the failure shows in whatever is computed from the sums even if the flag is never read.
 * Mailboxes are fine-grained device memory (hipExtMallocWithFlags(hipDeviceMallocFinegrained), as RCCL's IPC buffers);
 * *kind_out (nullable) = 1, or 0 when that allocation / its IPC export failed and plain hipMalloc memory was used instead
 * (also forced by SM3_P2P_FINEGRAINED=0, for an A/B of the two). */
int sm3_p2p_mailbox_bytes(void);
int sm3_p2p_max_elems(void);
/* largest world size a mailbox has room for (8: one node), and the byte layout of a mailbox -- the data area
 * [data_first, data_first + data_bytes) source rank `src` writes for exchange slot `slot` (0 / 1) and the 8-byte arrival
 * flag of its block `block` (elems_per_block doubles each) -- so that a host-side check can prove, without a GPU, that the
 * areas of max_world ranks x 2 slots x every block are disjoint and inside sm3_p2p_mailbox_bytes(). */
int sm3_p2p_max_world(void);
int sm3_p2p_layout(int slot, int src, int block, int64_t* data_first, int64_t* data_bytes, int64_t* flag_off,
                   int* elems_per_block);
int sm3_p2p_alloc(void** ptr, void* ipc_handle_64, int* kind_out);
int sm3_p2p_open(const void* ipc_handle_64, void** ptr);
int sm3_p2p_close(void* ptr);
int sm3_p2p_free(void* ptr);
int sm3_p2p_allreduce_f64(double* buf, int n, void* const* mailboxes, int rank, int world, uint64_t seq, int* err_flag,
                          double timeout_s, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weighted k-nearest-neighbour vote (replaces KNNOnlineEvaluator.predict, src/models/evaluator.py:56-84, from the
 * similarity matrix on: topk -> gather -> exp(s / T) -> one-hot weighted sum).
 *   S [B, ld] f32, of which columns [0, N) are valid; targets [N, L] int32, one class per label; class_offsets: HOST array
 *   [L + 1], 0 = off[0] < off[1] < ... < off[L] <= 256, label l owning classes [0, off[l+1] - off[l]).
 *   scores [B, off[L]]: scores[b, off[l] + c] = sum of expf(s_j / T) over the k largest s_j of row b whose neighbour j has
 *   class c for label l (a target outside its label's range casts no vote).  nbr_idx / nbr_sim [B, k] (nullable): the
 *   neighbours' indices and similarities in rank order.
 * Equal similarities rank by the lower index first.  Each label's votes are added in rank order by one thread, no atomics:
 * the result is a function of the inputs alone.  1 <= k <= min(N, 1024), 1 <= L <= 16, T > 0, B, N, ld < 2^31.
 * ------------------------------------------------------------------------------------------ */
int sm3_knn_vote(const float* S, int64_t B, int64_t N, int64_t ld, const int32_t* targets, int L, const int32_t* class_offsets,
                 int k, float temperature, float* scores, int32_t* nbr_idx, float* nbr_sim, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grad-CAM of an encoder stage (csrc/cam.hip; ABI 9, additive).  A: the stage output [N][h][w][C] (NHWC, `dtype`, post-ReLU);
 * G: the gradients of T target logits with respect to A, [T][N][h*w][C] `dtype`.
 * sm3_cam_alpha: alpha [T][N][C] f32 = the mean of G over the h*w positions, added in ascending position order, then divided
 *   by h*w (HW = h*w).
 * sm3_cam_maps: low [N][T][h][w] f32 = ReLU(sum_c alpha[t][n][c] * A[n][p][c]) in a fixed channel order; maps [N][T][H][W] f32 =
 *   low upsampled as F.interpolate(mode="bilinear", align_corners=False) does, then (cam - min) / (1e-7 + max(cam - min)) per
 *   map.  C a multiple of 8 and A 16-byte aligned (SM3_EALIGN otherwise).
 * Sizes and dtypes are checked on the host (SM3_EINVAL / SM3_EALIGN / SM3_EDTYPE) before anything is launched.  No atomics:
 * equal inputs give equal bits whatever the grid and the batch position.
 * ------------------------------------------------------------------------------------------ */
int sm3_cam_alpha(int dtype, const void* g, float* alpha, int T, int N, int HW, int C, void* stream);
int sm3_cam_maps(int dtype, const void* a, const float* alpha, float* low, float* maps, int N, int T, int h, int w, int C, int H,
                 int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pixel-level attributions: Integrated Gradients and SmoothGrad (csrc/attr.hip; ABI 9, additive).  x: one modality's images
 * [N][E] f32, E = 3 * H * W, a multiple of 4; every pointer 16-byte aligned (SM3_EALIGN otherwise).  Every product and sum
 * below is a separately rounded f32 operation (no FMA) unless float64 is named.
 * sm3_attr_path: out [c][N][E] = base + alpha_k * (x - base), k = k0 .. k0 + c - 1, alpha_k = (float)(2k + 1) / (float)(2 *
 *   steps) (midpoint rule); base [base_n][E], base_n = 1 (shared) or N.  k0 + c <= steps <= 2^23.
 * sm3_attr_noise: out [c][N][E] = x + sigma[n] * z(seed, sample, n, e), sample = k0 + j * stride for j < c; z: Philox4x32-10,
 *   key = (seed low word, seed high word), counter = (e / 4, n, sample, 0), Box-Muller in float64 on the word pairs (w0, w1)
 *   and (w2, w3) with u = (w + 0.5) * 2^-32: r = sqrt(-2 log(u_a)), (r cos(2 pi u_b), r sin(2 pi u_b)), rounded to f32;
 *   element e takes lane e % 4.  The value depends on (seed, sample, n, e) alone, never on c, k0, stride or the grid.
 * sm3_attr_accumulate: acc [N][E] = (((acc + w * f(g[0])) + w * f(g[1])) + ...) over g [c][N][E], ascending, f = identity
 *   (squared = 0) or the square (squared = 1): cutting the c steps into several calls gives the same bits.
 * sm3_attr_finish: acc, attr [T][N][C][HW]; mode 0 (IG): attr = (x - base) * acc with x [N][C][HW] and base [base_n][C][HW];
 *   mode 1 (SmoothGrad): attr = acc (x, base unused).  maps [T][N][HW] = the sum over c (ascending) of |attr|.  sums [T][N]
 *   float64 = the sum of attr over (c, p) by a fixed tree: per-workgroup partials (partials: float64 workspace of T * N *
 *   sm3_attr_finish_blocks(HW) values, stored plainly), then one launch adding a row's partials in index order.  HW a multiple
 *   of 4, T * N <= 65535.
 * Sizes are checked on the host (SM3_EINVAL / SM3_EALIGN) before anything is launched.  No atomics.
 * ------------------------------------------------------------------------------------------ */
int sm3_attr_path(const float* x, const float* base, int base_n, float* out, int N, int64_t E, int k0, int c, int steps,
                  void* stream);
int sm3_attr_noise(const float* x, const float* sigma, float* out, int N, int64_t E, int k0, int c, int stride, uint64_t seed,
                   void* stream);
int sm3_attr_accumulate(const float* g, float* acc, int c, int N, int64_t E, float weight, int squared, void* stream);
int sm3_attr_finish_blocks(int HW);
int sm3_attr_finish(const float* acc, const float* x, const float* base, int base_n, float* attr, float* maps, double* sums,
                    double* partials, int T, int N, int C, int HW, int mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deletion / insertion faithfulness curves of attribution maps (csrc/faith.hip; ABI 9, additive).  Integers and bit copies
 * only: no float arithmetic, no float atomics.
 * sm3_faith_rank: ranks [rows][HW] int32 of maps [rows][HW] f32 (finite), per row with IEEE comparisons (-0 == +0):
 *   ranks[p] = #{q : map[q] > map[p]} + #{q < p : map[q] == map[p]} -- descending by value, ties by ascending index, a
 *   permutation of 0 .. HW - 1 and a function of the map alone.  A stable least-significant-digit radix sort (4 passes of 8
 *   bits over order-preserving keys), one workgroup per row; workspace: sm3_faith_rank_workspace(rows, HW) bytes (8-byte
 *   aligned; the size query returns SM3_EINVAL when the byte count does not fit an int).  1 <= HW <= 2^24.
 * sm3_faith_compose: one modality's perturbed inputs of curve steps k0 .. k0 + c - 1 for every label:
 *   out [c][T][N][3][HW] = (ranks[n][t][p] < c_k) != invert ? base[n or 0][ch][p] : x[n][ch][p],  k = k0 + j,
 *   c_k = (k * HW) / steps in 64-bit integers (c_0 = 0, c_steps = HW); invert = 0: deletion, 1: insertion.  x [N][3][HW], base
 *   [base_n][3][HW] with base_n = 1 (shared) or N; ranks[n][t][p] is read at ranks[n * rank_stride_n + t * rank_stride_t + p]
 *   (strides in elements, multiples of 4).  0 <= k0, k0 + c <= steps + 1, 1 <= steps <= HW, HW a multiple of 4, N * T <=
 *   65535, every pointer 16-byte aligned (SM3_EALIGN otherwise).
 * Sizes are checked on the host (SM3_EINVAL / SM3_EALIGN) before anything is launched.
 * ------------------------------------------------------------------------------------------ */
int sm3_faith_rank_workspace(int rows, int HW);
int sm3_faith_rank(const float* maps, int* ranks, int rows, int HW, void* workspace, int64_t workspace_bytes, void* stream);
int sm3_faith_compose(const float* x, const float* base, int base_n, const int* ranks, int64_t rank_stride_n,
                      int64_t rank_stride_t, float* out, int N, int T, int HW, int k0, int c, int steps, int invert,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * RISE black-box saliency maps (Petsiuk et al., BMVC 2018; csrc/rise.hip; ABI 9, additive).  An image [3][H][W] f32, H * W a
 * multiple of 4 and at most 2^24; a grid of s x s cells, 1 <= s <= min(H, W, 30); cells ch = ceil(H / s), cw = ceil(W / s);
 * corner grid G x G bits, G = s + 2.  Mask i of modality m at pixel (y, x), with Y = y + oy, X = x + ox, gy = Y / ch, ry = Y % ch,
 * gx = X / cw, rx = X % cw:
 *   A = (ch - ry) (cw - rx) g[gy][gx] + (ch - ry) rx g[gy][gx + 1] + ry (cw - rx) g[gy + 1][gx] + ry rx g[gy + 1][gx + 1],
 *   mask = (float)A / (float)(ch * cw): one correctly rounded f32 division.  Masks are regenerated from table rows, never stored.
 * sm3_rise_table: table [c][36] uint32, row j for mask i = i0 + j: words 0 .. 31 the grid bits (bit gy * G + gx of the row,
 *   little-endian in the words), word 32 oy, word 33 ox, words 34 and 35 zero.  Philox4x32-10 (as sm3_attr_noise), key = (seed
 *   low word, seed high word), counter (q, i, modality, 1): bit 4q + l = (word l of call q) < thr, thr = floor(p * 2^32) in
 *   float64; call ceil(G * G / 4): oy = (w0 * ch) >> 32, ox = (w1 * cw) >> 32 in 64-bit integers.  0 < p < 1 with thr > 0,
 *   modality 0 or 1, 0 <= i0, i0 + c <= 2^20.  A row depends on (seed, modality, i, H, W, s, p) alone.
 * sm3_rise_compose: out [c][N][3][HW] = base + mask_j * (x - base) as fadd(base, fmul(mask, fsub(x, base))), three separately
 *   rounded f32 operations, the three channels of a pixel with the pixel's mask value; table: the rows of the c masks; x
 *   [N][3][HW], base [base_n][3][HW] with base_n = 1 (shared) or N; N <= 65535, c <= 524 280 (groups of 8 masks on one grid
 *   axis of 65 535).
 * sm3_rise_accumulate: maps[n][t][p] (at maps[n * stride_n + t * stride_t + p], strides in elements, multiples of 4) =
 *   acc / d, acc = (((0 + w[0][r] * mask_0[p]) + w[1][r] * mask_1[p]) + ...) over all M masks in ascending order, every product
 *   and sum rounded on its own, r = n * T + t, weights [M][N * T] f32, table [M][36], d = (float)((double)M * p).  A thread owns 4
 *   pixels x 8 rows.  1 <= M <= 2^20.
 * Every pointer 16-byte aligned (weights: 4), SM3_EALIGN otherwise; sizes are checked on the host (SM3_EINVAL) before anything
 * is launched.  No atomics: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------ */
int sm3_rise_table(uint32_t* table, int i0, int c, int modality, int H, int W, int s, double p, uint64_t seed, void* stream);
int sm3_rise_compose(const float* x, const float* base, int base_n, const uint32_t* table, float* out, int N, int H, int W, int s,
                     int c, void* stream);
int sm3_rise_accumulate(const uint32_t* table, const float* weights, float* maps, int64_t stride_n, int64_t stride_t, int N, int T,
                        int M, int H, int W, int s, double p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation report: the integer counts behind AUROC, Recall, Spec and Prec of every (label, class) column, for the point
 * estimate and for case-resampling bootstrap replicates (csrc/report.hip, sm3hip/report.py; ABI 9, additive).
 * N cases, T labels, K columns; colmap [K][2] int32 = (label t, class c) of column k;
 * targets, yhat [N][T] int32 (class indices below 256; yhat = the predicted class, lowest index of the row maximum);
 * per column the score softmax(logits_t.double())[:, c] sorted ascending and stably ONCE: order [K][N] int32 = the case at sorted
 * position j, gs / ge [K][N] int32 = first and one-past-last sorted position of j's tie group (ties by == on the fp64 scores).
 * With integer case multiplicities m[n] >= 0, sum m = N:
 *   P = sum m[y == c], Q = N - P, S[j] = sum of m over the negative cases at sorted positions < j,
 *   A2 = sum over positive j of m_j * (S[gs[j]] + S[ge[j]])   (twice the negatives strictly below, plus the tied negatives),
 *   TP = sum m[y == c & yhat == c], FP = sum m[y != c & yhat == c], FN = sum m[y == c & yhat != c]   (TN = N - TP - FP - FN),
 * so that AUC = A2 / (2 P Q), Recall = TP / (TP + FN), Spec = TN / (TN + FP), Prec = TP / (TP + FP), one fp64 division each on
 * the host, 0 when the denominator is 0.
 * sm3_report_counts: out [c][K][6] int64 = (A2, P, Q, TP, FP, FN) for replicates r = r0 .. r0 + c - 1, one workgroup per
 *   (replicate, label); a column whose label is outside [0, T) is left unwritten.
 *   point != 0: m = 1 everywhere, c must be 1, no random words.  Otherwise draw d, 0 <= d < N, hits case (w * N) >> 32 in 64-bit
 *   integers, w = word d % 4 of Philox4x32-10 (as sm3_attr_noise), key = (seed low word, seed high word), counter (d / 4, r, 0, 2)
 *   -- the last word keeps the stream apart from SmoothGrad's 0 and RISE's 1 -- and m_r[i] = the number of draws that hit case
 *   i, shared by all columns.  A replicate is a function of (seed, r, N) alone.  1 <= N <= sm3_report_max_cases() (8192: m and S
 *   live in LDS), 1 <= T <= 64, 1 <= K <= 64, c >= 1, 0 <= r0, r0 + c <= 2^32; SM3_EINVAL otherwise, before anything is
 *   launched.  Entries of order are clamped to N - 1 and of gs / ge to N: no input can make an access leave its array.
 *   Integer sums only, no float anywhere: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------ */
int sm3_report_max_cases(void);
int sm3_report_counts(const int* order, const int* gs, const int* ge, const int* targets, const int* yhat, const int* colmap,
                      int64_t* out, int N, int T, int K, uint64_t seed, int64_t r0, int c, int point, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibration report: the integer bin tables behind ECE, MCE and the reliability diagram and the integer sums behind NLL and
 * the Brier score, for the point estimate and for case-resampling bootstrap replicates (csrc/calib.hip,
 * sm3hip/calibration.py; ABI 9, additive).
 * N cases, S series, X plain sums, T labels, M bins.  A series s is q [S][N] int64 (a probability in Q32, rint(p * 2^32), 0 <= q
 * <= 2^32) with the event ev [S][N] uint8 (0 / 1; any non-zero byte counts as 1); order [S][N] int32 = the case at sorted
 * position j of the series' stable ascending sort by q (a permutation of the cases); slabel [S] int32 = the label of series s;
 * xq [X][N] int64 = the per-case terms of plain sum x (each below 2^43, so that N of them stay below 2^56).
 * With integer case multiplicities m[n] >= 0, sum m = N:
 *   binning 0 (width): every copy of case n goes to bin min((q * M) >> 32, M - 1), in 64-bit integers;
 *   binning 1 (mass):  the case at sorted position j owns the copy ranks [R_j, R_j + m_j), R_j = the sum of m over the
 *                      positions < j; the copy at rank u goes to bin (u * M) / N (integer division), so a case whose ranks
 *                      straddle a boundary is split copy by copy, and M > N leaves empty bins;
 *   per series and bin: n_b = copies, E_b = sum of the copies' ev, Q_b = sum of the copies' q;  per plain sum: sum m[n] xq[x][n].
 * sm3_calib_counts: bins [c][S][M][3] int64 = (n_b, E_b, Q_b) and sums [c][X] int64 for replicates r = r0 .. r0 + c - 1, one
 *   workgroup per (replicate, label), which serves the series of its label and the plain sums x with x % T == label; a series
 *   whose label is outside [0, T) is left unwritten.  point != 0: m = 1 everywhere, c must be 1, no random words.  Otherwise
 *   m_r is the multiplicity vector of sm3_report_counts, exactly: draw d hits case (w * N) >> 32, w = word d % 4 of
 *   Philox4x32-10, key = (seed low word, seed high word), counter (d / 4, r, 0, 2) -- with one seed, replicate r of both
 *   reports resamples the same cases.  1 <= N <= sm3_report_max_cases(), 1 <= S, X, T <= 64, 1 <= M <= 64, binning 0 or 1,
 *   c >= 1, 0 <= r0, r0 + c <= 2^32; SM3_EINVAL otherwise, before anything is launched.  Entries of order are clamped to
 *   N - 1 and bin indices to M - 1: no input can make an access leave its array.  Integer sums only, no float anywhere: equal
 *   inputs give equal bits.
 * ------------------------------------------------------------------------------------------ */
int sm3_calib_counts(const int64_t* q, const uint8_t* ev, const int* order, const int* slabel, const int64_t* xq, int64_t* bins,
                     int64_t* sums, int N, int S, int X, int T, int M, int binning, uint64_t seed, int64_t r0, int c, int point,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Operating-point report: the integer counts behind average precision, the Youden and F1 optima, sensitivity at a specificity
 * floor, specificity at a sensitivity floor and the counts at given thresholds, for the point estimate and for case-resampling
 * bootstrap replicates (csrc/operating.hip, sm3hip/operating.py; ABI 9, additive).
 * N cases, T labels, K columns; colmap, targets, order, gs, ge as sm3_report_counts (the same ranking).  With integer case
 * multiplicities m[n] >= 0, sum m = N:
 *   Ppre[j] / S[j] = sum of m over the positive / negative cases at sorted positions < j,  P = Ppre[N],  Q = S[N];
 *   an operating point is a group start a (gs[a] == a: "positive iff score >= the group's value") or the empty point a = N;
 *   TP(a) = P - Ppre[a], FP(a) = Q - S[a].  Groups whose cases all have m = 0 stay points: they repeat a neighbour's counts and
 *   matter for the tie-breaks alone.
 *   APN    = sum over groups [a, b) of dTP * precQ, dTP = Ppre[b] - Ppre[a], precQ = (TP * 2^32 + den / 2) / den in integer
 *            division, den = TP + FP at a; a group with dTP = 0 contributes 0 and its quotient is never formed;
 *   Youden = the point that maximises (TP * Q - FP * P, a);
 *   F1     = the point that maximises 2 TP / (TP + FP + P), compared by cross-multiplication in int64, then a;
 *   sens at spec floor sigma [Ls] int64 (floor(s0 * 2^32), 0 .. 2^32): among the points with (Q - FP) * 2^32 >= sigma * Q the
 *            one that maximises (TP, -FP, a);
 *   spec at sens floor rho [Lr] int64 (floor(r0 * 2^32)): among the points with TP * 2^32 >= rho * P the one that maximises
 *            (-FP, TP, a);
 *   fixed  = (TP(f), FP(f)) at the positions fixpos [K][Lt] int32 (0 .. N; the host's searchsorted of a threshold).
 *   Each search is a maximum under a total order, so no reduction order shows.
 * sm3_operating_counts: out [c][K][9 + 3 Ls + 3 Lr + 2 Lt] int64 = (P, Q, APN, Youden (TP, FP, a), F1 (TP, FP, a), Ls x (TP, FP,
 *   a), Lr x (TP, FP, a), Lt x (TP, FP)) for replicates r = r0 .. r0 + c - 1, one workgroup per (replicate, label); a column whose
 *   label is outside [0, T) is left unwritten.  point != 0: m = 1 everywhere, c must be 1, no random words.  Otherwise m_r is the
 *   multiplicity vector of sm3_report_counts, exactly (Philox4x32-10, key = the seed, counter (d / 4, r, 0, 2), case (w * N) >>
 *   32): with one seed, replicate r of the three reports resamples the same cases.  1 <= N <= sm3_report_max_cases(), 1 <= T
 *   <= 64, 1 <= K <= 64, 0 <= Ls, Lr, Lt <= sm3_operating_max_levels() (32; a list of length 0 may be a null pointer), c >= 1,
 *   0 <= r0, r0 + c <= 2^32; SM3_EINVAL otherwise, before anything is launched; out, sigma and rho 8-byte aligned (SM3_EALIGN).
 *   Entries of order are clamped to N - 1, of gs / ge / fixpos to N and of sigma / rho to [0, 2^32]: no input can make an
 *   access leave its array.  Integers only, no float anywhere: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------ */
int sm3_operating_max_levels(void);
int sm3_operating_counts(const int* order, const int* gs, const int* ge, const int* targets, const int* colmap, const int64_t* sigma,
                         const int64_t* rho, const int* fixpos, int64_t* out, int N, int T, int K, int Ls, int Lr, int Lt,
                         uint64_t seed, int64_t r0, int c, int point, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cross-modal retrieval report: what lies between S = query . gallery^T and Recall@k, mean / median rank and MRR, for the point
 * estimate and for case-resampling bootstrap replicates (csrc/retrieval.hip, sm3hip/retrieval.py; ABI 9, additive).
 * N cases; row i of the queries and row i of the gallery belong to case i.  For j != i, b[i][j] = 1 iff S[i][j] > S[i][i], or
 * S[i][j] == S[i][i] and j < i (the lower index wins a tie, as in sm3_knn_vote); b[i][i] = 0.  Packed: bits [N][W] uint32,
 * W = ceil(N / 32), bit j & 31 of word j >> 5; the bits of j >= N are 0.  With integer case multiplicities m[n] >= 0, sum m = N:
 *   rho_i = sum_j m_j b[i][j]  (0-based rank; copies of case i in the gallery are its positive, not competitors),
 *   H_l = sum_i m_i [rho_i < k_l],  R = sum_i m_i rho_i,  Q = sum_i m_i floor(2^32 / (rho_i + 1)),
 *   M   = the least rho with 2 sum_i m_i [rho_i <= rho] >= N  (the lower weighted median).
 * sm3_retrieval_beats: for the n query rows q0 .. q0 + n - 1, whose similarities are the rows of S [n][ld] f32 (row r is query
 *   q0 + r, its positive is column q0 + r; columns N .. ld - 1 are not read): bits [n][W], rank [n] int32 = rho with m = 1, and
 *   term [n] f64 = log sum_{j < N} exp(S[r][j] / tau) - S[r][q0 + r] / tau, S widened to f64 before the division, the row maximum
 *   subtracted inside the exponential, the sum taken lane-strided in ascending j and folded by one shuffle tree: an order that
 *   depends on N alone.  One wave per row, the row is read once.  S must be finite (the caller checks).  1 <= N <=
 *   sm3_report_max_cases(), n >= 1, 0 <= q0, q0 + n <= N, ld >= N, 0 < tau < inf; SM3_EINVAL otherwise, before anything is
 *   launched; term 8-byte, the others 4-byte aligned (SM3_EALIGN).
 * sm3_retrieval_counts: out [c][L + 3] int64 = (H_1 .. H_L, R, Q, M) for replicates r = r0 .. r0 + c - 1, one workgroup per
 *   replicate.  ks [L] int32 is HOST memory (copied into the launch), 1 <= L <= 8, 1 <= k <= sm3_report_max_cases().  point != 0:
 *   m = 1 everywhere, c must be 1, no random words.  Otherwise m_r is the multiplicity vector of sm3_report_counts, exactly
 *   (Philox4x32-10, key = the seed, counter (d / 4, r, 0, 2), case (w * N) >> 32): with one seed, replicate r of the four reports
 *   resamples the same cases.  m is split into bit-planes M_p [W] in LDS (bit j of plane p = bit p of m_j), P = the bits of
 *   max m, and rho_i = sum_w sum_p 2^p popcount(bits[i][w] & M_p[w]); the planes are 0 past N, so whatever the padding bits of
 *   `bits` hold, rho <= N and no access leaves its array.  1 <= N <= sm3_report_max_cases(), c >= 1, 0 <= r0, r0 + c <= 2^32;
 *   SM3_EINVAL otherwise, before anything is launched; out 8-byte, bits 4-byte aligned (SM3_EALIGN).  Integers only, no float
 *   anywhere: a replicate is a function of (seed, r, N, bits) alone.
 * ------------------------------------------------------------------------------------------ */
int sm3_retrieval_beats(const float* S, int64_t ld, int n, int q0, int N, double tau, uint32_t* bits, int32_t* rank, double* term,
                        void* stream);
int sm3_retrieval_counts(const uint32_t* bits, int N, const int32_t* ks, int L, int64_t* out, uint64_t seed, int64_t r0, int c,
                         int point, void* stream);

/* ------------------------------------------------------------------------------------------
 * Seven-point checklist report: the integer counts behind "melanoma by checklist score" -- the joint table of the predicted
 * score, the annotated score and the diagnosis, and the AUROC counts of three continuous rankings -- for the point estimate and
 * for case-resampling bootstrap replicates (csrc/checklist.hip, sm3hip/checklist.py; ABI 9, additive).
 * N cases.  packed [N] int32 = shat | sstar << 4 | mel << 8: shat / sstar = the checklist score (0 .. 10) of the predicted / the
 * annotated criteria, mel = 1 iff the case is a melanoma (bits above the ninth are ignored, a score above 10 counts as 10).
 * order, gs, ge [3][N] int32: three rankings as sm3_report_counts' (ascending, stable, gs / ge = first and one-past-last sorted
 * position of a position's tie group).  With integer case multiplicities m[n] >= 0, sum m = N:
 *   J[shat][sstar][mel] = sum of m over the cases with that triple (11 x 11 x 2 = 242 entries, mel fastest);
 *   per ranking, with "positive" = melanoma: S[j] = sum of m over the negatives at positions < j,
 *   A2 = sum over positive j of m_j * (S[gs[j]] + S[ge[j]]),  P = sum of m over the positives,  Q = N - P.
 * sm3_checklist_counts: out [c][sm3_checklist_record() = 251] int64 = (J (242), 3 x (A2, P, Q)) for replicates r = r0 .. r0 + c -
 *   1; one workgroup per (replicate, part) -- part 0 the table, parts 1 .. 3 the rankings -- for a launch of at most 256
 *   replicates, one workgroup per replicate beyond; both write the same integers, every entry of every record.  point != 0: m =
 *   1 everywhere, c must be 1, no random words.  Otherwise m_r is the multiplicity vector of sm3_report_counts, exactly
 *   (Philox4x32-10, key = the seed, counter (d / 4, r, 0, 2), case (w * N) >> 32): with one seed, replicate r of the five reports
 *   resamples the same cases.  1 <= N <= sm3_report_max_cases(), c >= 1, 0 <= r0, r0 + c <= 2^32; SM3_EINVAL otherwise, before
 *   anything is launched; out 8-byte aligned (SM3_EALIGN).  Entries of order are clamped to N - 1 and of gs / ge to N: no input
 *   can make an access leave its array.  Integers only, no float anywhere: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------ */
int sm3_checklist_record(void);
int sm3_checklist_counts(const int* packed, const int* order, const int* gs, const int* ge, int64_t* out, int N, uint64_t seed,
                         int64_t r0, int c, int point, void* stream);

/* ------------------------------------------------------------------------------------------
 * Conformal prediction-set report: split conformal thresholds from a calibration split, refitted in every bootstrap
 * replicate, and the set counts of a test split under them (csrc/conformal.hip, sm3hip/conformal.py; ABI 9,
 * additive).  Integers only.
 *   cal_a [T][N_cal] int64 = the true-class score of a calibration case for label t; cal_order [T][N_cal] = the cases in
 *   ascending cal_a, ties by case index (one stable sort per label); cal_y [N_cal][T], y [N][T] the classes; s [K][N] int64 the
 *   score of column k = (label, class) = colmap[k], classes 0 .. 4; alpha: A levels (num, den) in HOST memory, the level is
 *   num / den.  With multiplicities w on the calibration cases:
 *     conditional 0 (marginal): n' = sum w = N_cal; conditional 1 (class): per class c of the label over the cases with y = c,
 *       n' = sum w [y = c];
 *     k = (n' + 1) - ((n' + 1) * num) / den in int64, integer division;
 *     qhat = cal_a at the first position j of cal_order (of the class) with R_j + w_j >= k, R_j = the sum of w (of the class)
 *       before j; qhat = 2^40, above any score, where k > n'.  The marginal qhat is the threshold of every class of the label.
 *   With multiplicities m on the test cases, the set of case n is {c : s[col(t, c)][n] <= thr[c]} and the record of a (label,
 *   level) is 24 int64: cov = sum m [true class in set], size = sum m |set|, single_hit = sum m [|set| = 1 and covered],
 *   hist[0 .. 5] = sum m [|set| = k], then for c = 0 .. 4: n_c = sum m [y = c], cov_c = sum m [y = c][c in set], in_c = sum m
 *   [c in set]; the slots of classes the label lacks are 0.  A y outside the label's classes counts in hist and size, is never
 *   covered and belongs to no class.
 * sm3_conformal_counts: counts [c][T][A][24] and thr [c][T][A][5] (the thresholds used; 0 in the slots of classes the label
 *   lacks) for replicates r = r0 .. r0 + c - 1, one workgroup per (replicate, label).  point != 0: w = m = 1, c must be 1.
 *   Otherwise m_r is the multiplicity vector of sm3_report_counts (counter (d / 4, r, 0, 2)) on N, and w_r follows the same
 *   rule on N_cal with counter (d / 4, r, 0, 6), both with key = (seed low word, seed high word).  fixed_thr: NULL, or
 *   [T][A][5] int64 thresholds used in every replicate instead of refitting (thr then repeats them).  1 <= N_cal, N <=
 *   sm3_report_max_cases(), 1 <= T <= 64, 1 <= K <= 256, 1 <= A <= 8, every level with 0 < num < den, conditional 0 or 1,
 *   c >= 1, 0 <= r0, r0 + c <= 2^32; SM3_EINVAL otherwise, before anything is launched.  Entries of cal_order are clamped to
 *   N_cal - 1 and those of cal_y to the label's classes: no input can make an access leave its array.
 * ------------------------------------------------------------------------------------------ */
int sm3_conformal_counts(const int64_t* cal_a, const int* cal_order, const int* cal_y, const int64_t* s, const int* y,
                         const int* colmap, const int* alpha, const int64_t* fixed_thr, int64_t* counts, int64_t* thr, int N_cal,
                         int N, int T, int K, int A, int conditional, uint64_t seed, int64_t r0, int c, int point, void* stream);

/* ------------------------------------------------------------------------------------------
 * Selective-prediction report: the integer counts behind the risk-coverage curve of "answer the confident cases, refer the
 * rest" -- its area, the 2 x 2 counts at fixed coverages, the largest coverage within a risk level, the counts at fixed
 * positions -- for the point estimate and for case-resampling bootstrap replicates (csrc/selective.hip, sm3hip/selective.py,
 * DESIGN.md 8.18; ABI 9, additive).  Integers only.
 *   8 labels, N cases.  order [8][N] int32 = per label the cases ranked ONCE by the host, most confident first.  packed [8][N]
 *   int32 = the flags of case n for label t: 1 err (the prediction is wrong), 2 pos (the case is of the selected class), 4 call
 *   (the selected class is predicted), 8 last (the case's sorted position ends a tie group of the primary key); higher bits are
 *   ignored.  table [N + 1] int64 = PH of the harmonic tails: PH[0] = 0, PH[r] - PH[r - 1] = round(2^32 * sum_{k = r .. N} 1 / k).
 *   kcuts [G] int32 in 1 .. N; risks [H][2] int32 = (a, b), the level a / b, 0 <= a <= b, 1 <= b; pcuts [8][Pc] int32 in 0 .. N.
 *   With integer case multiplicities m[n] >= 0, sum m = N, the case at sorted position j owns the copy ranks C_j + 1 .. C_j +
 *   m_j, C_j = the copies before j; E_j, TP_j, FP_j, FN_j = the err / call & pos / call & !pos / !call & pos copies before j.
 *   The record of a (replicate, label), sm3_selective_record(G, H, Pc) = 3 + 4 G + 2 H + 5 Pc int64:
 *     A = the sum over the err positions j of table[C_j + m_j] - table[C_j];  E = the err copies;  P = the pos copies;
 *     G x (err, TP, FP, FN) among the first k copies (the position that straddles k gives k - C_j of its copies);
 *     H x (the largest C_{j+1} over the positions j with `last`, C_{j+1} >= 1 and E_{j+1} * b <= a * C_{j+1}; the E_{j+1} there),
 *         (0, 0) where no position qualifies;
 *     Pc x (C_p, E_p, TP_p, FP_p, FN_p), p = N: the totals.
 * sm3_selective_counts: out [c][8][record] for replicates r = r0 .. r0 + c - 1, one workgroup per (replicate, label); every entry
 *   of every record is written.  point != 0: m = 1 everywhere, c must be 1, no random words.  Otherwise m_r is the multiplicity
 *   vector of sm3_report_counts, exactly (counter (d / 4, r, 0, 2)): with one seed, replicate r of every report resamples the same
 *   cases.  1 <= N <= sm3_report_max_cases(), 1 <= G <= 16, 0 <= H <= 8, 0 <= Pc <= 8, c >= 1, 0 <= r0, r0 + c <= 2^32, no null
 *   pointer (risks / pcuts may be null where H / Pc is 0); SM3_EINVAL otherwise, before anything is launched; table and out
 *   8-byte aligned (SM3_EALIGN).  Entries of order are clamped to N - 1 and the cuts and levels to the ranges above: no input can
 *   make an access leave its array.  No float anywhere, no global atomics: a record is a function of (inputs, seed, r, N) alone.
 * ------------------------------------------------------------------------------------------ */
int sm3_selective_record(int G, int H, int Pc);
int sm3_selective_counts(const int* packed, const int* order, const int64_t* table, const int* kcuts, const int* pcuts,
                         const int* risks, int64_t* out, int N, int G, int H, int Pc, uint64_t seed, int64_t r0, int c, int point,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Significance of a paired comparison: the integer counts behind the paired randomisation (permutation) test of two sets of
 * predictions of the same cases, and the integer placements behind DeLong's test (csrc/signif.hip, sm3hip/significance.py,
 * DESIGN.md 8.14; ABI 9, additive).
 * N cases, T labels, K columns; colmap, targets as sm3_report_counts; yhat_a, yhat_b [N][T] int32 = the two models' predicted
 * classes.  Per column the 2N scores are ranked jointly: element e = 2 i + w is model w's score of case i (w = 0: a, 1: b),
 * sorted ascending and stably once; order, gs, ge [K][2N] int32 = the element at joint position j and the bounds of j's tie group.
 * Replicate r swaps case i iff bit i & 31 of swap word i >> 5 is set, swap word d = word d % 4 of Philox4x32-10 (as
 * sm3_attr_noise), key = (seed low word, seed high word), counter (d / 4, r, 0, 5) -- stream 5, apart from 0 to 4.  Side A' takes
 * element w == swap_i of every case, side B' the other, yhat with it.  Per side, with positive = (y == c):
 *   S[j] = the side's negative elements at joint positions < j,  A2 = sum over the side's positive elements j of (S[gs[j]] +
 *   S[ge[j]]),  TP / FP = the side's elements with yhat == c that are positive / negative.
 * sm3_signif_counts: out [c][K][2][3] int64 = (A2, TP, FP) of A' then B' for replicates r = r0 .. r0 + c - 1, one workgroup per
 *   (replicate, label); a column whose label is outside [0, T) is left unwritten.  point != 0: nothing is swapped, c must be 1,
 *   no random words.  A replicate is a function of (seed, r, N) alone.  1 <= N <= sm3_report_max_cases() (the case words and the
 *   packed prefix sums of the 2N positions live in LDS), 1 <= T <= 64, 1 <= K <= 64, c >= 1, 0 <= r0, r0 + c <= 2^32; SM3_EINVAL
 *   otherwise, before anything is launched; out 8-byte aligned (SM3_EALIGN).  Entries of order are clamped to 2N - 1 and of gs /
 *   ge to 2N: no input can make an access leave its array.  Integers only, no atomics, no float anywhere.
 * sm3_signif_placements: order, gs, ge [K][N] as sm3_report_counts' (ONE model's own ranking).  out [K][N] int32 in case order:
 *   for a positive case 2 * (negatives ranked below) + tied negatives, in [0, 2Q]; for a negative case 2 * (positives ranked
 *   above) + tied positives, in [0, 2P].  One workgroup per column; every entry is written when order is a permutation.
 *   1 <= N <= sm3_report_max_cases(), 1 <= T, K <= 64; SM3_EINVAL otherwise; out 4-byte aligned.  The same clamps.
 * ------------------------------------------------------------------------------------------ */
int sm3_signif_counts(const int* order, const int* gs, const int* ge, const int* targets, const int* yhat_a, const int* yhat_b,
                      const int* colmap, int64_t* out, int N, int T, int K, uint64_t seed, int64_t r0, int c, int point,
                      void* stream);
int sm3_signif_placements(const int* order, const int* gs, const int* ge, const int* targets, const int* colmap, int32_t* out,
                          int N, int T, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact t-SNE maps of embeddings (csrc/tsne.hip, sm3hip/tsne.py; ABI 9, additive).  N points, 4 <= N <=
 * sm3_tsne_max_points() = 16384; every function refuses a null pointer or an N outside that range with SM3_EINVAL before anything
 * is launched, and a float / double pointer that is not 4 / 8-byte aligned with SM3_EALIGN (y: 8-byte, it is read as pairs).
 * No float atomics.  "The fixed order" of a sum over j: thread t of a 256-thread workgroup adds the terms j = t, t + 256, ... in
 * ascending j in fp64, then the 256 partials fold by the halving tree a[t] += a[t + h], h = 128, 64 .. 1 -- a function of the
 * terms and their number alone.  Products and sums are rounded separately (no contraction) unless fma is written.
 * sm3_tsne_sqdist: d2 [N][N] f32, d2[i][j] = sum_k (x_ik - x_jk)^2 as acc = fmaf(d, d, acc), k ascending, x [N][D] f32 row-major,
 *   1 <= D <= 4096; the diagonal is stored as 0; d2[i][j] and d2[j][i] are the same bits.
 * sm3_tsne_affinities: one workgroup per row i, fp64.  d'_j = d2[i][j] - min_{j != i} d2[i][j], e_j = exp(-(beta d'_j)),
 *   S0 = sum_{j != i} e_j, S1 = sum_{j != i} d'_j e_j (the fixed order), H = log S0 + beta S1 / S0.  From beta = 1, exactly 100
 *   steps of scikit-learn's _binary_search_perplexity (H > log perplexity: the lower end is beta, beta doubles while the upper end
 *   is infinite, else the midpoint; otherwise the mirror image), no tolerance.  cond [N][N] f32: cond[i][j] = e_j / S0 at the last
 *   beta, cond[i][i] = 0; beta [N] f64.  1 <= perplexity <= N - 1.  A row whose other points are all at one distance is uniform.
 * sm3_tsne_symmetrise: P[i][j] = f32((f64(cond[i][j]) + f64(cond[j][i])) / (2 N)); P must not be cond.
 * sm3_tsne_forces: one workgroup per point i; y [N][2] f32.  Per pair in f32: dx = y_i.x - y_j.x, dy likewise,
 *   q = fmaf(dy, dy, fmaf(dx, dx, 1)), w = 1 / q correctly rounded; widened to f64 and added over j != i in the fixed order:
 *   F[i] = (Z_i = sum w, A_i = sum (p_ij w) (dx, dy), R_i = sum (w w) (dx, dy)), F [N][5] f64.
 * sm3_tsne_update: one workgroup.  Z = sum_i Z_i (the fixed order); g = 4 (exaggeration A - R / Z); per coordinate, in f64 from
 *   the stored f32 state: gains + 0.2 where update g < 0, else gains 0.8, at least 0.01; update = momentum update - lr (gains g);
 *   y += update; each rounded once to f32 on store.  out [2] f64 = (sum_i ((gains g)_x^2 + (gains g)_y^2) in the fixed order, Z).
 *   exaggeration, momentum and lr must be finite.
 * sm3_tsne_kl: rows [N] f64 (scratch), rows[i] = sum_{j != i, p_ij > 0} p_ij ((log p_ij - log w_ij) + log Z), w as in
 *   sm3_tsne_forces, Z from F as in sm3_tsne_update; out[0] = sum_i rows[i], out[1] = Z, both in the fixed order; three launches.
 * ------------------------------------------------------------------------------------------ */
int sm3_tsne_max_points(void);
int sm3_tsne_sqdist(const float* x, int N, int D, float* d2, void* stream);
int sm3_tsne_affinities(const float* d2, int N, double perplexity, float* cond, double* beta, void* stream);
int sm3_tsne_symmetrise(const float* cond, int N, float* P, void* stream);
int sm3_tsne_forces(const float* P, const float* y, int N, double* F, void* stream);
int sm3_tsne_update(const double* F, int N, double exaggeration, double momentum, double lr, float* y, float* update, float* gains,
                    double* out, void* stream);
int sm3_tsne_kl(const float* P, const float* y, const double* F, int N, double* rows, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * L2-regularised multinomial logistic regression on cached features (csrc/logreg.hip, sm3hip/logreg.py; ABI 9,
 * additive).  X [N][D] f32 row-major, 1 <= N <= sm3_logreg_max_rows() = 16384, 1 <= D <= 4096; targets [N][8] int32; weights
 * [R][N] f64, all >= 0; table [P][4] int32 = (label, weight row, classes n_t of the label, 0) and Cs [P] f64 name the P problems.
 * Problem p: S = sum_i s_i over the classes of positive total weight ("present"), lambda = 1 / (C S),
 *   F(W, b) = (1 / S) sum_i s_i CE(softmax(W x_i + b), y_i) + (lambda / 2) |W|^2, the softmax over the present classes.
 * Per-class arrays have room for 8 classes: W, gW, coef [P][8][D], b, gb, intercept [P][8], logits [P][Q][8], all f64; rows
 * c >= n_t are written as 0.  One 256-thread workgroup owns one problem: its result does not depend on the other problems of the
 * launch (each problem reads X itself, on vector fma; the batched products are the lockstep solver's, below).  fp64 throughout, X
 * widened on load, no atomics, every sum in an order that (N, D, n_t) fix (csrc/logreg.hip states
 * them).  Every function refuses null pointers, sizes outside the caps and a workspace that is too small with SM3_EINVAL and a
 * misaligned pointer (4 bytes for f32 / int32, 8 for f64) with SM3_EALIGN before anything is launched; a table entry out of
 * range that reaches a kernel all the same is not followed (status 4, F = NaN).
 * sm3_logreg_workspace: the f64 elements of workspace ONE problem needs, of the fit (fit != 0) or of value_grad.
 * sm3_logreg_check_host: HOST arrays (what the device arrays will hold; n_classes [8]): SM3_EINVAL for a label outside [0, 8), a
 *   weight row outside [0, R), n_t that is not n_classes[label], a C that is not positive and finite, a class index of a used
 *   label outside [0, n_t), a weight that is negative or not finite.  Launches nothing, touches no device.
 * sm3_logreg_value_grad: F [P], gW, gb at the given W, b (an intercept of a class that is not present is not read).  A problem
 *   of total weight 0 gives zeros.
 * sm3_logreg_fit: L-BFGS (history 10) from zero until |grad F|_inf <= gtol or max_iter iterations.  A class that is not present
 *   gets coefficient row 0 and intercept -inf.  info [P][2] int32 = (status, iterations): 0 converged, 1 max_iter, 2 no step found,
 *   3 fewer than two present classes (nothing fitted), 4 bad table entry; res [P][2] f64 = (F, |grad F|_inf) at the returned point.
 *   A launch runs at most iters >= 1 iterations of every problem and saves each solver's state in ws; status 5 = not finished:
 *   call again with resume = 1 and the same arguments until no 5 is left (resume = 0 starts from zero).  The result does not
 *   depend on iters: the launches only bound the time one of them can take.
 * sm3_logreg_predict: logits[p][q][c] = coef[p][c] . Xq[q] + intercept[p][c] for c < nts[p] (k in the order of the fit's
 *   logits), Q <= 2^24, P <= 65535 a launch; a row's logits do not depend on the other rows.
 * ------------------------------------------------------------------------------------------ */
int sm3_logreg_max_rows(void);
int sm3_logreg_workspace(int N, int D, int fit, int64_t* doubles_per_problem);
int sm3_logreg_check_host(const int32_t* targets, const double* weights, const int32_t* table, const double* Cs,
                          const int32_t* n_classes, int N, int R, int P);
int sm3_logreg_value_grad(const float* X, const int32_t* targets, const double* weights, const int32_t* table, const double* Cs,
                          const double* W, const double* b, int N, int D, int R, int P, double* ws, int64_t ws_doubles, double* F,
                          double* gW, double* gb, void* stream);
int sm3_logreg_fit(const float* X, const int32_t* targets, const double* weights, const int32_t* table, const double* Cs, int N,
                   int D, int R, int P, double gtol, int max_iter, int resume, int iters, double* ws, int64_t ws_doubles, double* coef,
                   double* intercept, int32_t* info, double* res, void* stream);
int sm3_logreg_predict(const float* Xq, const double* coef, const double* intercept, const int32_t* nts, int Q, int D, int P,
                       double* logits, void* stream);

/* ------------------------------------------------------------------------------------------
 * The lockstep solver of the same problems (csrc/logreg.hip; ABI 9, additive): the problems of a call go through
 * every L-BFGS iteration side by side, and the two passes over X of an iteration are two batched products on
 * v_mfma_f64_16x16x4_f64 that all problems share.  Problems are COLUMNS: column j is one (problem, class) pair named by
 * cols [ncols] int32, cols[j] = 8 p + c, 1 <= ncols <= 8 P, the host lists the classes c < n_t of every problem; an entry
 * outside [0, 8 P) is not followed.  P <= 65535 a call.  Arrays and the caps are those above.
 * The orders of the sums depend on (N, D) alone -- not on P, a column's place or neighbours, the chunk, the calls, or which
 * problems are live:
 *   over features (logits):  groups of 16 features ascending; in a group four instructions j = 0 .. 3, instruction j adding the
 *                            features k0 + j, k0 + 4 + j, k0 + 8 + j, k0 + 12 + j; the intercept is added last;
 *   over rows (gradient):    slabs of sm3_logreg_lockstep_slab() = 2048 rows; in a slab groups of 16 rows ascending, the four
 *                            instructions of a group as above; the slabs' sums are stored plainly and added in slab order;
 *   gb and every scalar sum: thread t of 256 adds terms t, t + 256, ... ascending, then the halving tree.
 * No atomics; tails are zero operands; a row of weight 0 has residual exactly 0.
 * sm3_logreg_lockstep_workspace: the f64 elements one call of the fit (fit != 0) or of value_grad_lockstep needs for P problems in
 *   ncols columns (per-problem state, the slabs' partial sums, the modes).
 * sm3_logreg_batch_logits: Z[p][i][c] = sum_k X[i][k] V[p][c][k] + vb[p][c] for every column whose problem has active[p] != 0;
 *   V [P][8][D], vb [P][8] or null, Z [P][N][8].  Nothing of a problem with active[p] = 0 is written.
 * sm3_logreg_batch_grad: G[p][c][k] = sum_i Rm[p][i][c] X[i][k], gb[p][c] = sum_i Rm[p][i][c]; Rm [P][N][8], G [P][8][D], gb
 *   [P][8]; ws: at least ceil(N / 2048) * ncols * D f64 elements.  Nothing of a problem with active[p] = 0 is written.
 * sm3_logreg_value_grad_lockstep: what sm3_logreg_value_grad computes, through the two products.
 * sm3_logreg_fit_lockstep: what sm3_logreg_fit solves, by the same rules (history 10, the slope-bracketing line search, the
 *   certificate on fresh logits, statuses 0 .. 5).  A call enqueues iters (1 .. 1024) iterations of four steps -- per-problem
 *   direction kernel, logits product, per-problem line-search kernel, gradient product -- and returns; every problem's state lies
 *   in ws between two launches, a finished problem is not touched again.  Status 5 = not finished: call again with resume = 1.
 *   The result depends neither on iters nor on how the problems are split over calls.
 * ------------------------------------------------------------------------------------------ */
int sm3_logreg_lockstep_slab(void);
int sm3_logreg_lockstep_workspace(int N, int D, int P, int ncols, int fit, int64_t* doubles);
int sm3_logreg_batch_logits(const float* X, const double* V, const double* vb, const int32_t* cols, const int32_t* active, int N,
                            int D, int P, int ncols, double* Z, void* stream);
int sm3_logreg_batch_grad(const float* X, const double* Rm, const int32_t* cols, const int32_t* active, int N, int D, int P,
                          int ncols, double* ws, int64_t ws_doubles, double* G, double* gb, void* stream);
int sm3_logreg_value_grad_lockstep(const float* X, const int32_t* targets, const double* weights, const int32_t* table,
                                   const double* Cs, const int32_t* cols, const double* W, const double* b, int N, int D, int R,
                                   int P, int ncols, double* ws, int64_t ws_doubles, double* F, double* gW, double* gb,
                                   void* stream);
int sm3_logreg_fit_lockstep(const float* X, const int32_t* targets, const double* weights, const int32_t* table, const double* Cs,
                            const int32_t* cols, int N, int D, int R, int P, int ncols, double gtol, int max_iter, int resume,
                            int iters, double* ws, int64_t ws_doubles, double* coef, double* intercept, int32_t* info, double* res,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Test-time augmentation of the predictions (csrc/tta.hip, sm3hip/tta.py; ABI 9, additive).
 * sm3_tta_dihedral: out [rows][n_g][3][H][W] f32 from x [rows][3][H][W] f32: copy e is element g = elements[e] (a HOST array of
 *   n_g values 0 .. 7) of the dihedral group, g = fx | fy << 1 | tr << 2:
 *     out[r][e][ch][y][x] = x[r][ch][y'][x'],  a = fy ? H - 1 - y : y,  b = fx ? W - 1 - x : x,  (y', x') = tr ? (b, a) : (a, b)
 *   -- transpose the last two axes if tr, then reverse the rows if fy, then the columns if fx.  A pure copy (the bits of x).  Each
 *   32 x 32 source tile is read once, into a 32 x 33 dword LDS tile (conflict-free by rows and by columns), and stored once per
 *   element with every half-wave's store contiguous along the destination's x; edge tiles are clipped.  SM3_EINVAL, nothing
 *   launched: a null pointer, rows / H / W < 1, n_g outside 1 .. 8, an element outside 0 .. 7, a transposing element with
 *   H != W, more than 2^31 - 1 tiles.
 * sm3_tta_reduce: logits [B][V][24] f32, the 24 columns the classes of the 8 labels in the order 5, 3, 2, 3, 3, 3, 3, 2.  Per
 *   (case, view, label) in fp64: z = (double)logit, m = max z, e_c = exp(z_c - m), s = the sum of e_c in ascending c, p_c =
 *   e_c / s, q_c = rint(p_c * 2^32) as int64 (Q32, round half to even) -> q [B][V][24].  Over the views of a case: sum_q, min_q,
 *   max_q [B][24] int64.  view_class [B][V][8] int32: the lowest index of the maximum of the view's logits of the label;
 *   agg_class [B][8] int32: the lowest index of the maximum of sum_q among the label's classes; disagree [B][8] int32: the
 *   number of views with view_class != agg_class.  preds [B][24] f32 = (float)log((double)max(sum_q, 1) / (V * 2^32)): logits
 *   whose softmax is the mean probability.  One wave per case, lane = view; everything that crosses lanes is an integer sum,
 *   min, max or count, so no order of the views changes a bit.  The logits must be finite (the caller checks).  SM3_EINVAL: a
 *   null pointer, B < 1, V outside 1 .. 64.
 * ------------------------------------------------------------------------------------------ */
int sm3_tta_dihedral(const float* x, int rows, int H, int W, const int* elements, int n_g, float* out, void* stream);
int sm3_tta_reduce(const float* logits, int B, int V, int64_t* q, int64_t* sum_q, int64_t* min_q, int64_t* max_q,
                   int32_t* view_class, int32_t* agg_class, int32_t* disagree, float* preds, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image corruptions of the robustness report (csrc/corrupt.hip, sm3hip/corrupt.py, whose module text is the specification;
 * ABI 9, additive).  x, out: [B][3][H][W] f32 in [0, 1] on the device, the resampled image before Normalize; x != out.  Every
 * output element is a function of (image, operation, parameter, seed, case id, modality) alone.  Everything is checked before
 * anything is launched (SM3_EINVAL: a null pointer, B / H / W < 1, 3 H W > 2^31 - 1, and what each entry names).
 * sm3_corrupt_pointwise: op 0 gaussian_noise, out = clamp01(fadd(x, fmul((float)param, z))); op 1 impulse_noise, param = T as an
 *   integer in 0 .. 2^31: 0 where the element's word w < T, 1 where w >= 2^32 - T, else x; op 10 colour_cast, out =
 *   clamp01(fmul(x, g[ch])), g = (1 + c, 1, 1 - c) in f32, c = (float)param, reversed where the case word is odd.  ids: DEVICE
 *   int32 [B], the case's position in its split.  Philox4x32-10, key = seed (low word first); element e of a case's [3][H][W]
 *   image takes word e % 4 of counter (e / 4, id, modality << 16 | op << 8 | severity, 7), normals by sm3_attr_noise's rule;
 *   the case word is word 0 of counter (0xFFFFFFFF, id, op << 8 | severity, 7).  SM3_EINVAL: another op, severity outside
 *   1 .. 5, modality outside 0 .. 1, param outside [0, 1] (op 1: not an integer in 0 .. 2^31).
 * sm3_corrupt_taps: out[y][x] = (the sum over t < counts[k] of x[clamp(y + dy_t)][clamp(x + dx_t)], added in table order, every
 *   add rounded to f32) / counts[k], k = table_index[b].  tables: HOST int16 [n_tables][max_taps][2] (dy, dx), counts: HOST int32
 *   [n_tables], table_index: HOST int32 [B].  SM3_EINVAL: n_tables outside 1 .. 8, a count outside 1 .. max_taps, more than 336
 *   taps in all, an offset beyond +-10, a table index outside 0 .. n_tables - 1.
 * sm3_corrupt_pixelate: every pixel -> the mean of its f x f block (anchored at (0, 0); the in-image pixels added row-major,
 *   every add rounded, one division by their number).  SM3_EINVAL: f outside 1 .. 32, B > 65535.
 * sm3_corrupt_jpeg: a 4:4:4 baseline JPEG round trip in integers on 8 x 8 blocks of the edge-replicated image, with the HOST
 *   quantisation tables qt_luma, qt_chroma (int32 [64], [vertical][horizontal] frequency, as scaled for `quality`).
 *   SM3_EINVAL: quality outside 1 .. 100, a table entry outside 1 .. 255.
 * ------------------------------------------------------------------------------------------ */
int sm3_corrupt_pointwise(const float* x, int B, int H, int W, const int32_t* ids, int op, int severity, double param,
                          uint64_t seed, int modality, float* out, void* stream);
int sm3_corrupt_taps(const float* x, int B, int H, int W, const int16_t* tables, const int32_t* counts, int n_tables, int max_taps,
                     const int32_t* table_index, float* out, void* stream);
int sm3_corrupt_pixelate(const float* x, int B, int H, int W, int f, float* out, void* stream);
int sm3_corrupt_jpeg(const float* x, int B, int H, int W, int quality, const int32_t* qt_luma, const int32_t* qt_chroma, float* out,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
