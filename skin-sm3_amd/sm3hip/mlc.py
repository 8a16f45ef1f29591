"""Training of the multi-label heads on the HIP kernels (reference tools/mlc_train.py:58-90 `Model`,
:241-283 loop, :116-189 spherical k-means; tools/mlc_eval.py reuses the same model with biased prototypes).

    feats [B, 4096] -> S label projectors (--mlc-proj, src/models/projector.py) -> stack [S, B, D]
    -> nn.TransformerEncoderLayer(D, nhead, ff, dropout) in TRAIN mode over the S label tokens of each sample
    -> optional L2 norm -> per-label prototype Linear -> logits

Label projectors (mlc_train.py:352-361):
    v4      one biased Linear(4096, D) per label (S = 8): one GEMM + bias per label.
    v1-v3   per-label BN-MLPs (bias-free Linear -> BatchNorm1d -> ReLU, ..., BatchNorm1d(affine=False)).  A layer's
            activations for all labels are kept as ONE [B, S*C] tensor, label-major in the columns, so its S BatchNorm1d are
            one plain BatchNorm over S*C channels (bn_stats_reduce / bn_finalize / bn_act; backward bn_bwd_reduce /
            bn_bwd_apply) with the labels' gamma / beta / running buffers packed into banks (running statistics and
            num_batches_tracked written back to every label's module).  The first layer of all labels is ONE GEMM against the
            stacked [S*C, 4096] weights (every label reads the same features; its data gradient one GEMM with K = S*C); the
            per-label layers behind it are grouped GEMMs (sm3_grouped_gemm / sm3_grouped_wgrad_det: S groups, one launch).
            Each BatchNorm1d's own .training decides batch or running statistics (mlc_eval --finetune fc keeps the projectors
            in eval mode while the prototypes train; mlc_train's init_memory runs everything in eval mode).  Statistics are
            per rank, as in the reference (no SyncBatchNorm).
    v0      nn.Identity: ONE label token, the features themselves (S = 1, D = 4096).

Every Linear (forward, data gradient, weight gradient) is the exact-f32 MFMA gather-GEMM / weight-gradient kernel; the
attention over the 8 tokens, the two residual LayerNorms with their dropouts, bias + ReLU + dropout, the prototype heads
and the pseudo-label cross-entropy are csrc/heads_train.hip.  fp32 throughout, as the reference runs this part
(mlc_train.py:294-295).  One torch.autograd.Function spans the heads, so the frozen-extractor default
(mlc_train.py:347-348) and --finetune-backbone (gradient into the HIP encoders through sm3hip.bridge) both work, and the
caller keeps the reference's literal loop (CrossEntropyLoss on the predictions, torch.optim.AdamW).

A step is a function of its inputs: every float sum over rows (weight gradients: sm3_conv_wgrad_det; bias, LayerNorm and
prototype gradients and the k-means cluster sums: the sm3_mlc_*_det forms) has a fixed order, so two runs give the same bits.
SM3_WGRAD_DET=0 (read when the heads are built, or per clustering) runs the float-atomic forms instead, for A/B measurement."""
import os

import torch

from . import _lib, ops
from ._lib import SM3_F32, check

_P = ops._ptr


def _st():
    return ops._stream()


SLAB_ROWS = 256  # SM3_MLC_SLAB_ROWS: rows per slab of the fixed-order column sums


def _det_default():
    return os.environ.get("SM3_WGRAD_DET", "1") != "0"


def _nslab(rows):
    return (rows + SLAB_ROWS - 1) // SLAB_ROWS


def colsum_det(dy, db, groups=1, slabs=None):
    """db[g, :] += column sums of the g-th of `groups` row blocks of dy [groups * rows, N], fixed order (sm3_mlc_colsum_det)."""
    rows, N = dy.shape[0] // groups, dy.shape[1]
    if rows * groups != dy.shape[0] or db.numel() != groups * N:
        raise ValueError("colsum_det: dy [groups * rows, N], db [groups * N]")
    if slabs is None and _nslab(rows) > 1:
        slabs = torch.empty(_nslab(rows) * groups * N, dtype=torch.float32, device=dy.device)
    check(_lib.load().sm3_mlc_colsum_det(_P(dy), _P(db), _P(slabs), rows, N, groups, _st()), "sm3_mlc_colsum_det")


def heads_bwd_work(B, S, D, T, bias):
    """Floats of workspace sm3_mlc_heads_bwd_det needs."""
    return B * S + _nslab(B) * (T * D + (T if bias else 0))


def _projector_kind(projectors):
    """'v0' (nn.Identity), 'v4' (one biased Linear per label) or 'mlp' (v1 / v2 / v3) plus, for 'mlp', the layer list
    [(linear index, bn index, relu)] of one label's nn.Sequential."""
    if isinstance(projectors, torch.nn.Identity):
        return "v0", None
    seq = projectors.projectors[0]
    mods = list(seq)
    if len(mods) == 1 and isinstance(mods[0], torch.nn.Linear) and mods[0].bias is not None:
        return "v4", None
    layers, i = [], 0
    while i < len(mods):
        lin = mods[i]
        bn = mods[i + 1] if i + 1 < len(mods) else None
        if not isinstance(lin, torch.nn.Linear) or lin.bias is not None or not isinstance(bn, torch.nn.BatchNorm1d):
            raise NotImplementedError("label projectors: MultiLabelProjector{,2,3,4} of src/models/projector.py or nn.Identity")
        relu = i + 2 < len(mods) and isinstance(mods[i + 2], torch.nn.ReLU)
        layers.append((i, i + 1, relu))
        i += 3 if relu else 2
    return "mlp", layers


class MLCHeads:
    """Kernel sequencing for one `Model` (its projectors / mlc_sa / prototypes own the parameters)."""

    def __init__(self, model):
        self.model = model
        sa = model.mlc_sa
        if sa.norm_first or getattr(sa, "activation_relu_or_gelu", 1) != 1:
            raise NotImplementedError("only the post-norm ReLU TransformerEncoderLayer of mlc_train.py is built")
        self.kind, self.layers = _projector_kind(model.projectors)
        self.S = 1 if self.kind == "v0" else len(model.projectors.projectors)
        self.D = sa.self_attn.embed_dim
        if self.kind == "mlp":
            for s, seq in enumerate(model.projectors.projectors):
                for li, bi, _ in self.layers:
                    bn = seq[bi]
                    if not bn.track_running_stats or bn.momentum is None:
                        raise NotImplementedError("label projector BatchNorm1d: running statistics with a momentum")
            if model.projectors.projectors[0][self.layers[-1][0]].out_features != self.D:
                raise ValueError("label projector width must equal mlc_sa's d_model")
        self._bank_key, self._banks = None, None
        self.nhead = sa.self_attn.num_heads
        self.p = float(sa.dropout.p)
        if float(sa.self_attn.dropout) != self.p or float(sa.dropout1.p) != self.p or float(sa.dropout2.p) != self.p:
            raise NotImplementedError("one dropout rate for the whole layer, as nn.TransformerEncoderLayer builds it")
        self.sizes = [l.weight.shape[0] for l in model.prototypes]
        self.has_pbias = model.prototypes[0].bias is not None
        self.det = _det_default()  # fixed-order sums (SM3_WGRAD_DET=0: the float-atomic kernels)
        self._ws = None            # the slab workspace of the backward, grown on demand and reused by every site of a step

    def proj_params(self):
        m = self.model
        if self.kind == "v0":
            return []
        if self.kind == "v4":
            return [q for l in m.projectors.projectors for q in (l[0].weight, l[0].bias)]
        ps = []
        for seq in m.projectors.projectors:
            for li, bi, _ in self.layers:
                ps.append(seq[li].weight)
                if seq[bi].affine:
                    ps += [seq[bi].weight, seq[bi].bias]
        return ps

    def params(self):
        m, sa = self.model, self.model.mlc_sa
        ps = list(self.proj_params())
        ps += [sa.self_attn.in_proj_weight, sa.self_attn.in_proj_bias, sa.self_attn.out_proj.weight, sa.self_attn.out_proj.bias,
               sa.linear1.weight, sa.linear1.bias, sa.linear2.weight, sa.linear2.bias, sa.norm1.weight, sa.norm1.bias,
               sa.norm2.weight, sa.norm2.bias]
        for l in m.prototypes:
            ps.append(l.weight)
            if self.has_pbias:
                ps.append(l.bias)
        return ps

    # ---- primitives -----------------------------------------------------------------------------------------------
    @staticmethod
    def _gemm(x, w, out=None, addend=None):
        """out[rows, N] = x[rows, K] @ w[N, K]^T (+ addend), exact-f32 MFMA."""
        rows, K = x.shape
        N = w.shape[0]
        if out is None:
            out = torch.empty(rows, N, dtype=torch.float32, device=x.device)
        ops.conv_gemm(ops.fwd_desc(SM3_F32, rows, 1, 1, K, N, 1, 1, 0), x, w, out, addend, None)
        return out

    def _work(self, n, dev):
        """fp32 workspace of at least n floats, shared by the sequential launches of a backward on one stream."""
        if self._ws is None or self._ws.numel() < n or self._ws.device != dev:
            self._ws = torch.empty(max(n, 4), dtype=torch.float32, device=dev)
        return self._ws

    def _wgrad(self, x, dy, dw):
        """dw[N, K] += dy[rows, N]^T @ x[rows, K]."""
        rows, K = x.shape
        desc = ops.fwd_desc(SM3_F32, rows, 1, 1, K, dy.shape[1], 1, 1, 0)
        if not self.det:
            ops.conv_wgrad(desc, x, dy, dw)
            return
        n = dy.shape[1] * K
        cap = ops.grouped_wgrad_slab_cap(rows, n)
        # (capacity 1: one slice adds its tiles to dw itself and the slab buffer is never written)
        ops.conv_wgrad_det(desc, x, dy, dw, dw if cap == 1 else self._work(cap * n, x.device), cap)

    def _bias(self, y, bias, ones):
        rows, N = y.shape
        ops.bn_act(SM3_F32, y, ones[:N], bias, None, False, y, rows, N)

    def _colsum(self, dy, db, groups=1):
        if not self.det:
            check(_lib.load().sm3_mlc_colsum(_P(dy), _P(db), dy.shape[0], dy.shape[1], _st()), "sm3_mlc_colsum")
            return
        rows, N = dy.shape[0] // groups, dy.shape[1]
        colsum_det(dy, db, groups, self._work(_nslab(rows) * groups * N, dy.device) if _nslab(rows) > 1 else None)

    def _add_ln_bwd(self, dout, a, b, stats, gamma, p, seed, da, db, dgamma, dbeta):
        R, D = dout.shape
        if not self.det:
            check(_lib.load().sm3_mlc_add_ln_bwd(_P(dout), _P(a), _P(b), _P(stats), _P(gamma), p, seed, _P(da), _P(db), _P(dgamma),
                                                 _P(dbeta), R, D, _st()), "sm3_mlc_add_ln_bwd")
            return
        ws = self._work(_nslab(R) * 2 * D, dout.device)
        check(_lib.load().sm3_mlc_add_ln_bwd_det(_P(dout), _P(a), _P(b), _P(stats), _P(gamma), p, seed, _P(da), _P(db), _P(dgamma),
                                                 _P(dbeta), _P(ws), R, D, _st()), "sm3_mlc_add_ln_bwd_det")

    # ---- BN-MLP label projectors (v1 / v2 / v3) --------------------------------------------------------------------
    def _mlp_banks(self):
        """Per layer: the labels' Linear weights stacked [S*C, Cin] (layer 0: the one-GEMM form) or as S banks [S, C, Cin]
        (grouped), their transposes for the data gradient, and gamma / beta banks [S*C]; rebuilt when a parameter changes."""
        seqs = self.model.projectors.projectors
        ps = self.proj_params()
        key = tuple(q._version for q in ps) + tuple(q.data_ptr() for q in ps)
        if key == self._bank_key:
            return self._banks
        banks = []
        for j, (li, bi, relu) in enumerate(self.layers):
            w = torch.stack([seq[li].weight.detach() for seq in seqs], 0).contiguous()          # [S, C, Cin]
            S, C, Cin = w.shape
            wt = w.transpose(1, 2).contiguous()                                                   # [S, Cin, C]
            if j == 0:
                wt = w.reshape(S * C, Cin).t().contiguous()                                       # [Cin, S*C]
            aff = seqs[0][bi].affine
            g = torch.cat([seq[bi].weight.detach() for seq in seqs]).contiguous() if aff else None
            b = torch.cat([seq[bi].bias.detach() for seq in seqs]).contiguous() if aff else None
            banks.append(dict(w=w, wt=wt, C=C, Cin=Cin, gamma=g, beta=b, relu=relu))
        self._bank_key, self._banks = key, banks
        return banks

    def _mlp_forward(self, feats):
        """feats [B, in] -> [B, S*D] (label-major columns) and what the backward pass needs."""
        seqs, S, B, dev = self.model.projectors.projectors, self.S, feats.shape[0], feats.device
        banks, h, recs = self._mlp_banks(), feats, []
        for j, (li, bi, relu) in enumerate(self.layers):
            bk = banks[j]
            SC = S * bk["C"]
            bns = [seq[bi] for seq in seqs]
            train = bns[0].training
            if any(bn.training != train for bn in bns) or any(bn.eps != bns[0].eps for bn in bns):
                raise NotImplementedError("the labels' BatchNorm1d of one projector layer share mode and eps")
            y = torch.empty(B, SC, dtype=torch.float32, device=dev)
            prow = (B + 127) // 128
            part = torch.empty(prow, 2, SC, dtype=torch.float32, device=dev) if train else None
            if j == 0:
                ops.conv_gemm(ops.fwd_desc(SM3_F32, B, 1, 1, bk["Cin"], SC, 1, 1, 0), h, bk["w"].view(SC, bk["Cin"]), y, None, part)
            else:
                ops.grouped_gemm(h, bk["w"], y, S, part)
            scale = torch.empty(SC, dtype=torch.float32, device=dev)
            shift = torch.empty_like(scale)
            mean = invstd = None
            if train:
                if B < 2:
                    raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d)")
                rm = torch.cat([bn.running_mean for bn in bns]).contiguous()
                rv = torch.cat([bn.running_var for bn in bns]).contiguous()
                nbt = torch.zeros(1, dtype=torch.int64, device=dev)
                mean, invstd = torch.empty_like(scale), torch.empty_like(scale)
                ws, groups = ops.bn_stats_reduce(part, prow, SC, None)
                ops.bn_finalize(ws, B, SC, bk["gamma"], bk["beta"], bns[0].eps, float(bns[0].momentum), rm, rv, nbt, scale,
                                shift, mean, invstd, groups=groups)
                C = bk["C"]
                with torch.no_grad():
                    for s, bn in enumerate(bns):  # the running buffers stay in the labels' own modules
                        bn.running_mean.copy_(rm[s * C:(s + 1) * C])
                        bn.running_var.copy_(rv[s * C:(s + 1) * C])
                        bn.num_batches_tracked.add_(1)
            else:
                rm = torch.cat([bn.running_mean for bn in bns]).contiguous()
                rv = torch.cat([bn.running_var for bn in bns]).contiguous()
                ops.bn_eval_scale_shift(bk["gamma"], bk["beta"], rm, rv, bns[0].eps, SC, scale, shift)
            out = torch.empty_like(y)
            ops.bn_act(SM3_F32, y, scale, shift, None, relu, out, B, SC)
            recs.append(dict(x=h, y=y, out=out, mean=mean, invstd=invstd, train=train,
                             frozen=None if train else (rm, rv, bns[0].eps)))
            h = out
        return h, recs

    def _mlp_backward(self, recs, dh, need_dfeats, need_params):
        """dh [B, S*D] (label-major) -> projector parameter gradients (list in proj_params order, or None) and dfeats."""
        S, B, dev = self.S, dh.shape[0], dh.device
        banks = self._mlp_banks()
        grads_w, grads_g, grads_b = [None] * len(self.layers), [None] * len(self.layers), [None] * len(self.layers)
        dfeats = None
        for j in range(len(self.layers) - 1, -1, -1):
            bk, r = banks[j], recs[j]
            C, Cin = bk["C"], bk["Cin"]
            SC = S * C
            mean, invstd = r["mean"], r["invstd"]
            if not r["train"]:  # eval mode: the running statistics are constants (the encoders' frozen_stats form)
                rm, rv, eps = r["frozen"]
                mean, invstd = rm, torch.rsqrt(rv + eps)
            prow = ops.bn_bwd_partial_rows(B, SC)
            bpart = torch.empty(prow, 2, SC, dtype=torch.float32, device=dev)
            dz = torch.empty_like(dh)
            ops.bn_bwd_reduce(SM3_F32, dh, r["out"] if bk["relu"] else None, r["y"], mean, invstd, dz, B, SC, bpart)
            lsums = torch.empty(2 * SC, dtype=torch.float64, device=dev)
            ops.bn_stats_reduce(bpart, prow, SC, lsums)
            dgam = torch.zeros(SC, dtype=torch.float32, device=dev) if bk["gamma"] is not None else None
            dbet = torch.zeros(SC, dtype=torch.float32, device=dev) if bk["gamma"] is not None else None
            dy = torch.empty_like(dz)
            # eval mode: all-zero batch sums drop the mean(dz) / mean(dz * xhat) terms, so dy = gamma * invstd * dz, and
            # d(gamma), d(beta) are the plain sums
            gsums = lsums if r["train"] else torch.zeros_like(lsums)
            ops.bn_bwd_apply(SM3_F32, dz, r["y"], mean, invstd, bk["gamma"], gsums, B, lsums, dgam, dbet, dy, B, SC)
            grads_g[j], grads_b[j] = dgam, dbet
            if j == 0:
                if need_params:
                    dw = torch.zeros(SC, Cin, dtype=torch.float32, device=dev)
                    cap = ops.grouped_wgrad_slab_cap(B, SC * Cin)
                    # (capacity 1: one slice adds its tiles to dw itself and the slab buffer is never written)
                    slabs = dw if cap == 1 else torch.empty(cap * SC * Cin, dtype=torch.float32, device=dev)
                    ops.conv_wgrad_det(ops.fwd_desc(SM3_F32, B, 1, 1, Cin, SC, 1, 1, 0), r["x"], dy, dw, slabs, cap)
                    grads_w[j] = dw.view(S, C, Cin)
                if need_dfeats:
                    dfeats = torch.empty(B, Cin, dtype=torch.float32, device=dev)
                    ops.conv_gemm(ops.fwd_desc(SM3_F32, B, 1, 1, SC, Cin, 1, 1, 0), dy, bk["wt"], dfeats)
            else:
                if need_params:
                    dw = torch.zeros(S, C, Cin, dtype=torch.float32, device=dev)
                    cap = ops.grouped_wgrad_slab_cap(B, C * Cin)
                    slabs = dw if cap == 1 else None  # (see above)
                    ops.grouped_wgrad_det(r["x"], dy, dw, S, slabs)
                    grads_w[j] = dw
                dh = torch.empty(B, S * Cin, dtype=torch.float32, device=dev)
                ops.grouped_gemm(dy, bk["wt"], dh, S)
        if not need_params:
            return None, dfeats
        out = []
        for s in range(S):
            for j, (li, bi, relu) in enumerate(self.layers):
                C = banks[j]["C"]
                out.append(grads_w[j][s])
                if banks[j]["gamma"] is not None:
                    out += [grads_g[j][s * C:(s + 1) * C], grads_b[j][s * C:(s + 1) * C]]
        return out, dfeats

    # ---- forward / backward ---------------------------------------------------------------------------------------
    def forward(self, feats, seed, train=True):
        m, sa, lib = self.model, self.model.mlc_sa, _lib.load()
        if not feats.is_cuda or feats.dtype != torch.float32:
            raise ValueError("the SM3 HIP path has no CPU fallback; features must be fp32 CUDA")
        feats = feats.contiguous()
        dev, B, S, D = feats.device, feats.shape[0], self.S, self.D
        R, p = S * B, (self.p if train else 0.0)
        seed = int(seed) & 0x7FFFFFFF
        ones = torch.ones(max(3 * D, sa.linear1.out_features), dtype=torch.float32, device=dev)
        mlp = None
        if self.kind == "v4":
            x0 = torch.empty(R, D, dtype=torch.float32, device=dev)          # row = s*B + b (the reference's [S, B, D])
            for s, l in enumerate(m.projectors.projectors):
                blk = x0[s * B:(s + 1) * B]
                self._gemm(feats, l[0].weight.detach(), blk)
                self._bias(blk, l[0].bias.detach(), ones)
        elif self.kind == "v0":
            if feats.shape[1] != D:
                raise ValueError(f"--mlc-proj v0: features of width {feats.shape[1]} for d_model {D}")
            x0 = feats                                                        # the one label token (mlc_train.py:76-79)
        else:
            h, mlp = self._mlp_forward(feats)
            x0 = h.view(B, S, D).transpose(0, 1).contiguous().view(R, D)     # label-major columns -> [S, B, D] rows
        att = sa.self_attn
        qkv = self._gemm(x0, att.in_proj_weight.detach())
        self._bias(qkv, att.in_proj_bias.detach(), ones)
        a = torch.empty(R, D, dtype=torch.float32, device=dev)
        check(lib.sm3_mlc_attention_fwd(_P(qkv), _P(a), B, S, D, self.nhead, p, seed + 1, 1, _st()), "sm3_mlc_attention_fwd")
        o = self._gemm(a, att.out_proj.weight.detach())
        self._bias(o, att.out_proj.bias.detach(), ones)
        x1, st1 = torch.empty_like(x0), torch.empty(R, 2, dtype=torch.float32, device=dev)
        check(lib.sm3_mlc_add_ln_fwd(_P(x0), _P(o), _P(sa.norm1.weight.detach()), _P(sa.norm1.bias.detach()), sa.norm1.eps, p,
                                     seed + 2, _P(x1), _P(st1), R, D, _st()), "sm3_mlc_add_ln_fwd")
        y1 = self._gemm(x1, sa.linear1.weight.detach())
        F = y1.shape[1]
        h, hd = torch.empty_like(y1), torch.empty_like(y1)
        check(lib.sm3_mlc_bias_relu_drop_fwd(_P(y1), _P(sa.linear1.bias.detach()), p, seed + 3, _P(h), _P(hd), R, F, _st()),
              "sm3_mlc_bias_relu_drop_fwd")
        fo = self._gemm(hd, sa.linear2.weight.detach())
        self._bias(fo, sa.linear2.bias.detach(), ones)
        x2, st2 = torch.empty_like(x0), torch.empty(R, 2, dtype=torch.float32, device=dev)
        check(lib.sm3_mlc_add_ln_fwd(_P(x1), _P(fo), _P(sa.norm2.weight.detach()), _P(sa.norm2.bias.detach()), sa.norm2.eps, p,
                                     seed + 4, _P(x2), _P(st2), R, D, _st()), "sm3_mlc_add_ln_fwd")
        wp = torch.cat([l.weight.detach() for l in m.prototypes], 0).contiguous()          # [T, D]
        bp = torch.cat([l.bias.detach() for l in m.prototypes], 0).contiguous() if self.has_pbias else None
        T = wp.shape[0]
        tok = torch.tensor([i % S for i, n in enumerate(self.sizes) for _ in range(n)], dtype=torch.int32, device=dev)
        logits = torch.empty(B, T, dtype=torch.float32, device=dev)
        check(lib.sm3_mlc_heads_fwd(_P(x2), _P(wp), _P(bp), _P(tok), int(bool(m.l2_norm)), _P(logits), B, S, D, T, 1, _st()),
              "sm3_mlc_heads_fwd")
        saved = dict(feats=feats, mlp=mlp, x0=x0, qkv=qkv, a=a, o=o, x1=x1, st1=st1, h=h, hd=hd, fo=fo, x2=x2, st2=st2, wp=wp, tok=tok,
                     B=B, p=p, seed=seed)
        sa_feats = x2.view(S, B, D)
        if m.l2_norm:
            sa_feats = torch.nn.functional.normalize(sa_feats, dim=-1, p=2)
        return sa_feats, logits, saved

    def backward(self, sv, dlogits, need_dfeats, need_proj=True):
        m, sa, lib = self.model, self.model.mlc_sa, _lib.load()
        att = sa.self_attn
        B, S, D, p, seed = sv["B"], self.S, self.D, sv["p"], sv["seed"]
        R = S * B
        dev = dlogits.device
        z = lambda t: torch.zeros_like(t, dtype=torch.float32)
        skip = {id(q) for q in self.proj_params()} if self.kind == "mlp" else set()  # (filled by _mlp_backward, or None)
        pbias = None
        if self.kind == "v4" and self.det:  # the S label biases: one grouped column sum into a bank, handed out as views
            pbias = torch.zeros(S, D, dtype=torch.float32, device=dev)
            skip |= {id(l[0].bias) for l in m.projectors.projectors}
        g = {id(q): (None if id(q) in skip else z(q)) for q in self.params()}
        if pbias is not None:
            for s, l in enumerate(m.projectors.projectors):
                g[id(l[0].bias)] = pbias[s]
        G = lambda q: g[id(q)]
        dlogits = dlogits.contiguous().float()
        T = sv["wp"].shape[0]
        dx2 = torch.empty(R, D, dtype=torch.float32, device=dev)
        dwp = torch.zeros(T, D, dtype=torch.float32, device=dev)
        dbp = torch.zeros(T, dtype=torch.float32, device=dev) if self.has_pbias else None
        if self.det:
            ws = self._work(heads_bwd_work(B, S, D, T, self.has_pbias), dev)
            check(lib.sm3_mlc_heads_bwd_det(_P(dlogits), _P(sv["x2"]), _P(sv["wp"]), _P(sv["tok"]), int(bool(m.l2_norm)), _P(dx2),
                                            _P(dwp), _P(dbp), _P(ws), B, S, D, T, 1, _st()), "sm3_mlc_heads_bwd_det")
        else:
            check(lib.sm3_mlc_heads_bwd(_P(dlogits), _P(sv["x2"]), _P(sv["wp"]), _P(sv["tok"]), int(bool(m.l2_norm)), _P(dx2),
                                        _P(dwp), _P(dbp), B, S, D, T, 1, _st()), "sm3_mlc_heads_bwd")
        off = 0
        for l, n in zip(m.prototypes, self.sizes):
            G(l.weight).copy_(dwp[off:off + n])
            if self.has_pbias:
                G(l.bias).copy_(dbp[off:off + n])
            off += n
        # LayerNorm 2 (+ dropout2): d(x1 + drop(fo))
        dx1, dfo = torch.empty_like(dx2), torch.empty_like(dx2)
        self._add_ln_bwd(dx2, sv["x1"], sv["fo"], sv["st2"], sa.norm2.weight.detach(), p, seed + 4, dx1, dfo, G(sa.norm2.weight),
                         G(sa.norm2.bias))
        # feed-forward
        self._colsum(dfo, G(sa.linear2.bias))
        self._wgrad(sv["hd"], dfo, G(sa.linear2.weight))
        dhd = self._gemm(dfo, sa.linear2.weight.detach().t().contiguous())
        dh = torch.empty_like(dhd)
        check(lib.sm3_mlc_relu_drop_bwd(_P(dhd), _P(sv["h"]), p, seed + 3, _P(dh), _P(None if self.det else G(sa.linear1.bias)), R,
                                        dh.shape[1], _st()), "sm3_mlc_relu_drop_bwd")
        if self.det:
            self._colsum(dh, G(sa.linear1.bias))
        self._wgrad(sv["x1"], dh, G(sa.linear1.weight))
        self._gemm(dh, sa.linear1.weight.detach().t().contiguous(), out=dx1, addend=dx1)
        # LayerNorm 1 (+ dropout1): d(x0 + drop(o))
        dx0, do = torch.empty_like(dx2), torch.empty_like(dx2)
        self._add_ln_bwd(dx1, sv["x0"], sv["o"], sv["st1"], sa.norm1.weight.detach(), p, seed + 2, dx0, do, G(sa.norm1.weight),
                         G(sa.norm1.bias))
        # attention
        self._colsum(do, G(att.out_proj.bias))
        self._wgrad(sv["a"], do, G(att.out_proj.weight))
        da = self._gemm(do, att.out_proj.weight.detach().t().contiguous())
        dqkv = torch.empty(R, 3 * D, dtype=torch.float32, device=dev)
        check(lib.sm3_mlc_attention_bwd(_P(sv["qkv"]), _P(da), _P(dqkv), B, S, D, self.nhead, p, seed + 1, 1, _st()),
              "sm3_mlc_attention_bwd")
        self._colsum(dqkv, G(att.in_proj_bias))
        self._wgrad(sv["x0"], dqkv, G(att.in_proj_weight))
        self._gemm(dqkv, att.in_proj_weight.detach().t().contiguous(), out=dx0, addend=dx0)
        # label projectors
        dfeats = None
        if self.kind == "v0":
            return [g[id(q)] for q in self.params()], (dx0 if need_dfeats else None)
        if self.kind == "mlp":
            if not (need_proj or need_dfeats):
                return [g[id(q)] for q in self.params()], None
            dh = dx0.view(S, B, D).transpose(0, 1).contiguous().view(B, S * D)
            pg, dfeats = self._mlp_backward(sv["mlp"], dh, need_dfeats, need_proj)
            if pg is not None:
                for q, t in zip(self.proj_params(), pg):
                    g[id(q)] = t
            return [g[id(q)] for q in self.params()], dfeats
        if pbias is not None:
            self._colsum(dx0, pbias, groups=S)
        for s, l in enumerate(m.projectors.projectors):
            blk = dx0[s * B:(s + 1) * B]
            if pbias is None:
                self._colsum(blk, G(l[0].bias))
            self._wgrad(sv["feats"], blk, G(l[0].weight))
            if need_dfeats:
                wt = l[0].weight.detach().t().contiguous()
                if dfeats is None:
                    dfeats = self._gemm(blk, wt)
                else:
                    self._gemm(blk, wt, out=dfeats, addend=dfeats)
        return [g[id(q)] for q in self.params()], dfeats


class _HeadsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heads, seed, train, feats, *params):
        sa_feats, logits, saved = heads.forward(feats, seed, train)
        ctx.heads, ctx.saved = heads, saved
        ctx.need_dfeats = feats.requires_grad
        ctx.need_proj = any(q.requires_grad for q in heads.proj_params())
        ctx.mark_non_differentiable(sa_feats)  # the memory bank takes it detached (mlc_train.py:268-271)
        return sa_feats, logits

    @staticmethod
    def backward(ctx, _dsa, dlogits):
        with ops.stream_scope():
            grads, dfeats = ctx.heads.backward(ctx.saved, dlogits, ctx.need_dfeats, ctx.need_proj)
        ctx.saved = None
        return (None, None, None, dfeats) + tuple(grads)


def heads_forward(model, feats, seed=None):
    """(sa_feats [S, B, D], [logits_i [B, n_i]]) of `model` (projectors / mlc_sa / prototypes) on the HIP kernels, with
    autograd attached to the head parameters (and to `feats` when it requires grad)."""
    heads = model.__dict__.get("_sm3_mlc_heads")
    if heads is None:
        heads = MLCHeads(model)
        model.__dict__["_sm3_mlc_heads"] = heads
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))  # torch's CPU generator: reproducible under fix_random_seeds
    with ops.stream_scope():
        sa_feats, logits = _HeadsFn.apply(heads, seed, model.mlc_sa.training, feats.float(), *heads.params())
    return sa_feats, list(logits.split(heads.sizes, dim=1))


# ---- pseudo-labels: spherical k-means over the memory bank (mlc_train.py:116-189) -----------------------------------
@torch.no_grad()
def spherical_kmeans(embeddings, K, iters=10, generator=None, det=None):
    """embeddings [N, D] fp32 CUDA (one label's memory bank) -> (centroids [K, D], assignments [N] int64): random
    samples as the initial centroids, `iters` rounds of (assign by largest dot product; centroid = L2-normalised mean of
    its members), then the final assignment.  det (default: SM3_WGRAD_DET != 0): the cluster sums in a fixed order
    (sm3_mlc_kmeans_assign_det), so the centroids and assignments are a function of the bank and the generator."""
    if not embeddings.is_cuda or embeddings.dtype != torch.float32:
        raise ValueError("spherical_kmeans: fp32 CUDA embeddings")
    emb = embeddings.contiguous()
    N, D = emb.shape
    if N < K:
        raise ValueError("please reduce the number of centroids")  # mlc_train.py:148
    idx = torch.randperm(N, generator=generator)[:K].to(emb.device)
    cent = emb[idx].contiguous()
    assign = torch.empty(N, dtype=torch.int64, device=emb.device)
    sums = torch.empty(K, D, dtype=torch.float32, device=emb.device)
    counts = torch.empty(K, dtype=torch.int32, device=emb.device)
    lib = _lib.load()
    det = _det_default() if det is None else bool(det)
    slabs = torch.empty(_nslab(N) * K * D, dtype=torch.float32, device=emb.device) if det and _nslab(N) > 1 else None
    with ops.stream_scope():
        for _ in range(iters):
            sums.zero_()
            counts.zero_()
            if det:
                check(lib.sm3_mlc_kmeans_assign_det(_P(emb), _P(cent), _P(assign), _P(sums), _P(counts), _P(slabs), N, D, K, _st()),
                      "sm3_mlc_kmeans_assign_det")
            else:
                check(lib.sm3_mlc_kmeans_assign(_P(emb), _P(cent), _P(assign), _P(sums), _P(counts), N, D, K, _st()),
                      "sm3_mlc_kmeans_assign")
            check(lib.sm3_mlc_kmeans_update(_P(cent), _P(sums), _P(counts), K, D, _st()), "sm3_mlc_kmeans_update")
        check(lib.sm3_mlc_kmeans_assign(_P(emb), _P(cent), _P(assign), None, None, N, D, K, _st()), "sm3_mlc_kmeans_assign")
    return cent, assign


def pseudo_label_loss(logits, targets, temperature):
    """Fused form of the loop body mlc_train.py:252-261 (forward only, for monitoring): mean over heads of
    CrossEntropyLoss(pred / temperature, target).  logits: list of [B, n_i]; targets: [H, B] int64."""
    cat = torch.cat(logits, 1).contiguous().float()
    B, T = cat.shape
    H = len(logits)
    off = torch.tensor([0] + list(torch.tensor([l.shape[1] for l in logits]).cumsum(0)), dtype=torch.int32, device=cat.device)
    loss = torch.zeros(1, dtype=torch.float32, device=cat.device)
    dl = torch.empty_like(cat)
    with ops.stream_scope():
        check(_lib.load().sm3_mlc_ce(_P(cat), _P(targets.contiguous()), _P(off), H, B, T, float(temperature), _P(loss), _P(dl),
                                     _st()), "sm3_mlc_ce")
    return loss, dl
