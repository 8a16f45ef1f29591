"""Grad-CAM (Selvaraju et al., ICCV 2017) class activation maps of the linear probe (src/models/baseline.py `Baseline`) and
of the SM3 multi-label model (inference.py `Model`) on the HIP engine: one map per derm7pt label and image modality, showing
which region of the dermoscopic and the clinical image drives that label's prediction.

For stage L (layer1 .. layer4) of one encoder, A [h, w, C] is the stage output (post-ReLU, the output of its last block) and
G = dy/dA the gradient of the target logit y with respect to it (not masked by A's own ReLU):

    alpha_c = mean_p G[p, c];  cam = ReLU(sum_c alpha_c A[:, :, c]);  maps = normalise(upsample(cam))

upsample: F.interpolate(mode="bilinear", align_corners=False) to the input's H x W; normalise: (cam - min) /
(1e-7 + max(cam - min)).  The pieces:

  * the heads give d y / d feats for each label's target logit.  Baseline: the classifier row (no launch).  inference.py
    Model: the eval-mode heads of sm3hip/mlc.py (exact f32, dropout off, BatchNorm1d on running statistics), forward once
    on the T = 8 target copies of the batch and backward once with a one-hot seed per copy;
  * layer4: G = dfeat / (h*w) at every position (the average pool's backward), so alpha = dfeat / (h*w) and no encoder
    backward runs;  layer1-3: one data-only encoder backward per target from the shared forward, stopped once the stage
    output's gradient is complete (engine.encoder_backward(stop_at=...)).  The T seeds are not batched into one backward:
    that would need the saved activations T times over (a T-fold forward) -- the backward kernels read them per row;
  * sm3_cam_alpha (the spatial mean, ascending positions) and sm3_cam_maps (channel sum, ReLU, upsample, normalisation),
    csrc/cam.hip.

Everything runs under torch.no_grad: parameters, .grad fields, BatchNorm buffers and the engines' flat gradient buffers are
left as they were (the BatchNorm parameter gradients a data-gradient launch produces go to a scratch buffer)."""
from itertools import accumulate

import torch

from . import ops
from .metrics import CLS_WEIGHTS, NUM_CLASSES

STAGES = ("layer1", "layer2", "layer3", "layer4")
TARGETS = ("pred", "cls")


def _parts(model, who="grad_cam"):
    """(kind, derm encoder, clinic encoder) of a Baseline ("baseline") or an inference.py Model ("mlc")."""
    if hasattr(model, "classifier") and hasattr(model, "derm_backbone"):
        return "baseline", model.derm_backbone, model.clinic_backbone
    if hasattr(model, "extractor") and hasattr(model, "prototypes") and hasattr(model, "mlc_sa"):
        return "mlc", model.extractor.derm_backbone, model.extractor.clinic_backbone
    raise TypeError(f"{who}: model must be a Baseline (src/models/baseline.py) or an inference.py Model")


def _check(model, derm, clinic, layer, target, who="grad_cam"):
    kind = _parts(model, who)[0]
    if layer not in STAGES:
        raise ValueError(f"{who}: layer must be one of {', '.join(STAGES)}, got {layer!r}")
    train = [n for n, m in model.named_modules() if m.training]
    if train:
        raise ValueError(f"{who}: the model must be in eval mode (model.eval()); in train mode: {train[0] or 'model'}")
    for name, x in (("derm", derm), ("clinic", clinic)):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"{who}: {name} must be a CUDA tensor (the SM3 HIP path has no CPU fallback)")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"{who}: {name} must be float32 [N, 3, H, W]")
    if derm.shape != clinic.shape:
        raise ValueError(f"{who}: derm and clinic must have the same shape")
    if any(not p.is_cuda for p in model.parameters()):
        raise ValueError(f"{who}: the model's parameters must be on the GPU")
    N = derm.shape[0]
    if isinstance(target, str):
        if target not in TARGETS:
            raise ValueError(f"{who}: target must be 'pred', 'cls' or a LongTensor [N, 8], got {target!r}")
    else:
        if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or tuple(target.shape) != (N, len(NUM_CLASSES)):
            raise ValueError(f"{who}: a target tensor must be int64 [N, 8]")
        t = target.cpu()
        for i, n in enumerate(NUM_CLASSES):
            if bool(((t[:, i] < 0) | (t[:, i] >= n)).any()):
                raise ValueError(f"{who}: target class out of range for label {i} ({n} classes)")
    return kind


def _mlc_heads(model):
    from .mlc import MLCHeads
    heads = model.__dict__.get("_sm3_mlc_heads")
    if heads is None:
        heads = MLCHeads(model)
        model.__dict__["_sm3_mlc_heads"] = heads
    return heads


def _target_class(logits, target, N, dev):
    if isinstance(target, torch.Tensor):
        return target.to(dev)
    if target == "pred":
        return torch.stack([o.argmax(dim=1) for o in logits], dim=1)
    return torch.tensor(CLS_WEIGHTS, dtype=torch.long, device=dev).expand(N, -1).contiguous()


def _head_grads(kind, model, feats, target):
    """(logits: 8 x [N, n_i] fp32, target_class [N, 8], dfeats [T, N, F] fp32 = d logit_t[target] / d feats)."""
    N, dev, T = feats.shape[0], feats.device, len(NUM_CLASSES)
    if kind == "baseline":
        logits = [clf(feats) for clf in model.classifier]  # stock PyTorch heads, as Baseline.forward runs them
        tc = _target_class(logits, target, N, dev)
        dfeats = torch.stack([clf.weight.index_select(0, tc[:, t]) for t, clf in enumerate(model.classifier)])
        return logits, tc, dfeats.float().contiguous()
    heads = _mlc_heads(model)
    # the T target copies of the batch through the eval-mode heads (rows are independent: per-sample attention, running
    # BatchNorm1d statistics), one backward with a one-hot seed at copy t's target logit
    _, out, sv = heads.forward(feats.repeat(T, 1).contiguous(), 0, train=False)
    logits = list(out[:N].split(heads.sizes, dim=1))
    tc = _target_class(logits, target, N, dev)
    off = torch.tensor([0] + list(accumulate(heads.sizes))[:-1], dtype=torch.long, device=dev)
    seed = torch.zeros(T, N, out.shape[1], dtype=torch.float32, device=dev)
    seed.scatter_(2, (tc.t() + off[:, None]).unsqueeze(2), 1.0)
    _, dfeats = heads.backward(sv, seed.view(T * N, -1), need_dfeats=True, need_proj=False)
    return logits, tc, dfeats.view(T, N, -1)


def _stage_alpha(eng, ctx, dfeat, layer, hw, C):
    """alpha [T, N, C] of stage `layer` from dfeat [T, N, out_dim] fp32: one data-only backward per target, stopped at the
    stage output, whose gradient sm3_cam_alpha averages.  The BatchNorm parameter gradients that the data-gradient launches
    accumulate go to a scratch buffer swapped in for the engine's flat gradient buffer."""
    T, N, _ = dfeat.shape
    alpha = torch.empty(T, N, C, dtype=torch.float32, device=dfeat.device)
    d = torch.empty(N, dfeat.shape[2], dtype=eng.tdt, device=dfeat.device)
    flat_g = eng.store.flat_g
    eng.store.flat_g = torch.zeros_like(flat_g)
    try:
        for t in range(T):
            ops.cast_from_f32(eng.dtype, dfeat[t].contiguous(), d)
            g = eng.encoder_backward(ctx, d, last_view=True, params=False, stop_at=layer)
            ops.cam_alpha(eng.dtype, g, alpha[t], N, hw, C)
    finally:
        eng.store.flat_g = flat_g
    return alpha


def grad_cam(model, derm, clinic, layer="layer4", target="pred"):
    """Grad-CAM maps of the 8 derm7pt labels for a batch of (dermoscopic, clinical) image pairs.

    model: an eval-mode Baseline or inference.py Model on the GPU; derm, clinic: [N, 3, H, W] float32 CUDA (normalised as
    the model expects); layer: the stage (layer1 .. layer4); target: "pred" (each label's argmax class), "cls" (the class
    AUC_AVG scores, sm3hip.metrics.CLS_WEIGHTS) or an int64 tensor [N, 8] of classes.
    Returns {"maps": [N, 8, 2, H, W] fp32 in [0, 1] (modality 0 derm, 1 clinic), "low_res": [N, 8, 2, h, w] fp32 (the ReLU'd
    maps at the stage's resolution, before upsampling and normalisation), "logits": 8 x [N, n_i] fp32, "target_class":
    [N, 8] int64, "layer": layer}."""
    kind = _check(model, derm, clinic, layer, target)
    from .bridge import encoder_engine_for
    _, enc_d, enc_c = _parts(model)
    N, _, H, W = derm.shape
    with torch.no_grad(), ops.stream_scope():
        engs, ctxs, outs, feats = [], [], [], []
        for enc, x in ((enc_d, derm), (enc_c, clinic)):
            eng = encoder_engine_for(enc)
            keep = {"stage": layer}
            f, ctx = eng.encoder_only("main", x.contiguous(), False, layer != "layer4", keep=keep)
            engs.append(eng), ctxs.append(ctx), outs.append(keep["out"]), feats.append(f)
        logits, tc, dfeats = _head_grads(kind, model, torch.cat(feats, dim=1), target)
        T = dfeats.shape[0]
        maps, low = [], []
        off = 0
        for eng, ctx, (A, h, w), f in zip(engs, ctxs, outs, feats):
            C, F_ = A.shape[1], f.shape[1]
            dfeat = dfeats[:, :, off:off + F_]
            off += F_
            if layer == "layer4":  # the average pool's backward: G = dfeat / (h*w) at every position
                alpha = (dfeat / float(h * w)).contiguous()
            else:
                alpha = _stage_alpha(eng, ctx, dfeat, layer, h * w, C)
            lo = torch.empty(N, T, h, w, dtype=torch.float32, device=derm.device)
            mp = torch.empty(N, T, H, W, dtype=torch.float32, device=derm.device)
            ops.cam_maps(eng.dtype, A, alpha, lo, mp, N, h, w, C)
            maps.append(mp), low.append(lo)
        return {"maps": torch.stack(maps, dim=2), "low_res": torch.stack(low, dim=2), "logits": [o.float() for o in logits],
                "target_class": tc, "layer": layer}
