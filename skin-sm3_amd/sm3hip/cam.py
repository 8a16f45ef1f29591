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
import torch

from . import ops
from .bridge import scratch_grads
from .explain import TARGETS, Subject  # noqa: F401  (TARGETS: part of this module's interface)

STAGES = ("layer1", "layer2", "layer3", "layer4")


def _stage_alpha(eng, ctx, dfeat, layer, hw, C):
    """alpha [T, N, C] of stage `layer` from dfeat [T, N, out_dim] fp32: one data-only backward per target, stopped at the
    stage output, whose gradient sm3_cam_alpha averages.  The BatchNorm parameter gradients that the data-gradient launches
    accumulate go to a scratch buffer (bridge.scratch_grads)."""
    T, N, _ = dfeat.shape
    alpha = torch.empty(T, N, C, dtype=torch.float32, device=dfeat.device)
    d = torch.empty(N, dfeat.shape[2], dtype=eng.tdt, device=dfeat.device)
    with scratch_grads(eng):
        for t in range(T):
            ops.cast_from_f32(eng.dtype, dfeat[t].contiguous(), d)
            g = eng.encoder_backward(ctx, d, last_view=True, params=False, stop_at=layer)
            ops.cam_alpha(eng.dtype, g, alpha[t], N, hw, C)
    return alpha


def grad_cam(model, derm, clinic, layer="layer4", target="pred"):
    """Grad-CAM maps of the 8 derm7pt labels for a batch of (dermoscopic, clinical) image pairs.

    model: an eval-mode Baseline or inference.py Model on the GPU; derm, clinic: [N, 3, H, W] float32 CUDA (normalised as
    the model expects); layer: the stage (layer1 .. layer4); target: "pred" (each label's argmax class), "cls" (the class
    AUC_AVG scores, sm3hip.metrics.CLS_WEIGHTS) or an int64 tensor [N, 8] of classes.
    Returns {"maps": [N, 8, 2, H, W] fp32 in [0, 1] (modality 0 derm, 1 clinic), "low_res": [N, 8, 2, h, w] fp32 (the ReLU'd
    maps at the stage's resolution, before upsampling and normalisation), "logits": 8 x [N, n_i] fp32, "target_class":
    [N, 8] int64, "layer": layer}."""
    sub = Subject(model, "grad_cam")
    if layer not in STAGES:
        raise ValueError(f"grad_cam: layer must be one of {', '.join(STAGES)}, got {layer!r}")
    engs = sub.check(derm, clinic, target).engs
    N, _, H, W = derm.shape
    with torch.no_grad(), ops.stream_scope():
        ctxs, outs, feats = [], [], []
        for eng, x in zip(engs, (derm, clinic)):
            keep = {"stage": layer}
            f, ctx = eng.encoder_only("main", x.contiguous(), False, layer != "layer4", keep=keep)
            ctxs.append(ctx), outs.append(keep["out"]), feats.append(f)
        logits, tc, dfeats = sub.head_grads(torch.cat(feats, dim=1), target)
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
        return {"maps": torch.stack(maps, dim=2), "low_res": torch.stack(low, dim=2), "logits": logits, "target_class": tc,
                "layer": layer}
