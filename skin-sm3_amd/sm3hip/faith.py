"""Deletion / insertion faithfulness curves (Petsiuk, Das, Saenko: RISE, BMVC 2018) of attribution maps of the linear probe
(src/models/baseline.py `Baseline`) and of the SM3 multi-label model (inference.py `Model`) on the HIP engine: does a label's
prediction fall when the pixels its map calls important are taken away, and rise when only they are shown?

For images derm, clinic [N, 3, H, W], maps [N, 8, 2, H, W] (the "maps" of sm3hip.cam.grad_cam, sm3hip.attr.integrated_gradients
or smooth_grad, or anything else of that shape; modality 0 derm, 1 clinic), baseline images b and S curve steps:

  * rank, per (n, label t, modality m), over the HW pixels of maps[n, t, m], with IEEE comparisons (so -0 == +0):
        rank[p] = #{q : map[q] > map[p]} + #{q < p : map[q] == map[p]}
    -- descending by value, ties by ascending flat index; a permutation of 0 .. HW - 1.  Non-finite maps are refused.
  * counts c_k = (k * HW) // S in integers, k = 0 .. S (c_0 = 0, c_S = HW); 1 <= S <= HW.
  * deletion input at step k: pixel p (all 3 channels) is b where rank[p] < c_k, else x.  insertion: x where rank[p] < c_k,
    else b.
  * modality "joint": both images of the pair are perturbed at step k, each by its own map; "derm" / "clinic": only that image,
    the other stays x.
  * curve value: softmax(logits_t.double())[target_class[n, t]] of the model at the perturbed pair, the target classes chosen
    once, at x.
  * AUC = (p_0 / 2 + p_1 + ... + p_{S-1} + p_S / 2) / S in float64, the terms added in ascending k.

Low deletion AUC and high insertion AUC = a faithful map.  The pieces: sm3_faith_rank (a stable segmented radix sort) ranks the
16 N maps once; per chunk of c curve steps and perturbed modality sm3_faith_compose writes the [c * 8 * N, 3, H, W] masked
inputs (each label has its own masks, so the labels do not share a forward) and ONE eval-mode encoder forward without saved
records gives their features; an unperturbed modality's feature rows are repeated, not recomputed.  For label t's rows only label
t's logits are taken: Baseline applies classifier[t] to those rows; the inference.py Model goes through the eval-mode heads of
sm3hip/mlc.py once per chunk.  Steps 0 and S are the unperturbed pair and the fully perturbed pair, shared by all labels and by
both curves: they are computed once ("logits", "baseline_logits") and the curves' end points are taken from them.

Everything runs under torch.no_grad: parameters, .grad fields, BatchNorm buffers and the engines' flat gradient buffers are left
as they were.  The curves do not depend on the chunk (eval-mode rows are independent of batch position and batch size)."""
import torch

from . import ops
from .attr import plan_chunk
from .explain import Subject, baseline_images, expand_baseline, forward_measured, target_class
from .metrics import NUM_CLASSES

MODES = ("both", "deletion", "insertion")
MODALITIES = ("joint", "derm", "clinic")
# Images per encoder forward when the chunk is planned: a choice, the order of the largest batches the engine is otherwise run at
# (an explicit chunk is not capped).  Measured at 8 pairs, 224^2, bf16: 1 984 images per forward are 2.5 % faster.
MAX_FORWARD_IMAGES = 1024


def counts(HW, steps):
    """c_k = (k * HW) // steps, k = 0 .. steps: how many of the top-ranked pixels are perturbed at step k."""
    return [(k * HW) // steps for k in range(steps + 1)]


def _step_bytes(saved_bytes, E, T, perturbed):
    """Device bytes per curve step of one image pair: T masked fp32 inputs per perturbed modality and, as an upper bound of what
    one image's eval forward holds at once, the size of the records a forward would save for it (explain.forward_measured)."""
    return T * perturbed * (4 * E + saved_bytes)


def _saved_bytes(eng, x):
    """What one image's saved records hold: one forward of x that keeps them, dropped at once.  Only when the chunk is planned,
    and once per engine, arithmetic mode and image size (the figure is kept on the engine)."""
    known = eng._faith_saved_bytes
    key = (eng.dtype, tuple(x.shape[1:]))
    if key not in known:
        known[key] = forward_measured(eng, x)[1]
    return known[key]


def _check_maps(maps, derm, steps, who):
    if not isinstance(maps, torch.Tensor) or maps.dtype != torch.float32 or maps.dim() != 5:
        raise ValueError(f"{who}: maps must be a float32 tensor [N, 8, 2, H, W]")
    if isinstance(derm, torch.Tensor) and derm.dim() == 4 and tuple(maps.shape) != (
            derm.shape[0], len(NUM_CLASSES), 2, derm.shape[2], derm.shape[3]):
        raise ValueError(f"{who}: maps must be [N, 8, 2, H, W] = {(derm.shape[0], len(NUM_CLASSES), 2) + tuple(derm.shape[2:])}, "
                         f"got {tuple(maps.shape)}")
    if not bool(torch.isfinite(maps).all()):
        raise ValueError(f"{who}: maps must be finite (a NaN or an infinity has no rank)")
    HW = maps.shape[3] * maps.shape[4]
    if HW % 4:
        raise ValueError(f"{who}: H * W must be a multiple of 4")
    if steps > HW:
        raise ValueError(f"{who}: steps must be at most H * W = {HW}")


def _target_probs(sub, feats, tc):
    """p [c, T, N] fp64 = softmax(logits_t.double())[tc[n, t]] at feats [c, T, N, F]: label t's logits of label t's rows only."""
    c, T, N, _ = feats.shape
    p = torch.empty(c, T, N, dtype=torch.float64, device=feats.device)
    for t, lg in enumerate(sub.label_logits(feats)):
        p[:, t] = torch.softmax(lg.double(), dim=1).gather(1, tc[:, t].repeat(c)[:, None]).view(c, N)
    return p


def _picked_probs(logits, tc):
    """[N, T] fp64: softmax(logits_t.double()) at the target classes."""
    return torch.stack([torch.softmax(o.double(), dim=1).gather(1, tc[:, t:t + 1])[:, 0] for t, o in enumerate(logits)], dim=1)


def auc(curve):
    """Trapezoid area [..] fp64 under curve [.., S + 1] fp64 over [0, 1]: (p_0 / 2 + p_1 + ... + p_{S-1} + p_S / 2) / S, the
    terms added one by one in ascending k (on the host: a few thousand numbers)."""
    c = curve.detach().cpu().double().numpy()
    S = c.shape[-1] - 1
    if S < 1:
        raise ValueError("auc: a curve needs at least two points")
    acc = c[..., 0] / 2
    for k in range(1, S):
        acc = acc + c[..., k]
    acc = (acc + c[..., S] / 2) / S
    return torch.from_numpy(acc).to(curve.device)


def deletion_insertion(model, derm, clinic, maps, target="pred", steps=32, baseline="zero", modality="joint", mode="both",
                       chunk=None):
    """Deletion and insertion curves of the 8 derm7pt labels for a batch of (dermoscopic, clinical) image pairs and their maps.

    model, derm, clinic, target: as sm3hip.cam.grad_cam takes them.  maps: [N, 8, 2, H, W] fp32, finite.  steps: S, 1 <= S <=
    H * W (a multiple of 4).  baseline: "zero" (zero in normalised space: the dataset-mean image) or a pair (derm, clinic) of
    tensors broadcastable to the images.  modality: "joint", "derm" or "clinic".  mode: "both", "deletion" or "insertion".
    chunk: curve steps per encoder forward (None: from the free device memory); every 1 <= chunk <= steps gives the same bits.
    Returns {"deletion", "insertion": [N, 8, S + 1] fp64, "deletion_auc", "insertion_auc": [N, 8] fp64 (the keys of the curve
    not asked for are absent), "ranks": [N, 8, 2, H, W] int32, "logits": 8 x [N, n_i] fp32 at the images, "baseline_logits":
    8 x [N, n_i] fp32 at the fully perturbed pair (the baselines; with modality "derm" / "clinic" the other image stays),
    "target_class": [N, 8] int64, "steps", "chunk", "modality"}."""
    who = "deletion_insertion"
    if not isinstance(steps, int) or isinstance(steps, bool) or steps < 1:
        raise ValueError(f"{who}: steps must be a positive integer")
    if mode not in MODES:
        raise ValueError(f"{who}: mode must be one of {', '.join(MODES)}, got {mode!r}")
    if modality not in MODALITIES:
        raise ValueError(f"{who}: modality must be one of {', '.join(MODALITIES)}, got {modality!r}")
    if chunk is not None and (not isinstance(chunk, int) or isinstance(chunk, bool) or not 1 <= chunk <= steps):
        raise ValueError(f"{who}: chunk must be None or an integer in [1, {steps}], got {chunk!r}")
    pair = baseline_images(baseline, who)
    _check_maps(maps, derm, steps, who)
    sub = Subject(model, who).check(derm, clinic, target)
    if not maps.is_cuda:
        raise ValueError(f"{who}: maps must be a CUDA tensor (the SM3 HIP path has no CPU fallback)")
    N, _, H, W = derm.shape
    HW, T = H * W, len(NUM_CLASSES)
    engs, dev = sub.engs, derm.device
    perturbed = [m for m, name in enumerate(MODALITIES[1:]) if modality in ("joint", name)]
    with torch.no_grad(), ops.stream_scope():
        x = [derm.contiguous(), clinic.contiguous()]
        bases = [expand_baseline(None if pair is None else pair[m], x[m]) for m in range(2)]
        # steps 0 and S: the pair itself and the fully perturbed pair
        feats_x = [eng.encoder_only("main", xm, False, False)[0] for eng, xm in zip(engs, x)]
        logits = sub.logits(torch.cat(feats_x, dim=1))
        tc = target_class(logits, target, N, dev)
        feats_b = [engs[m].encoder_only("main", bases[m].expand_as(x[m]).contiguous(), False, False)[0] if m in perturbed
                   else feats_x[m] for m in range(2)]
        base_logits = sub.logits(torch.cat(feats_b, dim=1))
        ends = (_picked_probs(logits, tc), _picked_probs(base_logits, tc))  # [N, T] at k = 0 and k = S of the deletion curve

        ranks = torch.empty((N, T, 2, H, W), dtype=torch.int32, device=dev)
        ops.faith_rank(maps.contiguous().view(N, T, 2, HW), ranks.view(N, T, 2, HW))

        if chunk is None:
            free, _ = torch.cuda.mem_get_info(dev)
            saved = max(_saved_bytes(engs[m], x[m]) for m in perturbed)
            c = plan_chunk(steps, N, _step_bytes(saved, 3 * HW, T, len(perturbed)), free)
            c = max(1, min(c, MAX_FORWARD_IMAGES // (T * N)))
        else:
            c = chunk
        out = {}
        for name, invert in (("deletion", False), ("insertion", True)):
            if mode not in ("both", name):
                continue
            curve = torch.empty(N, T, steps + 1, dtype=torch.float64, device=dev)
            curve[:, :, 0], curve[:, :, steps] = ends[int(invert)], ends[1 - int(invert)]
            for k0 in range(1, steps, c):
                n = min(c, steps - k0)
                feats = []
                for m in range(2):
                    if m in perturbed:
                        xin = torch.empty((n, T, N, 3, H, W), dtype=torch.float32, device=dev)
                        ops.faith_compose(x[m], bases[m], ranks[:, :, m], xin, k0, steps, invert)
                        feats.append(engs[m].encoder_only("main", xin.view(n * T * N, 3, H, W), False, False)[0])
                        del xin
                    else:
                        feats.append(feats_x[m].repeat(n * T, 1))
                p = _target_probs(sub, torch.cat(feats, dim=1).view(n, T, N, -1), tc)
                curve[:, :, k0:k0 + n] = p.permute(2, 1, 0)
            out[name], out[name + "_auc"] = curve, auc(curve)
        out.update(ranks=ranks, logits=logits, baseline_logits=base_logits, target_class=tc, steps=steps, chunk=c,
                   modality=modality)
        return out
