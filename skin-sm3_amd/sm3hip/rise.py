"""RISE saliency maps (Petsiuk, Das, Saenko: Randomized Input Sampling for Explanation of Black-box Models, BMVC 2018) of the
linear probe (src/models/baseline.py `Baseline`) and of the SM3 multi-label model (inference.py `Model`) on the HIP engine: the
black-box, forward-only map maker beside the gradient methods of cam.py and attr.py.  Mask the input with M random smooth masks,
ask the model for the target class's probability under each, and average the masks weighted by those probabilities.

For images derm, clinic [N, 3, H, W] (H * W a multiple of 4), M masks, a grid of s x s cells, keep probability p, a 64-bit seed
and baseline images b:

  * cells ch = ceil(H / s), cw = ceil(W / s); corner grid G = s + 2.
  * random words: Philox4x32-10 as sm3_attr_noise has it, key = seed (low word first), counter (q, i, m, 1): i the mask, m the
    modality (0 derm, 1 clinic); the last word keeps the stream apart from SmoothGrad's (e / 4, n, sample, 0).
  * grid bit g[gy][gx] (j = gy * G + gx) = word j % 4 of call j // 4 < thr, thr = floor(p * 2^32) in float64 (refused if 0).
  * shift, from call ceil(G * G / 4): oy = (w0 * ch) >> 32, ox = (w1 * cw) >> 32 in 64-bit integers.
  * mask value at (y, x): Y = y + oy, gy = Y // ch, ry = Y % ch, likewise X, gx, rx; the integer
        A = (ch - ry) (cw - rx) g[gy][gx] + (ch - ry) rx g[gy][gx + 1] + ry (cw - rx) g[gy + 1][gx] + ry rx g[gy + 1][gx + 1]
    and mask = (float)A / (float)(ch * cw), one correctly rounded f32 division: the paper's "upsample an s x s binary grid
    bilinearly to (s + 1) cells and crop at a random shift", in integers.
  * masks are a function of (seed, m, i, H, W, s, p) alone -- the paper's fixed mask set: the same for every image of a batch
    and every batch of a run, so a case's map does not depend on what else is in its batch.
  * masked input: b + mask * (x - b) as three separately rounded f32 operations, all three channels of a pixel with the pixel's
    mask value.  modality "joint": both images masked, derm by stream m = 0, clinic by m = 1; "derm" / "clinic": only that
    image, the other stays x.
  * score P[n, t, i] = softmax(logits_t.double())[target_class[n, t]] in float64 at masked pair i, the target classes chosen
    once, at x.  Weight w = (float)P.
  * map: acc = 0; for i = 0 .. M - 1: acc = acc + w[n, t, i] * mask_i^m[y, x], every product and sum rounded on its own, in
    ascending i; maps[n, t, m] = acc / (float)(M * p).  The map of an unperturbed modality is zeros.

The pieces: sm3_rise_table writes one 144-byte row per mask and modality (the grid bits and the shift), from which the two
other kernels regenerate mask values instead of storing them; per chunk of c masks and perturbed modality sm3_rise_compose
writes the [c * N, 3, H, W] masked inputs and ONE eval-mode encoder forward without saved records gives their features (the masks
do not depend on the label, so the 8 labels share every forward); an unperturbed modality's feature rows are repeated, not
recomputed; the weights of a chunk go to their slice of [M, N * 8], and after the last chunk ONE sm3_rise_accumulate launch per
modality sums over all M masks in registers -- so the bits do not depend on the chunk.

Everything runs under torch.no_grad: parameters, .grad fields, BatchNorm buffers and the engines' flat gradient buffers are left
as they were."""
import torch

from . import ops
from .attr import plan_chunk
from .explain import Subject, baseline_images, expand_baseline, target_class
from .faith import MAX_FORWARD_IMAGES, MODALITIES, _saved_bytes, _step_bytes
from .metrics import NUM_CLASSES

MAX_MASKS = 2 ** 20
MAX_CELLS = 30  # (cells + 2)^2 grid bits fit the 1024 of a table row
MAX_CHUNK = 8 * 65535  # masks per sm3_rise_compose launch (groups of 8 masks on one grid axis)


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def threshold(p):
    """floor(p * 2^32) in float64: a grid bit is set when its random word is below it."""
    return int(float(p) * 4294967296.0)


def check_settings(masks, cells, p, seed, chunk, modality, who="rise"):
    """The refusals that need neither a tensor nor a device."""
    if not _is_int(masks) or not 1 <= masks <= MAX_MASKS:
        raise ValueError(f"{who}: masks must be an integer in [1, 2^20], got {masks!r}")
    if not _is_int(cells) or not 1 <= cells <= MAX_CELLS:
        raise ValueError(f"{who}: cells must be an integer in [1, {MAX_CELLS}], got {cells!r}")
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 < p < 1 or threshold(p) == 0:
        raise ValueError(f"{who}: p must be a number with 0 < p < 1 and floor(p * 2^32) > 0, got {p!r}")
    if not _is_int(seed) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64), got {seed!r}")
    if chunk is not None and (not _is_int(chunk) or not 1 <= chunk <= min(masks, MAX_CHUNK)):
        raise ValueError(f"{who}: chunk must be None or an integer in [1, {min(masks, MAX_CHUNK)}], got {chunk!r}")
    if modality not in MODALITIES:
        raise ValueError(f"{who}: modality must be one of {', '.join(MODALITIES)}, got {modality!r}")


def _check_size(derm, cells, who):
    """What the kernels ask of the image size (only when derm has one: Subject.check refuses the rest)."""
    if isinstance(derm, torch.Tensor) and derm.dim() == 4:
        H, W = derm.shape[2:]
        if (H * W) % 4:
            raise ValueError(f"{who}: H * W must be a multiple of 4")
        if H * W > 2 ** 24:
            raise ValueError(f"{who}: H * W must be at most 2^24")
        if cells > min(H, W):
            raise ValueError(f"{who}: cells must be at most min(H, W) = {min(H, W)}, got {cells}")


def rise(model, derm, clinic, target="pred", masks=4000, cells=7, p=0.5, seed=0, baseline="zero", modality="joint",
         chunk=None):
    """RISE maps of the 8 derm7pt labels for a batch of (dermoscopic, clinical) image pairs.

    model, derm, clinic, target: as sm3hip.cam.grad_cam takes them.  masks: M, 1 <= M <= 2^20.  cells: s, 1 <= s <= min(H, W,
    30).  p: the probability that a grid corner keeps the image, 0 < p < 1.  seed: the masks are a function of (seed, modality,
    mask index, H, W, cells, p) alone.  baseline: what a masked-out pixel shows: "zero" (zero in normalised space: the
    dataset-mean image) or a pair (derm, clinic) of tensors broadcastable to the images.  modality: "joint", "derm" or "clinic".
    chunk: masks per encoder forward (None: from the free device memory, at most MAX_FORWARD_IMAGES images per forward; an
    explicit chunk puts chunk * N images into one forward and is bounded only by masks and MAX_CHUNK); every such chunk gives the
    same bits.
    Returns {"maps": [N, 8, 2, H, W] fp32 (modality 0 derm, 1 clinic; zeros for an unperturbed modality), "scores": [N, 8, M]
    fp64 (the target class's probability under each mask), "logits": 8 x [N, n_i] fp32 at the images, "target_class": [N, 8]
    int64, "masks", "cells", "p", "seed", "chunk", "modality"}."""
    who = "rise"
    check_settings(masks, cells, p, seed, chunk, modality, who)
    pair = baseline_images(baseline, who)
    _check_size(derm, cells, who)
    sub = Subject(model, who).check(derm, clinic, target)
    N, _, H, W = derm.shape
    M, T = masks, len(NUM_CLASSES)
    engs, dev = sub.engs, derm.device
    perturbed = [m for m, name in enumerate(MODALITIES[1:]) if modality in ("joint", name)]
    with torch.no_grad(), ops.stream_scope():
        x = [derm.contiguous(), clinic.contiguous()]
        bases = [expand_baseline(None if pair is None else pair[m], x[m]) for m in range(2)]
        feats_x = [eng.encoder_only("main", xm, False, False)[0] for eng, xm in zip(engs, x)]
        logits = sub.logits(torch.cat(feats_x, dim=1))
        tc = target_class(logits, target, N, dev)

        if chunk is None:
            free, _ = torch.cuda.mem_get_info(dev)
            saved = max(_saved_bytes(engs[m], x[m]) for m in perturbed)
            c = plan_chunk(M, N, _step_bytes(saved, 3 * H * W, 1, len(perturbed)), free)
            c = max(1, min(c, MAX_FORWARD_IMAGES // N))
        else:
            c = chunk
        tables = {}
        for m in perturbed:
            tables[m] = torch.empty((M, ops.RISE_ROW_WORDS), dtype=torch.int32, device=dev)
            ops.rise_table(tables[m], 0, m, H, W, cells, p, seed)
        scores = torch.empty(N, T, M, dtype=torch.float64, device=dev)
        weights = torch.empty(M, N * T, dtype=torch.float32, device=dev)
        for i0 in range(0, M, c):
            n = min(c, M - i0)
            feats = []
            for m in range(2):
                if m in perturbed:
                    xin = torch.empty((n, N, 3, H, W), dtype=torch.float32, device=dev)
                    ops.rise_compose(x[m], bases[m], tables[m][i0:i0 + n], xin, cells)
                    feats.append(engs[m].encoder_only("main", xin.view(n * N, 3, H, W), False, False)[0])
                    del xin
                else:
                    feats.append(feats_x[m].repeat(n, 1))
            prob = torch.empty(n, N, T, dtype=torch.float64, device=dev)
            for t, lg in enumerate(sub.logits(torch.cat(feats, dim=1))):  # the labels share the rows
                prob[:, :, t] = torch.softmax(lg.double(), dim=1).gather(1, tc[:, t].repeat(n)[:, None]).view(n, N)
            scores[:, :, i0:i0 + n] = prob.permute(1, 2, 0)
            weights[i0:i0 + n] = prob.view(n, N * T).float()
        maps = torch.zeros((N, T, 2, H, W), dtype=torch.float32, device=dev)
        for m in perturbed:
            ops.rise_accumulate(tables[m], weights, maps[:, :, m], cells, p)
        return {"maps": maps, "scores": scores, "logits": logits, "target_class": tc, "masks": M, "cells": cells, "p": p,
                "seed": seed, "chunk": c, "modality": modality}
