"""A robustness report under image corruptions made on the GPU: what happens to the predictions of the linear probe
(src/models/baseline.py `Baseline`) and the SM3 multi-label model (inference.py `Model`) when the photograph gets worse -- noise,
blur, pixelation, hard JPEG compression, exposure, contrast, saturation and white balance, at five severities, in both images of a
case or in one of them (csrc/corrupt.hip).  This text is the specification of the corruptions.

A corruption acts on R [B, 3, H, W] fp32 in [0, 1], the resampled image BEFORE Normalize (augment.resample_ragged), and gives an
image in [0, 1] again; Normalize follows as everywhere else.  The result is a function of (image, name, severity, seed, case id,
modality) alone: not of the batch, the chunk or the position in a launch.  Severities run from 1 to 5.  The constants are in
pixels, factors or JPEG quality and do not scale with the image size; they are this project's tables, following ImageNet-C
(Hendrycks & Dietterich, ICLR 2019) where the operation is the same -- no parity with that code is claimed.

  code name            operation                                                          severity 1 .. 5
  0    gaussian_noise  clamp01(fadd(x, fmul(sigma, z)))                                   sigma 0.08, 0.12, 0.18, 0.26, 0.38
  1    impulse_noise   element -> 0 if its word w < T; -> 1 if w >= 2^32 - T; T = int(p * 2**31)   p 0.03, 0.06, 0.09, 0.17, 0.27
  2    defocus_blur    mean over the disk dy^2 + dx^2 <= r^2                              r 3, 4, 6, 8, 10
  3    motion_blur     mean over a line of L taps in one of 8 directions                  L 5, 9, 13, 17, 21
  4    pixelate        every pixel -> the mean of its f x f block, blocks anchored at (0, 0)       f 2, 3, 4, 6, 8
  5    jpeg            4:4:4 baseline JPEG round trip in integers                         quality 25, 18, 15, 10, 7
  6    darken          augment's brightness op (sm3_aug_color_op 1)                       factor 0.8, 0.65, 0.5, 0.35, 0.2
  7    brighten        the same                                                           factor 1.2, 1.4, 1.6, 1.8, 2.0
  8    contrast        augment's contrast op (2)                                          factor 0.75, 0.6, 0.45, 0.3, 0.15
  9    desaturate      augment's saturation op (3)                                        factor 0.8, 0.6, 0.4, 0.2, 0.0
  10   colour_cast     clamp01(fmul(x, g[ch])), g = (1 + c, 1, 1 - c) (warm) or reversed (cool)    c 0.05, 0.1, 0.15, 0.2, 0.3

fadd / fmul / fsub: one f32 operation each, rounded on its own, never fused (csrc/exact_f32.h).  sigma, c and 1 + c, 1 - c are f32.

RANDOMNESS.  Philox4x32-10 as in csrc/exact_f32.h, key = the 64-bit seed, low word first; the last counter word is 7 (the streams
are listed in resample.philox_words).
  * case word (motion direction, cast sign): counter (0xFFFFFFFF, case, code << 8 | severity, 7), word 0.  Direction k = w & 7,
    theta = k * pi / 8; the cast is warm where w & 1 == 0, cool where it is 1.  Both modalities of a case share it.
  * element words (the two noises): counter (e / 4, case, modality << 16 | code << 8 | severity, 7), word e % 4; e is the element's
    index in its [3, H, W] image, modality 0 for derm and 1 for clinic.  The normal is sm3_attr_noise's rule: float64 Box-Muller
    on the word pairs (w0, w1) and (w2, w3) -- u = (w + 0.5) * 2^-32, r = sqrt(-2 log u_a), z = r cos(2 pi u_b), r sin(2 pi u_b)
    -- rounded to f32 once.
  * case is the case's position in its split, low 32 bits, given explicitly (`ids`), never taken from the batch position.

SUMS.  The blurs and pixelate add f32 values one at a time, starting from 0, in a stated order -- the tap order of the table, or
row-major within a block -- every add rounded on its own, then one IEEE division by the tap or pixel count.  Borders replicate
the edge pixel (clamped coordinates), so any image size is defined, one smaller than the kernel included.  A pixelate block cut by
the image edge averages its in-image pixels.

TAP TABLES are integer (dy, dx) lists made on the host, once (TAP_TABLES).  The disk lists its offsets row-major (dy ascending,
then dx).  The line is t = -(L - 1) / 2 .. (L - 1) / 2 -> (round(t sin theta), round(t cos theta)) with Python's round, duplicates
kept; the device never evaluates a sine.  The largest offset is 10 in both blurs.

JPEG, all integers, per 8 x 8 block of the image edge-replicated up to multiples of 8:
  1. q8 = clamp(rint(fmul(x, 255)), 0, 255).
  2. Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;
     Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16  (JFIF's matrix in 16-bit fixed point).
  3. F = C13 . (X - 128) . C13^T in int64, C13[k][n] = rint(2^13 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = sqrt(2/8).
  4. The luminance and chrominance tables of ITU T.81 Annex K, scaled as libjpeg does: s = 5000 // q if q < 50 else 200 - 2 q,
     t = clamp((base * s + 50) // 100, 1, 255)  (quant_tables).
  5. d = t << 26, qv = sign(F) . ((2 |F| + d) // (2 d)).
  6. y = (C13^T . (qv . t) . C13 + 2^25) >> 26 (arithmetic shift), + 128, clamped to 0 .. 255.
  7. With Cb' = Cb - 128, Cr' = Cr - 128: R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16),
     B = Y + ((116130 Cb' + 32768) >> 16), clamped to 0 .. 255; out = (float)q / 255 (one IEEE f32 division).
Against Pillow's own round trip (quality q, subsampling 0) the numpy restatement of this (tests/corrupt_inputs.py) differs by a
few percent of Pillow's own distortion: one quantisation rounding flip moves a coefficient by a whole step.

THE REPORT (robustness_report) is report.evaluation_report of the clean predictions and of every (name, severity),
report.compare(corrupted, clean) for the paired difference of every metric -- with a bootstrap, on the replicates every report
draws -- and two label-free stability values from tta.reduce on the two "views" [clean, corrupted] of every case: the flip rate
per label (view_class[:, 0] != view_class[:, 1]) and the mean |delta p| at the column of CLS_WEIGHTS[t], (max_q - min_q) summed
in integers and divided once by N * 2^32.  auc_drop[name] is the mean over its severities (ascending, one division) of the
difference of the AUC "8 avg"; mean_drop the mean of those over the corruptions, in the table's order.

The encoders run in eval mode under torch.no_grad on chunks of cases; rows are independent there and in the heads, so every batch
size gives the same bits (the contract of tta.py)."""
import csv
import json
import math
import os

import numpy as np
import torch

from . import ops, report, resample, tta
from .metrics import CLASSES_NAME, CLS_WEIGHTS, NUM_CLASSES

CORRUPTIONS = {"gaussian_noise": 0, "impulse_noise": 1, "defocus_blur": 2, "motion_blur": 3, "pixelate": 4, "jpeg": 5, "darken": 6,
               "brighten": 7, "contrast": 8, "desaturate": 9, "colour_cast": 10}
SEVERITIES = (1, 2, 3, 4, 5)
MODALITIES = ("both", "derm", "clinic")
STREAM = 7  # the last counter word (resample.philox_words lists the streams)
_TABLE = {"gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38), "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),
          "defocus_blur": (3, 4, 6, 8, 10), "motion_blur": (5, 9, 13, 17, 21), "pixelate": (2, 3, 4, 6, 8),
          "jpeg": (25, 18, 15, 10, 7), "darken": (0.8, 0.65, 0.5, 0.35, 0.2), "brighten": (1.2, 1.4, 1.6, 1.8, 2.0),
          "contrast": (0.75, 0.6, 0.45, 0.3, 0.15), "desaturate": (0.8, 0.6, 0.4, 0.2, 0.0),
          "colour_cast": (0.05, 0.1, 0.15, 0.2, 0.3)}
_COLOUR_OP = {"darken": 1, "brighten": 1, "contrast": 2, "desaturate": 3}  # augment.OPS
DIRECTIONS = 8

# ITU T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), [vertical][horizontal] frequency
_K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
       100, 103, 99)
_K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + \
    (99,) * 32


def _check(name, severity, who="corrupt"):
    if name not in CORRUPTIONS:
        raise ValueError(f"{who}: the corruption must be one of {', '.join(CORRUPTIONS)}, got {name!r}")
    if isinstance(severity, bool) or not isinstance(severity, int) or severity not in SEVERITIES:
        raise ValueError(f"{who}: the severity must be an integer in 1 .. 5, got {severity!r}")


def parameters(name, severity):
    """The table's constant of (name, severity): sigma, p, r, L, f, quality, factor or c."""
    _check(name, severity, "corrupt.parameters")
    return _TABLE[name][severity - 1]


def _disk(r):
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r]


def _line(L, k):
    theta, h = k * math.pi / DIRECTIONS, (L - 1) // 2
    return [(round(t * math.sin(theta)), round(t * math.cos(theta))) for t in range(-h, h + 1)]


def _pack(lists):
    counts = np.array([len(l) for l in lists], dtype=np.int32)
    tables = np.zeros((len(lists), int(counts.max()), 2), dtype=np.int16)
    for i, l in enumerate(lists):
        tables[i, :len(l)] = np.array(l, dtype=np.int16)
    return tables, counts


# (name, severity) -> (tables int16 [n_tables, max_taps, 2] of (dy, dx), counts int32 [n_tables]): one disk, or the 8 lines
TAP_TABLES = {("defocus_blur", s): _pack([_disk(_TABLE["defocus_blur"][s - 1])]) for s in SEVERITIES}
TAP_TABLES.update({("motion_blur", s): _pack([_line(_TABLE["motion_blur"][s - 1], k) for k in range(DIRECTIONS)]) for s in SEVERITIES})


def tap_tables(name, severity):
    """(tables, counts) of a blur: see TAP_TABLES.  The arrays are the module's own: do not write to them."""
    _check(name, severity, "corrupt.tap_tables")
    if (name, severity) not in TAP_TABLES:
        raise ValueError(f"corrupt.tap_tables: {name} is not a blur")
    return TAP_TABLES[(name, severity)]


def quant_tables(quality):
    """(luminance, chrominance) int32 [64] at a JPEG quality in 1 .. 100: Annex K scaled as libjpeg's jpeg_set_quality does."""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"corrupt.quant_tables: quality must be an integer in 1 .. 100, got {quality!r}")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.array([min(max((b * s + 50) // 100, 1), 255) for b in base], dtype=np.int32) for base in (_K1, _K2))


def _ids(ids, B, who):
    """The cases' positions as uint32 numpy [B] (low 32 bits); None: 0 .. B - 1."""
    if ids is None:
        return np.arange(B, dtype=np.uint32)
    a = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64).reshape(-1)
    if a.shape != (B,):
        raise ValueError(f"{who}: ids must hold one position per case ({B}), got {a.shape[0]}")
    return (a & 0xFFFFFFFF).astype(np.uint32)


def case_words(ids, name, severity, seed=0):
    """The case word of every case (uint32 numpy): word 0 of Philox4x32-10 at counter (0xFFFFFFFF, case, code << 8 | severity, 7)."""
    _check(name, severity, "corrupt.case_words")
    ids = np.asarray(ids, dtype=np.uint64)
    w = resample.philox4x32_10(np.uint64(0xFFFFFFFF), ids, np.uint64(CORRUPTIONS[name] << 8 | severity), np.uint64(STREAM),
                               seed & 0xFFFFFFFF, seed >> 32)[0]
    return w.astype(np.uint32)


def apply(x01, name, severity, ids=None, seed=0, modality=0):
    """The corruption (name, severity) of x01 [B, 3, H, W] fp32 on the GPU in [0, 1] -> a new [B, 3, H, W] in [0, 1].  ids: the
    cases' positions in their split (default 0 .. B - 1); modality 0 derm, 1 clinic."""
    who = "corrupt.apply"
    _check(name, severity, who)
    if not isinstance(x01, torch.Tensor) or x01.dim() != 4 or x01.shape[1] != 3 or min(x01.shape) < 1 or x01.dtype != torch.float32:
        raise ValueError(f"{who}: x01 must be a float32 [B >= 1, 3, H >= 1, W >= 1] tensor")
    if not x01.is_cuda:
        raise ValueError(f"{who}: x01 must be a CUDA tensor (the SM3 HIP path has no CPU fallback)")
    if modality not in (0, 1):
        raise ValueError(f"{who}: modality must be 0 (derm) or 1 (clinic), got {modality!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in 0 .. 2^64 - 1, got {seed!r}")
    x = x01.contiguous()
    B = x.shape[0]
    ids = _ids(ids, B, who)
    p = parameters(name, severity)
    if name in _COLOUR_OP:  # the existing arithmetic, in place on a copy
        from .augment import colour_ops
        out = x.clone()
        host = torch.zeros(4, B, dtype=torch.int32)
        host[0] = _COLOUR_OP[name]
        opsd, facd = host.to(x.device), torch.full((4, B), float(p), dtype=torch.float32, device=x.device)
        colour_ops(out, host, opsd, facd)
        return out
    out = torch.empty_like(x)
    if name in ("gaussian_noise", "impulse_noise", "colour_cast"):
        dev_ids = torch.from_numpy(ids.view(np.int32)).to(x.device)
        ops.corrupt_pointwise(x, dev_ids, CORRUPTIONS[name], severity, int(p * 2 ** 31) if name == "impulse_noise" else p, seed,
                              modality, out)
    elif name == "defocus_blur":
        ops.corrupt_taps(x, *TAP_TABLES[(name, severity)], np.zeros(B, dtype=np.int32), out)
    elif name == "motion_blur":
        ops.corrupt_taps(x, *TAP_TABLES[(name, severity)], (case_words(ids, name, severity, seed) & 7).astype(np.int32), out)
    elif name == "pixelate":
        ops.corrupt_pixelate(x, p, out)
    else:
        ops.corrupt_jpeg(x, p, *quant_tables(p), out)
    return out


def _size(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def store_corrupted(arena, offset, img_h, img_w, index, size, mean, std, name, severity, ids, seed=0, modality=0):
    """The images index[b] of a packed uint8 arena (what augment.apply_ragged takes) at output size `size`, corrupted before
    Normalize -> [B, 3, H, W] fp32 normalised, what the model reads.  name=None: the clean image, apply_ragged with
    whole_image_params bit for bit."""
    from .augment import SimCLRAugment, whole_image_params
    if name is not None:
        _check(name, severity, "corrupt.store_corrupted")
    index = torch.as_tensor(index, dtype=torch.int32).contiguous()
    aug = SimCLRAugment(_size(size), mean, std)
    params = whole_image_params(img_h[index.long()], img_w[index.long()])
    img, on_device = aug.resample_ragged(arena, offset, img_h, img_w, index, params)
    if name is not None:
        img = apply(img, name, severity, ids, seed, modality)
    return aug._colour_finish(img, params, *on_device)


def _names(corruptions, who):
    names = list(CORRUPTIONS) if corruptions in ("all", ["all"], ("all",)) else \
        ([corruptions] if isinstance(corruptions, str) else list(corruptions))
    for n in names:
        if n not in CORRUPTIONS:
            raise ValueError(f"{who}: the corruption must be one of {', '.join(CORRUPTIONS)}, got {n!r}")
    if not names or len(set(names)) != len(names):
        raise ValueError(f"{who}: at least one corruption, none twice")
    return sorted(names, key=lambda n: CORRUPTIONS[n])  # the table's order


def _severities(severities, who):
    sev = [severities] if isinstance(severities, int) and not isinstance(severities, bool) else list(severities)
    if not sev or len(set(sev)) != len(sev) or any(isinstance(s, bool) or not isinstance(s, int) or s not in SEVERITIES for s in sev):
        raise ValueError(f"{who}: severities must be distinct integers in 1 .. 5, got {severities!r}")
    return sorted(sev)


def predict_split(model, store, split, size, mean, std, corruptions="all", severities=SEVERITIES, modality="both", seed=0,
                  batch_size=32):
    """The predictions of an eval-mode Baseline or inference.py Model (explain.Subject) over a split of an imagestore.ImageStore, in
    the split's own order: clean, and under every (name, severity).  modality "derm" / "clinic" corrupts that image only; the
    other is the clean one.  The case id of a case is its position in the split.
    -> {"clean": 8 x [N, n_t], "preds": {(name, s): 8 x [N, n_t]}, "targets" [N, 8], "modality", "seed"}."""
    from .augment import SimCLRAugment, whole_image_params
    from .explain import Subject
    from .faith import MAX_FORWARD_IMAGES
    who = "corrupt.predict_split"
    names, sev = _names(corruptions, who), _severities(severities, who)
    if modality not in MODALITIES:
        raise ValueError(f"{who}: modality must be one of {', '.join(MODALITIES)}, got {modality!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in 0 .. 2^64 - 1, got {seed!r}")
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"{who}: batch_size must be a positive integer, got {batch_size!r}")
    cases = max(1, min(batch_size, MAX_FORWARD_IMAGES))
    aug = SimCLRAugment(_size(size), mean, std)
    sub = Subject(model, who)
    keys = [None] + [(n, s) for n in names for s in sev]
    parts = {k: [] for k in keys}
    hit = {"both": (0, 1), "derm": (0,), "clinic": (1,)}[modality]
    with torch.no_grad(), ops.stream_scope():
        for n0 in range(0, len(split), cases):
            pos = np.arange(n0, min(n0 + cases, len(split)))
            res = []  # per modality: the resampled image in [0, 1], its parameters, and the clean normalised image
            for ids in (split.derm_ids, split.clinic_ids):
                index = torch.as_tensor(ids[n0:n0 + cases], dtype=torch.int32).contiguous()
                params = whole_image_params(store.img_h[index.long()], store.img_w[index.long()])
                img, on_device = aug.resample_ragged(store.arena, store.offset, store.img_h, store.img_w, index, params)
                res.append((img, params, on_device, aug._colour_finish(img, params, *on_device)))
            if n0 == 0:
                sub.check(res[0][3], res[1][3], "pred")
            for k in keys:
                pair = [r[3] if k is None or m not in hit else
                        aug._colour_finish(apply(r[0], k[0], k[1], pos, seed, m), r[1], *r[2]) for m, r in enumerate(res)]
                lg = tta._view_logits(sub, pair[0][:, None], pair[1][:, None], len(pos))
                parts[k].append([l[:, 0] for l in lg])
    cat = lambda k: [torch.cat([p[t] for p in parts[k]]) for t in range(len(NUM_CLASSES))]
    return {"clean": cat(None), "preds": {k: cat(k) for k in keys[1:]}, "targets": split.labels, "modality": modality, "seed": seed}


def _two_views(clean, corrupted):
    return tta.reduce([torch.stack([a.float(), b.float()], dim=1) for a, b in zip(clean, corrupted)])


def stability(clean, corrupted):
    """The label-free stability of one (name, severity) from tta.reduce on the views [clean, corrupted]: per label and "AVG"
    (ascending label order, one division by 8) flip_rate and mean_abs_dp, with the integers they are made of (flips, abs_dp_sum)."""
    red = _two_views([p.cuda() for p in clean], [p.cuda() for p in corrupted])
    vc, lo, hi = red["view_class"].cpu(), red["min_q"].cpu(), red["max_q"].cpu()
    N = vc.shape[0]
    out = {"flips": {}, "abs_dp_sum": {}, "flip_rate": {}, "mean_abs_dp": {}}
    col = 0
    for t, name in enumerate(CLASSES_NAME):
        k = col + CLS_WEIGHTS[t]
        out["flips"][name] = int((vc[:, 0, t] != vc[:, 1, t]).sum())
        out["abs_dp_sum"][name] = int((hi[:, k] - lo[:, k]).sum())
        out["flip_rate"][name] = out["flips"][name] / N
        out["mean_abs_dp"][name] = out["abs_dp_sum"][name] / (N * tta.ONE)
        col += NUM_CLASSES[t]
    for stat in (out["flip_rate"], out["mean_abs_dp"]):
        total = 0.0
        for name in CLASSES_NAME:
            total = total + stat[name]
        stat["AVG"] = total / len(CLASSES_NAME)
    return out


def _auc_avg(values):
    return float(values[report.METRICS.index("AUC"), report.COLUMNS.index("8 avg")])


def robustness_report(record, bootstrap=0, confidence=0.95, seed=0):
    """The report of predict_split's record (see the module text).
    -> {"clean": evaluation_report, "corrupted": {(name, s): evaluation_report}, "compare": {(name, s): report.compare(corrupted,
    clean)}, "stability": {(name, s): stability()}, "auc_drop": {name: float}, "mean_drop": float, "names", "severities",
    "modality", "corrupt_seed", "n"}."""
    targets = record["targets"].long()
    keys = list(record["preds"])
    names = sorted({k[0] for k in keys}, key=lambda n: CORRUPTIONS[n])
    if not keys:
        raise ValueError("corrupt.robustness_report: the record holds no corrupted predictions")
    rep = lambda preds: report.evaluation_report([p.float() for p in preds], targets, bootstrap, confidence, seed)
    out = {"clean": rep(record["clean"]), "corrupted": {}, "compare": {}, "stability": {}, "auc_drop": {}}
    for k in keys:
        out["corrupted"][k] = rep(record["preds"][k])
        out["compare"][k] = report.compare(out["corrupted"][k], out["clean"])
        out["stability"][k] = stability(record["clean"], record["preds"][k])
    total = 0.0
    for n in names:
        sev, s = sorted(k[1] for k in keys if k[0] == n), 0.0
        for v in sev:
            s = s + _auc_avg(out["compare"][(n, v)]["delta"])
        out["auc_drop"][n] = s / len(sev)
        total = total + out["auc_drop"][n]
    out["mean_drop"] = total / len(names)
    out.update(names=names, severities=sorted({k[1] for k in keys}), modality=record.get("modality", "both"),
               corrupt_seed=record.get("seed", 0), n=int(targets.shape[0]))
    return out


def csv_rows(rep):
    """One row per (name, severity): the AUC "8 avg", its difference to the clean one (with the interval when the report has a
    bootstrap), the two stability averages."""
    rows = []
    i, k8 = report.METRICS.index("AUC"), report.COLUMNS.index("8 avg")
    for key, cmp in rep["compare"].items():
        row = {"name": key[0], "severity": key[1], "AUC_AVG": _auc_avg(rep["corrupted"][key]["values"]),
               "delta_AUC_AVG": _auc_avg(cmp["delta"])}
        if "lo" in cmp:
            row.update(delta_lo=float(cmp["lo"][i, k8]), delta_hi=float(cmp["hi"][i, k8]))
        row.update(flip_rate=rep["stability"][key]["flip_rate"]["AVG"], mean_abs_dp=rep["stability"][key]["mean_abs_dp"]["AVG"])
        rows.append(row)
    return rows


def to_csv(rep, path):
    rows = csv_rows(rep)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        for row in rows:
            w.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in row.items()})


def to_json(rep, path):
    """The settings, the clean AUC, the rows of the CSV, every metric's paired difference, the stability values and the drops."""
    lists = lambda d: {k: v.tolist() for k, v in d.items() if k in ("delta", "lo", "hi", "frac_le_zero")}
    out = {"n": rep["n"], "modality": rep["modality"], "corrupt_seed": rep["corrupt_seed"], "names": rep["names"],
           "severities": rep["severities"], "metrics": list(report.METRICS), "columns": list(report.COLUMNS),
           "clean_AUC_AVG": _auc_avg(rep["clean"]["values"]), "rows": csv_rows(rep), "auc_drop": rep["auc_drop"],
           "mean_drop": rep["mean_drop"],
           "compare": {f"{n}_{s}": lists(c) for (n, s), c in rep["compare"].items()},
           "stability": {f"{n}_{s}": v for (n, s), v in rep["stability"].items()}}
    if "bootstrap" in rep["clean"]:
        out.update(bootstrap=rep["clean"]["bootstrap"], bootstrap_seed=rep["clean"]["seed"], confidence=rep["clean"]["confidence"])
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def save(rep, log_path, stem="val_robustness"):
    to_json(rep, os.path.join(log_path, stem + ".json"))
    to_csv(rep, os.path.join(log_path, stem + ".csv"))


def add_flags(parser):
    parser.add_argument("--corrupt", nargs="+", default=None, metavar="NAME",
                        help="after the last validation pass, predict again under these image corruptions (real data only): 'all' "
                             "or any of " + ", ".join(CORRUPTIONS))
    parser.add_argument("--corrupt-severity", nargs="+", type=int, default=list(SEVERITIES), help="severities, 1 .. 5 (default: all)")
    parser.add_argument("--corrupt-modality", choices=list(MODALITIES), default="both", help="which image of a case is corrupted")
    parser.add_argument("--corrupt-seed", type=int, default=0, help="seed of the noises, the motion direction and the cast sign")
    return parser


def check_flags(args, real):
    """The refusals of the four flags; host only."""
    if args.corrupt is None:
        return
    try:
        _names(args.corrupt, "--corrupt")
        _severities(args.corrupt_severity, "--corrupt-severity")
    except ValueError as e:
        raise SystemExit(str(e))
    if not 0 <= args.corrupt_seed < 2 ** 64:
        raise SystemExit(f"--corrupt-seed must be in 0 .. 2^64 - 1, got {args.corrupt_seed}")
    if not real:
        raise SystemExit("--corrupt degrades the images of a real data set; synthetic batches are not images in [0, 1]")


def stats_lines(rep):
    """One line per corruption: the mean AUC difference and, per severity, the difference and the flip rate."""
    lines = []
    for n in rep["names"]:
        per = " ".join(f"s{s} {_auc_avg(rep['compare'][(n, s)]['delta']):+.4f}/{rep['stability'][(n, s)]['flip_rate']['AVG']:.3f}"
                       for (m, s) in rep["compare"] if m == n)
        lines.append(f"corrupt {n} ({rep['modality']}): AUC_AVG drop {rep['auc_drop'][n]:+.4f} | dAUC/flip_rate {per}")
    return lines


def stats_line(rep):
    """The summary line: the clean AUC and the mean drop over the corruptions."""
    return f"corrupt {len(rep['names'])} corruptions: clean AUC_AVG {_auc_avg(rep['clean']['values']):.4f} mean_drop {rep['mean_drop']:+.4f}"
