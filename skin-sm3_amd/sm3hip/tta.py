"""Test-time augmentation of the predictions: the mean probability over the dihedral views (flips and quarter turns) of a case,
optionally of five crops each, for the linear probe (src/models/baseline.py `Baseline`) and the SM3 multi-label model
(inference.py `Model`) on the HIP engine -- and, from the same pass, how much a case's prediction moves across its views.

VIEWS.  View v = c * |G| + gi is element G[gi] of the group applied to crop c.
  * element g in 0 .. 7: bit 0 fx (columns reversed), bit 1 fy (rows reversed), bit 2 tr (transpose, applied first).  For a
    resampled, normalised image R [3, H, W]: out[ch][y][x] = R[ch][y'][x'], a = fy ? H - 1 - y : y, b = fx ? W - 1 - x : x,
    (y', x') = tr ? (b, a) : (a, b) -- R.transpose(-1, -2) if tr, then .flip(-2) if fy, then .flip(-1) if fx.
  * GROUPS: none [0], hflip [0, 1], flips [0, 1, 2, 3], d4 [0 .. 7].  A group with a transposing element needs H == W.
  * crops (image-store form only): 1 = the whole image (augment.whole_image_params); 5 = centre, top-left, top-right,
    bottom-left, bottom-right boxes of ch = max(1, round(s * h)) by cw = max(1, round(s * w)) of the image's own h x w, s =
    crop_scale in (0, 1]; the centre box at ((h - ch) // 2, (w - cw) // 2).
  * R of crop c is augment.apply_ragged with that box and nothing else (no flip, colour op, grayscale or blur): the existing
    resample and Normalize, once per crop.  Normalize is per pixel, so it commutes with the group bit for bit; the views are
    copies of the normalised R (sm3_tta_dihedral: every source tile read once, stored once per element).

REDUCTION (sm3_tta_reduce) of the views' logits [B, V, 24].  Per (case, view, label) in fp64: p = softmax of the label's logits
(z - max, exp, the sum in ascending class order, one division), q = rint(p * 2^32) as int64 -- the Q32 of calibration.py.  Over
the views: sum_q, min_q, max_q; agg_class = the lowest index of the maximum of sum_q among the label's classes; view_class = the
lowest index of the maximum of the view's logits (the project's argmax rule); disagree = the number of views with view_class !=
agg_class; preds = (float)log(max(sum_q, 1) / (V * 2^32)), whose softmax is the mean probability (the max keeps it finite where
every view underflows), so every report reads the predictions as it reads any other.  Everything that crosses views is an
integer sum, min, max or count: no order of the views changes a bit.

The encoders run in eval mode without saved records on chunks of cases x views; rows are independent there and in the heads, so
every chunk gives the same bits (the contract of rise.py / faith.py).  Everything runs under torch.no_grad."""
import torch

from . import ops
from .metrics import CLASSES_NAME, CLS_WEIGHTS, NUM_CLASSES

GROUPS = {"none": [0], "hflip": [0, 1], "flips": [0, 1, 2, 3], "d4": [0, 1, 2, 3, 4, 5, 6, 7]}
CROPS = (1, 5)
ONE = 1 << 32  # 1.0 in Q32
_KEYS = ("q", "sum_q", "min_q", "max_q", "view_class", "agg_class", "disagree")


def elements(group):
    """The elements of a named group, in view order."""
    if group not in GROUPS:
        raise ValueError(f"tta: group must be one of {', '.join(GROUPS)}, got {group!r}")
    return list(GROUPS[group])


def n_views(group, crops=1):
    if crops not in CROPS:
        raise ValueError(f"tta: crops must be 1 or 5, got {crops!r}")
    return crops * len(elements(group))


def _check_scale(crop_scale):
    if isinstance(crop_scale, bool) or not isinstance(crop_scale, (int, float)) or not 0 < crop_scale <= 1:
        raise ValueError(f"tta: crop_scale must be a number in (0, 1], got {crop_scale!r}")


def _check_square(group, H, W, who):
    if H != W and any(g & 4 for g in elements(group)):
        raise ValueError(f"{who}: group {group!r} transposes and needs a square image, got {H} x {W}")


def five_crop_boxes(hs, ws, crop_scale=0.8):
    """int32 [5, B, 4]: the (i, j, h, w) boxes centre, top-left, top-right, bottom-left, bottom-right of images hs[b] x ws[b]."""
    _check_scale(crop_scale)
    B = len(hs)
    box = torch.empty(5, B, 4, dtype=torch.int32)
    for b in range(B):
        h, w = int(hs[b]), int(ws[b])
        ch, cw = max(1, round(crop_scale * h)), max(1, round(crop_scale * w))
        for c, (i, j) in enumerate((((h - ch) // 2, (w - cw) // 2), (0, 0), (0, w - cw), (h - ch, 0), (h - ch, w - cw))):
            box[c, b] = torch.tensor([i, j, ch, cw])
    return box


def dihedral(x, group):
    """x [B, 3, H, W] fp32 on the GPU -> [B, G, 3, H, W]: the group's copies of every image, in the group's order."""
    els = elements(group)
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("tta.dihedral: x must be a float32 [B, 3, H, W] tensor")
    _check_square(group, x.shape[2], x.shape[3], "tta.dihedral")
    if not x.is_cuda:
        raise ValueError("tta.dihedral: x must be a CUDA tensor (the SM3 HIP path has no CPU fallback)")
    x = x.contiguous()
    out = torch.empty((x.shape[0], len(els)) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    ops.tta_dihedral(x, els, out)
    return out


def store_views(arena, offset, img_h, img_w, index, size, mean, std, group="d4", crops=1, crop_scale=0.8):
    """The views of the images index[b] of a packed uint8 arena (what augment.apply_ragged takes) at output size `size`
    -> [B, V, 3, H, W] fp32 normalised, V = crops * |group|: apply_ragged once per crop, then one dihedral."""
    from .augment import SimCLRAugment, whole_image_params
    V = n_views(group, crops)
    _check_scale(crop_scale)
    size = (size, size) if isinstance(size, int) else tuple(size)
    _check_square(group, size[0], size[1], "tta.store_views")
    index = torch.as_tensor(index, dtype=torch.int32).contiguous()
    B = index.numel()
    hs, ws = img_h[index.long()], img_w[index.long()]
    aug = SimCLRAugment(size, mean, std)
    params = whole_image_params(hs, ws)
    boxes = params.box[None] if crops == 1 else five_crop_boxes(hs, ws, crop_scale)
    R = torch.empty((B, crops, 3) + size, dtype=torch.float32, device=arena.device)
    for c in range(crops):
        params.box = boxes[c].contiguous()
        R[:, c] = aug.apply_ragged(arena, offset, img_h, img_w, index, params)
    return dihedral(R.view((B * crops, 3) + size), group).view((B, V, 3) + size)


def _as_columns(view_logits):
    """[B, V, 24] from 8 x [B, V, n_t] or from [B, V, 24] itself."""
    if isinstance(view_logits, torch.Tensor):
        z = view_logits
    else:
        parts = list(view_logits)
        if len(parts) != len(NUM_CLASSES) or any(not isinstance(p, torch.Tensor) or p.dim() != 3 or p.shape[2] != n or
                                                 p.shape[:2] != parts[0].shape[:2] for p, n in zip(parts, NUM_CLASSES)):
            raise ValueError("tta.reduce: 8 tensors [B, V, n_t] with n_t = 5, 3, 2, 3, 3, 3, 3, 2")
        z = torch.cat(parts, dim=2)
    if z.dim() != 3 or z.shape[2] != sum(NUM_CLASSES) or z.shape[0] < 1 or not 1 <= z.shape[1] <= ops.TTA_MAX_VIEWS:
        raise ValueError(f"tta.reduce: logits must be [B >= 1, 1 <= V <= {ops.TTA_MAX_VIEWS}, 24]")
    return z


def reduce(view_logits):
    """The reduction over the views (see the module text).  view_logits: 8 tensors [B, V, n_t], or [B, V, 24].
    -> {"preds": 8 x [B, n_t] fp32, "q" [B, V, 24], "sum_q", "min_q", "max_q" [B, 24] int64, "view_class" [B, V, 8],
    "agg_class", "disagree" [B, 8] int64}."""
    z = _as_columns(view_logits)
    if not bool(torch.isfinite(z).all()):
        raise ValueError("tta.reduce: the logits must be finite")
    if not z.is_cuda:
        raise ValueError("tta.reduce: the logits must be CUDA tensors (the SM3 HIP path has no CPU fallback)")
    z = z.float().contiguous()
    B, V, K = z.shape
    T, dev = len(NUM_CLASSES), z.device
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {"q": new((B, V, K), torch.int64), "sum_q": new((B, K), torch.int64), "min_q": new((B, K), torch.int64),
           "max_q": new((B, K), torch.int64), "view_class": new((B, V, T), torch.int32), "agg_class": new((B, T), torch.int32),
           "disagree": new((B, T), torch.int32)}
    preds = new((B, K), torch.float32)
    ops.tta_reduce(z, *(out[k] for k in _KEYS), preds)
    for k in ("view_class", "agg_class", "disagree"):
        out[k] = out[k].long()
    out["preds"] = list(preds.split(NUM_CLASSES, dim=1))
    return out


def _view_logits(sub, dviews, cviews, rows):
    """8 x [n, V, n_t] fp32: the logits of the paired views dviews, cviews [n, V, 3, H, W], `rows` view pairs per encoder forward."""
    n, V = dviews.shape[:2]
    d, c = dviews.reshape((n * V,) + tuple(dviews.shape[2:])), cviews.reshape((n * V,) + tuple(cviews.shape[2:]))
    parts = []
    for r0 in range(0, n * V, rows):
        feats = [eng.encoder_only("main", x[r0:r0 + rows].contiguous(), False, False)[0] for eng, x in zip(sub.engs, (d, c))]
        parts.append(sub.logits(torch.cat(feats, dim=1)))
    return [torch.cat([p[t] for p in parts]).view(n, V, -1) for t in range(len(NUM_CLASSES))]


def _forward_rows(chunk, V):
    """View pairs per encoder forward: chunk cases x V views, or what faith.MAX_FORWARD_IMAGES allows."""
    from .faith import MAX_FORWARD_IMAGES
    return (max(1, MAX_FORWARD_IMAGES // V) if chunk is None else chunk) * V


def predict(model, derm, clinic, group="d4", chunk=None):
    """The view-averaged predictions of image pairs derm, clinic: float32 [N, 3, H, W] on the GPU (crops = 1).  model: an
    eval-mode Baseline or inference.py Model (explain.Subject).  View v of derm is paired with view v of clinic.  chunk: cases
    per encoder forward (None: from faith.MAX_FORWARD_IMAGES); every chunk gives the same bits.
    -> reduce()'s dict plus "logits" (8 x [N, V, n_t], the views' own), "group", "views"."""
    from .explain import Subject
    who = "tta.predict"
    els = elements(group)
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"{who}: chunk must be None or a positive integer, got {chunk!r}")
    if isinstance(derm, torch.Tensor) and derm.dim() == 4:
        _check_square(group, derm.shape[2], derm.shape[3], who)
    sub = Subject(model, who).check(derm, clinic, "pred")
    N, V = derm.shape[0], len(els)
    cases = N if chunk is None else chunk
    with torch.no_grad(), ops.stream_scope():
        parts = []
        for n0 in range(0, N, cases):  # the views of at most `cases` cases at a time
            dv, cv = dihedral(derm[n0:n0 + cases], group), dihedral(clinic[n0:n0 + cases], group)
            parts.append(_view_logits(sub, dv, cv, _forward_rows(chunk, V)))
        logits = [torch.cat([p[t] for p in parts]) for t in range(len(NUM_CLASSES))]
        out = reduce(logits)
    out.update(logits=logits, group=group, views=V)
    return out


def predict_split(model, store, split, size, mean, std, group="d4", crops=1, crop_scale=0.8, batch_size=32):
    """predict over a split of an imagestore.ImageStore, in the split's own order, with crops: the views come from store_views.
    -> predict's dict plus "targets" [N, 8] int64, "crops", "crop_scale"."""
    from .explain import Subject
    from .faith import MAX_FORWARD_IMAGES
    who = "tta.predict_split"
    V = n_views(group, crops)
    _check_scale(crop_scale)
    size = (size, size) if isinstance(size, int) else tuple(size)
    _check_square(group, size[0], size[1], who)
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"{who}: batch_size must be a positive integer, got {batch_size!r}")
    cases = max(1, min(batch_size, MAX_FORWARD_IMAGES // V))
    sub, parts = Subject(model, who), []
    with torch.no_grad(), ops.stream_scope():
        for n0 in range(0, len(split), cases):
            dv, cv = (store_views(store.arena, store.offset, store.img_h, store.img_w, ids[n0:n0 + cases], size, mean, std, group,
                                  crops, crop_scale) for ids in (split.derm_ids, split.clinic_ids))
            if not parts:
                sub.check(dv[:, 0], cv[:, 0], "pred")
            parts.append(_view_logits(sub, dv, cv, cases * V))
        logits = [torch.cat([p[t] for p in parts]) for t in range(len(NUM_CLASSES))]
        out = reduce(logits)
    out.update(logits=logits, group=group, views=V, crops=crops, crop_scale=crop_scale, targets=split.labels)
    return out


def stability(record):
    """How much the prediction moves across the views, per label and "AVG" (ascending label order, one division by 8), from the
    record's integers with one IEEE division each: flip_rate = the share of cases with disagree > 0; mean_disagree =
    sum(disagree) / (N * V); mean_range = the mean of (max_q - min_q) / 2^32 at the column of CLS_WEIGHTS[t]."""
    dis, lo, hi = (record[k].cpu() for k in ("disagree", "min_q", "max_q"))
    N, V = dis.shape[0], int(record["views"])
    out = {"flip_rate": {}, "mean_disagree": {}, "mean_range": {}}
    col = 0
    for t, name in enumerate(CLASSES_NAME):
        k = col + CLS_WEIGHTS[t]
        out["flip_rate"][name] = int((dis[:, t] > 0).sum()) / N
        out["mean_disagree"][name] = int(dis[:, t].sum()) / (N * V)
        out["mean_range"][name] = int((hi[:, k] - lo[:, k]).sum()) / (N * ONE)
        col += NUM_CLASSES[t]
    for stat in out.values():
        total = 0.0
        for name in CLASSES_NAME:
            total = total + stat[name]
        stat["AVG"] = total / len(CLASSES_NAME)
    return out


def add_flags(parser):
    parser.add_argument("--tta", choices=list(GROUPS), default="none",
                        help="average the last validation pass's predictions over this group's views of every case")
    parser.add_argument("--tta-crops", type=int, choices=list(CROPS), default=1,
                        help="5: centre and corner crops as well (real data only)")
    parser.add_argument("--tta-crop-scale", type=float, default=0.8, help="side of a crop as a share of the image's, in (0, 1]")
    return parser


def check_flags(args, real, size=None):
    """The refusals of the three flags; host only.  size: the validation size (--img-sz by default)."""
    H, W = tuple(size or args.img_sz)
    try:
        _check_square(args.tta, H, W, "--tta")
        _check_scale(args.tta_crop_scale)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.tta_crops != 1 and not real:
        raise SystemExit("--tta-crops 5 crops the images of a real data set; synthetic batches have none")


def tool_record(record, crop_scale=None):
    """What a tool saves under "tta" next to the predictions: the settings, the view statistics and the stability values."""
    out = {"group": record["group"], "crops": record.get("crops", 1), "crop_scale": record.get("crop_scale", crop_scale),
           "views": record["views"], "stability": stability(record)}
    out.update({k: record[k].cpu() for k in ("sum_q", "min_q", "max_q", "disagree")})
    return out


def stats_line(record):
    """The one printed line: the three stability averages."""
    s = stability(record)
    return (f"tta {record['group']} x {record.get('crops', 1)} crops = {record['views']} views: flip_rate {s['flip_rate']['AVG']:.4f} "
            f"mean_disagree {s['mean_disagree']['AVG']:.4f} mean_range {s['mean_range']['AVG']:.4f}")
