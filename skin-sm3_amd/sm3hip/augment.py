"""GPU-side SimCLR augmentation of the SM3 pre-training input: the transform chain of
tools/backbone_train.py:448-466

    RandomResizedCrop(img_sz, scale=(0.5, 1.0)) -> RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], p=0.8)
    -> RandomGrayscale(p=0.2) -> RandomHorizontalFlip() -> RandomApply([GaussianBlur((3, 3), (0.1, 2.0))], p=0.5)
    -> ToTensor() -> Normalize(mean, std)                       wrapped in NViewsTransform(., 2) (functional.py:43-49)

on a batch of decoded RGB images already resident in HBM ([B, Hs, Ws, 3] uint8), through csrc/augment.hip.  This module
is the host half: it draws the random parameters with torchvision 0.13's rules (RandomResizedCrop.get_params: 10 tries
of area ~ U(scale) x aspect ~ logU(3/4, 4/3), central-crop fallback; ColorJitter.get_params: a random permutation of
the four ops, factors U(1-s, 1+s) / hue U(-h, h); GaussianBlur.get_params: sigma ~ U(0.1, 2.0)) and sequences the
kernels.  The flip is folded into the resample (it commutes with every later op: they are per-pixel, a global mean, or a
symmetric filter with reflect padding).  Arithmetic is float (torchvision's tensor code path); the reference's PIL path
rounds to uint8 after every op."""
import ctypes as C
import math

import torch

from . import _lib, ops

OPS = {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4}


class AugParams:
    """Per-sample random parameters of one view batch (host tensors)."""
    __slots__ = ("box", "flip", "ops", "factors", "gray", "sigma")


def resized_crop_params(B, Hs, Ws, scale, ratio, gen):
    """torchvision.transforms.RandomResizedCrop.get_params for every sample of the batch -> int32 [B, 4] (i, j, h, w)."""
    box = torch.empty(B, 4, dtype=torch.int32)
    area = Hs * Ws
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for b in range(B):
        done = False
        for _ in range(10):
            target = area * float(torch.empty(1).uniform_(scale[0], scale[1], generator=gen))
            ar = math.exp(float(torch.empty(1).uniform_(lo, hi, generator=gen)))
            w, h = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < w <= Ws and 0 < h <= Hs:
                i = int(torch.randint(0, Hs - h + 1, (1,), generator=gen))
                j = int(torch.randint(0, Ws - w + 1, (1,), generator=gen))
                box[b] = torch.tensor([i, j, h, w])
                done = True
                break
        if not done:  # central crop
            in_ratio = Ws / Hs
            if in_ratio < min(ratio):
                w, h = Ws, int(round(Ws / min(ratio)))
            elif in_ratio > max(ratio):
                h, w = Hs, int(round(Hs * max(ratio)))
            else:
                w, h = Ws, Hs
            box[b] = torch.tensor([(Hs - h) // 2, (Ws - w) // 2, h, w])
    return box


def colour_ops(img, ops_host, opsd, facd):
    """ColorJitter's positions that any sample uses (ops_host [4, B] on the host; opsd, facd: its and the factors' device copies),
    in place on img [B, 3, H, W] in [0, 1]: torchvision's brightness / contrast / saturation / hue arithmetic."""
    lib, st = _lib.load(), ops._stream()
    B, _, H, W = img.shape
    gm = torch.empty(B, dtype=torch.float32, device=img.device)
    for pos in range(4):
        if bool((ops_host[pos] != 0).any()):
            _lib.check(lib.sm3_aug_color_op(ops._ptr(img), B, H, W, ops._ptr(opsd[pos]), ops._ptr(facd[pos]), ops._ptr(gm), st),
                       "sm3_aug_color_op")


class SimCLRAugment:
    def __init__(self, size, mean, std, scale=(0.5, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), jitter=(0.8, 0.8, 0.8, 0.2),
                 p_jitter=0.8, p_gray=0.2, p_flip=0.5, p_blur=0.5, sigma=(0.1, 2.0)):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self.scale, self.ratio, self.jitter = scale, ratio, jitter
        self.p_jitter, self.p_gray, self.p_flip, self.p_blur, self.sigma = p_jitter, p_gray, p_flip, p_blur, sigma

    def sample(self, B, Hs, Ws, gen=None):
        """Draw one view's parameters (CPU generator: the reference samples on DataLoader workers)."""
        p = AugParams()
        p.box = resized_crop_params(B, Hs, Ws, self.scale, self.ratio, gen)
        return self._sample_rest(p, B, gen)

    def sample_ragged(self, hs, ws, gen=None):
        """sample() for a batch of images of different sizes: sample b's crop box is drawn from its own image, hs[b] x ws[b],
        with the same rules.  Ops whose probability is 0 draw nothing (the chains without jitter, grayscale or blur); with
        every probability positive the random stream is sample()'s, so an equal-sized batch gets sample()'s parameters."""
        B = len(hs)
        p = AugParams()
        p.box = torch.cat([resized_crop_params(1, int(hs[b]), int(ws[b]), self.scale, self.ratio, gen) for b in range(B)])
        return self._sample_rest(p, B, gen, skip_zero=True)

    def _sample_rest(self, p, B, gen, skip_zero=False):
        u = lambda n=B: torch.rand(n, generator=gen)
        p.ops = torch.zeros(4, B, dtype=torch.int32)      # [position][sample]
        p.factors = torch.ones(4, B, dtype=torch.float32)
        if not (skip_zero and self.p_jitter == 0):
            self._sample_jitter(p, B, gen, u() < self.p_jitter)
        p.gray = torch.zeros(B, dtype=torch.uint8) if skip_zero and self.p_gray == 0 else (u() < self.p_gray).to(torch.uint8)
        p.flip = (u() < self.p_flip).to(torch.uint8)
        if skip_zero and self.p_blur == 0:
            p.sigma = torch.zeros(B)
        else:
            blur = u() < self.p_blur
            sig = torch.empty(B).uniform_(self.sigma[0], self.sigma[1], generator=gen)
            p.sigma = torch.where(blur, sig, torch.zeros(B))    # 0 = no blur
        return p

    def _sample_jitter(self, p, B, gen, apply_j):
        bj, cj, sj, hj = self.jitter
        for b in range(B):
            order = torch.randperm(4, generator=gen)        # ColorJitter.get_params
            f = [float(torch.empty(1).uniform_(max(0.0, 1 - bj), 1 + bj, generator=gen)),
                 float(torch.empty(1).uniform_(max(0.0, 1 - cj), 1 + cj, generator=gen)),
                 float(torch.empty(1).uniform_(max(0.0, 1 - sj), 1 + sj, generator=gen)),
                 float(torch.empty(1).uniform_(-hj, hj, generator=gen))]
            if bool(apply_j[b]):
                for pos in range(4):
                    fn = int(order[pos])                    # 0 brightness, 1 contrast, 2 saturation, 3 hue
                    p.ops[pos, b] = fn + 1
                    p.factors[pos, b] = f[fn]

    def apply(self, src, params):
        """src: [B, Hs, Ws, 3] uint8 on the GPU -> [B, 3, H, W] fp32 normalised (what the encoder's stem reads)."""
        if not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or not src.is_contiguous():
            raise ValueError("augmentation input must be a contiguous [B, Hs, Ws, 3] uint8 CUDA tensor")
        B, Hs, Ws, _ = src.shape
        H, W = self.size
        dev = src.device
        box = params.box.to(dev)
        if params.box.shape != (B, 4) or bool((params.box[:, 2] <= 0).any()) or bool((params.box[:, 3] <= 0).any()) or \
                bool((params.box[:, 0] < 0).any()) or bool((params.box[:, 1] < 0).any()) or \
                bool((params.box[:, 0] + params.box[:, 2] > Hs).any()) or bool((params.box[:, 1] + params.box[:, 3] > Ws).any()):
            raise ValueError("crop box outside the source image")
        lib, st = _lib.load(), ops._stream()
        # device copies of the parameters stay referenced until every launch is enqueued (a temporary handed to ctypes
        # would be recycled by the caching allocator for the next temporary)
        flip, gray, sigma = params.flip.to(dev), params.gray.to(dev), params.sigma.to(dev)
        opsd, facd = params.ops.contiguous().to(dev), params.factors.contiguous().to(dev)
        img = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        _lib.check(lib.sm3_aug_resized_crop(ops._ptr(src), B, Hs, Ws, ops._ptr(box), ops._ptr(flip), ops._ptr(img), H, W, st),
                   "sm3_aug_resized_crop")
        return self._colour_finish(img, params, opsd, facd, gray, sigma)

    def _colour_finish(self, img, params, opsd, facd, gray, sigma):
        """ColorJitter's positions that any sample uses, then grayscale / blur / Normalize, on img [B, 3, H, W] in [0, 1]."""
        lib, st = _lib.load(), ops._stream()
        B, _, H, W = img.shape
        colour_ops(img, params.ops, opsd, facd)
        out = torch.empty_like(img)
        m3, s3 = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        _lib.check(lib.sm3_aug_finish(ops._ptr(img), B, H, W, ops._ptr(gray), ops._ptr(sigma), m3, s3, ops._ptr(out), st),
                   "sm3_aug_finish")
        return out

    def apply_ragged(self, arena, offset, img_h, img_w, index, params):
        """The chain over images of different sizes packed in one uint8 arena (sm3hip.imagestore.ImageStore): sample b
        reads image index[b] (host int32 [B]); offset / img_h / img_w: host int64 / int32 / int32 per image.  The crop
        boxes are checked against each sample's own image by the library before anything is launched.
        -> [B, 3, H, W] fp32 normalised."""
        img, on_device = self.resample_ragged(arena, offset, img_h, img_w, index, params)
        return self._colour_finish(img, params, *on_device)

    def resample_ragged(self, arena, offset, img_h, img_w, index, params):
        """The first half of apply_ragged: the resample alone.  -> (img [B, 3, H, W] fp32 in [0, 1], the device copies (ops,
        factors, gray, sigma) of the parameters that _colour_finish takes).  sm3hip.corrupt works on img between the two."""
        if not arena.is_cuda or arena.dtype != torch.uint8 or arena.dim() != 1:
            raise ValueError("the arena must be a 1-D uint8 CUDA tensor")
        index = torch.as_tensor(index, dtype=torch.int32).contiguous()
        B = index.numel()
        H, W = self.size
        dev = arena.device
        offset, img_h, img_w = (t.contiguous() for t in (offset, img_h, img_w))
        box, flip = params.box.to(torch.int32).contiguous(), params.flip.to(torch.uint8).contiguous()
        if box.shape != (B, 4) or flip.shape != (B,) or offset.dtype != torch.int64 or img_h.dtype != torch.int32 or \
                img_w.dtype != torch.int32 or offset.is_cuda or img_h.is_cuda or img_w.is_cuda:
            raise ValueError("apply_ragged: box [B, 4] int32, flip [B] uint8, offset int64 / img_h, img_w int32 on the host")
        lib, st = _lib.load(), ops._stream()
        # per-sample parameters of the colour / finish kernels: pinned, copied without a host synchronise (the caching host
        # allocator keeps a pinned buffer alive until its copy has run); referenced until every launch is enqueued
        up = lambda t: t.contiguous().pin_memory().to(dev, non_blocking=True)
        gray, sigma = up(params.gray), up(params.sigma)
        opsd, facd = up(params.ops), up(params.factors)
        img = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        _lib.check(lib.sm3_aug_resized_crop_ragged(ops._ptr(arena), arena.numel(), offset.data_ptr(), img_h.data_ptr(),
                                                   img_w.data_ptr(), offset.numel(), index.data_ptr(), box.data_ptr(),
                                                   flip.data_ptr(), B, ops._ptr(img), H, W, st),
                   "sm3_aug_resized_crop_ragged")
        return img, (opsd, facd, gray, sigma)

    def __call__(self, src, gen=None, n_views=2):
        """NViewsTransform(self, n_views): independent parameters per view (functional.py:43-49)."""
        B, Hs, Ws, _ = src.shape
        return [self.apply(src, self.sample(B, Hs, Ws, gen)) for _ in range(n_views)]


def whole_image_params(hs, ws):
    """Parameters of the validation chain Resize(size) -> ToTensor -> Normalize on images of sizes hs[b] x ws[b]: PIL's
    Resize of a whole image is the resample with the whole image as the box; no flip, colour op, grayscale or blur."""
    B = len(hs)
    p = AugParams()
    p.box = torch.zeros(B, 4, dtype=torch.int32)
    p.box[:, 2] = torch.as_tensor(hs, dtype=torch.int32)
    p.box[:, 3] = torch.as_tensor(ws, dtype=torch.int32)
    p.flip = torch.zeros(B, dtype=torch.uint8)
    p.ops = torch.zeros(4, B, dtype=torch.int32)
    p.factors = torch.ones(4, B, dtype=torch.float32)
    p.gray = torch.zeros(B, dtype=torch.uint8)
    p.sigma = torch.zeros(B)
    return p


# The per-tool training chains of the reference on a real dataset (all: RandomResizedCrop -> ... -> RandomHorizontalFlip(0.5)
# -> ToTensor -> Normalize, one view unless the tool asks for NViewsTransform):
#   backbone_train  tools/backbone_train.py:447-470  the SimCLR chain (SimCLRAugment's defaults), two views
#   backbone_eval   tools/backbone_eval.py:234-262   RandomResizedCrop(img_sz, scale=(0.5, 1)), flip
#   mlc_train       tools/mlc_train.py:309-330       RandomResizedCrop(img_sz, (0.5, 1)), RandomApply(ColorJitter(.8, .8, .8,
#                                                    .2), p=0.5), flip
#   mlc_eval        tools/mlc_eval.py:294-322        RandomResizedCrop(train_sz, scale=(0.3, 1)), flip
# Validation everywhere: Resize(size) -> Normalize (whole_image_params).
CHAINS = {
    "backbone_train": dict(),
    "backbone_eval": dict(scale=(0.5, 1.0), p_jitter=0.0, p_gray=0.0, p_blur=0.0),
    "mlc_train": dict(scale=(0.5, 1.0), p_jitter=0.5, p_gray=0.0, p_blur=0.0),
    "mlc_eval": dict(scale=(0.3, 1.0), p_jitter=0.0, p_gray=0.0, p_blur=0.0),
}


def chain(tool, size, mean, std):
    """The training chain of `tool` (CHAINS) at output size `size`."""
    return SimCLRAugment(size, mean, std, **CHAINS[tool])
