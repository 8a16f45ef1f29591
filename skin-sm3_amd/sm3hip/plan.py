"""What describes a network and holds nothing per step: the flat parameter store, the conv / BatchNorm units of an encoder
and of a projector, the form each encoder block takes (decided once per forward pass, read by the backward pass), and the
records a forward pass saves for its backward.  sm3hip/engine.py sequences the kernels over these."""
import math
from dataclasses import dataclass

import torch

from . import ops

RESNET50_LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))


# ------------------------------------------------------------------------------------------
# flat parameter / gradient storage
# ------------------------------------------------------------------------------------------
class ParamStore:
    """All parameters of a module in one flat fp32 buffer (64-byte aligned slots); parameters become
    views, conv weights with channels_last strides so their memory is [Cout][kh][kw][Cin]."""

    def __init__(self, module, device):
        self.module = module
        self.device = device
        self.names, self.offsets, self.shapes = [], {}, {}
        off = 0
        for name, p in module.named_parameters():
            self.names.append(name)
            self.offsets[name] = off
            self.shapes[name] = tuple(p.shape)
            off += (p.numel() + 15) // 16 * 16
        self.total = off
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=device)
        self._bind()

    def _view(self, flat, name):
        shape = self.shapes[name]
        n = math.prod(shape) if shape else 1
        v = flat[self.offsets[name]: self.offsets[name] + n]
        if len(shape) == 4:
            o, i, h, w = shape
            return v.view(o, h, w, i).permute(0, 3, 1, 2)  # OIHW shape, OHWI memory
        return v.view(shape)

    def _bind(self):
        params = dict(self.module.named_parameters())
        with torch.no_grad():
            for name in self.names:
                p = params[name]
                v = self._view(self.flat_p, name)
                v.copy_(p.data.to(device=self.device, dtype=torch.float32))
                p.data = v
                p.grad = None
        self._ptrs = {n: params[n].data_ptr() for n in self.names}

    def bound(self):
        params = dict(self.module.named_parameters())
        return all(params[n].data_ptr() == self._ptrs[n] and params[n].device == self.flat_p.device
                   for n in self.names)

    def rebind_if_needed(self):
        if not self.bound():
            self._bind()

    def flat2d(self, flat, name):
        """[Cout, taps*Cin] (conv / linear) or [C] view of a slot."""
        shape = self.shapes[name]
        n = math.prod(shape)
        v = flat[self.offsets[name]: self.offsets[name] + n]
        return v.view(shape[0], -1) if len(shape) >= 2 else v

    def grad_views(self, flat=None):
        flat = self.flat_g if flat is None else flat
        return [self._view(flat, n) for n in self.names]


# ------------------------------------------------------------------------------------------
# layer units
# ------------------------------------------------------------------------------------------
class ConvUnit:
    """groups > 1: a grouped 3x3 convolution (ResNeXt conv2, Ci == Co) on the kernels of csrc/gconv.hip, whose banks are
    [9][Co / groups][Co] in forward and in data-gradient order (sm3_gconv_weight_prep); none of the dense-kernel forms
    (halo-resident A image, nine-tap owner weight gradient, fused data-gradient epilogues) applies to it.
    The stem unit (stem=True) only holds the direct stem's filter bank (csrc/stem.hip); its kernels take no descriptor."""

    def __init__(self, name, Ci, Co, k, stride, pad, stem=False, groups=1):
        self.name, self.Ci, self.Co, self.k, self.stride, self.pad, self.stem = name, Ci, Co, k, stride, pad, stem
        self.groups = groups
        if groups > 1 and (k != 3 or pad != 1 or Ci != Co or stem):
            raise ValueError("grouped convolutions: 3x3, pad 1, Ci == Co only")
        self.taps = k * k
        self.w_fwd = self.w_dgrad = None
        self._fd, self._dd = {}, {}

    def alloc(self, dtype, device):
        tdt = ops.TORCH_DTYPE[dtype]
        if self.stem:
            self.w_fwd = torch.empty(self.Co, ops.STEM_KDIRECT, dtype=tdt, device=device)
        elif self.groups > 1:
            n = self.taps * self.Co * (self.Ci // self.groups)
            self.w_fwd = torch.empty(n, dtype=tdt, device=device)
            self.w_dgrad = torch.empty(n, dtype=tdt, device=device)
        else:
            self.w_fwd = torch.empty(self.Co, self.taps * self.Ci, dtype=tdt, device=device)
            self.w_dgrad = torch.empty(self.Ci, self.taps, self.Co, dtype=tdt, device=device)

    def fwd_desc(self, dtype, N, H, W):
        key = (dtype, N, H, W)
        if key not in self._fd:
            self._fd[key] = ops.fwd_desc(dtype, N, H, W, self.Ci, self.Co, self.k, self.stride, self.pad)
        return self._fd[key]

    def compact_dgrad_desc(self, dtype, N, Hs, Ws):
        """Data gradient of a 1x1 / stride-2 convolution at the pixels it touches only: a plain GEMM over the
        [N, Hs, Ws, Co] output gradient with the transposed filter bank."""
        key = ("cdg", dtype, N, Hs, Ws)
        if key not in self._dd:
            self._dd[key] = ops.fwd_desc(dtype, N, Hs, Ws, self.Co, self.Ci, 1, 1, 0)
        return self._dd[key]

    def dgrad_descs(self, dtype, N, H, W):
        key = (dtype, N, H, W)
        if key not in self._dd:
            self._dd[key] = ops.dgrad_descs(dtype, N, H, W, self.Ci, self.Co, self.k, self.stride, self.pad)
        return self._dd[key]

    def dgrad_fusable(self, dtype, N, H, W, V):
        """Whether this unit's data gradient over an [N, H, W] input with V views in the batch can run the BatchNorm-backward
        phase 1 of the unit before it in its epilogue (sm3_conv_dgrad_bnfuse): its launches cover every input pixel, and
        with two views each launch's rows split into whole 128-row tiles per view."""
        descs, full = self.dgrad_descs(dtype, N, H, W)
        return full and (V == 1 or all((dd.N * dd.Ho * dd.Wo) % 256 == 0 for dd in descs))


class BNUnit:
    def __init__(self, name, C, affine=True):
        self.name, self.C, self.affine = name, C, affine


class EncoderPlan:
    """Units of a torchvision ResNet encoder.  block="bottleneck": c1 (1x1) / b1, c2 (3x3, stride s) / b2, c3 (1x1, x4) /
    b3 per block; block="basic" (resnet18/34): c1 (3x3, stride s) / b1, c2 (3x3) / b2.  cd / bd (1x1 downsample, stride
    s) where the block changes the stride or the width (reference resnet.py:251-262) -- every stage entry of a Bottleneck
    network, layer2..4 of a BasicBlock one.  The last unit of a block is always its join (bn + identity + ReLU)."""

    def __init__(self, prefix, block_counts=(3, 4, 6, 3), block="bottleneck", groups=1, width_per_group=64):
        """groups / width_per_group (Bottleneck only): a ResNeXt -- c1 / c2 / c3 are inplanes -> width -> width -> 4 * planes,
        width = int(planes * width_per_group / 64) * groups, c2 grouped (reference resnet.py:142-148)."""
        if block not in ("bottleneck", "basic"):
            raise ValueError(block)
        if block == "basic" and (groups != 1 or width_per_group != 64):
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        self.prefix = prefix
        self.basic = block == "basic"
        self.stem = ConvUnit(prefix + "conv1", 3, 64, 7, 2, 3, stem=True)
        self.stem_bn = BNUnit(prefix + "bn1", 64)
        self.blocks = []
        exp = 1 if self.basic else 4
        inpl = 64
        for li, ((planes, _, stride), nblocks) in enumerate(zip(RESNET50_LAYERS, block_counts), start=1):
            for b in range(nblocks):
                p = f"{prefix}layer{li}.{b}."
                s = stride if b == 0 else 1
                if self.basic:
                    blk = {
                        "c1": ConvUnit(p + "conv1", inpl, planes, 3, s, 1), "b1": BNUnit(p + "bn1", planes),
                        "c2": ConvUnit(p + "conv2", planes, planes, 3, 1, 1), "b2": BNUnit(p + "bn2", planes),
                    }
                else:
                    wd = int(planes * (width_per_group / 64.0)) * groups
                    blk = {
                        "c1": ConvUnit(p + "conv1", inpl, wd, 1, 1, 0), "b1": BNUnit(p + "bn1", wd),
                        "c2": ConvUnit(p + "conv2", wd, wd, 3, s, 1, groups=groups), "b2": BNUnit(p + "bn2", wd),
                        "c3": ConvUnit(p + "conv3", wd, planes * 4, 1, 1, 0), "b3": BNUnit(p + "bn3", planes * 4),
                    }
                if s != 1 or inpl != planes * exp:
                    blk["cd"] = ConvUnit(p + "downsample.0", inpl, planes * exp, 1, s, 0)
                    blk["bd"] = BNUnit(p + "downsample.1", planes * exp)
                    inpl = planes * exp
                self.blocks.append(blk)
        self.out_dim = inpl

    def conv_units(self):
        yield self.stem
        for blk in self.blocks:
            for k in ("c1", "c2", "c3", "cd"):
                if k in blk:
                    yield blk[k]


class ProjectorPlan:
    def __init__(self, prefix, in_dim, proj_dim):
        self.prefix = prefix
        self.l0 = ConvUnit(prefix + "0", in_dim, in_dim, 1, 1, 0)
        self.b1 = BNUnit(prefix + "1", in_dim)
        self.l3 = ConvUnit(prefix + "3", in_dim, in_dim, 1, 1, 0)
        self.b4 = BNUnit(prefix + "4", in_dim)
        self.l6 = ConvUnit(prefix + "6", in_dim, proj_dim, 1, 1, 0)
        self.b7 = BNUnit(prefix + "7", proj_dim, affine=False)

    def conv_units(self):
        return (self.l0, self.l3, self.l6)


def enc_mod_out_dim(enc_mod):
    """Width of the pooled features of a src.models.resnet.ResNet: 512 (BasicBlock) or 2048 (Bottleneck)."""
    return 512 if enc_block(enc_mod) == "basic" else 512 * 4


def enc_block(enc_mod):
    return getattr(enc_mod, "block_type", "bottleneck")


def enc_plan(prefix, enc_mod):
    """The EncoderPlan of a src.models.resnet.ResNet: block type, block counts, groups and width per group from the module."""
    return EncoderPlan(prefix, enc_mod.block_counts, enc_block(enc_mod), getattr(enc_mod, "groups", 1),
                       getattr(enc_mod, "base_width", 64))


def stage_of(blk):
    """"layer1" ... "layer4": the stage a block of an EncoderPlan belongs to."""
    return blk["c1"].name.rsplit(".", 3)[-3]


# ------------------------------------------------------------------------------------------
# the form of a block: decided once, by the forward pass that saves records; the backward pass reads it
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True, slots=True)
class BlockForm:
    """All False: the two-pass form (every unit convolution, statistics, apply pass; two-pass BatchNorm backward)."""
    lin: bool = False           # conv3 -> bn3 backward by linearity (csrc/linbn.hip); the forward pass takes the moments of y2
    conv3_fused: bool = False   # ... and forward: conv3 -> bn3 -> + identity -> ReLU in one launch (conv3_bn3_fused)
    lin_d: bool = False         # the downsample conv -> BatchNorm backward by linearity too
    join_fused: bool = False    # ... and forward: the whole join as one two-segment GEMM (join_fused)
    sparse_join: bool = False   # stride-2 downsample: its data gradient, compact, can be conv1's data-gradient addend


TWO_PASS = BlockForm()


def block_form(blk, bi, sw, train, dtype, V, N, h, w):
    """The form block `bi` (blk, of an EncoderPlan) takes in a pass that saves records for a backward pass.
    sw: the switches .linbn / .linbn_fwd / .linbn_ds / .linbn_join (the engine); train: batch statistics; V: views in the
    batch of N images; h, w: the block's input map.
    By linearity (16-bit modes, train mode, Bottleneck): conv3 -> bn3 wherever the widths fit the kernels' tiles.  The
    downsample unit as well when its input width does and its data gradient can join conv1's: added in place at stride 1; at
    stride 2 as a compact addend, which needs the previous block's BatchNorm-backward phase 1 in conv1's data-gradient
    epilogue -- there is no previous block for block 0.  The forward halves need what their backward needs."""
    cd = blk.get("cd")
    sparse = cd is not None and cd.stride == 2 and bi > 0 and blk["c1"].dgrad_fusable(dtype, N, h, w, V)
    lin = bool(sw.linbn and train and "c3" in blk and blk["c3"].Co % 128 == 0 and blk["c3"].Ci % 64 == 0)
    lin_d = lin and cd is not None and sw.linbn_ds and cd.Ci % 64 == 0 and (cd.stride == 1 or sparse)
    return BlockForm(lin=lin, conv3_fused=lin and cd is None and sw.linbn_fwd, lin_d=lin_d,
                     join_fused=lin_d and sw.linbn_fwd and sw.linbn_join, sparse_join=sparse)


# ------------------------------------------------------------------------------------------
# what a forward pass saves for its backward
# ------------------------------------------------------------------------------------------
@dataclass(slots=True)
class Rec:
    """What one conv+BN(+act) application saves for backward."""
    cu: ConvUnit
    bu: BNUnit
    N: int
    H: int
    W: int
    Ho: int
    Wo: int
    x_in: object = None      # the unit's input (the stem: the images or their StemImage)
    xo: object = None        # pre-BatchNorm convolution output; None where the forward pass never stored it
    mean: object = None
    invstd: object = None
    y: object = None         # the unit's output; None when a consumer applies the BatchNorm (apply=False)
    relu: bool = False
    mask: object = None      # 1 bit per element of (y > 0)
    V: int = 1
    frozen_stats: bool = False  # eval-mode BatchNorm inside a graph: the statistics are constants
    scale: object = None     # the stem only: what its fused BN + ReLU + max-pool pass applied
    shift: object = None
    linbn: bool = False      # backward by linearity: no pass over xo
    colsum: object = None    # by linearity: moments of the unit's output (conv2) or of its strided input (downsample) ...
    gram: object = None
    Tm: object = None        # ... and W G of the unit, from sm3_linbn_fwd_stats
    in_s: object = None      # downsample unit of a fused join: the compact (strided) block input


@dataclass(slots=True)
class BlockRec:
    """The records of one encoder block: r1 / r2 / r3 of conv1 / conv2 / conv3 (r3 None: BasicBlock), rd of the downsample
    unit (None: identity), and the form the forward pass gave the block."""
    form: BlockForm
    r1: Rec
    r2: Rec
    r3: Rec = None
    rd: Rec = None

    @property
    def join(self):
        """The block's last unit: bn + identity + ReLU."""
        return self.r3 if self.r3 is not None else self.r2


@dataclass(slots=True)
class EncoderCtx:
    """One encoder pass, as encoder_backward needs it."""
    plan: EncoderPlan
    N: int
    img_hw: tuple
    stem: Rec
    stem_hw: tuple
    argmax: object       # the max-pool's argmax bytes
    blocks: list         # BlockRec per block
    last_hw: tuple
