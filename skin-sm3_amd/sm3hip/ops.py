"""Tensor-level wrappers over the C ABI (include/sm3_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every kernel is ours.  Each wrapper
checks on the host that shapes/dtypes/devices match what the kernel's grid assumes before launching.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, SM3_BF16, SM3_F16, SM3_F32, check

TORCH_DTYPE = {SM3_F32: torch.float32, SM3_BF16: torch.bfloat16, SM3_F16: torch.float16}
K_CHUNK = {SM3_F32: 32, SM3_BF16: 64, SM3_F16: 64}  # elements per 128-byte K chunk


_PROFILER = None


def set_profiler(p):
    """Install a sm3hip.profiler.Profiler (or None): wrappers then bracket their launches with HIP events."""
    global _PROFILER
    _PROFILER = p


class _prof:
    """with _prof(tag, flops, bytes): launch  -- no-op unless a profiler that wants `tag` is installed."""
    __slots__ = ("tag", "flops", "nbytes", "start")

    def __init__(self, tag, flops=0.0, nbytes=0.0):
        self.tag, self.flops, self.nbytes, self.start = tag, flops, nbytes, None

    def __enter__(self):
        p = _PROFILER
        if p is not None and p.wants(self.tag):
            self.start = p.begin()

    def __exit__(self, *exc):
        if self.start is not None:
            _PROFILER.end(self.tag, self.flops, self.nbytes, self.start)
        return False


def _sz(dtype):
    return 4 if dtype == SM3_F32 else 2


# torch.cuda.current_stream() costs ~8 us of host time and every wrapper needs the handle: 2 400 calls = 30 % of the
# host side of a step.  A caller that owns the stream context (the engine: one scope per lane entry / step) pins the
# raw handle with stream_scope(); outside such a scope the handle is looked up per launch as before.
_PINNED_STREAM = None


class stream_scope:
    """with ops.stream_scope(): every launch inside goes to torch's current stream AS OF ENTRY (raw handle cached).
    Nest a new scope whenever the current stream changes (torch.cuda.stream(...))."""

    def __enter__(self):
        global _PINNED_STREAM
        self.prev = _PINNED_STREAM
        _PINNED_STREAM = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0
        return self

    def __exit__(self, *exc):
        global _PINNED_STREAM
        _PINNED_STREAM = self.prev
        return False


def _stream_handle():
    if _PINNED_STREAM is not None:
        return _PINNED_STREAM
    return torch.cuda.current_stream().cuda_stream


def _stream():
    return C.c_void_p(_stream_handle())


def _ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _chk(t, dtype=None, name="tensor"):
    if t is None:
        return
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (the SM3 HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")


def dtype_code(torch_dtype):
    if torch_dtype == torch.float32:
        return SM3_F32
    if torch_dtype == torch.bfloat16:
        return SM3_BF16
    if torch_dtype == torch.float16:
        return SM3_F16
    raise ValueError(f"unsupported activation dtype {torch_dtype}")


# ------------------------------------------------------------------------------------------
# conv descriptors
# ------------------------------------------------------------------------------------------
def make_desc(dtype, N, Hi, Wi, Ci, Ho, Wo, Co, sy, sx, taps, w_row_stride, Hout=None, Wout=None,
              osy=1, osx=1, ooy=0, oox=0):
    """taps: list of (dy, dx, wtap)."""
    d = ConvDesc()
    d.dtype = dtype
    d.N, d.Hi, d.Wi, d.Ci = N, Hi, Wi, Ci
    d.Ho, d.Wo, d.Co = Ho, Wo, Co
    d.sy, d.sx = sy, sx
    d.ntaps = len(taps)
    if not 1 <= len(taps) <= _lib.MAX_TAPS:
        raise ValueError("1..9 taps")
    for i, (dy, dx, wt) in enumerate(taps):
        d.dy[i], d.dx[i], d.wtap[i] = dy, dx, wt
    d.w_row_stride = w_row_stride
    d.Hout = Ho if Hout is None else Hout
    d.Wout = Wo if Wout is None else Wout
    d.osy, d.osx, d.ooy, d.oox = osy, osx, ooy, oox
    return d


def fwd_desc(dtype, N, Hi, Wi, Ci, Co, k, stride, pad):
    """Forward conv k x k / stride / pad over NHWC x with OHWI weights [Co][k*k][Ci]."""
    Ho = (Hi + 2 * pad - k) // stride + 1
    Wo = (Wi + 2 * pad - k) // stride + 1
    taps = [(kh - pad, kw - pad, kh * k + kw) for kh in range(k) for kw in range(k)]
    return make_desc(dtype, N, Hi, Wi, Ci, Ho, Wo, Co, stride, stride, taps, k * k * Ci)


def dgrad_descs(dtype, N, Hi, Wi, Ci, Co, k, stride, pad):
    """Data gradient of fwd_desc(...) as gather-GEMMs over dY [N,Ho,Wo,Co] with the transposed filter
    bank w_dgrad [Ci][k*k][Co]: one descriptor per output-parity class (stride^2 of them), each with
    only the taps that hit real dY pixels.  Returns (descs, covers_everything)."""
    Ho = (Hi + 2 * pad - k) // stride + 1
    Wo = (Wi + 2 * pad - k) // stride + 1
    descs, full = [], True
    for py in range(stride):
        for px in range(stride):
            Hq = (Hi - py + stride - 1) // stride
            Wq = (Wi - px + stride - 1) // stride
            if Hq <= 0 or Wq <= 0:
                continue
            taps = [((py + pad - kh) // stride, (px + pad - kw) // stride, kh * k + kw)
                    for kh in range(k) for kw in range(k)
                    if (py + pad - kh) % stride == 0 and (px + pad - kw) % stride == 0]
            if not taps:
                full = False
                continue
            descs.append(make_desc(dtype, N, Ho, Wo, Co, Hq, Wq, Ci, 1, 1, taps, k * k * Co,
                                   Hout=Hi, Wout=Wi, osy=stride, osx=stride, ooy=py, oox=px))
    return descs, full


def conv_partial_rows(desc):
    return _lib.load().sm3_conv_partial_rows(C.byref(desc))


def _conv_tag(desc):
    """Profiler class = the tile the library picks (csrc/conv_igemm.hip, conv_gather_gemm_impl): 128 x 64 for Co <= 64 and
    for the small-M Linears whose 128-column grid would leave most CUs idle (those also take the 4-stage K-loop)."""
    M = desc.N * desc.Ho * desc.Wo
    nsteps = desc.ntaps * (desc.Ci * _sz(desc.dtype) // 128)
    tiles128 = ((M + 127) // 128) * ((desc.Co + 127) // 128)
    return "conv_gemm_128x64" if desc.Co <= 64 or (tiles128 <= 96 and nsteps >= 6) else "conv_gemm_128x128"


def conv_gemm(desc, x, w, y, addend=None, partials=None):
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(w, tdt, "w"); _chk(y, tdt, "y"); _chk(addend, tdt, "addend")
    _chk(partials, torch.float32, "partials")
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci:
        raise ValueError(f"x has {x.numel()} elements, descriptor says {desc.N}x{desc.Hi}x{desc.Wi}x{desc.Ci}")
    if y.numel() != desc.N * desc.Hout * desc.Wout * desc.Co:
        raise ValueError("y size does not match descriptor")
    if addend is not None and addend.numel() != y.numel():
        raise ValueError("addend size does not match y")
    need_w = (desc.Co - 1) * desc.w_row_stride + max(desc.wtap[i] for i in range(desc.ntaps)) * desc.Ci + desc.Ci
    if w.numel() < need_w:
        raise ValueError("w too small for descriptor")
    if desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError(f"Ci={desc.Ci} is not a multiple of {K_CHUNK[desc.dtype]}")
    if partials is not None and partials.numel() < conv_partial_rows(desc) * 2 * desc.Co:
        raise ValueError("partials workspace too small")
    M = desc.N * desc.Ho * desc.Wo
    flops = 2.0 * M * desc.Co * desc.ntaps * desc.Ci
    sz = _sz(desc.dtype)
    nbytes = sz * (min(x.numel(), M * desc.ntaps * desc.Ci) + M * desc.Co * (2 if addend is not None else 1)
                   + desc.Co * desc.ntaps * desc.Ci)
    tag = _conv_tag(desc)
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.ntaps}x{desc.Ci}_N{desc.Co}_s{desc.osy}"
    with _prof(tag, flops, nbytes):
        check(_lib.load().sm3_conv_gather_gemm(C.byref(desc), _ptr(x), _ptr(w), _ptr(y), _ptr(addend),
                                               _ptr(partials), _stream()), "sm3_conv_gather_gemm")


def conv_dgrad_bnfuse(desc, dy_in, w_dgrad, dz_out, addend, mask, bn_x, mean, invstd, partials, row_offset,
                      views=1, row_offset_view1=0, addend_sparse=None):
    """Data-gradient launch that also masks with the producer BN's ReLU bits and emits its backward partial sums
    (see sm3_conv_dgrad_bnfuse).  Returns the number of partial rows this launch wrote (both views together).
    views=2: the launch's rows are two views back to back (each a multiple of 128 rows), mean/invstd are [2][C],
    view 0's tiles write partial rows from row_offset, view 1's from row_offset_view1."""
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(dy_in, tdt, "dy_in"); _chk(w_dgrad, tdt, "w"); _chk(dz_out, tdt, "dz_out"); _chk(addend, tdt, "addend")
    _chk(bn_x, tdt, "bn_x"); _chk(mask, torch.uint8, "mask"); _chk(mean, torch.float32); _chk(invstd, torch.float32)
    _chk(partials, torch.float32, "partials")
    if dy_in.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci:
        raise ValueError("dy_in size does not match descriptor")
    n_out = desc.N * desc.Hout * desc.Wout * desc.Co
    if dz_out.numel() != n_out or (bn_x is not None and bn_x.numel() != n_out):
        raise ValueError("dz_out / bn_x size does not match descriptor")
    if addend_sparse is not None:  # compact [N, Hs, Ws, Co] addend for the even output positions
        hs, ws = addend_sparse
        dense = (desc.osy, desc.osx, desc.ooy, desc.oox) == (1, 1, 0, 0) and (desc.Hout, desc.Wout) == (desc.Ho, desc.Wo)
        # dense output: the addend covers the even pixels of the launch's grid; the (0, 0) parity class of a stride-2 data
        # gradient: the launch's own grid IS the even pixels, so the addend has its shape
        want = ((desc.Ho + 1) // 2, (desc.Wo + 1) // 2) if dense else (desc.Ho, desc.Wo)
        even_class = (desc.osy, desc.osx, desc.ooy, desc.oox) == (2, 2, 0, 0)
        if addend is None or (not dense and not even_class) or (hs, ws) != want or \
                addend.numel() != desc.N * hs * ws * desc.Co:
            raise ValueError("sparse addend size does not match descriptor")
    elif addend is not None and addend.numel() != n_out:
        raise ValueError("addend size does not match descriptor")
    if mask is not None and mask.numel() != n_out // (16 // _sz(desc.dtype)):
        raise ValueError("mask size mismatch")
    f = _bn_fuse_struct(desc, mask, bn_x, mean, invstd, partials, row_offset, views, row_offset_view1, addend_sparse)
    prow = conv_partial_rows(desc)
    if desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError(f"Ci={desc.Ci} is not a multiple of {K_CHUNK[desc.dtype]}")
    M = desc.N * desc.Ho * desc.Wo
    sz = _sz(desc.dtype)
    tag = _conv_tag(desc)
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.ntaps}x{desc.Ci}_N{desc.Co}_s{desc.osy}_fz"
    with _prof(tag, 2.0 * M * desc.Co * desc.ntaps * desc.Ci,
               sz * (min(dy_in.numel(), M * desc.ntaps * desc.Ci)
                     + M * desc.Co * (1 + (addend is not None) + (bn_x is not None)))):
        check(_lib.load().sm3_conv_dgrad_bnfuse(C.byref(desc), _ptr(dy_in), _ptr(w_dgrad), _ptr(dz_out), _ptr(addend),
                                                C.byref(f), _stream()), "sm3_conv_dgrad_bnfuse")
    return prow


def _bn_fuse_struct(desc, mask, bn_x, mean, invstd, partials, row_offset, views, row_offset_view1, addend_sparse=None):
    """sm3_bn_bwd_fuse for a data-gradient launch over `desc` (sizes checked).  bn_x None: mask + sum(dz) only."""
    n_out = desc.N * desc.Hout * desc.Wout * desc.Co
    if mask is not None and mask.numel() != n_out // (16 // _sz(desc.dtype)):
        raise ValueError("mask size mismatch")
    if bn_x is not None and (mean is None or invstd is None or mean.numel() < views * desc.Co
                             or invstd.numel() < views * desc.Co):
        raise ValueError("mean/invstd too small")
    prow = conv_partial_rows(desc)
    if views == 1:
        if partials.numel() < (row_offset + prow) * 2 * desc.Co:
            raise ValueError("partials workspace too small")
    else:
        if views != 2 or (desc.N * desc.Ho * desc.Wo) % 256 or prow % 2:
            raise ValueError("two views need a multiple of 128 rows each")
        if partials.numel() < (max(row_offset, row_offset_view1) + prow // 2) * 2 * desc.Co:
            raise ValueError("partials workspace too small")
    f = _lib.BnBwdFuse()
    f.relu_mask = mask.data_ptr() if mask is not None else None
    f.x = bn_x.data_ptr() if bn_x is not None else None
    f.mean = mean.data_ptr() if bn_x is not None else None
    f.invstd = invstd.data_ptr() if bn_x is not None else None
    f.partials = partials.data_ptr()
    f.partial_row_offset = row_offset
    f.views, f.partial_row_offset_view1 = views, row_offset_view1
    f.addend_sp_h, f.addend_sp_w = addend_sparse if addend_sparse is not None else (0, 0)
    return f


def conv_dgrad_seg_bnfuse(desc, x0, w0, x1, w1, col_bias, dz_out, mask, bn_x, mean, invstd, partials, row_offset,
                          views=1, row_offset_view1=0, w_view_stride=0, w1_view_stride=0):
    """dz_out = mask(x0 w0^T + x1 w1^T + col_bias) with the producer BatchNorm's backward phase 1 in the epilogue
    (sm3_conv_dgrad_seg_bnfuse): the data gradient of conv -> BatchNorm by linearity.  desc: the 1x1 data-gradient
    descriptor of x0 ([pixels][desc.Ci]); x1: [pixels][Ci1]; w0: [views][Co][Ci], w1: [views][Co][Ci1]; col_bias:
    fp32 [views][Co].  Returns the number of partial rows written."""
    tdt = TORCH_DTYPE[desc.dtype]
    for t, n in ((x0, "x0"), (w0, "w0"), (x1, "x1"), (w1, "w1"), (dz_out, "dz_out"), (bn_x, "bn_x")):
        _chk(t, tdt, n)
    _chk(col_bias, torch.float32, "col_bias"); _chk(mask, torch.uint8, "mask"); _chk(partials, torch.float32, "partials")
    _chk(mean, torch.float32); _chk(invstd, torch.float32)
    if desc.dtype == SM3_F32:
        raise ValueError("conv_dgrad_seg_bnfuse: 16-bit activation types only")
    M = desc.N * desc.Ho * desc.Wo
    if desc.ntaps != 1 or desc.Hout != desc.Ho or desc.Wout != desc.Wo or desc.Hi != desc.Ho or desc.Wi != desc.Wo:
        raise ValueError("conv_dgrad_seg_bnfuse: 1x1 / stride-1 descriptor expected")
    if x0.numel() != M * desc.Ci or x1.numel() % M or dz_out.numel() != M * desc.Co:
        raise ValueError("conv_dgrad_seg_bnfuse: operand size does not match descriptor")
    Ci1 = x1.numel() // M
    if Ci1 % K_CHUNK[desc.dtype] or desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError("conv_dgrad_seg_bnfuse: channel counts must be multiples of the K chunk")
    if w0.numel() < (views - 1) * w_view_stride + desc.Co * desc.w_row_stride or \
            w1.numel() < (views - 1) * w1_view_stride + desc.Co * Ci1:
        raise ValueError("conv_dgrad_seg_bnfuse: weight bank too small")
    if col_bias is not None and col_bias.numel() < views * desc.Co:
        raise ValueError("conv_dgrad_seg_bnfuse: col_bias too small")
    if bn_x is not None and bn_x.numel() != dz_out.numel():
        raise ValueError("conv_dgrad_seg_bnfuse: bn_x size mismatch")
    f = _bn_fuse_struct(desc, mask, bn_x, mean, invstd, partials, row_offset, views, row_offset_view1)
    sg = _lib.ConvSeg()
    sg.x1, sg.w1, sg.Ci1 = x1.data_ptr(), w1.data_ptr(), Ci1
    sg.w_view_stride, sg.w1_view_stride = w_view_stride, w1_view_stride
    sg.col_bias = col_bias.data_ptr() if col_bias is not None else None
    sz = _sz(desc.dtype)
    tag = _conv_tag(desc)
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.Ci}+{Ci1}_N{desc.Co}_seg_fz"
    # algorithmic work = the convolution's data gradient (K = desc.Ci); the second segment is this implementation's cost
    with _prof(tag, 2.0 * M * desc.Co * desc.Ci,
               sz * (x0.numel() + x1.numel() + M * desc.Co * (1 + (bn_x is not None)))):
        check(_lib.load().sm3_conv_dgrad_seg_bnfuse(C.byref(desc), _ptr(x0), _ptr(w0), C.byref(sg), _ptr(dz_out), None,
                                                    C.byref(f), _stream()), "sm3_conv_dgrad_seg_bnfuse")
    return conv_partial_rows(desc)


def conv_gemm_seg(desc, x0, w0, x1, w1, col_bias, y, addend=None, views=1, w_view_stride=0, w1_view_stride=0):
    """y = x0 w0^T + x1 w1^T + col_bias (+ addend, which may be y itself) with per-view banks (sm3_conv_gather_gemm_seg):
    the data gradient of a downsample conv -> BatchNorm pair by linearity."""
    tdt = TORCH_DTYPE[desc.dtype]
    for t, n in ((x0, "x0"), (w0, "w0"), (x1, "x1"), (w1, "w1"), (y, "y"), (addend, "addend")):
        _chk(t, tdt, n)
    _chk(col_bias, torch.float32, "col_bias")
    if desc.dtype == SM3_F32:
        raise ValueError("conv_gemm_seg: 16-bit activation types only")
    M = desc.N * desc.Ho * desc.Wo
    if desc.ntaps != 1 or desc.Hout != desc.Ho or desc.Wout != desc.Wo or desc.Hi != desc.Ho or desc.Wi != desc.Wo:
        raise ValueError("conv_gemm_seg: 1x1 / stride-1 descriptor expected")
    if x0.numel() != M * desc.Ci or x1.numel() % M or y.numel() != M * desc.Co or \
            (addend is not None and addend.numel() != y.numel()):
        raise ValueError("conv_gemm_seg: operand size does not match descriptor")
    Ci1 = x1.numel() // M
    if Ci1 % K_CHUNK[desc.dtype] or desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError("conv_gemm_seg: channel counts must be multiples of the K chunk")
    if w0.numel() < (views - 1) * w_view_stride + desc.Co * desc.w_row_stride or \
            w1.numel() < (views - 1) * w1_view_stride + desc.Co * Ci1 or \
            (col_bias is not None and col_bias.numel() < views * desc.Co):
        raise ValueError("conv_gemm_seg: weight bank / col_bias too small")
    if views > 1 and (views != 2 or M % 256):
        raise ValueError("two views need a multiple of 128 rows each")
    sg = _lib.ConvSeg()
    sg.x1, sg.w1, sg.Ci1 = x1.data_ptr(), w1.data_ptr(), Ci1
    sg.w_view_stride, sg.w1_view_stride = w_view_stride, w1_view_stride
    sg.col_bias = col_bias.data_ptr() if col_bias is not None else None
    sg.views = views
    sz = _sz(desc.dtype)
    tag = _conv_tag(desc)
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.Ci}+{Ci1}_N{desc.Co}_seg"
    with _prof(tag, 2.0 * M * desc.Co * desc.Ci, sz * (x0.numel() + x1.numel() + M * desc.Co * (1 + (addend is not None)))):
        check(_lib.load().sm3_conv_gather_gemm_seg(C.byref(desc), _ptr(x0), _ptr(w0), C.byref(sg), _ptr(y), _ptr(addend),
                                                   _stream()), "sm3_conv_gather_gemm_seg")


def conv_seg_act(desc, x0, w0, x1, w1, col_bias, y, mask=None, relu=True, views=1, w_view_stride=0, w1_view_stride=0):
    """y = relu?(x0 w0^T + x1 w1^T + col_bias) with the ReLU bits in `mask` (sm3_conv_seg_act): with BatchNorm-scaled banks
    (linbn_scale_banks) the whole join of a Bottleneck that has a downsample branch."""
    tdt = TORCH_DTYPE[desc.dtype]
    for t, n in ((x0, "x0"), (w0, "w0"), (x1, "x1"), (w1, "w1"), (y, "y")):
        _chk(t, tdt, n)
    _chk(col_bias, torch.float32, "col_bias"); _chk(mask, torch.uint8, "mask")
    if desc.dtype == SM3_F32:
        raise ValueError("conv_seg_act: 16-bit activation types only")
    M = desc.N * desc.Ho * desc.Wo
    if desc.ntaps != 1 or desc.Hout != desc.Ho or desc.Wout != desc.Wo or desc.Hi != desc.Ho or desc.Wi != desc.Wo:
        raise ValueError("conv_seg_act: 1x1 / stride-1 descriptor expected")
    if x0.numel() != M * desc.Ci or x1.numel() % M or y.numel() != M * desc.Co:
        raise ValueError("conv_seg_act: operand size does not match descriptor")
    Ci1 = x1.numel() // M
    if Ci1 % K_CHUNK[desc.dtype] or desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError("conv_seg_act: channel counts must be multiples of the K chunk")
    if w0.numel() < (views - 1) * w_view_stride + desc.Co * desc.w_row_stride or \
            w1.numel() < (views - 1) * w1_view_stride + desc.Co * Ci1 or col_bias.numel() < views * desc.Co:
        raise ValueError("conv_seg_act: weight bank / col_bias too small")
    if mask is not None and (not relu or mask.numel() != M * desc.Co // (16 // _sz(desc.dtype))):
        raise ValueError("conv_seg_act: mask size mismatch")
    if views > 1 and (views != 2 or M % 256):
        raise ValueError("two views need a multiple of 128 rows each")
    sg = _lib.ConvSeg()
    sg.x1, sg.w1, sg.Ci1 = x1.data_ptr(), w1.data_ptr(), Ci1
    sg.w_view_stride, sg.w1_view_stride = w_view_stride, w1_view_stride
    sg.col_bias = col_bias.data_ptr()
    sg.views = views
    sz = _sz(desc.dtype)
    tag = _conv_tag(desc)
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.Ci}+{Ci1}_N{desc.Co}_segact"
    with _prof(tag, 2.0 * M * desc.Co * (desc.Ci + Ci1), sz * (x0.numel() + x1.numel() + M * desc.Co)):
        check(_lib.load().sm3_conv_seg_act(C.byref(desc), _ptr(x0), _ptr(w0), C.byref(sg), int(relu), _ptr(y), _ptr(mask),
                                           _stream()), "sm3_conv_seg_act")


def conv_bn_act_eval(desc, x, w, scale, shift, residual, relu, y):
    """conv + eval-mode BN (+residual) (+ReLU) in one launch (sm3_conv_bn_act_eval)."""
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(w, tdt, "w"); _chk(y, tdt, "y"); _chk(residual, tdt, "residual")
    _chk(scale, torch.float32, "scale"); _chk(shift, torch.float32, "shift")
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci:
        raise ValueError("x size does not match descriptor")
    n_out = desc.N * desc.Hout * desc.Wout * desc.Co
    if y.numel() != n_out or (residual is not None and residual.numel() != n_out):
        raise ValueError("y / residual size does not match descriptor")
    if scale.numel() < desc.Co or shift.numel() < desc.Co:
        raise ValueError("scale/shift too small")
    if desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError(f"Ci={desc.Ci} is not a multiple of {K_CHUNK[desc.dtype]}")
    M = desc.N * desc.Ho * desc.Wo
    sz = _sz(desc.dtype)
    with _prof(_conv_tag(desc), 2.0 * M * desc.Co * desc.ntaps * desc.Ci,
               sz * (min(x.numel(), M * desc.ntaps * desc.Ci) + M * desc.Co * (2 if residual is not None else 1))):
        check(_lib.load().sm3_conv_bn_act_eval(C.byref(desc), _ptr(x), _ptr(w), _ptr(scale), _ptr(shift),
                                               _ptr(residual), int(relu), _ptr(y), _stream()), "sm3_conv_bn_act_eval")


def conv_bn_eval(desc, x, w, gamma, beta, running_mean, running_var, eps, residual, relu, y):
    """conv + eval-mode BN (+residual) (+ReLU) in one launch, scale/shift derived in the epilogue (sm3_conv_bn_eval)."""
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(w, tdt, "w"); _chk(y, tdt, "y"); _chk(residual, tdt, "residual")
    for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _chk(t, torch.float32, n)
        if t is not None and t.numel() < desc.Co:
            raise ValueError(f"{n} too small")
    if running_mean is None or running_var is None:
        raise ValueError("running statistics are required")
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci:
        raise ValueError("x size does not match descriptor")
    n_out = desc.N * desc.Hout * desc.Wout * desc.Co
    if y.numel() != n_out or (residual is not None and residual.numel() != n_out):
        raise ValueError("y / residual size does not match descriptor")
    if desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError(f"Ci={desc.Ci} is not a multiple of {K_CHUNK[desc.dtype]}")
    M = desc.N * desc.Ho * desc.Wo
    sz = _sz(desc.dtype)
    with _prof(_conv_tag(desc), 2.0 * M * desc.Co * desc.ntaps * desc.Ci,
               sz * (min(x.numel(), M * desc.ntaps * desc.Ci) + M * desc.Co * (2 if residual is not None else 1))):
        check(_lib.load().sm3_conv_bn_eval(C.byref(desc), _ptr(x), _ptr(w), _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                           _ptr(running_var), float(eps), _ptr(residual), int(relu), _ptr(y), _stream()),
              "sm3_conv_bn_eval")


def conv_wgrad(desc, x, dy, dw):
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(dy, tdt, "dy"); _chk(dw, torch.float32, "dw")
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci:
        raise ValueError("x size does not match descriptor")
    if dy.numel() != desc.N * desc.Ho * desc.Wo * desc.Co:
        raise ValueError("dy size does not match descriptor")
    if dw.numel() < desc.Co * desc.w_row_stride:
        raise ValueError("dw too small")
    M = desc.N * desc.Ho * desc.Wo
    sz = _sz(desc.dtype)
    tag = "conv_wgrad"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.ntaps}x{desc.Ci}_N{desc.Co}"
    with _prof(tag, 2.0 * M * desc.Co * desc.ntaps * desc.Ci,
               sz * (x.numel() + dy.numel()) + 4 * desc.Co * desc.w_row_stride):
        check(_lib.load().sm3_conv_wgrad(C.byref(desc), _ptr(x), _ptr(dy), _ptr(dw), _stream()), "sm3_conv_wgrad")


WGRAD_SLAB_CAP = 512          # slabs a deterministic weight-gradient launch may use (sm3_conv_wgrad_det); 512: the nine-tap
                              # owner on 56 x 56 x 64 has ONE tile pair, so its slices are its workgroups (256 -> 512: 189 -> 140 us)
WGRAD_SLAB_FLOATS = 1 << 26   # ... within a workspace of at most max(this, 8 slabs) floats


def wgrad_det_cap(n):
    """Slabs of n floats the deterministic weight gradient gets: a function of n alone."""
    return max(8, min(WGRAD_SLAB_CAP, WGRAD_SLAB_FLOATS // max(n, 1)))


def conv_wgrad_det(desc, x, dy, dw, slabs, cap):
    """dw += dy^T x with a fixed-order split-K sum instead of float atomics (sm3_conv_wgrad_det): bit-reproducible.
    slabs: fp32 workspace with room for `cap` matrices [Co][taps * Ci]."""
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(dy, tdt, "dy"); _chk(dw, torch.float32, "dw"); _chk(slabs, torch.float32, "slabs")
    n = desc.Co * desc.w_row_stride
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci:
        raise ValueError("x size does not match descriptor")
    if dy.numel() != desc.N * desc.Ho * desc.Wo * desc.Co:
        raise ValueError("dy size does not match descriptor")
    if dw.numel() < n or desc.w_row_stride != desc.ntaps * desc.Ci:
        raise ValueError("dw too small / padded weight rows")
    if cap < 1 or slabs.numel() < cap * n:
        raise ValueError("conv_wgrad_det: slab buffer too small")
    M = desc.N * desc.Ho * desc.Wo
    sz = _sz(desc.dtype)
    tag = "conv_wgrad"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.ntaps}x{desc.Ci}_N{desc.Co}"
    with _prof(tag, 2.0 * M * desc.Co * desc.ntaps * desc.Ci, sz * (x.numel() + dy.numel()) + 4 * n):
        check(_lib.load().sm3_conv_wgrad_det(C.byref(desc), _ptr(x), _ptr(dy), _ptr(dw), _ptr(slabs), int(cap), _stream()),
              "sm3_conv_wgrad_det")


def slab_reduce(slabs, nslabs, n, out, accumulate=False):
    """out[:n] (+)= sum of nslabs slabs of n floats, fixed order (sm3_slab_reduce)."""
    _chk(slabs, torch.float32, "slabs"); _chk(out, torch.float32, "out")
    if slabs.numel() < nslabs * n or out.numel() < n or n % 4 or nslabs < 1:
        raise ValueError("slab_reduce: size mismatch")
    with _prof("slab_reduce", 0.0, 4.0 * n * (nslabs + 1)):
        check(_lib.load().sm3_slab_reduce(_ptr(slabs), int(nslabs), int(n), _ptr(out), int(bool(accumulate)), _stream()),
              "sm3_slab_reduce")


def grouped_gemm(x, w, y, groups, partials=None):
    """y[:, g*N:(g+1)*N] = x[:, g*K:(g+1)*K] @ w[g]^T for g < groups, one exact-f32 launch (sm3_grouped_gemm).  x: [rows, G*K],
    w: [G, N, K] (or [G*N, K]), y: [rows, G*N] fp32; partials: [ceil(rows / 128), 2, G*N] BatchNorm sums of y, or None.
    The data gradient is the same call with the transposed banks [G, K, N]."""
    for t, n in ((x, "x"), (w, "w"), (y, "y")):
        _chk(t, torch.float32, n)
    _chk(partials, torch.float32, "partials")
    rows = x.shape[0]
    K, N = x.shape[1] // groups, y.shape[1] // groups
    if x.dim() != 2 or y.dim() != 2 or y.shape[0] != rows or K * groups != x.shape[1] or N * groups != y.shape[1]:
        raise ValueError("grouped_gemm: x [rows, G*K] and y [rows, G*N]")
    if w.numel() != groups * N * K:
        raise ValueError("grouped_gemm: w must hold G banks [N, K]")
    if K % K_CHUNK[SM3_F32] or N % 4:
        raise ValueError(f"grouped_gemm: K a multiple of {K_CHUNK[SM3_F32]}, N of 4")
    if partials is not None and partials.numel() < ((rows + 127) // 128) * 2 * groups * N:
        raise ValueError("grouped_gemm: partials too small")
    with _prof("grouped_gemm", 2.0 * rows * groups * N * K, 4.0 * (x.numel() + w.numel() + y.numel())):
        check(_lib.load().sm3_grouped_gemm(SM3_F32, _ptr(x), _ptr(w), _ptr(y), _ptr(partials), rows, groups, K, N, _stream()),
              "sm3_grouped_gemm")


def grouped_wgrad_slab_cap(rows, n):
    """Slabs sm3_grouped_wgrad_det may fill for one group of n floats: wgrad_det_cap(n), and never more than the slices a
    1x1 f32 product of `rows` pixels is cut into (32 pixels per K-group pair x 8) -- a function of (rows, n) alone."""
    return max(1, min(wgrad_det_cap(n), (rows + 255) // 256))


def grouped_wgrad_det(x, dy, dw, groups, slabs=None):
    """dw[g] += dy[:, g*N:(g+1)*N]^T @ x[:, g*K:(g+1)*K], fixed order (sm3_grouped_wgrad_det).  dw: [G, N, K] fp32."""
    for t, n in ((x, "x"), (dy, "dy"), (dw, "dw")):
        _chk(t, torch.float32, n)
    rows = x.shape[0]
    K, N = x.shape[1] // groups, dy.shape[1] // groups
    if dy.shape[0] != rows or K * groups != x.shape[1] or N * groups != dy.shape[1] or dw.numel() != groups * N * K:
        raise ValueError("grouped_wgrad_det: x [rows, G*K], dy [rows, G*N], dw [G, N, K]")
    cap = grouped_wgrad_slab_cap(rows, N * K)
    if slabs is None:
        slabs = torch.empty(cap * groups * N * K, dtype=torch.float32, device=x.device)
    _chk(slabs, torch.float32, "slabs")
    if slabs.numel() < cap * groups * N * K:
        raise ValueError("grouped_wgrad_det: slab buffer too small")
    with _prof("grouped_wgrad", 2.0 * rows * groups * N * K, 4.0 * (x.numel() + dy.numel() + dw.numel())):
        check(_lib.load().sm3_grouped_wgrad_det(SM3_F32, _ptr(x), _ptr(dy), _ptr(dw), _ptr(slabs), int(cap), rows, groups, K, N,
                                                _stream()), "sm3_grouped_wgrad_det")


# ------------------------------------------------------------------------------------------
# grouped 3x3 convolution (ResNeXt conv2, csrc/gconv.hip): NHWC, pad 1, G groups of C / G channels
# ------------------------------------------------------------------------------------------
def _gconv_chk(dtype, N, H, W, C, groups, stride):
    if C % groups or (C // groups) not in (4, 8, 16, 32, 64) or C % 64 or stride not in (1, 2):
        raise ValueError(f"grouped 3x3 conv: C={C}, groups={groups}, stride={stride} not supported")
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def gconv_weight_prep(dtype, master, C, groups, w_fwd, w_dgrad, only_if=None):
    """fp32 master [C][3][3][C/groups] (OHWI) -> `dtype` banks w_fwd / w_dgrad [9][C/groups][C] (sm3_gconv_weight_prep)."""
    tdt = TORCH_DTYPE[dtype]
    _chk(master, torch.float32, "master"); _chk(w_fwd, tdt, "w_fwd"); _chk(w_dgrad, tdt, "w_dgrad")
    _chk(only_if, torch.int32, "only_if")
    n = C * 9 * (C // groups)
    if master.numel() != n or w_fwd.numel() != n or w_dgrad.numel() != n:
        raise ValueError("gconv_weight_prep: size mismatch")
    with _prof("weight_prep", 0.0, n * (4.0 + 2 * _sz(dtype))):
        check(_lib.load().sm3_gconv_weight_prep(dtype, _ptr(master), _ptr(w_fwd), _ptr(w_dgrad), C, groups, _ptr(only_if),
                                                _stream()), "sm3_gconv_weight_prep")


def gconv_fwd(dtype, x, w_fwd, y, partials, N, H, W, C, groups, stride):
    """y [N*Ho*Wo, C] = grouped 3x3 conv of x [N*H*W, C]; partials: [ceil(rows / 128)][2][C] BatchNorm sums, or None."""
    tdt = TORCH_DTYPE[dtype]
    Ho, Wo = _gconv_chk(dtype, N, H, W, C, groups, stride)
    _chk(x, tdt, "x"); _chk(w_fwd, tdt, "w_fwd"); _chk(y, tdt, "y"); _chk(partials, torch.float32, "partials")
    M = N * Ho * Wo
    if x.numel() != N * H * W * C or y.numel() != M * C or w_fwd.numel() != 9 * C * (C // groups):
        raise ValueError("gconv_fwd: size mismatch")
    if partials is not None and partials.numel() < (M + 127) // 128 * 2 * C:
        raise ValueError("gconv_fwd: partials workspace too small")
    sz = _sz(dtype)
    with _prof("gconv_fwd", 2.0 * M * C * 9 * (C // groups), sz * (x.numel() + y.numel() + w_fwd.numel())):
        check(_lib.load().sm3_gconv_fwd(dtype, _ptr(x), _ptr(w_fwd), _ptr(y), _ptr(partials), N, H, W, C, groups, stride,
                                        _stream()), "sm3_gconv_fwd")


def gconv_dgrad(dtype, dy, w_dgrad, dx, N, H, W, C, groups, stride):
    """dx [N*H*W, C] = data gradient of the grouped 3x3 conv from dy [N*Ho*Wo, C] (sm3_gconv_dgrad)."""
    tdt = TORCH_DTYPE[dtype]
    Ho, Wo = _gconv_chk(dtype, N, H, W, C, groups, stride)
    _chk(dy, tdt, "dy"); _chk(w_dgrad, tdt, "w_dgrad"); _chk(dx, tdt, "dx")
    if dy.numel() != N * Ho * Wo * C or dx.numel() != N * H * W * C or w_dgrad.numel() != 9 * C * (C // groups):
        raise ValueError("gconv_dgrad: size mismatch")
    sz = _sz(dtype)
    with _prof("gconv_dgrad", 2.0 * N * Ho * Wo * C * 9 * (C // groups), sz * (dy.numel() + dx.numel() + w_dgrad.numel())):
        check(_lib.load().sm3_gconv_dgrad(dtype, _ptr(dy), _ptr(w_dgrad), _ptr(dx), N, H, W, C, groups, stride, _stream()),
              "sm3_gconv_dgrad")


def gconv_wgrad_slabs(N, H, W, stride, cap):
    """Slabs a grouped weight gradient over this geometry uses with `cap` slabs of room."""
    return _lib.load().sm3_gconv_wgrad_slabs(N, H, W, stride, cap)


def gconv_wgrad_det(dtype, x, dy, dw, slabs, cap, N, H, W, C, groups, stride):
    """dw [C, 9*C/groups] += dy^T x of the grouped 3x3 conv, fixed-order slab sum (sm3_gconv_wgrad_det): bit-reproducible."""
    tdt = TORCH_DTYPE[dtype]
    Ho, Wo = _gconv_chk(dtype, N, H, W, C, groups, stride)
    _chk(x, tdt, "x"); _chk(dy, tdt, "dy"); _chk(dw, torch.float32, "dw"); _chk(slabs, torch.float32, "slabs")
    n = C * 9 * (C // groups)
    if x.numel() != N * H * W * C or dy.numel() != N * Ho * Wo * C or dw.numel() != n:
        raise ValueError("gconv_wgrad_det: size mismatch")
    if cap < 1 or slabs.numel() < gconv_wgrad_slabs(N, H, W, stride, cap) * n:
        raise ValueError("gconv_wgrad_det: slab buffer too small")
    sz = _sz(dtype)
    with _prof("gconv_wgrad", 2.0 * N * Ho * Wo * C * 9 * (C // groups), sz * (x.numel() + dy.numel()) + 4 * n):
        check(_lib.load().sm3_gconv_wgrad_det(dtype, _ptr(x), _ptr(dy), _ptr(dw), _ptr(slabs), int(cap), N, H, W, C, groups,
                                              stride, _stream()), "sm3_gconv_wgrad_det")


def conv_wgrad_cat(desc, x, dy, dw, dy1=None, dw1=None, views=1):
    """P[v] = dy_v^T x_v -> dw [views][Co][Ci] (and, with dy1, G[v] = dy1_v^T x_v -> dw1 [views][Co1][Ci]) in one launch
    (sm3_conv_wgrad_cat), accumulated into fp32 buffers the caller zeroed."""
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(dy, tdt, "dy"); _chk(dy1, tdt, "dy1"); _chk(dw, torch.float32, "dw"); _chk(dw1, torch.float32, "dw1")
    M = desc.N * desc.Ho * desc.Wo
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci or dy.numel() != M * desc.Co or M % views:
        raise ValueError("conv_wgrad_cat: operand size does not match descriptor")
    if (dy1 is None) != (dw1 is None) or (dy1 is not None and dy1.numel() % M):
        raise ValueError("conv_wgrad_cat: dy1 and dw1 go together, dy1 over the same pixels")
    Co1 = dy1.numel() // M if dy1 is not None else 0
    if (Co1 and desc.Co % 128) or dw.numel() < views * desc.Co * desc.w_row_stride or \
            (Co1 and dw1.numel() < views * Co1 * desc.w_row_stride):
        raise ValueError("conv_wgrad_cat: Co must be a multiple of 128; dw / dw1 sized [views][rows][w_row_stride]")
    sz = _sz(desc.dtype)
    tag = "conv_wgrad"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.ntaps}x{desc.Ci}_N{desc.Co}+{Co1}_v{views}"
    with _prof(tag, 2.0 * M * desc.Co * desc.ntaps * desc.Ci,
               sz * (x.numel() + dy.numel()) + 4 * views * (desc.Co + Co1) * desc.w_row_stride):
        check(_lib.load().sm3_conv_wgrad_cat(C.byref(desc), _ptr(x), _ptr(dy), _ptr(dw), _ptr(dy1), Co1, _ptr(dw1), views,
                                             desc.Co * desc.w_row_stride, Co1 * desc.w_row_stride, _stream()),
              "sm3_conv_wgrad_cat")


SLAB_CAP = 256  # slabs per view a plain-store split-K launch may use (sm3_conv_wgrad_slabs)


def conv_wgrad_slabs(desc, x, dy, slabs, views=1, cap=None):
    """dy_v^T x_v without atomics: every pixel slice stores its partial [Co][taps*Ci] product into a slab of its own
    (sm3_conv_wgrad_slabs).  slabs: fp32 with room for views * SLAB_CAP slabs.  Returns the slabs used per view; the slabs
    of view v are slabs[(v * used + j) * Co * taps * Ci ...]."""
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(dy, tdt, "dy"); _chk(slabs, torch.float32, "slabs")
    M = desc.N * desc.Ho * desc.Wo
    n = desc.Co * desc.w_row_stride
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci or dy.numel() != M * desc.Co or M % views or \
            desc.w_row_stride != desc.ntaps * desc.Ci:
        raise ValueError("conv_wgrad_slabs: operand size does not match descriptor")
    # cap: slabs per view the launch may use.  It takes part in the partition of the pixel axis, so a caller that wants a view's
    # slabs to add up to the same bits in every launch configuration passes a cap that depends on n only (engine._slab_buf) --
    # the default, derived from the buffer's size, moves with whatever else grew a shared workspace.
    room = slabs.numel() // (views * n)
    cap = min(SLAB_CAP, room) if cap is None else int(cap)
    if cap < 1 or cap > room or cap > SLAB_CAP:
        raise ValueError("conv_wgrad_slabs: slab buffer too small")
    used = C.c_int(0)
    sz = _sz(desc.dtype)
    tag = "conv_wgrad"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.ntaps}x{desc.Ci}_N{desc.Co}_v{views}_slabs"
    with _prof(tag, 2.0 * M * desc.Co * desc.ntaps * desc.Ci, sz * (x.numel() + dy.numel())):
        check(_lib.load().sm3_conv_wgrad_slabs(C.byref(desc), _ptr(x), _ptr(dy), _ptr(slabs), cap, views, C.byref(used),
                                               _stream()), "sm3_conv_wgrad_slabs")
    return used.value


def _lin_tag(name, a, b):
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        return f"linbn_small|{name[6:]}_{a}_{b}"
    return "linbn_small"


def linbn_moments(slabs, nslabs, n, out, views=1, colsum=None, colsum_rows=0, s_out=None, p=0):
    """out[v] = sum of view v's nslabs slabs (fixed order); with colsum partial rows also s_out[v] = their sum
    (sm3_linbn_moments)."""
    _chk(slabs, torch.float32, "slabs"); _chk(out, torch.float32, "out"); _chk(colsum, torch.float32, "colsum")
    _chk(s_out, torch.float64, "s_out")
    if slabs.numel() < views * nslabs * n or out.numel() < views * n or n % 4:
        raise ValueError("linbn_moments: size mismatch")
    if colsum is not None and (s_out is None or colsum.numel() < views * colsum_rows * p or s_out.numel() < views * p):
        raise ValueError("linbn_moments: colsum / s_out size mismatch")
    with _prof(_lin_tag("linbn_moments", n, nslabs), 0.0, 4.0 * views * n * (nslabs + 1)):
        check(_lib.load().sm3_linbn_moments(_ptr(slabs), nslabs, n, _ptr(out), _ptr(colsum), colsum_rows, _ptr(s_out), p,
                                            views, _stream()), "sm3_linbn_moments")


def linbn_fwd_stats(dtype, G, w_dgrad, w_fwd, s, Tm, sums_ws, Cn, p, views=1):
    """Tm[v] = W G_v and the batch sums of x = y W^T as [views][p/32][2C] fp64 partial rows for bn_finalize(groups=p/32)
    (sm3_linbn_fwd_stats).  Returns the number of groups."""
    tdt = TORCH_DTYPE[dtype]
    _chk(G, torch.float32, "G"); _chk(w_dgrad, tdt, "w_dgrad"); _chk(w_fwd, tdt, "w_fwd"); _chk(s, torch.float64, "s")
    _chk(Tm, torch.float32, "Tm"); _chk(sums_ws, torch.float64, "sums_ws")
    if Cn % 32 or p % 32 or G.numel() < views * p * p or w_dgrad.numel() != p * Cn or w_fwd.numel() != Cn * p or \
            s.numel() < views * p or Tm.numel() < views * Cn * p or sums_ws.numel() < views * (p // 32) * 2 * Cn:
        raise ValueError("linbn_fwd_stats: size mismatch")
    with _prof(_lin_tag("linbn_fwd_stats", Cn, p), 2.0 * views * Cn * p * p, 4.0 * views * (Cn * p + p * p) + _sz(dtype) * 2 * Cn * p):
        check(_lib.load().sm3_linbn_fwd_stats(dtype, _ptr(G), _ptr(w_dgrad), _ptr(w_fwd), _ptr(s), _ptr(Tm), _ptr(sums_ws),
                                              Cn, p, views, _stream()), "sm3_linbn_fwd_stats")
    return p // 32


def linbn_fold(sums_ws, groups, n, out, views=1):
    """out[v] = sum of the `groups` partial rows of sums_ws [views][groups][n] (sm3_linbn_fold)."""
    _chk(sums_ws, torch.float64, "sums_ws"); _chk(out, torch.float64, "out")
    if sums_ws.numel() < views * groups * n or out.numel() < views * n:
        raise ValueError("linbn_fold: size mismatch")
    with _prof(_lin_tag("linbn_fold", n, groups), 0.0, 8.0 * views * n * (groups + 1)):
        check(_lib.load().sm3_linbn_fold(_ptr(sums_ws), groups, n, views, _ptr(out), _stream()), "sm3_linbn_fold")


def linbn_scale_banks(dtype, w3, scale3, shift3, out3, wd, scaled, shiftd, outd, bias, Cn, views=1):
    """out3[v] = diag(scale3[v]) w3, outd[v] = diag(scaled[v]) wd, bias[v] = shift3[v] + shiftd[v] (sm3_linbn_scale_banks)."""
    tdt = TORCH_DTYPE[dtype]
    for t in (w3, out3, wd, outd):
        _chk(t, tdt)
    for t in (scale3, shift3, scaled, shiftd, bias):
        _chk(t, torch.float32)
    if w3.numel() % Cn or wd.numel() % Cn:
        raise ValueError("linbn_scale_banks: bank size is not a multiple of C")
    K3, Kd = w3.numel() // Cn, wd.numel() // Cn
    if K3 % 8 or Kd % 8 or out3.numel() < views * Cn * K3 or outd.numel() < views * Cn * Kd or bias.numel() < views * Cn or \
            min(scale3.numel(), shift3.numel(), scaled.numel(), shiftd.numel()) < views * Cn:
        raise ValueError("linbn_scale_banks: size mismatch")
    with _prof(_lin_tag("linbn_scale_banks", Cn, K3 + Kd), 0.0, _sz(dtype) * (1 + views) * Cn * (K3 + Kd)):
        check(_lib.load().sm3_linbn_scale_banks(dtype, _ptr(w3), K3, _ptr(scale3), _ptr(shift3), _ptr(out3), _ptr(wd), Kd,
                                                _ptr(scaled), _ptr(shiftd), _ptr(outd), _ptr(bias), Cn, views, _stream()),
              "sm3_linbn_scale_banks")


def linbn_stats(dtype, P, w_fwd, mean, invstd, gamma, reduce_ws, groups, lsums, dgamma, dbeta, count, coef, Cn, p, views=1):
    """lsums[v] = (sum dz | sum dz * xhat): the first from stage A of bn_stats_reduce (reduce_ws, groups), the second from
    P = dz^T y; d(gamma), d(beta) accumulated; count > 0: coef [views][C][4] written too (sm3_linbn_stats)."""
    _chk(P, torch.float32, "P"); _chk(w_fwd, TORCH_DTYPE[dtype], "w_fwd")
    for t in (mean, invstd, gamma, dgamma, dbeta, coef):
        _chk(t, torch.float32)
    _chk(lsums, torch.float64, "lsums"); _chk(reduce_ws, torch.float64, "reduce_ws")
    if P.numel() < views * Cn * p or w_fwd.numel() != Cn * p or mean.numel() < views * Cn or invstd.numel() < views * Cn or \
            lsums.numel() < views * 2 * Cn or reduce_ws.numel() < views * groups * 2 * Cn or \
            (count > 0 and (coef is None or coef.numel() < views * 4 * Cn)):
        raise ValueError("linbn_stats: size mismatch")
    with _prof(_lin_tag("linbn_stats", Cn, p), 0.0, 4.0 * views * Cn * p):
        check(_lib.load().sm3_linbn_stats(dtype, _ptr(P), _ptr(w_fwd), _ptr(mean), _ptr(invstd), _ptr(gamma),
                                          _ptr(reduce_ws), groups, _ptr(lsums), _ptr(dgamma), _ptr(dbeta), float(count),
                                          _ptr(coef), Cn, p, views, _stream()), "sm3_linbn_stats")


def linbn_coef(gsums, count, gamma, mean, invstd, coef, Cn, views=1):
    _chk(gsums, torch.float64)
    for t in (gamma, mean, invstd, coef):
        _chk(t, torch.float32)
    if gsums.numel() < views * 2 * Cn or mean.numel() < views * Cn or invstd.numel() < views * Cn or coef.numel() < views * 4 * Cn:
        raise ValueError("linbn_coef: size mismatch")
    check(_lib.load().sm3_linbn_coef(_ptr(gsums), float(count), _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(coef), Cn, views,
                                     _stream()), "sm3_linbn_coef")


def linbn_banks(dtype, w_dgrad, coef, wa, wbn, col_const, Cn, p, views=1):
    tdt = TORCH_DTYPE[dtype]
    _chk(w_dgrad, tdt, "w_dgrad"); _chk(wa, tdt, "wa"); _chk(wbn, tdt, "wbn")
    _chk(coef, torch.float32); _chk(col_const, torch.float32)
    if w_dgrad.numel() != p * Cn or wa.numel() < views * p * Cn or wbn.numel() < views * p * Cn or \
            col_const.numel() < views * p or coef.numel() < views * 4 * Cn:
        raise ValueError("linbn_banks: size mismatch")
    if Cn % 8:
        raise ValueError(f"linbn_banks: C = {Cn} is not a multiple of 8 (the rows are walked in 16-byte vectors)")
    with _prof(_lin_tag("linbn_banks", Cn, p), 0.0, _sz(dtype) * p * Cn * (1 + 2 * views)):
        check(_lib.load().sm3_linbn_banks(dtype, _ptr(w_dgrad), _ptr(coef), _ptr(wa), _ptr(wbn), _ptr(col_const), Cn, p,
                                          views, _stream()), "sm3_linbn_banks")


def linbn_post(dtype, wbn, w_dgrad, hn, P, G, Tm, s, coef, dw, Cn, p, views=1):
    """hn[v] = wbn_v w_dgrad^T (= -H_v, dtype [views][p][p]);  dw += sum_v diag(a)(P_v - m1 s^T) - diag(b)(W G_v - mu s^T),
    W G_v from Tm or (Tm None) recomputed from G (sm3_linbn_post)."""
    tdt = TORCH_DTYPE[dtype]
    for t, n in ((wbn, "wbn"), (w_dgrad, "w_dgrad"), (hn, "hn")):
        _chk(t, tdt, n)
    for t in (P, G, Tm, coef, dw):
        _chk(t, torch.float32)
    _chk(s, torch.float64, "s")
    if wbn.numel() < views * p * Cn or w_dgrad.numel() != p * Cn or hn.numel() < views * p * p or \
            P.numel() < views * Cn * p or (G is None and Tm is None) or (G is not None and G.numel() < views * p * p) or \
            (Tm is not None and Tm.numel() < views * Cn * p) or s.numel() < views * p or \
            coef.numel() < views * 4 * Cn or dw.numel() != Cn * p or Cn % 128 or p % 32:
        raise ValueError("linbn_post: size mismatch")
    flops = 2.0 * views * p * p * Cn * (1 if Tm is not None else 2)
    with _prof(_lin_tag("linbn_post", Cn, p), flops, 4.0 * Cn * p * (2 + views) + _sz(dtype) * p * Cn * (1 + views)):
        check(_lib.load().sm3_linbn_post(dtype, _ptr(wbn), _ptr(w_dgrad), _ptr(hn), _ptr(P), _ptr(G), _ptr(Tm), _ptr(s),
                                         _ptr(coef), _ptr(dw), Cn, p, views, _stream()), "sm3_linbn_post")


def linbn_banks_post(dtype, w_dgrad, coef, wa, col_const, hn, P, G, Tm, s, dw, Cn, p, views=1):
    """linbn_banks + linbn_post in one launch (sm3_linbn_banks_post): same wa / col_const / hn / dw, bit for bit."""
    tdt = TORCH_DTYPE[dtype]
    for t, n in ((w_dgrad, "w_dgrad"), (wa, "wa"), (hn, "hn")):
        _chk(t, tdt, n)
    for t in (P, G, Tm, coef, dw, col_const):
        _chk(t, torch.float32)
    _chk(s, torch.float64, "s")
    if wa.numel() < views * p * Cn or w_dgrad.numel() != p * Cn or hn.numel() < views * p * p or \
            col_const.numel() < views * p or P.numel() < views * Cn * p or (G is None and Tm is None) or \
            (G is not None and G.numel() < views * p * p) or (Tm is not None and Tm.numel() < views * Cn * p) or \
            s.numel() < views * p or coef.numel() < views * 4 * Cn or dw.numel() != Cn * p or Cn % 128 or p % 32:
        raise ValueError("linbn_banks_post: size mismatch")
    flops = 2.0 * views * p * p * Cn * (1 if Tm is not None else 2)
    with _prof(_lin_tag("linbn_banks_post", Cn, p), flops,
               4.0 * Cn * p * (2 + views) + _sz(dtype) * p * Cn * (2 + views)):
        check(_lib.load().sm3_linbn_banks_post(dtype, _ptr(w_dgrad), _ptr(coef), _ptr(wa), _ptr(col_const), _ptr(hn), _ptr(P),
                                               _ptr(G), _ptr(Tm), _ptr(s), _ptr(dw), Cn, p, views, _stream()),
              "sm3_linbn_banks_post")


def conv_bn_act_fused(desc, x, w, scale, shift, residual, relu, y, mask=None, views=1):
    """y = relu?(conv(x, w) * scale[v] + shift[v] (+ residual)) with the ReLU bits in `mask`: conv -> train-mode BatchNorm ->
    (+identity) -> ReLU in one launch (sm3_conv_bn_act_fused); scale / shift [views][Co] from bn_finalize."""
    tdt = TORCH_DTYPE[desc.dtype]
    _chk(x, tdt, "x"); _chk(w, tdt, "w"); _chk(y, tdt, "y"); _chk(residual, tdt, "residual")
    _chk(scale, torch.float32, "scale"); _chk(shift, torch.float32, "shift"); _chk(mask, torch.uint8, "mask")
    if x.numel() != desc.N * desc.Hi * desc.Wi * desc.Ci:
        raise ValueError("x size does not match descriptor")
    n_out = desc.N * desc.Hout * desc.Wout * desc.Co
    if y.numel() != n_out or (residual is not None and residual.numel() != n_out):
        raise ValueError("y / residual size does not match descriptor")
    if scale.numel() < views * desc.Co or shift.numel() < views * desc.Co:
        raise ValueError("scale/shift too small")
    if mask is not None and (not relu or mask.numel() != n_out // (16 // _sz(desc.dtype))):
        raise ValueError("mask size mismatch")
    M = desc.N * desc.Ho * desc.Wo
    if views > 1 and (views != 2 or M % 256):
        raise ValueError("two views need a multiple of 128 rows each")
    if desc.Ci % K_CHUNK[desc.dtype]:
        raise ValueError(f"Ci={desc.Ci} is not a multiple of {K_CHUNK[desc.dtype]}")
    sz = _sz(desc.dtype)
    tag = _conv_tag(desc)
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|M{M}_K{desc.ntaps}x{desc.Ci}_N{desc.Co}_s{desc.osy}_bnact"
    with _prof(tag, 2.0 * M * desc.Co * desc.ntaps * desc.Ci,
               sz * (min(x.numel(), M * desc.ntaps * desc.Ci) + M * desc.Co * (2 if residual is not None else 1))):
        check(_lib.load().sm3_conv_bn_act_fused(C.byref(desc), _ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(residual),
                                                int(relu), _ptr(y), _ptr(mask), views, _stream()), "sm3_conv_bn_act_fused")


# ------------------------------------------------------------------------------------------
# batch norm
# ------------------------------------------------------------------------------------------
BN_REDUCE_GROUPS = 64
_bn_ws = {}


def _bn_workspace(device, Cn, views=1):
    """fp64 scratch of the two-stage statistics reduction (stream-ordered reuse: one per device AND stream)."""
    device = (device, _stream_handle() if device.type == "cuda" else 0)
    t = _bn_ws.get(device)
    need = views * BN_REDUCE_GROUPS * 2 * Cn
    if t is None or t.numel() < need:
        t = torch.empty(max(need, 2 * BN_REDUCE_GROUPS * 2 * 2048), dtype=torch.float64, device=device[0])
        _bn_ws[device] = t
    return t


def bn_reduce_groups(rows):
    return min(BN_REDUCE_GROUPS, (rows + 31) // 32)


def bn_stats_reduce(partials, rows, Cn, sums, views=1):
    """sums: fp64 [views][2C] output, or None to run stage A only -- then returns (workspace, groups) for bn_finalize.
    rows: partial rows of ONE view; partials holds `views` such blocks back to back."""
    _chk(partials, torch.float32, "partials"); _chk(sums, torch.float64, "sums")
    if partials.numel() < views * rows * 2 * Cn or (sums is not None and sums.numel() < views * 2 * Cn):
        raise ValueError("bn_stats_reduce: buffer too small")
    ws = _bn_workspace(partials.device, Cn, views)
    with _prof("bn_stats_reduce", 0.0, 4.0 * views * rows * 2 * Cn):
        check(_lib.load().sm3_bn_stats_reduce(_ptr(partials), rows, Cn, _ptr(sums), _ptr(ws), views, _stream()),
              "sm3_bn_stats_reduce")
    return ws, bn_reduce_groups(rows)


def bn_finalize(sums, count, Cn, gamma, beta, eps, momentum, running_mean, running_var, nbt, scale, shift,
                save_mean, save_invstd, groups=1, views=1):
    """count: elements per channel of ONE view; scale / shift / save_mean / save_invstd: [views][C]."""
    for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _chk(t, torch.float32, n)
        if t is not None and t.numel() < Cn:
            raise ValueError(f"{n} too small")
    for t, n in ((scale, "scale"), (shift, "shift"), (save_mean, "save_mean"), (save_invstd, "save_invstd")):
        _chk(t, torch.float32, n)
        if t is not None and t.numel() < views * Cn:
            raise ValueError(f"{n} too small")
    _chk(sums, torch.float64, "sums"); _chk(nbt, torch.int64, "num_batches_tracked")
    if sums.numel() < views * groups * 2 * Cn:
        raise ValueError("bn_finalize: sums too small for groups")
    with _prof("bn_finalize", 0.0, 40.0 * Cn):
        check(_lib.load().sm3_bn_finalize(_ptr(sums), groups, views, float(count), Cn, _ptr(gamma), _ptr(beta), eps,
                                          momentum, _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(scale),
                                          _ptr(shift), _ptr(save_mean), _ptr(save_invstd), _stream()), "sm3_bn_finalize")


def bn_eval_scale_shift(gamma, beta, running_mean, running_var, eps, Cn, scale, shift):
    for t in (gamma, beta, running_mean, running_var, scale, shift):
        _chk(t, torch.float32)
    check(_lib.load().sm3_bn_eval_scale_shift(_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), eps,
                                              Cn, _ptr(scale), _ptr(shift), _stream()), "sm3_bn_eval_scale_shift")


def subsample_colsum_rows(dtype, rows, Cn):
    return _lib.load().sm3_subsample_colsum_rows(rows, Cn, dtype)


def subsample_colsum(dtype, x, y, colsum, N, H, W, Cn, stride, views=1):
    """Column-sum partial rows of x [N, H, W, C] at the stride-th pixels (and, y given, those pixels as a compact tensor):
    sm3_subsample_colsum."""
    tdt = TORCH_DTYPE[dtype]
    _chk(x, tdt, "x"); _chk(y, tdt, "y"); _chk(colsum, torch.float32, "colsum")
    Hs, Ws = (H - 1) // stride + 1, (W - 1) // stride + 1
    if x.numel() != N * H * W * Cn or (y is not None and y.numel() != N * Hs * Ws * Cn) or N % views:
        raise ValueError("subsample_colsum: size mismatch")
    if colsum.numel() < views * subsample_colsum_rows(dtype, N // views * Hs * Ws, Cn) * Cn:
        raise ValueError("subsample_colsum: colsum too small")
    with _prof("subsample", 0.0, _sz(dtype) * N * Hs * Ws * Cn * (2 if y is not None else 1)):
        check(_lib.load().sm3_subsample_colsum(dtype, _ptr(x), _ptr(y), _ptr(colsum), N, H, W, Cn, stride, views, _stream()),
              "sm3_subsample_colsum")


def bn_act_colsum_rows(dtype, rows, Cn):
    return _lib.load().sm3_bn_act_colsum_rows(rows, Cn, dtype)


def bn_act(dtype, x, scale, shift, residual, relu, y, rows, Cn, out_f32=False, mask=None, views=1, colsum=None):
    """rows: rows of ONE view; tensors hold `views` row ranges back to back, scale/shift are [views][C].
    colsum: optional fp32 [views][bn_act_colsum_rows][C] -- per-block column sums of the stored outputs."""
    tdt = TORCH_DTYPE[dtype]
    _chk(x, tdt, "x"); _chk(residual, tdt, "residual"); _chk(scale, torch.float32); _chk(shift, torch.float32)
    _chk(y, torch.float32 if out_f32 else tdt, "y")
    n = views * rows * Cn
    if x.numel() != n or y.numel() != n or (residual is not None and residual.numel() != n):
        raise ValueError("bn_act: size mismatch")
    if scale.numel() < views * Cn or shift.numel() < views * Cn:
        raise ValueError("bn_act: scale/shift too small")
    _chk(mask, torch.uint8, "mask")
    if mask is not None and mask.numel() != n // (16 // _sz(dtype)):
        raise ValueError("bn_act: mask size mismatch")
    tag = "bn_act"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|rows{views * rows}_C{Cn}_res{int(residual is not None)}"
    _chk(colsum, torch.float32, "colsum")
    if colsum is not None and (out_f32 or colsum.numel() < views * bn_act_colsum_rows(dtype, rows, Cn) * Cn):
        raise ValueError("bn_act: colsum needs the storage dtype and [views][colsum_rows][C] floats")
    with _prof(tag, 0.0, _sz(dtype) * n * (2 if residual is None else 3)):
        if colsum is not None:
            check(_lib.load().sm3_bn_act_colsum(dtype, _ptr(x), _ptr(scale), _ptr(shift), _ptr(residual), int(relu),
                                                _ptr(y), _ptr(mask), _ptr(colsum), rows, Cn, views, _stream()),
                  "sm3_bn_act_colsum")
        else:
            check(_lib.load().sm3_bn_act(dtype, _ptr(x), _ptr(scale), _ptr(shift), _ptr(residual), int(relu),
                                         int(out_f32), _ptr(y), _ptr(mask), rows, Cn, views, _stream()), "sm3_bn_act")


def bn_add_bn_act(dtype, x, scale, shift, x2, scale2, shift2, relu, y, rows, Cn, mask=None, views=1):
    """y = relu?(x*scale + shift + x2*scale2 + shift2): the join of a Bottleneck whose identity is a downsample
    conv + BatchNorm, with BOTH normalisations applied in this one pass (sm3_bn_add_bn_act)."""
    tdt = TORCH_DTYPE[dtype]
    for t in (x, x2, y):
        _chk(t, tdt)
    for t in (scale, shift, scale2, shift2):
        _chk(t, torch.float32)
        if t.numel() < views * Cn:
            raise ValueError("bn_add_bn_act: scale/shift too small")
    n = views * rows * Cn
    if x.numel() != n or x2.numel() != n or y.numel() != n:
        raise ValueError("bn_add_bn_act: size mismatch")
    _chk(mask, torch.uint8, "mask")
    if mask is not None and mask.numel() != n // (16 // _sz(dtype)):
        raise ValueError("bn_add_bn_act: mask size mismatch")
    tag = "bn_act"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|rows{views * rows}_C{Cn}_res2"
    with _prof(tag, 0.0, _sz(dtype) * n * 3):
        check(_lib.load().sm3_bn_add_bn_act(dtype, _ptr(x), _ptr(scale), _ptr(shift), _ptr(x2), _ptr(scale2),
                                            _ptr(shift2), int(relu), _ptr(y), _ptr(mask), rows, Cn, views, _stream()),
              "sm3_bn_add_bn_act")


def bn_bwd_apply2(dtype, dz, count, side_a, side_b, rows, Cn, views=1):
    """One pass for two BatchNorms that received the same dz.  side = dict(x, mean, invstd, gamma, gsums, lsums, dgamma,
    dbeta, dx)."""
    tdt = TORCH_DTYPE[dtype]
    _chk(dz, tdt, "dz")
    n = views * rows * Cn
    if dz.numel() != n:
        raise ValueError("bn_bwd_apply2: dz size mismatch")
    sides = []
    for sd in (side_a, side_b):
        for k in ("x", "dx"):
            _chk(sd[k], tdt, k)
            if sd[k].numel() != n:
                raise ValueError(f"bn_bwd_apply2: {k} size mismatch")
        for k in ("mean", "invstd", "gamma", "dgamma", "dbeta"):
            _chk(sd.get(k), torch.float32, k)
        for k in ("gsums", "lsums"):
            _chk(sd.get(k), torch.float64, k)
            if sd.get(k) is not None and sd[k].numel() < views * 2 * Cn:
                raise ValueError("bn_bwd_apply2: sums too small")
        if sd["mean"].numel() < views * Cn or sd["invstd"].numel() < views * Cn:
            raise ValueError("bn_bwd_apply2: mean/invstd too small")
        a = _lib.BnApplySide()
        a.x, a.mean, a.invstd, a.dx = sd["x"].data_ptr(), sd["mean"].data_ptr(), sd["invstd"].data_ptr(), sd["dx"].data_ptr()
        a.global_sums = sd["gsums"].data_ptr()
        for k, f in (("gamma", "gamma"), ("lsums", "local_sums"), ("dgamma", "dgamma"), ("dbeta", "dbeta")):
            setattr(a, f, sd[k].data_ptr() if sd.get(k) is not None else None)
        sides.append(a)
    tag = "bn_bwd_apply"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|rows{views * rows}_C{Cn}_dual"
    with _prof(tag, 0.0, _sz(dtype) * n * 5):
        check(_lib.load().sm3_bn_bwd_apply2(dtype, _ptr(dz), float(count), C.byref(sides[0]), C.byref(sides[1]), rows, Cn,
                                            views, _stream()), "sm3_bn_bwd_apply2")


def bn_relu_maxpool_fwd(dtype, x, scale, shift, y, N, H, W, Cn, argmax=None, views=1):
    """Stem: y = maxpool3x3s2(relu(x*scale + shift)) in one pass (sm3_bn_relu_maxpool_fwd)."""
    tdt = TORCH_DTYPE[dtype]
    _chk(x, tdt, "x"); _chk(y, tdt, "y"); _chk(scale, torch.float32); _chk(shift, torch.float32); _chk(argmax, torch.uint8)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if x.numel() != N * H * W * Cn or y.numel() != N * Ho * Wo * Cn or N % views:
        raise ValueError("bn_relu_maxpool_fwd: size mismatch")
    if scale.numel() < views * Cn or shift.numel() < views * Cn:
        raise ValueError("bn_relu_maxpool_fwd: scale/shift too small")
    if argmax is not None and argmax.numel() != y.numel():
        raise ValueError("bn_relu_maxpool_fwd: argmax size mismatch")
    with _prof("bn_relu_maxpool", 0.0, _sz(dtype) * (x.numel() + y.numel()) + (y.numel() if argmax is not None else 0)):
        check(_lib.load().sm3_bn_relu_maxpool_fwd(dtype, _ptr(x), _ptr(scale), _ptr(shift), _ptr(y), _ptr(argmax), N, H, W,
                                                  Cn, views, _stream()), "sm3_bn_relu_maxpool_fwd")


def maxpool_bn_bwd_partial_rows(N, H, W, views=1):
    return _lib.load().sm3_maxpool_bn_bwd_partial_rows(N, H, W, views)


def maxpool_bn_bwd(dtype, argmax, dy, x, scale, shift, mean, invstd, dz, partials, N, H, W, Cn, views=1):
    """Stem backward: maxpool gradient gather + recomputed ReLU mask + BatchNorm-backward phase 1 (sm3_maxpool_bn_bwd)."""
    tdt = TORCH_DTYPE[dtype]
    _chk(argmax, torch.uint8); _chk(dy, tdt, "dy"); _chk(x, tdt, "x"); _chk(dz, tdt, "dz"); _chk(partials, torch.float32)
    for t in (scale, shift, mean, invstd):
        _chk(t, torch.float32)
        if t.numel() < views * Cn:
            raise ValueError("maxpool_bn_bwd: per-channel vector too small")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if x.numel() != N * H * W * Cn or dz.numel() != x.numel() or dy.numel() != N * Ho * Wo * Cn or \
            argmax.numel() != dy.numel() or N % views:
        raise ValueError("maxpool_bn_bwd: size mismatch")
    if partials.numel() < views * maxpool_bn_bwd_partial_rows(N, H, W, views) * 2 * Cn:
        raise ValueError("maxpool_bn_bwd: partials too small")
    with _prof("maxpool_bn_bwd", 0.0, _sz(dtype) * (2 * x.numel() + dy.numel()) + argmax.numel()):
        check(_lib.load().sm3_maxpool_bn_bwd(dtype, _ptr(argmax), _ptr(dy), _ptr(x), _ptr(scale), _ptr(shift), _ptr(mean),
                                             _ptr(invstd), _ptr(dz), _ptr(partials), N, H, W, Cn, views, _stream()),
              "sm3_maxpool_bn_bwd")


def bn_bwd_partial_rows(rows, Cn):
    return _lib.load().sm3_bn_bwd_partial_rows(rows, Cn)


def bn_bwd_reduce(dtype, dy, y, x, mean, invstd, dz, rows, Cn, partials, mask=None, views=1):
    """rows: rows of ONE view; partials: [views][bn_bwd_partial_rows(rows)][2][C]; mean/invstd: [views][C]."""
    tdt = TORCH_DTYPE[dtype]
    n = views * rows * Cn
    for t, nm in ((dy, "dy"), (y, "y"), (x, "x"), (dz, "dz")):
        _chk(t, tdt, nm)
        if t is not None and t.numel() != n:
            raise ValueError(f"bn_bwd_reduce: {nm} size mismatch")
    _chk(partials, torch.float32)
    if partials.numel() < views * bn_bwd_partial_rows(rows, Cn) * 2 * Cn:
        raise ValueError("bn_bwd_reduce: partials too small")
    _chk(mask, torch.uint8, "mask")
    if mask is not None and mask.numel() != n // (16 // _sz(dtype)):
        raise ValueError("bn_bwd_reduce: mask size mismatch")
    if x is not None and (mean.numel() < views * Cn or invstd.numel() < views * Cn):
        raise ValueError("bn_bwd_reduce: mean/invstd too small")
    reads = 1 + (x is not None) + (1 if (y is not None and mask is None) else 0) + (1 if dz is not None else 0)
    with _prof("bn_bwd_reduce", 0.0, _sz(dtype) * n * reads + (n // 8 if mask is not None else 0)):
        check(_lib.load().sm3_bn_bwd_reduce(dtype, _ptr(dy), _ptr(y), _ptr(mask), _ptr(x), _ptr(mean), _ptr(invstd),
                                            _ptr(dz), rows, Cn, _ptr(partials), views, _stream()), "sm3_bn_bwd_reduce")


def bn_bwd_apply(dtype, dz, x, mean, invstd, gamma, gsums, count, lsums, dgamma, dbeta, dx, rows, Cn, views=1):
    """rows / count: of ONE view; gsums / lsums: [views][2C]; mean / invstd: [views][C]."""
    tdt = TORCH_DTYPE[dtype]
    for t, n in ((dz, "dz"), (x, "x"), (dx, "dx")):
        _chk(t, tdt, n)
        if t.numel() != views * rows * Cn:
            raise ValueError(f"bn_bwd_apply: {n} size mismatch")
    _chk(gsums, torch.float64); _chk(lsums, torch.float64)
    _chk(dgamma, torch.float32); _chk(dbeta, torch.float32); _chk(gamma, torch.float32)
    if gsums.numel() < views * 2 * Cn or (lsums is not None and lsums.numel() < views * 2 * Cn):
        raise ValueError("bn_bwd_apply: sums too small")
    tag = "bn_bwd_apply"
    if _PROFILER is not None and getattr(_PROFILER, "detail", False):
        tag += f"|rows{views * rows}_C{Cn}"
    with _prof(tag, 0.0, _sz(dtype) * views * rows * Cn * 3):
        check(_lib.load().sm3_bn_bwd_apply(dtype, _ptr(dz), _ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma),
                                           _ptr(gsums), float(count), _ptr(lsums), _ptr(dgamma), _ptr(dbeta), _ptr(dx),
                                           rows, Cn, views, _stream()), "sm3_bn_bwd_apply")


# ------------------------------------------------------------------------------------------
# stem / pooling / weights
# ------------------------------------------------------------------------------------------
STEM_KDIRECT = 176  # K of the direct stem's filter bank: (kh, c) groups x 8 (kw padded), 22nd group zero


def stem_partial_rows(N, H, W):
    return _lib.load().sm3_stem_partial_rows(N, H, W)


def stem_weight_prep(dtype, w_master, w_stem, only_if=None):
    _chk(w_master, torch.float32, "w_master"); _chk(w_stem, TORCH_DTYPE[dtype], "w_stem"); _chk(only_if, torch.int32, "only_if")
    if w_master.numel() != 64 * 147 or w_stem.numel() != 64 * STEM_KDIRECT:
        raise ValueError("stem_weight_prep: size mismatch")
    check(_lib.load().sm3_stem_weight_prep_if(dtype, _ptr(w_master), _ptr(w_stem), _ptr(only_if), _stream()),
          "sm3_stem_weight_prep_if")


def stem_conv_fwd(dtype, x_nchw, w_stem, y, partials=None):
    """Direct 7x7/2 stem convolution from the NCHW fp32 batch (sm3_stem_conv_fwd; bf16 / fp16 / exact f32)."""
    _chk(x_nchw, torch.float32, "x"); _chk(w_stem, TORCH_DTYPE[dtype], "w_stem"); _chk(y, TORCH_DTYPE[dtype], "y")
    _chk(partials, torch.float32, "partials")
    N, Cc, H, W = x_nchw.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if Cc != 3 or w_stem.numel() != 64 * STEM_KDIRECT or y.numel() != N * Ho * Wo * 64:
        raise ValueError("stem_conv_fwd: size mismatch")
    if partials is not None and partials.numel() < stem_partial_rows(N, H, W) * 2 * 64:
        raise ValueError("stem_conv_fwd: partials too small")
    M = N * Ho * Wo
    with _prof("stem_conv_fwd", 2.0 * M * 64 * 147, 4.0 * x_nchw.numel() + _sz(dtype) * y.numel()):
        check(_lib.load().sm3_stem_conv_fwd(dtype, _ptr(x_nchw), _ptr(w_stem), _ptr(y), _ptr(partials), N, H, W, _stream()),
              "sm3_stem_conv_fwd")


STEM_WGRAD_SLABS = 768  # SM3_STEM_WGRAD_SLABS (include/sm3_hip.h)


class StemImage:
    """The images of one encoder pass rounded to the 16-bit type once (sm3_stem_image_prep): t is [N, 3, H, Wp] `dtype` with
    the 7x7 convolution's left / right zero padding materialised; shape is the NCHW shape of the fp32 images it came from."""
    __slots__ = ("t", "shape")

    def __init__(self, t, shape):
        self.t, self.shape = t, tuple(shape)

    def record_stream(self, st):
        self.t.record_stream(st)


def stem_image_cols(W):
    return (W + 6 + 7) // 8 * 8


def stem_image_prep(dtype, views):
    """views: one or two NCHW fp32 tensors of equal shape -> StemImage of the batch `views[0]` then `views[1]` (no torch.cat)."""
    x0 = views[0]
    x1 = views[1] if len(views) > 1 else None
    _chk(x0, torch.float32, "x0"); _chk(x1, torch.float32, "x1")
    if x0.dim() != 4 or x0.shape[1] != 3 or (x1 is not None and x1.shape != x0.shape) or len(views) > 2:
        raise ValueError("stem_image_prep: NCHW fp32 views of equal shape")
    B, _, H, W = x0.shape
    V = len(views)
    out = torch.empty(V * B, 3, H, stem_image_cols(W), dtype=TORCH_DTYPE[dtype], device=x0.device)
    with _prof("stem_image_prep", 0.0, 4.0 * V * x0.numel() + _sz(dtype) * out.numel()):
        check(_lib.load().sm3_stem_image_prep(dtype, _ptr(x0), _ptr(x1), _ptr(out), B, V, H, W, _stream()),
              "sm3_stem_image_prep")
    return StemImage(out, (V * B, 3, H, W))


def stem_conv_fwd16(dtype, img, w_stem, y, partials=None):
    """sm3_stem_conv_fwd16: the direct stem on a StemImage (LDS-DMA staged 16-bit rows, no conversion in the kernel)."""
    tdt = TORCH_DTYPE[dtype]
    _chk(img.t, tdt, "ximg"); _chk(w_stem, tdt, "w_stem"); _chk(y, tdt, "y"); _chk(partials, torch.float32, "partials")
    N, Cc, H, W = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if Cc != 3 or w_stem.numel() != 64 * STEM_KDIRECT or y.numel() != N * Ho * Wo * 64 or \
            img.t.numel() != N * 3 * H * stem_image_cols(W):
        raise ValueError("stem_conv_fwd16: size mismatch")
    if partials is not None and partials.numel() < stem_partial_rows(N, H, W) * 2 * 64:
        raise ValueError("stem_conv_fwd16: partials too small")
    M = N * Ho * Wo
    with _prof("stem_conv_fwd", 2.0 * M * 64 * 147, _sz(dtype) * (img.t.numel() + y.numel())):
        check(_lib.load().sm3_stem_conv_fwd16(dtype, _ptr(img.t), _ptr(w_stem), _ptr(y), _ptr(partials), N, H, W, _stream()),
              "sm3_stem_conv_fwd16")


def stem_wgrad_bn16(dtype, img, dz, xo, mean, invstd, gamma, gsums, count, lsums, dgamma, dbeta, dw, views=1, slabs=None):
    """sm3_stem_wgrad_bn16: stem_wgrad_bn on a StemImage."""
    tdt = TORCH_DTYPE[dtype]
    _chk(img.t, tdt, "ximg"); _chk(dz, tdt, "dz"); _chk(xo, tdt, "xo"); _chk(dw, torch.float32, "dw")
    for t in (mean, invstd, gamma, dgamma, dbeta):
        _chk(t, torch.float32)
    _chk(gsums, torch.float64); _chk(lsums, torch.float64); _chk(slabs, torch.float32, "slabs")
    N, Cc, H, W = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if Cc != 3 or dz.numel() != N * Ho * Wo * 64 or xo.numel() != dz.numel() or dw.numel() < 64 * 147 or N % views or \
            img.t.numel() != N * 3 * H * stem_image_cols(W):
        raise ValueError("stem_wgrad_bn16: size mismatch")
    if mean.numel() < views * 64 or invstd.numel() < views * 64 or gsums.numel() < views * 128 or \
            (lsums is not None and lsums.numel() < views * 128):
        raise ValueError("stem_wgrad_bn16: per-channel vector too small")
    if slabs is not None and slabs.numel() < STEM_WGRAD_SLABS * 64 * 147:
        raise ValueError("stem_wgrad_bn16: slab workspace too small")
    M = N * Ho * Wo
    with _prof("stem_wgrad_bn", 2.0 * M * 64 * 147, _sz(dtype) * (img.t.numel() + 2 * dz.numel())):
        check(_lib.load().sm3_stem_wgrad_bn16(dtype, _ptr(img.t), _ptr(dz), _ptr(xo), _ptr(mean), _ptr(invstd), _ptr(gamma),
                                              _ptr(gsums), float(count), _ptr(lsums), _ptr(dgamma), _ptr(dbeta), _ptr(dw),
                                              _ptr(slabs), N, H, W, views, _stream()), "sm3_stem_wgrad_bn16")


def stem_dgrad_bn(dtype, dz, xo, mean, invstd, gamma, gsums, count, w_master, dx, views=1):
    """Image gradient of the stem (sm3_stem_dgrad_bn): dx [N, 3, H, W] fp32 (written, not accumulated) from the stem
    BatchNorm's output gradient dz and its saved input xo ([N*Ho*Wo, 64] `dtype`), the BatchNorm-backward apply computed on
    the fly as in stem_wgrad_bn (gsums all zero: frozen statistics); w_master: the fp32 [64, 3, 7, 7]-sized master weight in
    [64][kh][kw][c] order."""
    tdt = TORCH_DTYPE[dtype]
    _chk(dz, tdt, "dz"); _chk(xo, tdt, "xo"); _chk(dx, torch.float32, "dx"); _chk(w_master, torch.float32, "w")
    for t in (mean, invstd, gamma):
        _chk(t, torch.float32)
    _chk(gsums, torch.float64)
    if dx.dim() != 4 or dx.shape[1] != 3:
        raise ValueError("stem_dgrad_bn: dx must be [N, 3, H, W]")
    N, _, H, W = dx.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if dz.numel() != N * Ho * Wo * 64 or xo.numel() != dz.numel() or w_master.numel() != 64 * 147 or views < 1 or N % views:
        raise ValueError("stem_dgrad_bn: size mismatch")
    if mean.numel() < views * 64 or invstd.numel() < views * 64 or gsums.numel() < views * 128 or \
            (gamma is not None and gamma.numel() < 64):
        raise ValueError("stem_dgrad_bn: per-channel vector too small")
    M = N * Ho * Wo
    with _prof("stem_dgrad_bn", 2.0 * M * 64 * 147, 2.0 * _sz(dtype) * dz.numel() + 4.0 * dx.numel()):
        check(_lib.load().sm3_stem_dgrad_bn(dtype, _ptr(dz), _ptr(xo), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(gsums),
                                            float(count), _ptr(w_master), _ptr(dx), N, H, W, views, _stream()),
              "sm3_stem_dgrad_bn")


def cam_alpha(dtype, g, alpha, N, HW, C):
    """Grad-CAM channel weights (sm3_cam_alpha): alpha [T, N, C] fp32 = the mean over the HW positions of g [T, N, HW, C]
    (`dtype`), positions added in ascending order."""
    _chk(g, TORCH_DTYPE[dtype], "g"); _chk(alpha, torch.float32, "alpha")
    T = alpha.numel() // (N * C) if N * C > 0 else 0
    if T < 1 or alpha.numel() != T * N * C or g.numel() != T * N * HW * C:
        raise ValueError("cam_alpha: g [T, N, HW, C] and alpha [T, N, C] do not match")
    with _prof("cam_alpha", float(g.numel()), _sz(dtype) * g.numel() + 4.0 * alpha.numel()):
        check(_lib.load().sm3_cam_alpha(dtype, _ptr(g), _ptr(alpha), T, N, HW, C, _stream()), "sm3_cam_alpha")


def cam_maps(dtype, a, alpha, low, maps, N, h, w, C):
    """Grad-CAM maps (sm3_cam_maps) of the stage output a [N, h*w, C] (`dtype`, NHWC) weighted by alpha [T, N, C] fp32: low
    [N, T, h, w] = ReLU(sum_c alpha * a) and maps [N, T, H, W] = low upsampled (bilinear, align_corners=False) and
    normalised to [0, 1] per map, both fp32."""
    _chk(a, TORCH_DTYPE[dtype], "a")
    for t, n in ((alpha, "alpha"), (low, "low"), (maps, "maps")):
        _chk(t, torch.float32, n)
    T = alpha.numel() // (N * C) if N * C > 0 else 0
    if maps.dim() != 4 or tuple(maps.shape[:2]) != (N, T) or tuple(low.shape) != (N, T, h, w):
        raise ValueError("cam_maps: low must be [N, T, h, w] and maps [N, T, H, W]")
    if T < 1 or alpha.numel() != T * N * C or a.numel() != N * h * w * C:
        raise ValueError("cam_maps: a [N, h*w, C] and alpha [T, N, C] do not match")
    H, W = maps.shape[2], maps.shape[3]
    with _prof("cam_maps", 2.0 * N * h * w * C * T, _sz(dtype) * a.numel() + 4.0 * (low.numel() + maps.numel())):
        check(_lib.load().sm3_cam_maps(dtype, _ptr(a), _ptr(alpha), _ptr(low), _ptr(maps), N, T, h, w, C, H, W, _stream()),
              "sm3_cam_maps")


def _attr_rows(x, name):
    """(N, E) of one modality's images [N, 3, H, W] (or [N, E]) fp32."""
    _chk(x, torch.float32, name)
    if x.dim() < 2 or x.shape[0] < 1:
        raise ValueError(f"{name} must be [N, ...]")
    return x.shape[0], x.numel() // x.shape[0]


def attr_path(x, base, out, k0, steps):
    """Integrated-Gradients path points (sm3_attr_path): out [c, N, ...] fp32 = base + alpha_k (x - base), k = k0 .. k0 + c - 1,
    alpha_k = (2k + 1) / (2 steps); base: [1, ...] (shared by the batch) or [N, ...]."""
    N, E = _attr_rows(x, "x")
    _chk(base, torch.float32, "base"); _chk(out, torch.float32, "out")
    c = out.shape[0] if out.dim() > 1 else 0
    if c < 1 or out.numel() != c * N * E or base.numel() not in (E, N * E):
        raise ValueError("attr_path: x [N, E], base [1 | N, E] and out [c, N, E] do not match")
    with _prof("attr_path", 3.0 * out.numel(), 4.0 * (x.numel() + base.numel() + out.numel())):
        check(_lib.load().sm3_attr_path(_ptr(x), _ptr(base), base.numel() // E, _ptr(out), N, E, k0, c, steps, _stream()),
              "sm3_attr_path")


def attr_noise(x, sigma, out, k0, seed, stride=1):
    """SmoothGrad samples (sm3_attr_noise): out [c, N, ...] fp32 = x + sigma[n] * z(seed, k0 + j * stride, n, e), z standard
    normal (Philox4x32-10 + Box-Muller), a function of (seed, sample, n, e) alone."""
    N, E = _attr_rows(x, "x")
    _chk(sigma, torch.float32, "sigma"); _chk(out, torch.float32, "out")
    c = out.shape[0] if out.dim() > 1 else 0
    if c < 1 or out.numel() != c * N * E or sigma.numel() != N:
        raise ValueError("attr_noise: x [N, E], sigma [N] and out [c, N, E] do not match")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("attr_noise: seed must fit 64 bits")
    with _prof("attr_noise", 2.0 * out.numel(), 4.0 * (x.numel() + out.numel())):
        check(_lib.load().sm3_attr_noise(_ptr(x), _ptr(sigma), _ptr(out), N, E, k0, c, stride, seed, _stream()),
              "sm3_attr_noise")


def attr_accumulate(g, acc, weight, squared=False):
    """acc [N, ...] fp32 = (((acc + w * f(g[0])) + w * f(g[1])) + ...) over g [c, N, ...] fp32 (or [c * N, ...]) in ascending
    order (sm3_attr_accumulate), f the identity or the square."""
    N, E = _attr_rows(acc, "acc")
    _chk(g, torch.float32, "g")
    c = g.numel() // (N * E)
    if c < 1 or g.numel() != c * N * E:
        raise ValueError("attr_accumulate: g [c, N, E] and acc [N, E] do not match")
    with _prof("attr_accumulate", 2.0 * g.numel(), 4.0 * (g.numel() + 2 * acc.numel())):
        check(_lib.load().sm3_attr_accumulate(_ptr(g), _ptr(acc), c, N, E, float(weight), int(bool(squared)), _stream()),
              "sm3_attr_accumulate")


def attr_finish(acc, x, base, attr, maps, sums, mode):
    """The attributions of one modality (sm3_attr_finish).  acc, attr [T, N, C, H, W] fp32; mode 0 (IG): attr = (x - base) *
    acc, x [N, C, H, W], base [1 | N, C, H, W]; mode 1 (SmoothGrad): attr = acc.  maps [T, N, H, W] = sum_c |attr|; sums
    [T, N] fp64 = the sum of attr per (t, n) by a fixed tree."""
    if acc.dim() != 5 or attr.shape != acc.shape:
        raise ValueError("attr_finish: acc and attr must be [T, N, C, H, W]")
    T, N, Cc, H, W = acc.shape
    for t, n in ((acc, "acc"), (attr, "attr"), (maps, "maps")):
        _chk(t, torch.float32, n)
    _chk(sums, torch.float64, "sums")
    if tuple(maps.shape) != (T, N, H, W) or tuple(sums.shape) != (T, N) or mode not in (0, 1):
        raise ValueError("attr_finish: maps must be [T, N, H, W], sums [T, N], mode 0 or 1")
    base_n = 1
    if mode == 0:
        _chk(x, torch.float32, "x"); _chk(base, torch.float32, "base")
        E = Cc * H * W
        if x.numel() != N * E or base.numel() not in (E, N * E):
            raise ValueError("attr_finish: x [N, C, H, W] and base [1 | N, C, H, W] do not match acc")
        base_n = base.numel() // E
    else:
        x = base = None
    lib = _lib.load()
    blocks = lib.sm3_attr_finish_blocks(H * W)
    if blocks < 1:
        raise ValueError("attr_finish: empty images")
    partials = torch.empty(T * N * blocks, dtype=torch.float64, device=acc.device)
    with _prof("attr_finish", 4.0 * acc.numel(), 4.0 * (2 * acc.numel() + maps.numel())):
        check(lib.sm3_attr_finish(_ptr(acc), _ptr(x), _ptr(base), base_n, _ptr(attr), _ptr(maps), _ptr(sums), _ptr(partials),
                                  T, N, Cc, H * W, mode, _stream()), "sm3_attr_finish")


FAITH_RANK_WORKSPACE = 256 << 20  # bytes of sort workspace per sm3_faith_rank launch, at most (one map's pairs at the least)


def faith_rank(maps, ranks):
    """ranks [..., HW] int32 of maps [..., HW] fp32 (finite): per row, descending by value, ties by ascending index
    (sm3_faith_rank).  The rows are ranked in groups whose sort workspace stays within FAITH_RANK_WORKSPACE."""
    _chk(maps, torch.float32, "maps"); _chk(ranks, torch.int32, "ranks")
    if maps.dim() < 1 or maps.shape != ranks.shape or maps.numel() < 1:
        raise ValueError("faith_rank: maps [..., HW] fp32 and ranks [..., HW] int32 must have the same, non-empty shape")
    HW = maps.shape[-1]
    rows = maps.numel() // HW
    lib = _lib.load()
    one = lib.sm3_faith_rank_workspace(1, HW)
    if one < 1:
        raise ValueError(f"faith_rank: HW = {HW} is out of range")
    group = max(1, min(rows, FAITH_RANK_WORKSPACE // one))
    ws = torch.empty(group * one, dtype=torch.uint8, device=maps.device)
    m2, r2 = maps.view(rows, HW), ranks.view(rows, HW)
    with _prof("faith_rank", 0.0, 4.0 * 2 * maps.numel() + 8.0 * 8 * maps.numel()):
        for r0 in range(0, rows, group):
            g = min(group, rows - r0)
            check(lib.sm3_faith_rank(_ptr(m2[r0:]), _ptr(r2[r0:]), g, HW, _ptr(ws), ws.numel(), _stream()), "sm3_faith_rank")


def faith_compose(x, base, ranks, out, k0, steps, invert):
    """One modality's deletion (invert False) or insertion (True) inputs of curve steps k0 .. k0 + c - 1 (sm3_faith_compose):
    out [c, T, N, 3, H, W] fp32 = base where (ranks[n, t] < (k * HW) // steps) != invert, else x.  x [N, 3, H, W], base [1 | N,
    3, H, W]; ranks [N, T, H, W] int32, a view whose pixels are contiguous (one modality of the [N, T, 2, H, W] tensor)."""
    N, E = _attr_rows(x, "x")
    _chk(base, torch.float32, "base"); _chk(out, torch.float32, "out")
    if x.dim() != 4 or x.shape[1] != 3 or out.dim() != 6 or ranks.dim() != 4:
        raise ValueError("faith_compose: x [N, 3, H, W], ranks [N, T, H, W], out [c, T, N, 3, H, W]")
    H, W = x.shape[2:]
    c, T = out.shape[:2]
    if not ranks.is_cuda or ranks.dtype != torch.int32 or tuple(ranks.shape) != (N, T, H, W) or ranks.stride(3) != 1 or \
            ranks.stride(2) != W:
        raise ValueError("faith_compose: ranks must be int32 [N, T, H, W] on the GPU with contiguous pixels")
    if c < 1 or tuple(out.shape) != (c, T, N, 3, H, W) or base.numel() not in (E, N * E):
        raise ValueError("faith_compose: x [N, 3, H, W], base [1 | N, 3, H, W] and out [c, T, N, 3, H, W] do not match")
    with _prof("faith_compose", 0.0, 4.0 * (T * x.numel() + T * base.numel() + ranks.numel() + out.numel())):
        check(_lib.load().sm3_faith_compose(_ptr(x), _ptr(base), base.numel() // E, _ptr(ranks), ranks.stride(0), ranks.stride(1),
                                            _ptr(out), N, T, H * W, k0, c, steps, int(bool(invert)), _stream()),
              "sm3_faith_compose")


RISE_ROW_WORDS = 36  # a mask's table row: 32 words of grid bits, oy, ox, two words of padding


def _rise_table(table, name):
    """The number of rows of a mask table [c, 36] int32."""
    _chk(table, torch.int32, name)
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != RISE_ROW_WORDS:
        raise ValueError(f"{name} must be int32 [masks, {RISE_ROW_WORDS}]")
    return table.shape[0]


def rise_table(table, i0, modality, H, W, cells, p, seed):
    """The table rows of RISE masks i0 .. i0 + c - 1 of one modality (sm3_rise_table): table [c, 36] int32 -- the (cells + 2)^2
    grid bits, then the shift (oy, ox).  A function of (seed, modality, mask, H, W, cells, p) alone."""
    c = _rise_table(table, "table")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("rise_table: seed must fit 64 bits")
    check(_lib.load().sm3_rise_table(_ptr(table), int(i0), c, int(modality), int(H), int(W), int(cells), float(p), seed,
                                     _stream()), "sm3_rise_table")


def rise_compose(x, base, table, out, cells):
    """One modality's masked inputs (sm3_rise_compose): out [c, N, 3, H, W] fp32 = base + mask_j * (x - base) for the c masks of
    table [c, 36]; x [N, 3, H, W], base [1 | N, 3, H, W]."""
    N, E = _attr_rows(x, "x")
    _chk(base, torch.float32, "base"); _chk(out, torch.float32, "out")
    c = _rise_table(table, "table")
    if x.dim() != 4 or x.shape[1] != 3 or out.dim() != 5:
        raise ValueError("rise_compose: x [N, 3, H, W], out [c, N, 3, H, W]")
    H, W = x.shape[2:]
    if tuple(out.shape) != (c, N, 3, H, W) or base.numel() not in (E, N * E):
        raise ValueError("rise_compose: x [N, 3, H, W], base [1 | N, 3, H, W], table [c, 36] and out [c, N, 3, H, W] do not match")
    with _prof("rise_compose", 3.0 * out.numel(), 4.0 * (x.numel() + base.numel() + out.numel())):
        check(_lib.load().sm3_rise_compose(_ptr(x), _ptr(base), base.numel() // E, _ptr(table), _ptr(out), N, H, W, int(cells), c,
                                           _stream()), "sm3_rise_compose")


def rise_accumulate(table, weights, maps, cells, p):
    """maps [N, T, H, W] fp32 (a view whose pixels are contiguous: one modality of [N, T, 2, H, W]) = the sum over the M masks of
    table [M, 36], in ascending order, of weights[i, n * T + t] * mask_i, every product and sum rounded on its own, divided by
    (float)(M * p) (sm3_rise_accumulate).  weights [M, N * T] fp32."""
    M = _rise_table(table, "table")
    _chk(weights, torch.float32, "weights")
    if maps.dim() != 4 or not maps.is_cuda or maps.dtype != torch.float32:
        raise ValueError("rise_accumulate: maps must be fp32 [N, T, H, W] on the GPU (the SM3 HIP path has no CPU fallback)")
    N, T, H, W = maps.shape
    if maps.stride(3) != 1 or maps.stride(2) != W:
        raise ValueError("rise_accumulate: the pixels of maps must be contiguous")
    if tuple(weights.shape) != (M, N * T):
        raise ValueError(f"rise_accumulate: weights must be [{M}, {N * T}] for table [{M}, 36] and maps {tuple(maps.shape)}")
    with _prof("rise_accumulate", 2.0 * M * maps.numel(), 4.0 * (weights.numel() + maps.numel())):
        check(_lib.load().sm3_rise_accumulate(_ptr(table), _ptr(weights), _ptr(maps), maps.stride(0), maps.stride(1), N, T, M, H,
                                              W, int(cells), float(p), _stream()), "sm3_rise_accumulate")


REPORT_MAX_CASES = 8192  # sm3_report_max_cases(): the multiplicities and the prefix sums of a replicate live in LDS


def _replicates_chk(who, seed, point, c, one="table"):
    """What the five *_counts wrappers ask of the replicates (sm3hip/resample.py: the rule): a 64-bit seed, one point table."""
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must fit 64 bits")
    if point and c != 1:
        raise ValueError(f"{who}: the point estimate is one {one}")


def report_counts(order, gs, ge, targets, yhat, colmap, out, seed, r0, point=False):
    """out [c, K, 6] int64 = (A2, P, Q, TP, FP, FN) of the K columns for bootstrap replicates r0 .. r0 + c - 1, or for the point
    estimate (point: c = 1, every case once) (sm3_report_counts).  order, gs, ge [K, N] int32: per column the cases in ascending
    score order and the bounds of each position's tie group; targets, yhat [N, T] int32; colmap [K, 2] int32 = (label, class)."""
    for t, n in ((order, "order"), (gs, "gs"), (ge, "ge"), (targets, "targets"), (yhat, "yhat"), (colmap, "colmap")):
        _chk(t, torch.int32, n)
    _chk(out, torch.int64, "out")
    if order.dim() != 2 or targets.dim() != 2 or out.dim() != 3:
        raise ValueError("report_counts: order [K, N], targets [N, T] and out [c, K, 6]")
    K, N = order.shape
    T = targets.shape[1]
    c = out.shape[0]
    if N > REPORT_MAX_CASES:
        raise ValueError(f"report_counts: {N} cases, at most {REPORT_MAX_CASES} supported")
    if tuple(gs.shape) != (K, N) or tuple(ge.shape) != (K, N) or tuple(targets.shape) != (N, T) or \
            tuple(yhat.shape) != (N, T) or tuple(colmap.shape) != (K, 2) or tuple(out.shape) != (c, K, 6):
        raise ValueError("report_counts: order, gs, ge [K, N], targets, yhat [N, T], colmap [K, 2] and out [c, K, 6] do not match")
    _replicates_chk("report_counts", seed, point, c)
    with _prof("report_counts", 0.0, 4.0 * 3 * K * N * c):
        check(_lib.load().sm3_report_counts(_ptr(order), _ptr(gs), _ptr(ge), _ptr(targets), _ptr(yhat), _ptr(colmap), _ptr(out),
                                            N, T, K, seed, int(r0), c, int(bool(point)), _stream()), "sm3_report_counts")


RETRIEVAL_MAX_LEVELS = 8  # Recall@k levels of one sm3_retrieval_counts record


def retrieval_beats(S, q0, N, temperature, bits, rank, term):
    """For the query rows q0 .. q0 + n - 1, whose similarities to the N gallery rows are S [n, ld >= N] float32 (the positive of row
    r is column q0 + r): bits [n, ceil(N / 32)] int32 = the packed "gallery row j comes back before the positive" flags (equal
    similarities: the lower index first), rank [n] int32 = their number, term [n] float64 = log sum_j exp(S_rj / T) - S_rr / T
    (sm3_retrieval_beats)."""
    _chk(S, torch.float32, "S"); _chk(bits, torch.int32, "bits"); _chk(rank, torch.int32, "rank"); _chk(term, torch.float64, "term")
    if S.dim() != 2 or bits.dim() != 2 or rank.dim() != 1 or term.dim() != 1:
        raise ValueError("retrieval_beats: S [n, ld], bits [n, W], rank [n] and term [n]")
    n, ld = S.shape
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"retrieval_beats: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    W = (N + 31) // 32
    if n < 1 or ld < N or tuple(bits.shape) != (n, W) or tuple(rank.shape) != (n,) or tuple(term.shape) != (n,):
        raise ValueError(f"retrieval_beats: S [n, ld >= {N}], bits [n, {W}], rank [n] and term [n] do not match")
    if not 0 <= q0 <= N - n:
        raise ValueError(f"retrieval_beats: rows {q0} .. {q0 + n - 1} are not among the {N} cases")
    if not 0 < temperature < float("inf"):
        raise ValueError("retrieval_beats: the temperature must be positive and finite")
    with _prof("retrieval_beats", 0.0, 4.0 * n * N + 4.0 * n * W):
        check(_lib.load().sm3_retrieval_beats(_ptr(S), ld, n, int(q0), int(N), float(temperature), _ptr(bits), _ptr(rank), _ptr(term),
                                              _stream()), "sm3_retrieval_beats")


def retrieval_counts(bits, ks, out, seed, r0, point=False):
    """out [c, L + 3] int64 = (H_1 .. H_L, R, Q, M) of the packed flags bits [N, ceil(N / 32)] int32 for bootstrap replicates r0 ..
    r0 + c - 1, or for the point estimate (point: c = 1, every case once) (sm3_retrieval_counts).  ks: the L Recall@k levels, a
    sequence of integers in [1, REPORT_MAX_CASES], L <= RETRIEVAL_MAX_LEVELS."""
    _chk(bits, torch.int32, "bits"); _chk(out, torch.int64, "out")
    if bits.dim() != 2 or out.dim() != 2:
        raise ValueError("retrieval_counts: bits [N, W] and out [c, L + 3]")
    N, c = bits.shape[0], out.shape[0]
    ks = list(ks)
    L = len(ks)
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"retrieval_counts: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    if not 1 <= L <= RETRIEVAL_MAX_LEVELS or not all(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= REPORT_MAX_CASES
                                                     for k in ks):
        raise ValueError(f"retrieval_counts: 1 to {RETRIEVAL_MAX_LEVELS} integer levels in [1, {REPORT_MAX_CASES}], got {ks!r}")
    if bits.shape[1] != (N + 31) // 32 or c < 1 or tuple(out.shape) != (c, L + 3):
        raise ValueError(f"retrieval_counts: bits [N, {(N + 31) // 32}] and out [c, {L + 3}] do not match")
    _replicates_chk("retrieval_counts", seed, point, c, "record")
    with _prof("retrieval_counts", 0.0, 4.0 * bits.numel() * c):
        check(_lib.load().sm3_retrieval_counts(_ptr(bits), N, (C.c_int32 * L)(*ks), L, _ptr(out), seed, int(r0), c, int(bool(point)),
                                               _stream()), "sm3_retrieval_counts")


TSNE_MAX_POINTS = 16384  # sm3_tsne_max_points()
TSNE_MAX_DIM = 4096


def _tsne_n(who, N):
    if not 4 <= N <= TSNE_MAX_POINTS:
        raise ValueError(f"{who}: {N} points, 4 to {TSNE_MAX_POINTS} are supported")


def tsne_sqdist(x, d2):
    """d2 [N, N] float32 = the squared distances of the rows of x [N, D] float32, by differences, k ascending; the diagonal 0 and
    d2 == d2.T in bits (sm3_tsne_sqdist)."""
    _chk(x, torch.float32, "x"); _chk(d2, torch.float32, "d2")
    if x.dim() != 2 or d2.dim() != 2:
        raise ValueError("tsne_sqdist: x [N, D] and d2 [N, N]")
    N, D = x.shape
    _tsne_n("tsne_sqdist", N)
    if not 1 <= D <= TSNE_MAX_DIM or tuple(d2.shape) != (N, N):
        raise ValueError(f"tsne_sqdist: x [N, 1 <= D <= {TSNE_MAX_DIM}] and d2 [{N}, {N}] do not match")
    with _prof("tsne_sqdist", 3.0 * N * N * D, 4.0 * N * N):
        check(_lib.load().sm3_tsne_sqdist(_ptr(x), N, D, _ptr(d2), _stream()), "sm3_tsne_sqdist")


def tsne_affinities(d2, perplexity, cond, beta):
    """cond [N, N] float32 = the conditional affinities of the rows of d2 [N, N] float32 at the given perplexity (100 bisection
    steps in fp64, cond[i, i] = 0), beta [N] float64 = the precisions found (sm3_tsne_affinities)."""
    _chk(d2, torch.float32, "d2"); _chk(cond, torch.float32, "cond"); _chk(beta, torch.float64, "beta")
    N = d2.shape[0]
    _tsne_n("tsne_affinities", N)
    if tuple(d2.shape) != (N, N) or tuple(cond.shape) != (N, N) or tuple(beta.shape) != (N,):
        raise ValueError(f"tsne_affinities: d2 [{N}, {N}], cond [{N}, {N}] and beta [{N}] do not match")
    if not 1 <= perplexity <= N - 1:
        raise ValueError(f"tsne_affinities: the perplexity must lie in [1, N - 1], got {perplexity!r}")
    with _prof("tsne_affinities", 0.0, 8.0 * N * N):
        check(_lib.load().sm3_tsne_affinities(_ptr(d2), N, float(perplexity), _ptr(cond), _ptr(beta), _stream()),
              "sm3_tsne_affinities")


def tsne_symmetrise(cond, P):
    """P [N, N] float32 = float32((cond + cond.T in fp64) / (2 N)) (sm3_tsne_symmetrise)."""
    _chk(cond, torch.float32, "cond"); _chk(P, torch.float32, "P")
    N = cond.shape[0]
    _tsne_n("tsne_symmetrise", N)
    if tuple(cond.shape) != (N, N) or tuple(P.shape) != (N, N) or cond.data_ptr() == P.data_ptr():
        raise ValueError(f"tsne_symmetrise: cond [{N}, {N}] and another P [{N}, {N}]")
    with _prof("tsne_symmetrise", 0.0, 12.0 * N * N):
        check(_lib.load().sm3_tsne_symmetrise(_ptr(cond), N, _ptr(P), _stream()), "sm3_tsne_symmetrise")


def _tsne_state(who, N, P=None, y=None, F=None):
    _tsne_n(who, N)
    if (P is not None and tuple(P.shape) != (N, N)) or (y is not None and tuple(y.shape) != (N, 2)) or \
            (F is not None and tuple(F.shape) != (N, 5)):
        raise ValueError(f"{who}: P [{N}, {N}], y [{N}, 2] and F [{N}, 5] do not match")


def tsne_forces(P, y, F):
    """F [N, 5] float64 = (Z_i, A_i.x, A_i.y, R_i.x, R_i.y) of the map y [N, 2] float32 under P [N, N] float32 (sm3_tsne_forces)."""
    _chk(P, torch.float32, "P"); _chk(y, torch.float32, "y"); _chk(F, torch.float64, "F")
    N = y.shape[0]
    _tsne_state("tsne_forces", N, P, y, F)
    with _prof("tsne_forces", 20.0 * N * N, 4.0 * N * N):
        check(_lib.load().sm3_tsne_forces(_ptr(P), _ptr(y), N, _ptr(F), _stream()), "sm3_tsne_forces")


def tsne_update(F, exaggeration, momentum, lr, y, update, gains, out):
    """One gradient step from the force sums F [N, 5]: y, update and gains [N, 2] float32 are rewritten in place, out [2] float64 =
    (sum (gains g)^2, Z) (sm3_tsne_update)."""
    _chk(F, torch.float64, "F"); _chk(out, torch.float64, "out")
    N = y.shape[0]
    for t, n in ((y, "y"), (update, "update"), (gains, "gains")):
        _chk(t, torch.float32, n)
        if tuple(t.shape) != (N, 2):
            raise ValueError(f"tsne_update: {n} must be [{N}, 2]")
    _tsne_state("tsne_update", N, None, y, F)
    if out.numel() != 2:
        raise ValueError("tsne_update: out [2]")
    with _prof("tsne_update", 0.0, 64.0 * N):
        check(_lib.load().sm3_tsne_update(_ptr(F), N, float(exaggeration), float(momentum), float(lr), _ptr(y), _ptr(update),
                                          _ptr(gains), _ptr(out), _stream()), "sm3_tsne_update")


def tsne_kl(P, y, F, rows, out):
    """out [2] float64 = (KL(P || Q) of the map y, Z), from F = tsne_forces(P, y); rows [N] float64 is scratch (sm3_tsne_kl)."""
    _chk(P, torch.float32, "P"); _chk(y, torch.float32, "y"); _chk(F, torch.float64, "F")
    _chk(rows, torch.float64, "rows"); _chk(out, torch.float64, "out")
    N = y.shape[0]
    _tsne_state("tsne_kl", N, P, y, F)
    if tuple(rows.shape) != (N,) or out.numel() != 2:
        raise ValueError(f"tsne_kl: rows [{N}] and out [2]")
    with _prof("tsne_kl", 0.0, 4.0 * N * N):
        check(_lib.load().sm3_tsne_kl(_ptr(P), _ptr(y), _ptr(F), N, _ptr(rows), _ptr(out), _stream()), "sm3_tsne_kl")


LOGREG_MAX_ROWS = 16384  # sm3_logreg_max_rows()
LOGREG_MAX_DIM = 4096
LOGREG_MAX_CLASSES = 8   # the stride of every per-class array of csrc/logreg.hip; n_t <= 8


def _logreg_shape(who, N, D):
    if not 1 <= N <= LOGREG_MAX_ROWS or not 1 <= D <= LOGREG_MAX_DIM:
        raise ValueError(f"{who}: X [{N}, {D}], at most [{LOGREG_MAX_ROWS}, {LOGREG_MAX_DIM}] and at least [1, 1] are supported")


def logreg_workspace(N, D, fit=True):
    """The float64 elements of workspace one problem needs (sm3_logreg_workspace)."""
    _logreg_shape("logreg_workspace", N, D)
    out = C.c_int64(0)
    check(_lib.load().sm3_logreg_workspace(int(N), int(D), int(bool(fit)), C.byref(out)), "sm3_logreg_workspace")
    return int(out.value)


def logreg_check_host(targets, weights, table, Cs, n_classes):
    """The refusals that read the problem data, on HOST tensors before anything is uploaded or launched (sm3_logreg_check_host):
    targets [N, 8] int32, weights [R, N] float64, table [P, 4] int32 = (label, weight row, n_t, 0), Cs [P] float64."""
    for t, dt, n in ((targets, torch.int32, "targets"), (weights, torch.float64, "weights"), (table, torch.int32, "table"),
                     (Cs, torch.float64, "Cs")):
        if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"logreg_check_host: {n} must be a contiguous host tensor of {dt}")
    n_classes = [int(c) for c in n_classes]
    if targets.dim() != 2 or targets.shape[1] != LOGREG_MAX_CLASSES or len(n_classes) != LOGREG_MAX_CLASSES:
        raise ValueError("logreg_check_host: targets [N, 8] and the classes of 8 labels")
    N, P = targets.shape[0], table.shape[0]
    if weights.dim() != 2 or weights.shape[1] != N or weights.shape[0] < 1:
        raise ValueError(f"logreg_check_host: weights [R >= 1, {N}]")
    if table.dim() != 2 or table.shape[1] != 4 or tuple(Cs.shape) != (P,) or P < 1:
        raise ValueError("logreg_check_host: table [P >= 1, 4] and Cs [P]")
    if not 1 <= N <= LOGREG_MAX_ROWS:
        raise ValueError(f"logreg_check_host: {N} rows, 1 to {LOGREG_MAX_ROWS} are supported")
    rc = _lib.load().sm3_logreg_check_host(_ptr(targets), _ptr(weights), _ptr(table), _ptr(Cs), (C.c_int32 * 8)(*n_classes),
                                           N, weights.shape[0], P)
    if rc != 0:
        raise ValueError("logreg: a class index outside [0, n_t), a negative or non-finite weight, a C that is not positive and "
                         "finite, or a problem that names no label / weight row (sm3_logreg_check_host)")


def _logreg_problem_tensors(who, X, targets, weights, table, Cs):
    _chk(X, torch.float32, "X"); _chk(targets, torch.int32, "targets"); _chk(weights, torch.float64, "weights")
    _chk(table, torch.int32, "table"); _chk(Cs, torch.float64, "Cs")
    if X.dim() != 2 or targets.dim() != 2 or weights.dim() != 2 or table.dim() != 2 or Cs.dim() != 1:
        raise ValueError(f"{who}: X [N, D], targets [N, 8], weights [R, N], table [P, 4] and Cs [P]")
    N, D = X.shape
    _logreg_shape(who, N, D)
    R, P = weights.shape[0], table.shape[0]
    if tuple(targets.shape) != (N, LOGREG_MAX_CLASSES) or weights.shape[1] != N or R < 1 or P < 1 or \
            tuple(table.shape) != (P, 4) or tuple(Cs.shape) != (P,):
        raise ValueError(f"{who}: X [{N}, {D}], targets [{N}, 8], weights [R, {N}], table [P, 4] and Cs [P] do not match")
    return N, D, R, P


def logreg_value_grad(X, targets, weights, table, Cs, W, b, ws, F, gW, gb):
    """F [P], gW [P, 8, D], gb [P, 8] float64 = value and gradient of the P problems of (table, Cs) at W [P, 8, D], b [P, 8]
    (sm3_logreg_value_grad); ws: float64 workspace of at least P * logreg_workspace(N, D, fit=False) elements."""
    N, D, R, P = _logreg_problem_tensors("logreg_value_grad", X, targets, weights, table, Cs)
    for t, n in ((W, "W"), (b, "b"), (ws, "ws"), (F, "F"), (gW, "gW"), (gb, "gb")):
        _chk(t, torch.float64, n)
    K = LOGREG_MAX_CLASSES
    if tuple(W.shape) != (P, K, D) or tuple(gW.shape) != (P, K, D) or tuple(b.shape) != (P, K) or tuple(gb.shape) != (P, K) or \
            tuple(F.shape) != (P,) or ws.numel() < P * logreg_workspace(N, D, False):
        raise ValueError(f"logreg_value_grad: W, gW [{P}, {K}, {D}], b, gb [{P}, {K}], F [{P}] and the workspace do not match")
    with _prof("logreg_value_grad", 4.0 * N * D * K * P, 4.0 * N * D * P):
        check(_lib.load().sm3_logreg_value_grad(_ptr(X), _ptr(targets), _ptr(weights), _ptr(table), _ptr(Cs), _ptr(W), _ptr(b),
                                                N, D, R, P, _ptr(ws), ws.numel(), _ptr(F), _ptr(gW), _ptr(gb), _stream()),
              "sm3_logreg_value_grad")


LOGREG_RUNNING = 5  # info status of a problem whose launch ran out of its iterations


def logreg_fit(X, targets, weights, table, Cs, gtol, max_iter, ws, coef, intercept, info, res, resume=False, iters=None):
    """The minimisers of the P problems: coef [P, 8, D], intercept [P, 8] float64, info [P, 2] int32 = (status, iterations), res
    [P, 2] float64 = (F, |grad F|_inf) (sm3_logreg_fit); ws: at least P * logreg_workspace(N, D) float64 elements.  ONE launch
    of at most `iters` iterations a problem (None: max_iter); a problem it leaves unfinished has status LOGREG_RUNNING and goes
    on in a call with resume=True and the same tensors."""
    N, D, R, P = _logreg_problem_tensors("logreg_fit", X, targets, weights, table, Cs)
    for t, n in ((ws, "ws"), (coef, "coef"), (intercept, "intercept"), (res, "res")):
        _chk(t, torch.float64, n)
    _chk(info, torch.int32, "info")
    K = LOGREG_MAX_CLASSES
    if tuple(coef.shape) != (P, K, D) or tuple(intercept.shape) != (P, K) or tuple(info.shape) != (P, 2) or \
            tuple(res.shape) != (P, 2) or ws.numel() < P * logreg_workspace(N, D, True):
        raise ValueError(f"logreg_fit: coef [{P}, {K}, {D}], intercept [{P}, {K}], info, res [{P}, 2] and the workspace do not match")
    if isinstance(gtol, bool) or not isinstance(gtol, (int, float)) or not 0 <= gtol < float("inf"):
        raise ValueError(f"logreg_fit: gtol must be a finite number >= 0, got {gtol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 0 <= max_iter < 2 ** 31:
        raise ValueError(f"logreg_fit: max_iter must be an integer >= 0, got {max_iter!r}")
    iters = max(max_iter, 1) if iters is None else iters
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters < 2 ** 31:
        raise ValueError(f"logreg_fit: iters must be an integer >= 1, got {iters!r}")
    with _prof("logreg_fit", 0.0, 0.0):
        check(_lib.load().sm3_logreg_fit(_ptr(X), _ptr(targets), _ptr(weights), _ptr(table), _ptr(Cs), N, D, R, P, float(gtol),
                                         max_iter, int(bool(resume)), iters, _ptr(ws), ws.numel(), _ptr(coef), _ptr(intercept), _ptr(info), _ptr(res),
                                         _stream()), "sm3_logreg_fit")


def logreg_predict(Xq, coef, intercept, nts, logits):
    """logits [P, Q, 8] float64 of the rows Xq [Q, D] float32 under coef [P, 8, D], intercept [P, 8]; nts [P] int32 = the classes
    of each problem (sm3_logreg_predict)."""
    _chk(Xq, torch.float32, "Xq"); _chk(coef, torch.float64, "coef"); _chk(intercept, torch.float64, "intercept")
    _chk(nts, torch.int32, "nts"); _chk(logits, torch.float64, "logits")
    if Xq.dim() != 2 or coef.dim() != 3:
        raise ValueError("logreg_predict: Xq [Q, D] and coef [P, 8, D]")
    (Q, D), P, K = Xq.shape, coef.shape[0], LOGREG_MAX_CLASSES
    if not 1 <= Q <= 2 ** 24 or not 1 <= D <= LOGREG_MAX_DIM or not 1 <= P <= 65535:
        raise ValueError(f"logreg_predict: Q in [1, 2^24], D in [1, {LOGREG_MAX_DIM}] and P in [1, 65535] a launch")
    if tuple(coef.shape) != (P, K, D) or tuple(intercept.shape) != (P, K) or tuple(nts.shape) != (P,) or \
            tuple(logits.shape) != (P, Q, K):
        raise ValueError(f"logreg_predict: coef [{P}, {K}, {D}], intercept [{P}, {K}], nts [{P}] and logits [{P}, {Q}, {K}] do not match")
    with _prof("logreg_predict", 2.0 * Q * D * K * P, 4.0 * Q * D * P):
        check(_lib.load().sm3_logreg_predict(_ptr(Xq), _ptr(coef), _ptr(intercept), _ptr(nts), Q, D, P, _ptr(logits), _stream()),
              "sm3_logreg_predict")


LOGREG_LOCKSTEP_SLAB = 2048        # sm3_logreg_lockstep_slab(): the rows of one slab of the batched gradient product
LOGREG_LOCKSTEP_MAX_PROBLEMS = 65535
LOGREG_LOCKSTEP_MAX_ITERS = 1024   # iterations one sm3_logreg_fit_lockstep call may enqueue


def logreg_columns(nts):
    """The column table of the lockstep solver for problems of nts[p] classes: int32 [sum nts], entry 8 p + c for c < nts[p]."""
    nts = [int(n) for n in nts]
    if not nts or not all(1 <= n <= LOGREG_MAX_CLASSES for n in nts):
        raise ValueError(f"logreg_columns: every problem has 1 to {LOGREG_MAX_CLASSES} classes")
    return torch.tensor([LOGREG_MAX_CLASSES * p + c for p, n in enumerate(nts) for c in range(n)], dtype=torch.int32)


def _logreg_batch(who, N, D, P, ncols):
    _logreg_shape(who, N, D)
    if not 1 <= P <= LOGREG_LOCKSTEP_MAX_PROBLEMS or not 1 <= ncols <= LOGREG_MAX_CLASSES * P:
        raise ValueError(f"{who}: 1 to {LOGREG_LOCKSTEP_MAX_PROBLEMS} problems a call in 1 to 8 P columns, got P = {P}, {ncols} columns")


def logreg_lockstep_workspace(N, D, P, ncols, fit=True):
    """The float64 elements of workspace ONE call of the lockstep fit (or of logreg_value_grad_lockstep) needs for P problems in
    ncols columns (sm3_logreg_lockstep_workspace)."""
    _logreg_batch("logreg_lockstep_workspace", N, D, P, ncols)
    out = C.c_int64(0)
    check(_lib.load().sm3_logreg_lockstep_workspace(int(N), int(D), int(P), int(ncols), int(bool(fit)), C.byref(out)),
          "sm3_logreg_lockstep_workspace")
    return int(out.value)


def logreg_batch_logits(X, V, vb, cols, active, Z):
    """Z [P, N, 8] float64: Z[p, i, c] = sum_k X[i, k] V[p, c, k] + vb[p, c] for the columns cols (logreg_columns) of the problems
    with active[p] != 0, on the f64 MFMA (sm3_logreg_batch_logits).  V [P, 8, D], vb [P, 8] or None, active [P] int32.  Nothing
    of an inactive problem, and nothing outside the columns listed, is written."""
    _chk(X, torch.float32, "X"); _chk(V, torch.float64, "V"); _chk(cols, torch.int32, "cols"); _chk(active, torch.int32, "active")
    _chk(Z, torch.float64, "Z")
    if vb is not None:
        _chk(vb, torch.float64, "vb")
    if X.dim() != 2 or V.dim() != 3 or cols.dim() != 1:
        raise ValueError("logreg_batch_logits: X [N, D], V [P, 8, D] and cols [ncols]")
    (N, D), P, K, ncols = X.shape, V.shape[0], LOGREG_MAX_CLASSES, cols.shape[0]
    _logreg_batch("logreg_batch_logits", N, D, P, ncols)
    if tuple(V.shape) != (P, K, D) or tuple(Z.shape) != (P, N, K) or tuple(active.shape) != (P,) or \
            (vb is not None and tuple(vb.shape) != (P, K)):
        raise ValueError(f"logreg_batch_logits: V [{P}, {K}, {D}], vb [{P}, {K}], active [{P}] and Z [{P}, {N}, {K}] do not match")
    with _prof("logreg_batch_logits", 2.0 * N * D * ncols, 4.0 * N * D):
        check(_lib.load().sm3_logreg_batch_logits(_ptr(X), _ptr(V), None if vb is None else _ptr(vb), _ptr(cols), _ptr(active), N, D,
                                                  P, ncols, _ptr(Z), _stream()), "sm3_logreg_batch_logits")


def logreg_batch_grad(X, Rm, cols, active, ws, G, gb):
    """G [P, 8, D], gb [P, 8] float64: G[p, c, k] = sum_i Rm[p, i, c] X[i, k], gb[p, c] = sum_i Rm[p, i, c] for the columns cols
    of the problems with active[p] != 0, on the f64 MFMA (sm3_logreg_batch_grad).  Rm [P, N, 8]; ws: at least ceil(N /
    LOGREG_LOCKSTEP_SLAB) * ncols * D float64 elements.  Nothing of an inactive problem is written."""
    _chk(X, torch.float32, "X"); _chk(Rm, torch.float64, "Rm"); _chk(cols, torch.int32, "cols"); _chk(active, torch.int32, "active")
    _chk(ws, torch.float64, "ws"); _chk(G, torch.float64, "G"); _chk(gb, torch.float64, "gb")
    if X.dim() != 2 or Rm.dim() != 3 or cols.dim() != 1:
        raise ValueError("logreg_batch_grad: X [N, D], Rm [P, N, 8] and cols [ncols]")
    (N, D), P, K, ncols = X.shape, Rm.shape[0], LOGREG_MAX_CLASSES, cols.shape[0]
    _logreg_batch("logreg_batch_grad", N, D, P, ncols)
    need = -(-N // LOGREG_LOCKSTEP_SLAB) * ncols * D
    if tuple(Rm.shape) != (P, N, K) or tuple(G.shape) != (P, K, D) or tuple(gb.shape) != (P, K) or tuple(active.shape) != (P,) or \
            ws.numel() < need:
        raise ValueError(f"logreg_batch_grad: Rm [{P}, {N}, {K}], G [{P}, {K}, {D}], gb [{P}, {K}], active [{P}] and the workspace "
                         f"(at least {need} elements) do not match")
    with _prof("logreg_batch_grad", 2.0 * N * D * ncols, 4.0 * N * D):
        check(_lib.load().sm3_logreg_batch_grad(_ptr(X), _ptr(Rm), _ptr(cols), _ptr(active), N, D, P, ncols, _ptr(ws), ws.numel(),
                                                _ptr(G), _ptr(gb), _stream()), "sm3_logreg_batch_grad")


def logreg_value_grad_lockstep(X, targets, weights, table, Cs, cols, W, b, ws, F, gW, gb):
    """logreg_value_grad through the two batched products (sm3_logreg_value_grad_lockstep); cols: logreg_columns of the problems'
    classes; ws: at least logreg_lockstep_workspace(N, D, P, ncols, fit=False) float64 elements."""
    who = "logreg_value_grad_lockstep"
    N, D, R, P = _logreg_problem_tensors(who, X, targets, weights, table, Cs)
    for t, n in ((W, "W"), (b, "b"), (ws, "ws"), (F, "F"), (gW, "gW"), (gb, "gb")):
        _chk(t, torch.float64, n)
    _chk(cols, torch.int32, "cols")
    K, ncols = LOGREG_MAX_CLASSES, cols.numel()
    _logreg_batch(who, N, D, P, ncols)
    if cols.dim() != 1 or tuple(W.shape) != (P, K, D) or tuple(gW.shape) != (P, K, D) or tuple(b.shape) != (P, K) or \
            tuple(gb.shape) != (P, K) or tuple(F.shape) != (P,) or ws.numel() < logreg_lockstep_workspace(N, D, P, ncols, False):
        raise ValueError(f"{who}: W, gW [{P}, {K}, {D}], b, gb [{P}, {K}], F [{P}], cols [ncols] and the workspace do not match")
    with _prof(who, 4.0 * N * D * ncols, 8.0 * N * D):
        check(_lib.load().sm3_logreg_value_grad_lockstep(_ptr(X), _ptr(targets), _ptr(weights), _ptr(table), _ptr(Cs), _ptr(cols),
                                                         _ptr(W), _ptr(b), N, D, R, P, ncols, _ptr(ws), ws.numel(), _ptr(F), _ptr(gW),
                                                         _ptr(gb), _stream()), "sm3_logreg_value_grad_lockstep")


def logreg_fit_lockstep(X, targets, weights, table, Cs, cols, gtol, max_iter, ws, coef, intercept, info, res, resume=False, iters=1):
    """logreg_fit's outputs by the lockstep solver (sm3_logreg_fit_lockstep): ONE call enqueues `iters` iterations (1 to
    LOGREG_LOCKSTEP_MAX_ITERS) of all P problems side by side; a problem it leaves unfinished has status LOGREG_RUNNING and goes on
    in a call with resume=True and the same tensors.  cols: logreg_columns of the problems' classes; ws: at least
    logreg_lockstep_workspace(N, D, P, ncols) float64 elements."""
    who = "logreg_fit_lockstep"
    N, D, R, P = _logreg_problem_tensors(who, X, targets, weights, table, Cs)
    for t, n in ((ws, "ws"), (coef, "coef"), (intercept, "intercept"), (res, "res")):
        _chk(t, torch.float64, n)
    _chk(info, torch.int32, "info"); _chk(cols, torch.int32, "cols")
    K, ncols = LOGREG_MAX_CLASSES, cols.numel()
    _logreg_batch(who, N, D, P, ncols)
    if cols.dim() != 1 or tuple(coef.shape) != (P, K, D) or tuple(intercept.shape) != (P, K) or tuple(info.shape) != (P, 2) or \
            tuple(res.shape) != (P, 2) or ws.numel() < logreg_lockstep_workspace(N, D, P, ncols, True):
        raise ValueError(f"{who}: coef [{P}, {K}, {D}], intercept [{P}, {K}], info, res [{P}, 2], cols [ncols] and the workspace do "
                         "not match")
    if isinstance(gtol, bool) or not isinstance(gtol, (int, float)) or not 0 <= gtol < float("inf"):
        raise ValueError(f"{who}: gtol must be a finite number >= 0, got {gtol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 0 <= max_iter < 2 ** 31:
        raise ValueError(f"{who}: max_iter must be an integer >= 0, got {max_iter!r}")
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= LOGREG_LOCKSTEP_MAX_ITERS:
        raise ValueError(f"{who}: iters must be an integer in [1, {LOGREG_LOCKSTEP_MAX_ITERS}], got {iters!r}")
    with _prof(who, 0.0, 0.0):
        check(_lib.load().sm3_logreg_fit_lockstep(_ptr(X), _ptr(targets), _ptr(weights), _ptr(table), _ptr(Cs), _ptr(cols), N, D, R,
                                                  P, ncols, float(gtol), max_iter, int(bool(resume)), iters, _ptr(ws), ws.numel(),
                                                  _ptr(coef), _ptr(intercept), _ptr(info), _ptr(res), _stream()),
              "sm3_logreg_fit_lockstep")


CALIB_MAX_BINS = 64
CALIB_BINNINGS = ("width", "mass")


def calib_counts(q, ev, order, slabel, xq, bins, sums, labels, binning, seed, r0, point=False):
    """bins [c, S, M, 3] int64 = (n_b, E_b, Q_b) of the S series and sums [c, X] int64 of the X plain sums for bootstrap replicates
    r0 .. r0 + c - 1, or for the point estimate (point: c = 1, every case once) (sm3_calib_counts).  q [S, N] int64 (Q32), ev
    [S, N] uint8, order [S, N] int32 (each series' cases in ascending q, stable), slabel [S] int32 = the label of a series, xq
    [X, N] int64; labels: T, the number of labels (plain sum x is served with label x % T); binning: "width" or "mass"."""
    for t, n in ((q, "q"), (xq, "xq"), (bins, "bins"), (sums, "sums")):
        _chk(t, torch.int64, n)
    _chk(ev, torch.uint8, "ev"); _chk(order, torch.int32, "order"); _chk(slabel, torch.int32, "slabel")
    if q.dim() != 2 or xq.dim() != 2 or bins.dim() != 4 or sums.dim() != 2:
        raise ValueError("calib_counts: q [S, N], xq [X, N], bins [c, S, M, 3] and sums [c, X]")
    S, N = q.shape
    X = xq.shape[0]
    c, M = bins.shape[0], bins.shape[2]
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"calib_counts: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    if not 1 <= M <= CALIB_MAX_BINS:
        raise ValueError(f"calib_counts: {M} bins, 1 to {CALIB_MAX_BINS} are supported")
    if tuple(ev.shape) != (S, N) or tuple(order.shape) != (S, N) or tuple(slabel.shape) != (S,) or tuple(xq.shape) != (X, N) or \
            tuple(bins.shape) != (c, S, M, 3) or tuple(sums.shape) != (c, X):
        raise ValueError("calib_counts: q, ev, order [S, N], slabel [S], xq [X, N], bins [c, S, M, 3] and sums [c, X] do not match")
    if binning not in CALIB_BINNINGS:
        raise ValueError(f"calib_counts: binning must be one of {CALIB_BINNINGS}, got {binning!r}")
    _replicates_chk("calib_counts", seed, point, c)
    with _prof("calib_counts", 0.0, (8.0 + 4 + 1) * S * N * c):
        check(_lib.load().sm3_calib_counts(_ptr(q), _ptr(ev), _ptr(order), _ptr(slabel), _ptr(xq), _ptr(bins), _ptr(sums), N, S, X,
                                           int(labels), M, CALIB_BINNINGS.index(binning), seed, int(r0), c, int(bool(point)),
                                           _stream()), "sm3_calib_counts")


CONFORMAL_MAX_LEVELS = 8
CONFORMAL_MAX_CLASSES = 5
CONFORMAL_RECORD = 24  # cov, size, single_hit, hist[0 .. 5], then (n_c, cov_c, in_c) of the classes 0 .. 4
CONFORMAL_CONDITIONALS = ("marginal", "class")


def conformal_counts(cal_a, cal_order, cal_y, s, y, colmap, alphas, counts, thr, conditional, seed, r0, point=False, fixed_thr=None):
    """counts [c, T, A, 24] int64, the set counts of the test split, and thr [c, T, A, 5] int64, the thresholds they were counted
    under, for bootstrap replicates r0 .. r0 + c - 1, or for the point estimate (point: c = 1, every case of both splits once)
    (sm3_conformal_counts).  cal_a [T, N_cal] int64 = the true-class scores of the calibration cases, cal_order [T, N_cal] int32
    = each label's cases in ascending cal_a (stable), cal_y [N_cal, T] int32; s [K, N] int64 = the scores of the test cases, y
    [N, T] int32; colmap [K, 2] int32 = (label, class); alphas: A pairs of integers (num, den), the level num / den;
    conditional: "marginal" or "class"; fixed_thr: None (thresholds refitted in every replicate) or [T, A, 5] int64."""
    for t, n in ((cal_a, "cal_a"), (s, "s"), (counts, "counts"), (thr, "thr"), (fixed_thr, "fixed_thr")):
        _chk(t, torch.int64, n)
    for t, n in ((cal_order, "cal_order"), (cal_y, "cal_y"), (y, "y"), (colmap, "colmap")):
        _chk(t, torch.int32, n)
    if cal_a.dim() != 2 or s.dim() != 2 or counts.dim() != 4 or thr.dim() != 4:
        raise ValueError("conformal_counts: cal_a [T, N_cal], s [K, N], counts [c, T, A, 24] and thr [c, T, A, 5]")
    T, N_cal = cal_a.shape
    K, N = s.shape
    c, A = counts.shape[0], counts.shape[2]
    for n, what in ((N_cal, "calibration"), (N, "test")):
        if not 1 <= n <= REPORT_MAX_CASES:
            raise ValueError(f"conformal_counts: {n} {what} cases, 1 to {REPORT_MAX_CASES} are supported")
    if not 1 <= A <= CONFORMAL_MAX_LEVELS:
        raise ValueError(f"conformal_counts: {A} levels, 1 to {CONFORMAL_MAX_LEVELS} are supported")
    if tuple(cal_order.shape) != (T, N_cal) or tuple(cal_y.shape) != (N_cal, T) or tuple(y.shape) != (N, T) or \
            tuple(colmap.shape) != (K, 2) or tuple(counts.shape) != (c, T, A, CONFORMAL_RECORD) or \
            tuple(thr.shape) != (c, T, A, CONFORMAL_MAX_CLASSES) or \
            (fixed_thr is not None and tuple(fixed_thr.shape) != (T, A, CONFORMAL_MAX_CLASSES)):
        raise ValueError("conformal_counts: cal_a, cal_order [T, N_cal], cal_y [N_cal, T], s [K, N], y [N, T], colmap [K, 2], "
                         "counts [c, T, A, 24], thr [c, T, A, 5] and fixed_thr [T, A, 5] do not match")
    alphas = [tuple(a) for a in alphas]
    if len(alphas) != A or not all(len(a) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in a)
                                   and 0 < a[0] < a[1] < 2 ** 31 for a in alphas):
        raise ValueError(f"conformal_counts: alphas must be {A} pairs of integers (num, den) with 0 < num < den < 2^31, got {alphas!r}")
    if conditional not in CONFORMAL_CONDITIONALS:
        raise ValueError(f"conformal_counts: conditional must be one of {CONFORMAL_CONDITIONALS}, got {conditional!r}")
    _replicates_chk("conformal_counts", seed, point, c, one="record")
    levels = (C.c_int * (2 * A))(*[v for a in alphas for v in a])
    with _prof("conformal_counts", 0.0, (8.0 + 4 + 4) * N_cal * T * c + 8.0 * K * N * A * c):
        check(_lib.load().sm3_conformal_counts(_ptr(cal_a), _ptr(cal_order), _ptr(cal_y), _ptr(s), _ptr(y), _ptr(colmap), levels,
                                               _ptr(fixed_thr), _ptr(counts), _ptr(thr), N_cal, N, T, K, A,
                                               CONFORMAL_CONDITIONALS.index(conditional), seed, int(r0), c, int(bool(point)),
                                               _stream()), "sm3_conformal_counts")


SELECTIVE_MAX_COVERAGES = 16
SELECTIVE_MAX_RISKS = 8
SELECTIVE_MAX_THRESHOLDS = 8
SELECTIVE_LABELS = 8


def selective_record(G, H, Pc):
    """int64 entries of one (replicate, label) record of sm3_selective_counts (sm3_selective_record)."""
    return 3 + 4 * G + 2 * H + 5 * Pc


def selective_counts(packed, order, table, kcuts, pcuts, risks, out, seed, r0, point=False):
    """out [c, 8, 3 + 4 G + 2 H + 5 Pc] int64 = (A, E, P, G x (err, TP, FP, FN) among the first k copies, H x (the largest cut
    within the risk level, its errors), Pc x (C, E, TP, FP, FN) at a fixed position) of the 8 labels for bootstrap replicates
    r0 .. r0 + c - 1, or for the point estimate (point: c = 1, every case once) (sm3_selective_counts).  packed [8, N] int32 = err
    | pos << 1 | call << 2 | last << 3 per (label, case); order [8, N] int32 = the cases, most confident first; table [N + 1]
    int64 = selective.harmonic_table(N); kcuts [G] int32 in [1, N]; pcuts [8, Pc] int32 in [0, N]; risks [H, 2] int32 = (a, b)
    with 0 <= a <= b, 1 <= b; pcuts and risks may be empty."""
    for t, n in ((packed, "packed"), (order, "order"), (kcuts, "kcuts"), (pcuts, "pcuts"), (risks, "risks")):
        _chk(t, torch.int32, n)
    for t, n in ((table, "table"), (out, "out")):
        _chk(t, torch.int64, n)
    if packed.dim() != 2 or table.dim() != 1 or kcuts.dim() != 1 or pcuts.dim() != 2 or risks.dim() != 2 or out.dim() != 3:
        raise ValueError("selective_counts: packed, order [8, N], table [N + 1], kcuts [G], pcuts [8, Pc], risks [H, 2] and out [c, 8, R]")
    L, N = packed.shape
    G, Pc, H, c = kcuts.shape[0], pcuts.shape[1], risks.shape[0], out.shape[0]
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"selective_counts: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    if not 1 <= G <= SELECTIVE_MAX_COVERAGES or H > SELECTIVE_MAX_RISKS or Pc > SELECTIVE_MAX_THRESHOLDS:
        raise ValueError(f"selective_counts: {G} coverage cuts, {H} risk levels, {Pc} position cuts; 1 to {SELECTIVE_MAX_COVERAGES}, "
                         f"at most {SELECTIVE_MAX_RISKS} and at most {SELECTIVE_MAX_THRESHOLDS} are supported")
    if L != SELECTIVE_LABELS or tuple(order.shape) != (L, N) or tuple(table.shape) != (N + 1,) or tuple(pcuts.shape) != (L, Pc) or \
            tuple(risks.shape) != (H, 2) or tuple(out.shape) != (c, L, selective_record(G, H, Pc)):
        raise ValueError("selective_counts: packed, order [8, N], table [N + 1], kcuts [G], pcuts [8, Pc], risks [H, 2] and out [c, 8, "
                         "3 + 4 G + 2 H + 5 Pc] do not match")
    _replicates_chk("selective_counts", seed, point, c, "record")
    with _prof("selective_counts", 0.0, 4.0 * 2 * L * N * c):
        check(_lib.load().sm3_selective_counts(_ptr(packed), _ptr(order), _ptr(table), _ptr(kcuts), _ptr(pcuts) if Pc else None,
                                               _ptr(risks) if H else None, _ptr(out), N, G, H, Pc, seed, int(r0), c,
                                               int(bool(point)), _stream()), "sm3_selective_counts")


OPERATING_MAX_LEVELS = 32  # sm3_operating_max_levels(): entries of each of the two floor lists and of the fixed positions


def operating_record(Ls, Lr, Lt):
    """int64 entries of one (replicate, column) record of sm3_operating_counts."""
    return 9 + 3 * (Ls + Lr) + 2 * Lt


def operating_counts(order, gs, ge, targets, colmap, sigma, rho, fixpos, out, seed, r0, point=False):
    """out [c, K, 9 + 3 Ls + 3 Lr + 2 Lt] int64 = (P, Q, APN, Youden (TP, FP, pos), F1 (TP, FP, pos), Ls x sens at a spec floor (TP,
    FP, pos), Lr x spec at a sens floor (TP, FP, pos), Lt x (TP, FP) at a fixed position) of the K columns for bootstrap replicates
    r0 .. r0 + c - 1, or for the point estimate (point: c = 1, every case once) (sm3_operating_counts).  order, gs, ge, targets,
    colmap: as report_counts.  sigma [Ls], rho [Lr] int64 = floor(floor value * 2^32) in [0, 2^32]; fixpos [K, Lt] int32 in
    [0, N]; each may be empty."""
    for t, n in ((order, "order"), (gs, "gs"), (ge, "ge"), (targets, "targets"), (colmap, "colmap"), (fixpos, "fixpos")):
        _chk(t, torch.int32, n)
    for t, n in ((sigma, "sigma"), (rho, "rho"), (out, "out")):
        _chk(t, torch.int64, n)
    if order.dim() != 2 or targets.dim() != 2 or out.dim() != 3 or sigma.dim() != 1 or rho.dim() != 1 or fixpos.dim() != 2:
        raise ValueError("operating_counts: order [K, N], targets [N, T], sigma [Ls], rho [Lr], fixpos [K, Lt] and out [c, K, R]")
    K, N = order.shape
    T = targets.shape[1]
    c = out.shape[0]
    Ls, Lr, Lt = sigma.shape[0], rho.shape[0], fixpos.shape[1]
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"operating_counts: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    if max(Ls, Lr, Lt) > OPERATING_MAX_LEVELS:
        raise ValueError(f"operating_counts: {Ls} spec floors, {Lr} sens floors, {Lt} fixed positions, at most "
                         f"{OPERATING_MAX_LEVELS} of each are supported")
    if tuple(gs.shape) != (K, N) or tuple(ge.shape) != (K, N) or tuple(targets.shape) != (N, T) or tuple(colmap.shape) != (K, 2) or \
            tuple(fixpos.shape) != (K, Lt) or tuple(out.shape) != (c, K, operating_record(Ls, Lr, Lt)):
        raise ValueError("operating_counts: order, gs, ge [K, N], targets [N, T], colmap [K, 2], fixpos [K, Lt] and out [c, K, 9 + "
                         "3 Ls + 3 Lr + 2 Lt] do not match")
    _replicates_chk("operating_counts", seed, point, c)
    with _prof("operating_counts", 0.0, 4.0 * 3 * K * N * c):
        check(_lib.load().sm3_operating_counts(_ptr(order), _ptr(gs), _ptr(ge), _ptr(targets), _ptr(colmap),
                                               _ptr(sigma) if Ls else None, _ptr(rho) if Lr else None, _ptr(fixpos) if Lt else None,
                                               _ptr(out), N, T, K, Ls, Lr, Lt, seed, int(r0), c, int(bool(point)), _stream()),
              "sm3_operating_counts")


CHECKLIST_RECORD = 242 + 3 * 3  # sm3_checklist_record(): the joint table J[11][11][2], then (A2, P, Q) of three rankings


def checklist_counts(packed, order, gs, ge, out, seed, r0, point=False):
    """out [c, 251] int64 = (J[shat][sstar][mel] (242), 3 x (A2, P, Q)) for bootstrap replicates r0 .. r0 + c - 1, or for the point
    estimate (point: c = 1, every case once) (sm3_checklist_counts).  packed [N] int32 = shat | sstar << 4 | mel << 8 (scores in
    0 .. 10); order, gs, ge [3, N] int32: three rankings as report.ranking forms them; "positive" = mel."""
    for t, n in ((packed, "packed"), (order, "order"), (gs, "gs"), (ge, "ge")):
        _chk(t, torch.int32, n)
    _chk(out, torch.int64, "out")
    if packed.dim() != 1 or order.dim() != 2 or out.dim() != 2:
        raise ValueError("checklist_counts: packed [N], order, gs, ge [3, N] and out [c, 251]")
    N = packed.shape[0]
    c = out.shape[0]
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"checklist_counts: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    if tuple(order.shape) != (3, N) or tuple(gs.shape) != (3, N) or tuple(ge.shape) != (3, N) or \
            tuple(out.shape) != (c, CHECKLIST_RECORD):
        raise ValueError(f"checklist_counts: packed [N], order, gs, ge [3, N] and out [c, {CHECKLIST_RECORD}] do not match")
    _replicates_chk("checklist_counts", seed, point, c, "record")
    with _prof("checklist_counts", 0.0, 4.0 * (1 + 3 * 3) * N * c):
        check(_lib.load().sm3_checklist_counts(_ptr(packed), _ptr(order), _ptr(gs), _ptr(ge), _ptr(out), N, seed, int(r0), c,
                                               int(bool(point)), _stream()), "sm3_checklist_counts")


def signif_counts(order, gs, ge, targets, yhat_a, yhat_b, colmap, out, seed, r0, point=False):
    """out [c, K, 2, 3] int64 = (A2, TP, FP) of the sides A' and B' of the K columns for the swap replicates r0 .. r0 + c - 1 of
    the paired randomisation test, or for the point record (point: c = 1, nothing swapped) (sm3_signif_counts).  order, gs, ge
    [K, 2N] int32: per column the JOINT ranking of the two models' scores, element 2 * i + w = model w's score of case i, and
    the bounds of each position's tie group; targets, yhat_a, yhat_b [N, T] int32; colmap [K, 2] int32 = (label, class)."""
    for t, n in ((order, "order"), (gs, "gs"), (ge, "ge"), (targets, "targets"), (yhat_a, "yhat_a"), (yhat_b, "yhat_b"),
                 (colmap, "colmap")):
        _chk(t, torch.int32, n)
    _chk(out, torch.int64, "out")
    if order.dim() != 2 or targets.dim() != 2 or out.dim() != 4:
        raise ValueError("signif_counts: order [K, 2N], targets [N, T] and out [c, K, 2, 3]")
    K = order.shape[0]
    N, T = targets.shape
    c = out.shape[0]
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"signif_counts: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    if tuple(order.shape) != (K, 2 * N) or tuple(gs.shape) != (K, 2 * N) or tuple(ge.shape) != (K, 2 * N) or \
            tuple(yhat_a.shape) != (N, T) or tuple(yhat_b.shape) != (N, T) or tuple(colmap.shape) != (K, 2) or \
            tuple(out.shape) != (c, K, 2, 3):
        raise ValueError("signif_counts: order, gs, ge [K, 2N], targets, yhat_a, yhat_b [N, T], colmap [K, 2] and out [c, K, 2, 3] "
                         "do not match")
    _replicates_chk("signif_counts", seed, point, c, "record")
    with _prof("signif_counts", 0.0, 4.0 * 3 * K * 2 * N * c):
        check(_lib.load().sm3_signif_counts(_ptr(order), _ptr(gs), _ptr(ge), _ptr(targets), _ptr(yhat_a), _ptr(yhat_b),
                                            _ptr(colmap), _ptr(out), N, T, K, seed, int(r0), c, int(bool(point)), _stream()),
              "sm3_signif_counts")


def signif_placements(order, gs, ge, targets, colmap, out):
    """out [K, N] int32, in case order = DeLong's placements times two of ONE model's own ranking (sm3_signif_placements): for a
    positive case of column k 2 * (negatives ranked below) + tied negatives, for a negative one 2 * (positives ranked above) +
    tied positives.  order, gs, ge [K, N] int32 as report.ranking forms them; targets [N, T] int32; colmap [K, 2] int32."""
    for t, n in ((order, "order"), (gs, "gs"), (ge, "ge"), (targets, "targets"), (colmap, "colmap"), (out, "out")):
        _chk(t, torch.int32, n)
    if order.dim() != 2 or targets.dim() != 2 or out.dim() != 2:
        raise ValueError("signif_placements: order [K, N], targets [N, T] and out [K, N]")
    K, N = order.shape
    T = targets.shape[1]
    if not 1 <= N <= REPORT_MAX_CASES:
        raise ValueError(f"signif_placements: {N} cases, 1 to {REPORT_MAX_CASES} are supported")
    if tuple(gs.shape) != (K, N) or tuple(ge.shape) != (K, N) or tuple(targets.shape) != (N, T) or \
            tuple(colmap.shape) != (K, 2) or tuple(out.shape) != (K, N):
        raise ValueError("signif_placements: order, gs, ge, out [K, N], targets [N, T] and colmap [K, 2] do not match")
    with _prof("signif_placements", 0.0, 4.0 * 4 * K * N):
        check(_lib.load().sm3_signif_placements(_ptr(order), _ptr(gs), _ptr(ge), _ptr(targets), _ptr(colmap), _ptr(out), N, T, K,
                                                _stream()), "sm3_signif_placements")


def stem_wgrad_bn(dtype, x_nchw, dz, xo, mean, invstd, gamma, gsums, count, lsums, dgamma, dbeta, dw, views=1, slabs=None):
    """Stem weight gradient with bn1's backward apply fused into the operand load (sm3_stem_wgrad_bn; bf16 / fp16 / exact f32).
    slabs: fp32 workspace of STEM_WGRAD_SLABS * 64 * 147 floats -> fixed-order sum instead of float atomics."""
    tdt = TORCH_DTYPE[dtype]
    _chk(x_nchw, torch.float32, "x"); _chk(dz, tdt, "dz"); _chk(xo, tdt, "xo"); _chk(dw, torch.float32, "dw")
    for t in (mean, invstd, gamma, dgamma, dbeta):
        _chk(t, torch.float32)
    _chk(gsums, torch.float64); _chk(lsums, torch.float64)
    N, Cc, H, W = x_nchw.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if Cc != 3 or dz.numel() != N * Ho * Wo * 64 or xo.numel() != dz.numel() or dw.numel() < 64 * 147 or N % views:
        raise ValueError("stem_wgrad_bn: size mismatch")
    if mean.numel() < views * 64 or invstd.numel() < views * 64 or gsums.numel() < views * 128 or \
            (lsums is not None and lsums.numel() < views * 128):
        raise ValueError("stem_wgrad_bn: per-channel vector too small")
    _chk(slabs, torch.float32, "slabs")
    if slabs is not None and slabs.numel() < STEM_WGRAD_SLABS * 64 * 147:
        raise ValueError("stem_wgrad_bn: slab workspace too small")
    M = N * Ho * Wo
    with _prof("stem_wgrad_bn", 2.0 * M * 64 * 147, 4.0 * x_nchw.numel() + 2 * _sz(dtype) * dz.numel()):
        check(_lib.load().sm3_stem_wgrad_bn(dtype, _ptr(x_nchw), _ptr(dz), _ptr(xo), _ptr(mean), _ptr(invstd), _ptr(gamma),
                                            _ptr(gsums), float(count), _ptr(lsums), _ptr(dgamma), _ptr(dbeta), _ptr(dw),
                                            _ptr(slabs), N, H, W, views, _stream()), "sm3_stem_wgrad_bn")


def maxpool_fwd(dtype, x, y, N, H, W, Cn, argmax=None):
    _chk(x, TORCH_DTYPE[dtype]); _chk(y, TORCH_DTYPE[dtype]); _chk(argmax, torch.uint8)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if x.numel() != N * H * W * Cn or y.numel() != N * Ho * Wo * Cn:
        raise ValueError("maxpool_fwd: size mismatch")
    if argmax is not None and argmax.numel() != y.numel():
        raise ValueError("maxpool_fwd: argmax size mismatch")
    with _prof("maxpool_fwd", 0.0, _sz(dtype) * (x.numel() + y.numel())):
        check(_lib.load().sm3_maxpool3x3s2_fwd(dtype, _ptr(x), _ptr(y), _ptr(argmax), N, H, W, Cn, _stream()),
              "sm3_maxpool3x3s2_fwd")


def maxpool_bwd(dtype, argmax, dy, dx, N, H, W, Cn):
    _chk(argmax, torch.uint8); _chk(dy, TORCH_DTYPE[dtype]); _chk(dx, TORCH_DTYPE[dtype])
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if dx.numel() != N * H * W * Cn or dy.numel() != N * Ho * Wo * Cn or argmax.numel() != dy.numel():
        raise ValueError("maxpool_bwd: size mismatch")
    with _prof("maxpool_bwd", 0.0, _sz(dtype) * (dx.numel() + dy.numel()) + argmax.numel()):
        check(_lib.load().sm3_maxpool3x3s2_bwd(dtype, _ptr(argmax), _ptr(dy), _ptr(dx), N, H, W, Cn, _stream()),
              "sm3_maxpool3x3s2_bwd")


def avgpool_fwd(dtype, x, feat_f32, feat_t, N, HW, Cn):
    _chk(x, TORCH_DTYPE[dtype]); _chk(feat_f32, torch.float32); _chk(feat_t, TORCH_DTYPE[dtype])
    if x.numel() != N * HW * Cn:
        raise ValueError("avgpool_fwd: size mismatch")
    for t in (feat_f32, feat_t):
        if t is not None and t.numel() != N * Cn:
            raise ValueError("avgpool_fwd: feature size mismatch")
    with _prof("avgpool", 0.0, _sz(dtype) * x.numel()):
        check(_lib.load().sm3_avgpool_fwd(dtype, _ptr(x), _ptr(feat_f32), _ptr(feat_t), N, HW, Cn, _stream()),
              "sm3_avgpool_fwd")


def avgpool_bwd(dtype, dfeat, dx, N, HW, Cn):
    _chk(dfeat, TORCH_DTYPE[dtype]); _chk(dx, TORCH_DTYPE[dtype])
    if dfeat.numel() != N * Cn or dx.numel() != N * HW * Cn:
        raise ValueError("avgpool_bwd: size mismatch")
    with _prof("avgpool", 0.0, _sz(dtype) * dx.numel()):
        check(_lib.load().sm3_avgpool_bwd(dtype, _ptr(dfeat), _ptr(dx), N, HW, Cn, _stream()), "sm3_avgpool_bwd")


def weight_prep(dtype, w, Co, taps, Ci, w_fwd, ld_fwd, w_dgrad):
    _chk(w, torch.float32, "w"); _chk(w_fwd, TORCH_DTYPE[dtype]); _chk(w_dgrad, TORCH_DTYPE[dtype])
    if w.numel() != Co * taps * Ci:
        raise ValueError("weight_prep: master size mismatch")
    if w_fwd is not None and w_fwd.numel() != Co * ld_fwd:
        raise ValueError("weight_prep: w_fwd size mismatch")
    if w_dgrad is not None and w_dgrad.numel() != Co * taps * Ci:
        raise ValueError("weight_prep: w_dgrad size mismatch")
    with _prof("weight_prep", 0.0, w.numel() * (4.0 + 2 * _sz(dtype))):
        check(_lib.load().sm3_weight_prep(dtype, _ptr(w), Co, taps, Ci, _ptr(w_fwd), ld_fwd, _ptr(w_dgrad), _stream()),
              "sm3_weight_prep")


def weight_prep_table(items, device):
    """items: list of (w_master fp32, w_fwd or None, w_dgrad or None, Co, taps, Ci, ld_fwd).  Returns the device
    table (keep it alive, together with the tensors it points to) for weight_prep_batch."""
    arr = (_lib.WPrepItem * len(items))()
    total = 0
    for a, (w, wf, wd, Co, taps, Ci, ld) in zip(arr, items):
        _chk(w, torch.float32, "w")
        if w.numel() != Co * taps * Ci or (wf is not None and wf.numel() != Co * ld) or \
                (wd is not None and wd.numel() != Co * taps * Ci) or ld < taps * Ci:
            raise ValueError("weight_prep_table: size mismatch")
        a.w, a.w_fwd, a.w_dgrad = w.data_ptr(), (wf.data_ptr() if wf is not None else None), \
            (wd.data_ptr() if wd is not None else None)
        a.Co, a.taps, a.Ci, a.ld_fwd = Co, taps, Ci, ld
        total += w.numel()
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device), len(items), total


def weight_prep_batch(dtype, table, only_if=None):
    """only_if: optional 1-element int32 device tensor; the launch does nothing when it holds 0 (see weights_changed)."""
    dev_table, n, total = table
    _chk(dev_table, torch.uint8, "table"); _chk(only_if, torch.int32, "only_if")
    with _prof("weight_prep", 0.0, total * (4.0 + 2 * _sz(dtype))):
        check(_lib.load().sm3_weight_prep_batch_if(dtype, _ptr(dev_table), n, _ptr(only_if), _stream()),
              "sm3_weight_prep_batch_if")


def weights_changed(flat, state, changed):
    """changed[0] = 1 iff the fp32 words of `flat` differ from those of the previous call with this `state` (2 x int64 on
    the device, zeros before the first call).  Device-side only: no host read."""
    _chk(flat, torch.float32, "flat"); _chk(state, torch.int64, "state"); _chk(changed, torch.int32, "changed")
    if state.numel() < 2 or changed.numel() < 1:
        raise ValueError("weights_changed: state needs 2 words, changed 1")
    with _prof("weights_hash", 0.0, 4.0 * flat.numel()):
        check(_lib.load().sm3_weights_changed(_ptr(flat), flat.numel(), _ptr(state), _ptr(changed), _stream()),
              "sm3_weights_changed")


def cast_from_f32(dtype, src, dst):
    _chk(src, torch.float32); _chk(dst, TORCH_DTYPE[dtype])
    if src.numel() != dst.numel():
        raise ValueError("cast: size mismatch")
    check(_lib.load().sm3_cast_from_f32(dtype, _ptr(src), _ptr(dst), src.numel(), _stream()), "sm3_cast_from_f32")


def cast_to_f32(dtype, src, dst):
    _chk(src, TORCH_DTYPE[dtype]); _chk(dst, torch.float32)
    if src.numel() != dst.numel():
        raise ValueError("cast: size mismatch")
    check(_lib.load().sm3_cast_to_f32(dtype, _ptr(src), _ptr(dst), src.numel(), _stream()), "sm3_cast_to_f32")


# ------------------------------------------------------------------------------------------
# NT-Xent
# ------------------------------------------------------------------------------------------
def ntxent_logits(z, temperature, zn, inv_norm, logits):
    for t in (z, zn, inv_norm, logits):
        _chk(t, torch.float32)
    R, D = z.shape
    if zn.numel() != R * D or inv_norm.numel() != R or logits.numel() != R * (R - 1):
        raise ValueError("ntxent_logits: size mismatch")
    check(_lib.load().sm3_ntxent_logits(_ptr(z), R, D, temperature, _ptr(zn), _ptr(inv_norm), _ptr(logits), _stream()),
          "sm3_ntxent_logits")


def ntxent_logits_bwd(dtype, dlogits, zn, inv_norm, temperature, dz):
    _chk(dlogits, torch.float32); _chk(zn, torch.float32); _chk(inv_norm, torch.float32); _chk(dz, TORCH_DTYPE[dtype])
    R, D = zn.shape
    if dlogits.numel() != R * (R - 1) or dz.numel() != R * D:
        raise ValueError("ntxent_logits_bwd: size mismatch")
    check(_lib.load().sm3_ntxent_logits_bwd(dtype, _ptr(dlogits), _ptr(zn), _ptr(inv_norm), R, D, temperature, _ptr(dz),
                                            _stream()), "sm3_ntxent_logits_bwd")


def ce_label0(logits, weight, loss, dlogits):
    _chk(logits, torch.float32); _chk(loss, torch.float32); _chk(dlogits, torch.float32)
    R, Cc = logits.shape
    if dlogits is not None and dlogits.numel() != logits.numel():
        raise ValueError("ce_label0: size mismatch")
    # per-row terms, summed in a fixed order by the library (the loss is a function of the logits bit for bit)
    terms = torch.empty(R, dtype=torch.float32, device=logits.device) if loss is not None else None
    check(_lib.load().sm3_ce_label0(_ptr(logits), R, Cc, weight, _ptr(terms), _ptr(loss), _ptr(dlogits), _stream()),
          "sm3_ce_label0")


def ntxent_workspace_floats(R, D):
    """sm3_ntxent_fused's workspace: normalised rows, inverse norms, per-row logsumexp, per-row loss terms."""
    return R * D + 3 * R


def ntxent_fused(dtype, z, temperature, weight, workspace, loss, dz, dz_scale=None):
    """dz_scale: optional 1-element fp32 device tensor multiplied into dz (dynamic loss scale of the fp16 mode)."""
    _chk(z, torch.float32); _chk(workspace, torch.float32); _chk(loss, torch.float32); _chk(dz, TORCH_DTYPE[dtype])
    _chk(dz_scale, torch.float32, "dz_scale")
    R, D = z.shape
    if workspace.numel() < ntxent_workspace_floats(R, D) or dz.numel() != R * D:
        raise ValueError("ntxent_fused: size mismatch")
    with _prof("ntxent_fused", 6.0 * R * R * D, 4.0 * R * D * 3):
        if dz_scale is None:
            check(_lib.load().sm3_ntxent_fused(dtype, _ptr(z), R, D, temperature, weight, _ptr(workspace), _ptr(loss),
                                               _ptr(dz), _stream()), "sm3_ntxent_fused")
        else:
            check(_lib.load().sm3_ntxent_fused_scaled(dtype, _ptr(z), R, D, temperature, weight, _ptr(dz_scale),
                                                      _ptr(workspace), _ptr(loss), _ptr(dz), _stream()),
                  "sm3_ntxent_fused_scaled")


def ntxent_batch_workspace_floats(n, R, D):
    """Workspace of ntxent_fused_batch: n per-term blocks, each padded to a multiple of 4 floats."""
    return n * ((ntxent_workspace_floats(R, D) + 3) // 4 * 4)


def ntxent_fused_batch(dtype, zs, temperature, weights, workspace, loss, dzs, dz_scale=None):
    """The NT-Xent terms of a step (equal [R, D] fp32 projections, at most 4) in three launches instead of 3 per term
    (sm3_ntxent_fused_batch): loss and every dz bit-identical to ntxent_fused called term by term.  Returns False -- nothing
    launched -- when the shapes do not qualify (the caller then makes the per-term calls)."""
    n = len(zs)
    if not (1 <= n <= 4) or len(dzs) != n or len(weights) != n:
        return False
    R, D = zs[0].shape
    if D % 4 or D > 128 or R % 2 or any(tuple(z.shape) != (R, D) for z in zs):
        return False
    per = ntxent_batch_workspace_floats(1, R, D)
    _chk(workspace, torch.float32); _chk(loss, torch.float32); _chk(dz_scale, torch.float32, "dz_scale")
    for z, dz in zip(zs, dzs):
        _chk(z, torch.float32); _chk(dz, TORCH_DTYPE[dtype])
        if dz.numel() != R * D:
            raise ValueError("ntxent_fused_batch: dz size mismatch")
    if workspace.numel() < n * per:
        raise ValueError("ntxent_fused_batch: workspace too small")
    zp = (C.c_void_p * n)(*[z.data_ptr() for z in zs])
    dp = (C.c_void_p * n)(*[d.data_ptr() for d in dzs])
    wp = (C.c_float * n)(*[float(w) for w in weights])
    with _prof("ntxent_fused", 6.0 * n * R * R * D, 4.0 * n * R * D * 3):
        check(_lib.load().sm3_ntxent_fused_batch(dtype, n, zp, R, D, temperature, wp, _ptr(dz_scale), _ptr(workspace),
                                                 _ptr(loss), dp, _stream()), "sm3_ntxent_fused_batch")
    return True


def normalize_rows(z, zn, inv_norm):
    for t in (z, zn, inv_norm):
        _chk(t, torch.float32)
    R, D = z.shape
    if zn.numel() != R * D or inv_norm.numel() != R:
        raise ValueError("normalize_rows: size mismatch")
    check(_lib.load().sm3_normalize_rows(_ptr(z), R, D, _ptr(zn), _ptr(inv_norm), _stream()), "sm3_normalize_rows")


def ntxent_rect(S, self_offset, temperature, weight, loss, dz_scale=None):
    """Local anchors x gathered candidates: loss += weight * NT-Xent rows, S <- dloss/dS in place (sm3_ntxent_rect)."""
    _chk(S, torch.float32, "S"); _chk(loss, torch.float32, "loss"); _chk(dz_scale, torch.float32, "dz_scale")
    Rl, Rg = S.shape
    if Rl % 2 or self_offset < 0 or self_offset + Rl > Rg:
        raise ValueError("ntxent_rect: bad geometry")
    terms = torch.empty(Rl, dtype=torch.float32, device=S.device)  # per-row terms, summed in a fixed order by the library
    with _prof("ntxent_rect", 0.0, 8.0 * Rl * Rg):
        check(_lib.load().sm3_ntxent_rect(_ptr(S), Rl, Rg, self_offset, temperature, weight, _ptr(dz_scale), _ptr(terms),
                                          _ptr(loss), _stream()), "sm3_ntxent_rect")


def normalize_rows_bwd(dtype, dzn_a, dzn_b, zn, inv_norm, dz):
    _chk(dzn_a, torch.float32); _chk(dzn_b, torch.float32); _chk(zn, torch.float32); _chk(inv_norm, torch.float32)
    _chk(dz, TORCH_DTYPE[dtype])
    R, D = zn.shape
    if dzn_a.numel() != R * D or (dzn_b is not None and dzn_b.numel() != R * D) or dz.numel() != R * D or inv_norm.numel() != R:
        raise ValueError("normalize_rows_bwd: size mismatch")
    check(_lib.load().sm3_normalize_rows_bwd(dtype, _ptr(dzn_a), _ptr(dzn_b), _ptr(zn), _ptr(inv_norm), R, D, _ptr(dz),
                                             _stream()), "sm3_normalize_rows_bwd")


# ------------------------------------------------------------------------------------------
# optimizer
# ------------------------------------------------------------------------------------------
def adamw(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, found_inf=None):
    for t in (p, g, m, v):
        _chk(t, torch.float32)
        if t.numel() != p.numel():
            raise ValueError("adamw: size mismatch")
    _chk(found_inf, torch.int32)
    with _prof("adamw", 0.0, 28.0 * p.numel()):
        check(_lib.load().sm3_adamw(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay,
                                    step, grad_scale, _ptr(found_inf), _stream()), "sm3_adamw")


def adamw_dynamic(p, g, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, loss_scale, steps_taken, found_inf):
    """AdamW under device-resident dynamic loss scaling (sm3_adamw_dynamic)."""
    for t in (p, g, m, v):
        _chk(t, torch.float32)
        if t.numel() != p.numel():
            raise ValueError("adamw_dynamic: size mismatch")
    _chk(loss_scale, torch.float32); _chk(steps_taken, torch.int32); _chk(found_inf, torch.int32)
    with _prof("adamw", 0.0, 28.0 * p.numel()):
        check(_lib.load().sm3_adamw_dynamic(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps,
                                            weight_decay, grad_scale, _ptr(loss_scale), _ptr(steps_taken), _ptr(found_inf),
                                            _stream()), "sm3_adamw_dynamic")


def loss_scale_update(loss_scale, found_inf, growth_tracker, steps_taken, growth_factor=2.0, backoff_factor=0.5,
                      growth_interval=2000):
    """torch.cuda.amp.GradScaler.update() on device state (sm3_loss_scale_update)."""
    _chk(loss_scale, torch.float32); _chk(found_inf, torch.int32); _chk(growth_tracker, torch.int32)
    _chk(steps_taken, torch.int32)
    check(_lib.load().sm3_loss_scale_update(_ptr(loss_scale), _ptr(found_inf), _ptr(growth_tracker), _ptr(steps_taken),
                                            growth_factor, backoff_factor, int(growth_interval), _stream()),
          "sm3_loss_scale_update")


def ema_update(target, online, momentum):
    _chk(target, torch.float32); _chk(online, torch.float32)
    if target.numel() != online.numel():
        raise ValueError("ema_update: size mismatch")
    check(_lib.load().sm3_ema_update(_ptr(target), _ptr(online), target.numel(), float(momentum), _stream()), "sm3_ema_update")


def check_finite(g, found_inf):
    _chk(g, torch.float32); _chk(found_inf, torch.int32)
    check(_lib.load().sm3_check_finite(_ptr(g), g.numel(), _ptr(found_inf), _stream()), "sm3_check_finite")


# ------------------------------------------------------------------------------------------
# multi-label heads (inference model)
# ------------------------------------------------------------------------------------------
def token_attention(dtype, qkv, out, B, S, D, nhead):
    tdt = TORCH_DTYPE[dtype]
    _chk(qkv, tdt, "qkv"); _chk(out, tdt, "out")
    if qkv.numel() != B * S * 3 * D or out.numel() != B * S * D:
        raise ValueError("token_attention: size mismatch")
    if S > 8 or nhead < 1 or nhead > 8 or D % nhead:
        raise ValueError("token_attention: at most 8 tokens / 8 heads, D divisible by nhead")
    check(_lib.load().sm3_token_attention(dtype, _ptr(qkv), _ptr(out), B, S, D, nhead, _stream()), "sm3_token_attention")


def add_layernorm(dtype, a, b, gamma, beta, eps, out, rows, D):
    tdt = TORCH_DTYPE[dtype]
    _chk(a, tdt, "a"); _chk(b, tdt, "b"); _chk(out, tdt, "out"); _chk(gamma, torch.float32); _chk(beta, torch.float32)
    if a.numel() != rows * D or out.numel() != rows * D or (b is not None and b.numel() != rows * D):
        raise ValueError("add_layernorm: size mismatch")
    if gamma.numel() != D or beta.numel() != D or D > 1024:
        raise ValueError("add_layernorm: gamma/beta must have D <= 1024 entries")
    check(_lib.load().sm3_add_layernorm(dtype, _ptr(a), _ptr(b), _ptr(gamma), _ptr(beta), float(eps), _ptr(out), rows, D,
                                        _stream()), "sm3_add_layernorm")


def token_heads(dtype, x, W, bias, token_of, l2_norm, out, B, S, D, T):
    _chk(x, TORCH_DTYPE[dtype], "x"); _chk(W, torch.float32, "W"); _chk(bias, torch.float32, "bias")
    _chk(token_of, torch.int32, "token_of"); _chk(out, torch.float32, "out")
    if x.numel() != B * S * D or W.numel() != T * D or bias.numel() != T or token_of.numel() != T or out.numel() != B * T:
        raise ValueError("token_heads: size mismatch")
    if S > 8:
        raise ValueError("token_heads: at most 8 tokens")
    check(_lib.load().sm3_token_heads(dtype, _ptr(x), _ptr(W), _ptr(bias), _ptr(token_of), int(bool(l2_norm)), _ptr(out),
                                      B, S, D, T, _stream()), "sm3_token_heads")


# ------------------------------------------------------------------------------------------
# weighted k-nearest-neighbour vote (KNNOnlineEvaluator, sm3hip/knn.py)
# ------------------------------------------------------------------------------------------
KNN_MAX_K, KNN_MAX_LABELS, KNN_MAX_CLASSES = 1024, 16, 256


def knn_vote(S, n_valid, targets, class_offsets, k, temperature, scores, nbr_idx=None, nbr_sim=None):
    """scores[b, off[l] + c] = sum of exp(s / T) over the k largest S[b, :n_valid] whose neighbour has class c for label l
    (sm3_knn_vote); nbr_idx / nbr_sim [B, k] (optional): the neighbours in rank order, equal similarities lower index
    first.  targets [N, L] int32, class_offsets: L + 1 host ints."""
    if S.dim() != 2 or targets.dim() != 2 or scores.dim() != 2:
        raise ValueError("knn_vote: S [B, ld], targets [N, L] and scores [B, sum C] are 2-D")
    B, ld = S.shape
    N, L = targets.shape
    offs = [int(o) for o in class_offsets]
    if not 1 <= L <= KNN_MAX_LABELS:
        raise ValueError(f"knn_vote: {L} labels, 1 to {KNN_MAX_LABELS} supported")
    if len(offs) != L + 1 or offs[0] != 0 or any(b <= a for a, b in zip(offs, offs[1:])):
        raise ValueError("knn_vote: class_offsets must be L + 1 increasing ints from 0")
    if offs[-1] > KNN_MAX_CLASSES:
        raise ValueError(f"knn_vote: {offs[-1]} classes over all labels, at most {KNN_MAX_CLASSES}")
    if not 1 <= n_valid <= ld or N != n_valid or max(B, ld) > 0x7fffffff:
        raise ValueError(f"knn_vote: {n_valid} valid columns of S [{B}, {ld}] against {N} targets")
    if not 1 <= k <= min(n_valid, KNN_MAX_K):
        raise ValueError(f"knn_vote: k = {k} outside [1, min(N = {n_valid}, {KNN_MAX_K})]")
    if not temperature > 0 or temperature == float("inf"):
        raise ValueError("knn_vote: temperature must be positive and finite")
    if tuple(scores.shape) != (B, offs[-1]):
        raise ValueError(f"knn_vote: scores must be [{B}, {offs[-1]}]")
    for t, n in ((nbr_idx, "nbr_idx"), (nbr_sim, "nbr_sim")):
        if t is not None and tuple(t.shape) != (B, k):
            raise ValueError(f"knn_vote: {n} must be [{B}, {k}]")
    _chk(S, torch.float32, "S"); _chk(targets, torch.int32, "targets"); _chk(scores, torch.float32, "scores")
    _chk(nbr_idx, torch.int32, "nbr_idx"); _chk(nbr_sim, torch.float32, "nbr_sim")
    off = (C.c_int32 * (L + 1))(*offs)
    with _prof("knn_vote", 0.0, 4.0 * 4 * B * n_valid):  # bytes: the 4 select passes over S
        check(_lib.load().sm3_knn_vote(_ptr(S), B, n_valid, ld, _ptr(targets), L, off, int(k), float(temperature),
                                       _ptr(scores), _ptr(nbr_idx), _ptr(nbr_sim), _stream()), "sm3_knn_vote")


# ------------------------------------------------------------------------------------------
# test-time augmentation of the predictions (sm3hip/tta.py, csrc/tta.hip)
# ------------------------------------------------------------------------------------------
TTA_MAX_VIEWS = 64  # one wave of sm3_tta_reduce: lane = view
TTA_COLUMNS = 24    # sum(metrics.NUM_CLASSES)


def tta_dihedral(x, elements, out):
    """out [rows, G, 3, H, W] fp32 = the G dihedral copies elements[e] (0 .. 7: fx | fy << 1 | tr << 2) of x [rows, 3, H, W]
    (sm3_tta_dihedral): transpose if tr, then reverse the rows if fy, then the columns if fx.  Refused before the device is
    touched: an element outside 0 .. 7, more than 8 of them, a transposing element with H != W."""
    els = [int(g) for g in elements]
    if not 1 <= len(els) <= 8 or any(not 0 <= g <= 7 for g in els):
        raise ValueError(f"tta_dihedral: 1 to 8 elements in 0 .. 7, got {els}")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError("tta_dihedral: x must be [rows >= 1, 3, H, W]")
    rows, _, H, W = x.shape
    if H != W and any(g & 4 for g in els):
        raise ValueError(f"tta_dihedral: a transposing element needs a square image, got {H} x {W}")
    _chk(x, torch.float32, "x"); _chk(out, torch.float32, "out")
    if tuple(out.shape) != (rows, len(els), 3, H, W):
        raise ValueError(f"tta_dihedral: out must be [{rows}, {len(els)}, 3, {H}, {W}]")
    arr = (C.c_int * len(els))(*els)
    with _prof("tta_dihedral", 0.0, 4.0 * (x.numel() + out.numel())):
        check(_lib.load().sm3_tta_dihedral(_ptr(x), rows, H, W, arr, len(els), _ptr(out), _stream()), "sm3_tta_dihedral")


def tta_reduce(logits, q, sum_q, min_q, max_q, view_class, agg_class, disagree, preds):
    """The view reduction of logits [B, V, 24] fp32 (sm3_tta_reduce): q [B, V, 24], sum_q / min_q / max_q [B, 24] int64;
    view_class [B, V, 8], agg_class / disagree [B, 8] int32; preds [B, 24] fp32."""
    if logits.dim() != 3 or logits.shape[0] < 1 or logits.shape[2] != TTA_COLUMNS or not 1 <= logits.shape[1] <= TTA_MAX_VIEWS:
        raise ValueError(f"tta_reduce: logits must be [B >= 1, 1 <= V <= {TTA_MAX_VIEWS}, {TTA_COLUMNS}]")
    B, V, K = logits.shape
    _chk(logits, torch.float32, "logits"); _chk(preds, torch.float32, "preds")
    for t, name, shape, dt in ((q, "q", (B, V, K), torch.int64), (sum_q, "sum_q", (B, K), torch.int64),
                               (min_q, "min_q", (B, K), torch.int64), (max_q, "max_q", (B, K), torch.int64),
                               (view_class, "view_class", (B, V, 8), torch.int32), (agg_class, "agg_class", (B, 8), torch.int32),
                               (disagree, "disagree", (B, 8), torch.int32), (preds, "preds", (B, K), torch.float32)):
        _chk(t, dt, name)
        if tuple(t.shape) != shape:
            raise ValueError(f"tta_reduce: {name} must be {list(shape)}")
    with _prof("tta_reduce", 0.0, 4.0 * logits.numel() + 8.0 * q.numel()):
        check(_lib.load().sm3_tta_reduce(_ptr(logits), B, V, _ptr(q), _ptr(sum_q), _ptr(min_q), _ptr(max_q), _ptr(view_class),
                                         _ptr(agg_class), _ptr(disagree), _ptr(preds), _stream()), "sm3_tta_reduce")


# ------------------------------------------------------------------------------------------
# image corruptions of the robustness report (sm3hip/corrupt.py, csrc/corrupt.hip)
# ------------------------------------------------------------------------------------------
def _corrupt_images(x, out, who):
    if x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1:
        raise ValueError(f"{who}: x must be [B >= 1, 3, H >= 1, W >= 1]")
    _chk(x, torch.float32, "x"); _chk(out, torch.float32, "out")
    if out.shape != x.shape or out.data_ptr() == x.data_ptr():
        raise ValueError(f"{who}: out must be another tensor of x's shape")
    return x.shape[0], x.shape[2], x.shape[3]


def corrupt_pointwise(x, ids, op, severity, param, seed, modality, out):
    """gaussian_noise (op 0, param sigma), impulse_noise (op 1, param T = int(p * 2^31)) or colour_cast (op 10, param c) of
    x [B, 3, H, W] fp32 in [0, 1] (sm3_corrupt_pointwise); ids: int32 [B] on the GPU, the cases' positions in their split."""
    B, H, W = _corrupt_images(x, out, "corrupt_pointwise")
    _chk(ids, torch.int32, "ids")
    if ids.numel() != B:
        raise ValueError("corrupt_pointwise: ids must be int32 [B]")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("corrupt_pointwise: seed must fit 64 bits")
    with _prof("corrupt_pointwise", 2.0 * x.numel(), 8.0 * x.numel()):
        check(_lib.load().sm3_corrupt_pointwise(_ptr(x), B, H, W, _ptr(ids), op, severity, float(param), seed, modality, _ptr(out),
                                                _stream()), "sm3_corrupt_pointwise")


def corrupt_taps(x, tables, counts, table_index, out):
    """The mean of x over a tap table per case (sm3_corrupt_taps): tables int16 [n_tables, max_taps, 2] (dy, dx), counts int32
    [n_tables], table_index int32 [B], numpy arrays on the host."""
    B, H, W = _corrupt_images(x, out, "corrupt_taps")
    tables, counts = np.ascontiguousarray(tables, dtype=np.int16), np.ascontiguousarray(counts, dtype=np.int32)
    table_index = np.ascontiguousarray(table_index, dtype=np.int32)
    if tables.ndim != 3 or tables.shape[2] != 2 or counts.shape != tables.shape[:1] or table_index.shape != (B,):
        raise ValueError("corrupt_taps: tables [n_tables, max_taps, 2], counts [n_tables], table_index [B]")
    with _prof("corrupt_taps", float(counts.max()) * x.numel(), 8.0 * x.numel()):
        check(_lib.load().sm3_corrupt_taps(_ptr(x), B, H, W, tables.ctypes.data, counts.ctypes.data, tables.shape[0],
                                           tables.shape[1], table_index.ctypes.data, _ptr(out), _stream()), "sm3_corrupt_taps")


def corrupt_pixelate(x, f, out):
    """Every pixel of x [B, 3, H, W] -> the mean of its f x f block (sm3_corrupt_pixelate)."""
    B, H, W = _corrupt_images(x, out, "corrupt_pixelate")
    with _prof("corrupt_pixelate", 1.0 * x.numel(), 8.0 * x.numel()):
        check(_lib.load().sm3_corrupt_pixelate(_ptr(x), B, H, W, int(f), _ptr(out), _stream()), "sm3_corrupt_pixelate")


def corrupt_jpeg(x, quality, qt_luma, qt_chroma, out):
    """The integer JPEG round trip of x [B, 3, H, W] (sm3_corrupt_jpeg); qt_luma, qt_chroma: int32 [64] numpy arrays."""
    B, H, W = _corrupt_images(x, out, "corrupt_jpeg")
    ql, qc = np.ascontiguousarray(qt_luma, dtype=np.int32).reshape(-1), np.ascontiguousarray(qt_chroma, dtype=np.int32).reshape(-1)
    if ql.size != 64 or qc.size != 64:
        raise ValueError("corrupt_jpeg: two quantisation tables of 64 entries")
    with _prof("corrupt_jpeg", 0.0, 8.0 * x.numel()):
        check(_lib.load().sm3_corrupt_jpeg(_ptr(x), B, H, W, int(quality), ql.ctypes.data, qc.ctypes.data, _ptr(out), _stream()),
              "sm3_corrupt_jpeg")
