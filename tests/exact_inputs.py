"""Test helper: exact-input generation and the checks of the bit-exact kernel suites (test_exact_gemm_gpu.py,
test_exact_bn_gpu.py, test_exact_stem_dgrad_gpu.py).

Every operand is a small integer times a power of two.  A product of such operands is exact in fp32, and so is every
partial sum whose magnitude stays below 2^24 quanta, whatever the summation order.  need_exact / need_repr assert those
preconditions in fp64 on the CPU; Guarded, same and env are what the GPU tests compare and launch with."""
import contextlib
import os

import torch

Q24 = float(1 << 24)
SENTINEL = 0xA5


# ------------------------------------------------------------------------------------------------------------------------
# exact-input generator and its preconditions (CPU only)
# ------------------------------------------------------------------------------------------------------------------------
def draw(gen, shape, amp, density, exp=0):
    """Integers in [-amp, amp], nonzero with probability `density`, times 2^exp (fp64)."""
    mag = torch.randint(1, amp + 1, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    keep = torch.rand(shape, generator=gen) < density
    return (mag * sign * keep).double() * 2.0 ** exp


def quantum(*ts):
    """Largest power of two that divides every element (1 for all-zero input)."""
    q = None
    for t in ts:
        nz = t[t != 0].abs().double()
        if nz.numel() == 0:
            continue
        m, e = torch.frexp(nz)
        mi = (m * 2.0 ** 53).long()
        low = (mi & -mi).double() * torch.pow(2.0, (e - 53).double())
        v = float(low.min())
        q = v if q is None else min(q, v)
    return 1.0 if q is None else q


def need_exact(abs_sum, q, what):
    """abs_sum: sum of |terms| of an fp32 accumulation (any order), every term a multiple of q."""
    worst = float(abs_sum.max()) / q if abs_sum.numel() else 0.0
    assert worst < Q24, f"{what}: worst-case partial sum is {worst:.0f} quanta (>= 2^24): not exact in fp32"


def need_repr(t, dt, what):
    assert torch.equal(t.to(dt).double(), t), f"{what}: not representable in {dt}"


def need_f32(t, what):
    """Every element of the fp64 tensor t is an fp32 value: the fp32 operation that produces it is exact."""
    assert bool(torch.isfinite(t).all()) and torch.equal(t.float().double(), t), f"{what}: not exact in fp32"


def ep_affine_exact(gamma, beta, rm, rv, eps, what):
    """ep_affine (csrc/conv_common.h) step by step in fp64, every intermediate asserted to be an fp32 value (so that the fp32
    operation that produces it is exact, contracted into an fma or not): rv + eps, its square root, the reciprocal,
    g * invstd, rm * g, that times invstd, and the subtraction.  gamma / beta None: 1 / 0.  -> (scale, shift), fp64."""
    var = rv + eps
    need_f32(var, f"{what}: rv + eps")
    sd = var.sqrt()
    need_f32(sd, f"{what}: sqrt(rv + eps)")
    assert torch.equal(sd * sd, var), f"{what}: sqrt(rv + eps) is not exact"
    invstd = 1.0 / sd
    need_f32(invstd, f"{what}: 1 / sqrt(rv + eps)")
    assert torch.equal(invstd * sd, torch.ones_like(sd)), f"{what}: the reciprocal is not exact"
    g = torch.ones_like(rv) if gamma is None else gamma
    b = torch.zeros_like(rv) if beta is None else beta
    for t, nm in ((g, "gamma"), (b, "beta"), (rm, "running_mean"), (rv, "running_var")):
        need_f32(t, f"{what}: {nm}")
    scale = g * invstd
    need_f32(scale, f"{what}: g * invstd")
    t = rm * g
    need_f32(t, f"{what}: rm * g")
    t = t * invstd
    need_f32(t, f"{what}: rm * g * invstd")
    shift = b - t
    need_f32(shift, f"{what}: b - rm * g * invstd")
    return scale, shift


def need_exact64(abs_sum, q, what):
    """need_exact for an fp64 accumulation: below 2^53 quanta."""
    worst = float(abs_sum.max()) / q if abs_sum.numel() else 0.0
    assert worst < 2.0 ** 53, f"{what}: worst-case partial sum is {worst:.0f} quanta (>= 2^53): not exact in fp64"


def stored(v, dt):
    """What a store of the fp64 value v in dt holds (one rounding, nearest even), as fp64."""
    return v.to(dt).double()


def pick(gen, vals, shape):
    """Elements of the 1-D tensor vals drawn uniformly."""
    return vals[torch.randint(0, len(vals), shape, generator=gen)]


def stem_wgrad_case(dt, N, H, W, views, seed):
    """Stem weight gradient with bn1's backward apply on the operand path: dw = conv2d_weight(x, dxo) with
    dxo = gamma * invstd * (dz - gs0 / count - xhat * gs1 / count), xhat = (xo - mean) * invstd, per view.  Dyadic inputs and a
    power-of-two count keep dxo exact in fp32 and representable in dt (the kernel rounds it to dt before the MFMA)."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M = N * Ho * Wo
    x = draw(g, (N, 3, H, W), 3, 0.6, -1)
    dz = draw(g, (M, 64), 3, 0.6, 0)
    xo = draw(g, (M, 64), 2, 0.9, 0)
    mean = draw(g, (views, 64), 1, 0.8, -1)
    invstd = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (views, 64), generator=g)].double()
    gamma = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (64,), generator=g)].double()
    count = 1024.0
    gs = torch.cat([draw(g, (views, 64), 2, 0.8, -1), draw(g, (views, 64), 1, 0.8, -1)], 1) * count
    ls = draw(g, (views, 128), 9, 0.9, 0)
    v = torch.arange(M) // (M // views)
    xh = (xo - mean[v]) * invstd[v]
    dxo = gamma * invstd[v] * (dz - gs[v, :64] / count - xh * gs[v, 64:] / count)
    need_repr(dxo, dt, "stem dxo")
    dxo_n = dxo.reshape(N, Ho, Wo, 64).permute(0, 3, 1, 2)
    dw = torch.nn.grad.conv2d_weight(x, (64, 3, 7, 7), dxo_n, stride=2, padding=3).permute(0, 2, 3, 1).reshape(64, 147)
    dwa = torch.nn.grad.conv2d_weight(x.abs(), (64, 3, 7, 7), dxo_n.abs(), stride=2, padding=3)
    need_exact(dwa, quantum(x) * quantum(dxo), "stem dw")
    for t, nm in ((dz, "dz"), (xo, "xo")):
        need_repr(t, dt, f"stem {nm}")
    return dict(x=x, dz=dz, xo=xo, mean=mean, invstd=invstd, gamma=gamma, count=count, gs=gs, ls=ls, dw=dw,
                dgamma=ls[:, 64:].sum(0), dbeta=ls[:, :64].sum(0))


# ------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


class Guarded:
    """A contiguous slice of a sentinel-filled buffer; guards() is True when the bytes around it are unchanged."""
    PAD = 512  # bytes either side (keeps the slice 16-byte aligned)

    def __init__(self, n, dtype, fill=None):
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.g = self.PAD // self.es
        self.buf = torch.empty(n + 2 * self.g, dtype=dtype, device=_dev())
        self.buf.view(torch.uint8).fill_(SENTINEL)
        self.t = self.buf[self.g:self.g + n]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def guards(self):
        b = self.buf.view(torch.uint8)
        return bool((b[:self.PAD] == SENTINEL).all()) and bool((b[-self.PAD:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf.view(torch.uint8) == SENTINEL).all())


@contextlib.contextmanager
def env(settings):
    old = {k: os.environ.get(k) for k in settings}
    try:
        for k, v in settings.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(got, ref, what):
    """Value equality in fp64 (+0 == -0), both on the GPU."""
    a = got.reshape(-1).double()
    b = ref.reshape(-1).to(_dev()).double()
    eq = (a == b) | (torch.isnan(a) & torch.isnan(b))
    if not bool(eq.all()):
        bad = (~eq).nonzero()[:, 0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} differ; first at {i}: got {float(a[i])!r}, "
                             f"want {float(b[i])!r}")


def mask_bytes(bits, epc):
    """ReLU bits [.., C] -> one byte per `epc` consecutive elements, element e in bit e."""
    b = bits.reshape(-1, epc).to(torch.int64)
    return (b << torch.arange(epc)).sum(1).to(torch.uint8)
