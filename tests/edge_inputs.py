"""Test helper of the edge suites (test_ntxent_edges_gpu.py, test_optimizer_edges_gpu.py, test_cast_hash_gpu.py,
test_augment_edges_gpu.py): the constructed inputs, the bounds, and fp32 restatements of the references.

Every bound of those suites is stated here once.  test_edge_refs_cpu.py runs the fp32 restatements against the fp64
references on the same inputs and holds them to a fraction of each bound, so a bound is shown to be reachable by fp32
arithmetic alone; the GPU suites hold the kernels to the full bound.  (CPU only: nothing here touches the library.)

record(): with SM3_EDGE_MEASURE=<file> every checked figure is appended to <file> as one JSON line
{"bound": name, "err": worst error, "limit": the bound}; profiles/edge_tests_measure.md is made from such a run."""
import itertools
import json
import math
import os

import numpy as np
import torch

from oracle import augment_oracle as A
from oracle import sm3_oracle as O


def record(name, err, limit):
    """-> err / limit; logs the figure when a measurement run asks for it."""
    err, limit = float(err), float(limit)
    path = os.environ.get("SM3_EDGE_MEASURE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"bound": name, "err": err, "limit": limit}) + "\n")
    return err / limit if limit > 0 else (0.0 if err == 0 else math.inf)


def f32(x):
    """The fp32 value a Python float becomes when it crosses the C ABI, as a Python float."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------------
# NT-Xent
# ------------------------------------------------------------------------------------------------------------------------
NTX_SHAPES = [(2, 128), (4, 128), (6, 128), (10, 36), (62, 64), (66, 128), (130, 128), (514, 128), (10, 130), (64, 160)]
NTX_TEMPS = [0.5, 0.07, 0.01]
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}  # one rounding, relative to |ref|


def clustered(R, D, seed, K=3, row_scale=False):
    """R = 2B projections [R, D] fp32: K cluster centres, pairs at noise 0.05 around them, the two views of a pair at
    noise 0.02 around the pair (positives: cosine ~ 1, same-cluster negatives ~ 0.99).  row_scale: every row times its
    own factor from logspace(-3, 3) (the loss does not change, the gradient of a row scales by 1 / its norm).
    K is cut to B // 2 so that every cluster holds two pairs at least: an anchor without a same-cluster negative has
    P(positive) = 1 - O(exp(-1/T)), and fp32's P - 1 then carries no relative precision whatever the kernel does
    (measured on the fp32 closed form at R = 4, T = 0.07: 0.4 % of max|dz|, 40 times the bound)."""
    g = torch.Generator().manual_seed(seed)
    B = R // 2
    K = max(1, min(K, B // 2))
    centres = torch.randn(K, D, generator=g, dtype=torch.float64)
    pair = centres[torch.arange(B) % K] + 0.05 * torch.randn(B, D, generator=g, dtype=torch.float64)
    z = torch.cat([pair + 0.02 * torch.randn(B, D, generator=g, dtype=torch.float64) for _ in range(2)])
    if row_scale:
        z = z * torch.logspace(-3, 3, R, dtype=torch.float64)[torch.randperm(R, generator=g)].unsqueeze(1)
    return z.float()


def ntxent_ref(z, temperature, weight=1.0):
    """fp64 oracle on the fp32 values of z: (weight * loss, its gradient [R, D])."""
    z64 = z.double().requires_grad_(True)
    loss = weight * O.ntxent_loss_closed_form(z64, f32(temperature))
    loss.backward()
    return float(loss.detach()), z64.grad


def ntxent_f32(z, temperature, weight=1.0):
    """The closed form in fp32 (autograd in fp32 too)."""
    z32 = z.float().clone().requires_grad_(True)
    loss = weight * O.ntxent_loss_closed_form(z32, f32(temperature))
    loss.backward()
    return float(loss.detach()), z32.grad


def loss_limit(ref_loss):
    return 2e-5 * max(1.0, abs(ref_loss))


def dz_limit(ref, dtype=torch.float32):
    """Element-wise: 1e-4 * max|ref| + 1e-7, plus one rounding of a 16-bit output."""
    return 1e-4 * float(ref.abs().max()) + 1e-7 + ref.abs() * HALF_ULP[dtype]


def worst_ratio(got, ref, limit):
    """max over the elements of |got - ref| / limit (NaN or inf in got -> inf)."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref).abs() / limit).max())


def rect_loss_from_s(S, offset, temperature, weight=1.0):
    """ntxent_global_rows stated on the cosine matrix S [Rl, Rg] itself (what sm3_ntxent_rect is handed)."""
    Rl = S.shape[0]
    s = S / temperature
    idx = torch.arange(Rl)
    pos = s[idx, offset + (idx + Rl // 2) % Rl]
    mask = torch.zeros_like(s, dtype=torch.bool)
    mask[idx, offset + idx] = True
    return weight * (torch.logsumexp(s.masked_fill(mask, float("-inf")), dim=1) - pos).mean()


# ------------------------------------------------------------------------------------------------------------------------
# AdamW
# ------------------------------------------------------------------------------------------------------------------------
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-5)
REL19 = 2.0 ** -19
FLT_MIN = 2.0 ** -126  # below it fp32 has absolute, not relative, precision (and a GPU may flush): the floor of v's bound


def adamw_tuples():
    """K = 37 distinct (p, g, m, v) fp32 tuples with the edge values of each slot."""
    g = torch.Generator().manual_seed(37)
    K = 37
    p = torch.randn(K, generator=g)
    gr = torch.randn(K, generator=g) * 0.01
    m = torch.randn(K, generator=g) * 0.01
    v = torch.rand(K, generator=g) * 1e-4
    p[:4] = torch.tensor([0.0, -0.0, 1e-30, 1e30])
    gr[2:5] = torch.tensor([0.0, 1e-20, 1e4])
    gr[7:10] = torch.tensor([0.0, 1e-20, 1e4])
    v[4:9] = 0.0
    m[5:8] = 0.0
    return p, gr, m, v


def adamw_grads(n, steps, seed):
    """`steps` gradients [n] fp32: magnitudes 10^U(-8, 1) with random signs, and exact zeros, 1e-20 and 1e4 entries."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 9.0 - 8.0)
        sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
        gr = (mag * sign).float()
        gr[0::97] = 0.0
        gr[1::97] = 1e-20
        gr[2::97] = 1e4
        gr[3::97] = -1e4
        out.append(gr)
    return out


def adamw_ref_step(p, g, m, v, step, wd, grad_scale):
    """oracle.sm3_oracle.adamw_step in fp64 with the hyper-parameters the kernel is handed: they cross the C ABI as fp32,
    so the fp64 reference gets those fp32 values (0.999f is not 0.999: 1 - beta2 differs by 1.3e-5 of itself)."""
    O.adamw_step(p, g * grad_scale, m, v, step, f32(ADAM["lr"]), f32(ADAM["beta1"]), f32(ADAM["beta2"]), f32(ADAM["eps"]),
                 f32(wd))


def adamw_f32_step(p, g, m, v, step, wd, grad_scale):
    """The kernel's formula in torch fp32 (bias corrections in double, handed over as fp32)."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    lr, b1, b2, eps, wdf = (t(ADAM["lr"]), t(ADAM["beta1"]), t(ADAM["beta2"]), t(ADAM["eps"]), t(wd))
    inv_bc1 = t(1.0 / (1.0 - f32(ADAM["beta1"]) ** step))
    inv_sqrt_bc2 = t(1.0 / math.sqrt(1.0 - f32(ADAM["beta2"]) ** step))
    gg = g * t(grad_scale)
    p.mul_(1.0 - lr * wdf)
    m.copy_(b1 * m + (1.0 - b1) * gg)
    v.copy_(b2 * v + (1.0 - b2) * gg * gg)
    denom = v.sqrt() * inv_sqrt_bc2 + eps
    p.sub_(lr * inv_bc1 * (m / denom))


def adamw_ratios(tag, p, m, v, pr, mr, vr, gsum):
    """Worst error / bound of p, m, v against fp64 (pr, mr, vr); gsum = sum_k |grad_scale * g_k| per element."""
    p, m, v = p.double(), m.double(), v.double()
    assert bool(torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all())
    rp = ((p - pr).abs() / (2e-6 + 1e-5 * pr.abs())).max()
    rv = ((v - vr).abs() / (REL19 * vr + FLT_MIN)).max()
    rm = ((m - mr).abs() / (REL19 * gsum + FLT_MIN)).max()
    return (record(f"adamw p ({tag})", rp, 1.0), record(f"adamw m ({tag})", rm, 1.0), record(f"adamw v ({tag})", rv, 1.0))


# ------------------------------------------------------------------------------------------------------------------------
# augmentation
# ------------------------------------------------------------------------------------------------------------------------
AUG_SIZES = [(61, 54), (7, 9), (33, 31), (25, 41)]
AUG_FACTORS = {1: [0.0, 0.2, 0.7, 1.0, 1.8], 2: [0.0, 0.2, 0.7, 1.0, 1.8], 3: [0.0, 0.2, 0.7, 1.0, 1.8],
               4: [-0.5, -0.2, -1.0 / 6, -1e-4, 0.0, 1e-4, 1.0 / 6, 0.2, 1.0 / 3, 0.5]}
AUG_OP_LIMIT, AUG_CHAIN_LIMIT, AUG_MEAN_LIMIT, AUG_FINISH_LIMIT = 1e-5, 2e-5, 2e-7, 5e-5
MEAN, STD = (0.7833, 0.6712, 0.6026), (0.2139, 0.2472, 0.2571)  # the run's Normalize constants


def pixel_table():
    """[P, 3] fp32 in [0, 1]: the 6^3 combinations of {0, 1/255, 127/255, 128/255, 254/255, 1} (cube corners, grey ramps, every
    channel tie), near-ties (a, a - e, a - 2e) in all arrangements, 3000 random pixels."""
    lv = torch.tensor([0.0, 1.0, 127.0, 128.0, 254.0, 255.0]) / 255.0
    rows = [torch.stack(c) for c in itertools.product(lv, repeat=3)]
    for a in (1.0, 0.75, 0.5, 0.3, 0.01):
        for e in (0.0, 2.0 ** -24, 2.0 ** -20, 1e-3):
            tri = torch.tensor([a, a - e, a - 2 * e], dtype=torch.float64).float()
            rows += [tri[list(perm)] for perm in itertools.permutations(range(3))]
    rnd = torch.rand(3000, 3, generator=torch.Generator().manual_seed(3000))
    return torch.cat([torch.stack(rows), rnd]).clamp(0, 1).contiguous()


def table_images(H, W, B=None, seed=0):
    """[B, 3, H, W] fp32 images whose pixels are the table's in a seeded order; B defaults to what holds every pixel once."""
    tab = pixel_table()
    P = tab.shape[0]
    if B is None:
        B = -(-P // (H * W))
    n = B * H * W
    perm = torch.cat([torch.randperm(P, generator=torch.Generator().manual_seed(seed + k)) for k in range(-(-n // P))])[:n]
    return tab[perm].view(B, H, W, 3).permute(0, 3, 1, 2).contiguous()


def color_ref(img, op, f, dtype=torch.float64):
    """oracle color_op on every image of [B, 3, H, W] in `dtype` (fp64: the reference; fp32: its restatement)."""
    x = img.to(dtype)
    return torch.stack([A.color_op(x[b], int(op), f32(f)) for b in range(x.shape[0])])


def draw_chains(B, seed):
    """ColorJitter.get_params B times: a random order of the four ops, factors U(0.2, 1.8) / hue U(-0.2, 0.2).
    -> ops int32 [4, B], factors fp32 [4, B]"""
    g = torch.Generator().manual_seed(seed)
    ops = torch.zeros(4, B, dtype=torch.int32)
    fac = torch.ones(4, B, dtype=torch.float32)
    for b in range(B):
        order = torch.randperm(4, generator=g)
        f = torch.cat([torch.empty(3).uniform_(0.2, 1.8, generator=g), torch.empty(1).uniform_(-0.2, 0.2, generator=g)])
        for pos in range(4):
            ops[pos, b] = int(order[pos]) + 1
            fac[pos, b] = f[int(order[pos])]
    return ops, fac


def chain_ref(img, ops, fac, dtype=torch.float64):
    x = img.to(dtype)
    out = []
    for b in range(x.shape[0]):
        y = x[b]
        for pos in range(4):
            y = A.color_op(y, int(ops[pos, b]), float(fac[pos, b]))
        out.append(y)
    return torch.stack(out)


def finish_ref(img, gray, sigma, mean, std):
    """RandomGrayscale -> GaussianBlur -> Normalize of the oracle (fp64) per sample of [B, 3, H, W]."""
    x = img.double()
    m = torch.tensor([f32(v) for v in mean], dtype=torch.float64).view(3, 1, 1)
    s = torch.tensor([f32(v) for v in std], dtype=torch.float64).view(3, 1, 1)
    out = []
    for b in range(x.shape[0]):
        y = x[b]
        if int(gray[b]):
            y = A.gray(y).unsqueeze(0).expand(3, -1, -1)
        if float(sigma[b]) > 0:
            y = A.blur3(y.contiguous(), float(sigma[b]))
        out.append((y - m) / s)
    return torch.stack(out)
