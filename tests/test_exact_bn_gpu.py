"""Bit-exact checks of the BatchNorm row walks (csrc/bn.hip), the pooling kernels and the stem's fused BN + ReLU + max-pool
pair (csrc/pool.hip) and the slab reductions of BatchNorm by linearity (csrc/linbn.hip), on integer inputs.

The method is test_exact_gemm_gpu.py's: every operand is a small integer times a power of two, and the generators below
check in fp64 that every fp32 operation a kernel performs is exact (the exact result of each step is an fp32 value) and
that every sum stays under 2^24 quanta.  Then every launch must return exactly torch's rounding of the fp64 result:
  representable: every stored value is exact in the storage type T;
  rounding:      the stored value equals ref_fp64.to(T) (nearest even), f16 overflow to +-inf and underflow to 0 included.
Kernels that evaluate the same expression (x * scale + shift) are compared bit for bit only where that expression is exact
in fp32, so whether the compiler contracts it into an FMA is not part of the contract.

Contracts pinned besides the values: a ReLU bit is `stored y > 0` (in f16, 0 < v <= 2^-25 stores +0 and its bit is 0); the
partial rows of a reduction are exactly as many as the *_rows / *_partial_rows entry points say and the bytes around them
stay untouched; the fp64 statistics of integer partials are the exact totals; a rejected launch writes nothing.  Every output
is a slice of a sentinel-filled buffer, and outputs are compared with +0 and -0 identified.

The row-walk knobs (SM3_BN_UNROLL[_ACT|_RED|_APP], SM3_BN_NT, SM3_BN_GRID_CAP) are read once per process:
test_row_walk_knobs_in_child_processes reruns the row-walk tests in a fresh process per setting.
"""
import ctypes
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from exact_inputs import Guarded, _dev, draw, mask_bytes, need_exact, need_repr, same

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IDS = ["f32", "bf16", "f16"]
E = {F32: 4, BF16: 8, F16: 8}   # elements per 16-byte vector = per ReLU-mask byte
LAUNCHES = [0]
CHILD_MARK = "SM3_EXACT_BN_CHILD"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------
# CPU helpers: exactness, the row cut of the walks
# ------------------------------------------------------------------------------------------------------------------------
def f32_exact(t, what):
    """Every element of the fp64 tensor t is an fp32 value (the fp32 step that produces it is exact); +-inf allowed."""
    fin = torch.isfinite(t)
    assert torch.equal(t[fin].float().double(), t[fin]), f"{what}: not exact in fp32"


def col_quantum(t):
    """[R, C] -> per-column largest power of two dividing every finite nonzero element (1 for none)."""
    a = t.abs()
    nz = (a != 0) & torch.isfinite(a)
    m, e = torch.frexp(torch.where(nz, a, torch.ones_like(a)))
    mi = (m * 2.0 ** 53).long()
    low = (mi & -mi).double() * torch.pow(2.0, (e - 53).double())
    low = torch.where(nz, low, torch.full_like(low, math.inf))
    q = low.min(0).values
    return torch.where(torch.isinf(q), torch.ones_like(q), q)


def need_exact_cols(terms, groups, ngroups, what):
    """Sums of the rows of terms [R, C] by group (any order inside a group) are exact in fp32."""
    a = terms.abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    s = torch.zeros(ngroups, terms.shape[1], dtype=torch.float64).index_add_(0, groups, a)
    need_exact((s / col_quantum(terms)).reshape(-1), 1.0, what)


def env_int(name, dflt):
    v = os.environ.get(name)
    return int(v) if v else dflt


def walk(rows, cvecs, views=1, max_gy=8192):
    """bn.hip make_walk: (tbx, tby, gx, gy)."""
    tbx = 256 if cvecs >= 256 else cvecs
    tby = max(1, 256 // tbx)
    gx = (cvecs + tbx - 1) // tbx
    gy = (rows + tby * 8 - 1) // (tby * 8)
    cap = env_int("SM3_BN_GRID_CAP", 768) // (gx * views)
    gy = max(1, min(gy, cap if cap > 0 else 1, max_gy))
    return tbx, tby, gx, gy


def row_block(rows, tby, gy):
    """Block (blockIdx.y) that walks each row: rows r, r + gy*tby, ... belong to block (r mod gy*tby) // tby."""
    return (torch.arange(rows) % (gy * tby)) // tby


def block_sums(t, blk, gy):
    return torch.zeros(gy, t.shape[1], dtype=torch.float64).index_add_(0, blk, t)


def stem_tby(cvecs):
    tbx = 1
    while tbx < cvecs and tbx < 256:
        tbx <<= 1
    return 256 // tbx


def ulp32(t):
    """fp32 ulp at |t| (fp64 tensor)."""
    a = t.abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(a)
    return torch.pow(2.0, (e - 24).double())


def ulp_t(t, dt):
    a = t.abs().clamp_min({F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -14}[dt])
    _, e = torch.frexp(a)
    return torch.pow(2.0, (e - {F32: 24, BF16: 8, F16: 11}[dt]).double())


POW2 = torch.tensor([0.25, 0.5, 1.0, 2.0, -0.5, -1.0, -2.0], dtype=torch.float64)


def pick(g, vals, shape):
    return vals[torch.randint(0, len(vals), shape, generator=g)]


# ------------------------------------------------------------------------------------------------------------------------
# statistics: sm3_bn_stats_reduce / sm3_bn_finalize
# ------------------------------------------------------------------------------------------------------------------------
STATS_ROWS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 2047, 2048, 4097]


def stats_plan():
    for rows in STATS_ROWS:
        for views in (1, 2, 3):
            yield rows, 40, views
    for C in (4, 8, 200):
        for rows in (1, 33, 65, 2047, 4097):
            yield rows, C, 1 + rows % 3
    for rows in (5, 64, 2048):
        yield rows, 2048, 2


def stats_case(rows, C, views):
    g = torch.Generator().manual_seed(rows * 7 + C * 3 + views)
    p = draw(g, (views, rows, 2, C), 1000, 0.9, 0)
    need_exact(p.abs().sum(1).reshape(-1), 1.0, "stats partials")  # fp32 inputs, fp64 sums: integers far below 2^53
    return dict(p=p, sums=p.sum(1))  # [views][2][C] exact


def finalize_case(kind, views, C, seed):
    """kind 'exact': count a power of two, eps 0, variance a power of 4, dyadic gamma / beta;
    'const': constant channels, eps 2^-16 (one of them with s2 slightly below count*mean^2: the clamp);
    'general': count 1000, eps 1e-5."""
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        count = 64.0
        mean = draw(g, (views, C), 40, 0.9, -2)
        var = torch.pow(4.0, torch.randint(-3, 4, (views, C), generator=g).double())
        eps = 0.0
    elif kind == "const":
        count = 128.0
        mean = draw(g, (views, C), 40, 0.9, -2)
        var = torch.zeros(views, C, dtype=torch.float64)
        eps = 2.0 ** -16
    else:
        count = 1000.0
        mean = torch.randn(views, C, generator=g, dtype=torch.float64)
        var = torch.rand(views, C, generator=g, dtype=torch.float64) * 4
        eps = float(np.float32(1e-5))
    s1 = mean * count
    s2 = (var + mean * mean) * count
    if kind == "const":
        s2[:, ::3] = s2[:, ::3] - s2[:, ::3].abs() * 2.0 ** -50  # fp64 variance below 0: clamped
    gamma = pick(g, torch.tensor([0.5, 1.0, 1.5, -2.0, 0.25]), (C,)).double()
    beta = draw(g, (C,), 16, 0.8, -3)
    rm0 = draw(g, (C,), 64, 0.9, -4)
    rv0 = draw(g, (C,), 64, 1.0, -4).abs()
    sums = torch.stack([s1, s2], 1)  # [views][2][C]
    m = s1 / count
    v = (s2 / count - m * m).clamp_min(0)
    invstd = 1.0 / torch.sqrt(v + eps)
    ref = dict(scale=gamma * invstd, shift=beta - m * gamma * invstd, save_mean=m, save_invstd=invstd)
    if kind in ("exact", "const"):
        for k, t in ref.items():
            f32_exact(t, f"finalize {kind} {k}")
    mom = 0.1
    rm, rv = rm0.float(), rv0.float()
    tol_m = tol_v = torch.zeros(C, dtype=torch.float64)
    for vi in range(views):  # fp64 update rounded to fp32 after each view, view 0 first
        unb = v[vi] * (count / max(count - 1.0, 1.0))
        # the kernel updates in fp32: 2 ulp of the larger term per view (the terms may cancel), carried forward
        tol_m = (1 - mom) * tol_m + 2 * ulp32((1 - mom) * rm.double().abs() + mom * m[vi].abs())
        tol_v = (1 - mom) * tol_v + 2 * ulp32((1 - mom) * rv.double().abs() + mom * unb.abs())
        rm = ((1 - mom) * rm.double() + mom * m[vi]).float()
        rv = ((1 - mom) * rv.double() + mom * unb).float()
    return dict(count=count, eps=eps, mom=mom, sums=sums, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, ref=ref,
                rm=rm.double(), rv=rv.double(), tol_m=tol_m, tol_v=tol_v)


# ------------------------------------------------------------------------------------------------------------------------
# forward row walks: sm3_bn_act / _colsum / sm3_bn_add_bn_act
# ------------------------------------------------------------------------------------------------------------------------
ACT_CVECS = [1, 3, 25, 255, 256, 257, 384]


def act_rows(cvecs):
    _, tby, _, _ = walk(1, cvecs)
    out = [1, tby - 1, tby + 1, 3 * tby + 1, 4 * tby - 1, 4 * tby + 1, 7 * tby + 3, 8 * tby - 1, 8 * tby + 1, 13 * tby + 5,
           29 * tby + 7]
    return sorted({r for r in out if r >= 1})


def act_plan(dt):
    """(rows, C, views, regime, seed)"""
    i = DTYPES.index(dt)
    for cv in ACT_CVECS:
        for j, rows in enumerate(act_rows(cv)):
            regime = "round" if (dt != F32 and j % 2) else "repr"
            yield rows, cv * E[dt], 2 if j % 3 == 0 else 1, regime, 1000 * i + 10 * cv + j
    if dt == BF16:  # the 768-block cap binds: C = 2048 from 6 144 rows, C = 64 from 196 608 rows
        yield 6144 + 768 + 5, 2048, 1, "repr", 77
        yield 196608 + 77, 64, 1, "round", 78


def act_case(dt, rows, C, views, regime, seed, residual=True, special=True):
    """x, scale, shift, residual (x2 / scale2 / shift2 of the add form), pre = the fp32-exact value before ReLU."""
    g = torch.Generator().manual_seed(seed)
    n = views * rows
    if regime == "repr":
        x = draw(g, (n, C), 8, 0.9, -2)
        sh = draw(g, (views, C), 16, 0.9, -2)
        res = draw(g, (n, C), 8, 0.7, -2)
    else:
        amp = 255 if dt == BF16 else 2047
        x = draw(g, (n, C), amp, 0.9, -4)
        sh = draw(g, (views, C), 255, 0.9, -9)
        res = draw(g, (n, C), 255, 0.7, -6)
    sc = pick(g, POW2, (views, C))
    sc2 = pick(g, POW2, (views, C))
    sh2 = draw(g, (views, C), 8, 0.9, -2)
    if dt == F16 and regime == "round" and special:
        # channel 0: overflow to +-inf; channel 1: the underflow probe v in {2^-26, 2^-25, 3 2^-26, -2^-26}
        x[:, 0] = pick(g, torch.tensor([60000.0, -60000.0, 1.0, 0.0]).double(), (n,))
        x[:, 1] = pick(g, torch.tensor([1.0, 2.0, 3.0, -1.0]).double(), (n,))
        sc[:, 0], sc[:, 1] = 2.0, 2.0 ** -26
        sh[:, :2] = 0.0
        res[:, :2] = 0.0
        sh2[:, :2] = 0.0
    vr = torch.arange(n) // rows
    xs = x * sc[vr]
    base = xs + sh[vr]
    pre = base + (res if residual else 0)
    pre2 = base + sh2[vr] + res * sc2[vr]
    for t, nm in ((xs, "x*scale"), (base, "x*scale+shift"), (pre, "pre"), (res * sc2[vr], "x2*scale2"),
                  (sh + sh2, "shift+shift2"), (xs + (sh + sh2)[vr], "x*scale+shifts"), (pre2, "pre2")):
        f32_exact(t, f"act {dt} {rows}x{C} {nm}")
    need_repr(x, dt, "act x")
    need_repr(res, dt, "act res")
    return dict(x=x, sc=sc, sh=sh, res=res, sc2=sc2, sh2=sh2, pre=pre, pre2=pre2, rows=rows, C=C, views=views, vr=vr,
                regime=regime)


def colsum_plan(dt):
    for rows, C, views, regime, seed in act_plan(dt):
        if views * rows * C <= 1 << 22:  # any cut (SM3_BN_GRID_CAP=1: one block per view) sums exactly
            yield rows, C, regime if rows <= 512 else "repr", seed + 500
    if dt == BF16:
        yield 3072 + 13, 2048, "repr", 580  # two views: the 384-block cap per view binds


def colsum_case(dt, rows, C, regime, seed):
    c = act_case(dt, rows, C, 2, regime, seed, special=False)
    c["want"] = stored(c["pre"].clamp_min(0), dt)
    need_exact_cols(c["want"], torch.arange(2 * rows) // rows, 2, "colsum")
    return c


SUB_CASES = [(2, 7, 5, 1, 2, 2), (1, 9, 9, 3, 1, 1), (4, 13, 11, 25, 2, 2), (2, 6, 8, 256, 2, 1), (3, 3, 5, 257, 1, 3),
             (2, 57, 55, 2, 2, 2)]  # N, H, W, cvecs, stride, views


def sub_case(dt, N, H, W, cv, stride, views, seed):
    C = cv * E[dt]
    g = torch.Generator().manual_seed(seed)
    x = draw(g, (N, H, W, C), 100, 0.9, -3)
    Hs, Ws = (H - 1) // stride + 1, (W - 1) // stride + 1
    sub = x[:, ::stride, ::stride].reshape(-1, C)
    need_exact_cols(sub, torch.arange(N * Hs * Ws) // (N // views * Hs * Ws), views, "subsample colsum")
    need_repr(x, dt, "subsample x")
    return dict(x=x, sub=sub, C=C, Hs=Hs, Ws=Ws, rows=N // views * Hs * Ws)


def pool_plan(dt):
    for i, (H, W) in enumerate(POOL_HW):
        yield 2, H, W, 2 * E[dt], 60 + i
        yield 1, H, W, 3 * E[dt], 160 + i


def stored(v, dt):
    """What a T store of the fp64 value v holds (nearest even), as fp64."""
    return v.to(dt).double()


# ------------------------------------------------------------------------------------------------------------------------
# backward row walks: sm3_bn_bwd_reduce / sm3_bn_bwd_apply / sm3_bn_bwd_apply2
# ------------------------------------------------------------------------------------------------------------------------
def red_plan(dt):
    i = DTYPES.index(dt)
    for cv in ACT_CVECS:
        for j, rows in enumerate(act_rows(cv)):
            yield rows, cv * E[dt], 2 if j % 3 == 1 else 1, 2000 + 1000 * i + 10 * cv + j
    yield 65536 + 64 * 3 + 5, 2 * E[dt], 1, 2999 + i   # above the 1 024-row cap
    yield 65536 * 2 + 1, E[dt], 2, 2990 + i


def red_case(dt, rows, C, views, seed):
    g = torch.Generator().manual_seed(seed)
    n = views * rows
    big = rows > 65536
    dy = draw(g, (n, C), 1 if big else 8, 0.5 if big else 0.9, 0 if big else -2)
    bits = torch.rand(n, C, generator=g) < 0.6
    y = torch.where(torch.rand(n, C, generator=g) < 0.6, draw(g, (n, C), 4, 1.0, -1).abs(), torch.zeros(n, C).double())
    y[(y == 0) & (torch.rand(n, C, generator=g) < 0.5)] = -0.0
    x = draw(g, (n, C), 4 if big else 16, 0.9, 0)
    mean = draw(g, (views, C), 8, 0.9, -2)
    invstd = pick(g, torch.tensor([0.25, 0.5, 1.0, 2.0]).double(), (views, C))
    vr = torch.arange(n) // rows
    xhat = (x - mean[vr]) * invstd[vr]
    tby = walk(rows, C // E[dt], views, 1 << 30)[1]
    gy = max(1, min(1024, (rows + 63) // 64))
    blk = row_block(rows, tby, gy)
    for dz in (torch.where(bits, dy, 0.0), torch.where(y > 0, dy, 0.0), dy):
        for vi in range(views):
            sl = slice(vi * rows, (vi + 1) * rows)
            f32_exact(dz[sl] * (x[sl] - mean[vi]), "dz*(x-mu)")
            need_exact_cols(dz[sl], blk, gy, "partial sum dz")
            need_exact_cols(dz[sl] * xhat[sl], blk, gy, "partial sum dz*xhat")
    need_repr(dy, dt, "dy")
    need_repr(x, dt, "x")
    return dict(dy=dy, bits=bits, y=y, x=x, mean=mean, invstd=invstd, xhat=xhat, rows=rows, C=C, views=views, gy=gy,
                tby=tby, blk=blk, vr=vr)


def apply_plan(dt):
    i = DTYPES.index(dt)
    for cv in ACT_CVECS:
        for j, rows in enumerate(act_rows(cv)[::2]):
            yield rows, cv * E[dt], 1 + j % 2, "exact" if j % 3 else "general", 4000 + 1000 * i + 10 * cv + j
    if dt == BF16:
        yield 6144 + 3, 2048, 1, "exact", 4999


def apply_side(g, dt, n, C, views, kind, vr):
    x = draw(g, (n, C), 16, 0.9, 0)
    mean = draw(g, (views, C), 16, 0.9, 0)
    invstd = pick(g, torch.tensor([0.25, 0.5, 1.0, 2.0]).double(), (views, C))
    gamma = pick(g, torch.tensor([0.5, 1.0, 1.5, -0.5, -2.0]).double(), (C,))
    count = 64.0 if kind == "exact" else 1000.0
    gs = torch.stack([draw(g, (views, C), 64, 0.9, -1), draw(g, (views, C), 64, 0.9, -3)], 1)  # [views][2][C]
    ls = torch.stack([draw(g, (views, C), 1 << 20, 0.9, -4), draw(g, (views, C), 1 << 20, 0.9, -6)], 1) * 1.0000001
    return dict(x=x, mean=mean, invstd=invstd, gamma=gamma, count=count, gs=gs, ls=ls,
                dg0=draw(g, (C,), 50, 1.0, 0), db0=draw(g, (C,), 50, 1.0, 0))


def apply_expect(s, dz, dt, vr, what):
    """dx = k0 (dz - k1) - (x - mu) q, k0 = gamma invstd, k1 = mean(dz), q = k0 invstd mean(dz xhat).  Returns (ref, tol)."""
    inv = 1.0 / s["count"]
    k0 = (s["gamma"] * s["invstd"])[vr]
    m1 = (s["gs"][:, 0] * inv)[vr]
    m2 = (s["gs"][:, 1] * inv)[vr]
    xm = s["x"] - s["mean"][vr]
    q = k0 * s["invstd"][vr] * m2
    ref = k0 * (dz - m1) - xm * q
    if s["count"] == 64.0:
        for t, nm in ((m1, "k1"), (q, "q"), (dz - m1, "dz-k1"), (k0 * (dz - m1), "k0(dz-k1)"), (xm * q, "(x-mu)q"),
                      (ref, "dx")):
            f32_exact(t, f"{what} {nm}")
        return ref, None
    err32 = 2.0 ** -24 * (4 * k0.abs() * (dz.abs() + m1.abs()) + 6 * (xm * q).abs() + ref.abs())
    return ref, err32 + ulp_t(ref.abs() + err32, dt)


def param_grad_expect(d0, ls, views):
    """dbeta / dgamma += the fp32 sum of the views' local sums (each rounded to fp32), in view order, in ONE add."""
    acc = np.zeros(d0.shape, dtype=np.float32)
    for v in range(views):
        acc = (acc + ls[v].numpy().astype(np.float32)).astype(np.float32)
    return torch.from_numpy((d0.numpy().astype(np.float32) + acc).astype(np.float32)).double()


def apply_case(dt, rows, C, views, kind, seed):
    g = torch.Generator().manual_seed(seed)
    n = views * rows
    vr = torch.arange(n) // rows
    dz = draw(g, (n, C), 8, 0.8, -2)
    a, b = apply_side(g, dt, n, C, views, kind, vr), apply_side(g, dt, n, C, views, kind, vr)
    for s, nm in ((a, "a"), (b, "b")):
        s["ref"], s["tol"] = apply_expect(s, dz, dt, vr, f"apply {nm}")
        s["dbeta"] = param_grad_expect(s["db0"], s["ls"][:, 0], views)
        s["dgamma"] = param_grad_expect(s["dg0"], s["ls"][:, 1], views)
        need_repr(s["x"], dt, "apply x")
    need_repr(dz, dt, "apply dz")
    return dict(dz=dz, a=a, b=b, rows=rows, C=C, views=views, kind=kind)


# ------------------------------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------------------------------
POOL_HW = [(1, 1), (1, 5), (2, 3), (3, 2), (4, 4), (5, 8), (8, 5), (3, 3), (8, 1), (5, 5), (2, 8)]
TIE_VALS = torch.tensor([-2.0, -1.0, -0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0])


def maxpool_ref(x):
    """x [N, H, W, C] fp64 -> (y, argmax in 0..8): the FIRST maximum in (kh, kw) scan order (strict >), as ATen."""
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((N, H + 2, W + 2, C), -math.inf, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    ok = torch.zeros(N, H + 2, W + 2, C, dtype=torch.bool)
    ok[:, 1:H + 1, 1:W + 1] = True
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=torch.float64)
    arg = torch.full((N, Ho, Wo, C), -1, dtype=torch.long)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
            o = ok[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
            upd = o & ((v > best) | (arg < 0))
            best = torch.where(upd, v, best)
            arg = torch.where(upd, torch.full_like(arg, kh * 3 + kw), arg)
    return best, arg


def maxpool_bwd_ref(arg, dy, H, W):
    N, Ho, Wo, C = dy.shape
    dxp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dxp[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2] += torch.where(arg == kh * 3 + kw, dy, 0.0)
    return dxp[:, 1:H + 1, 1:W + 1].contiguous()


def pool_case(dt, N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = pick(g, TIE_VALS, (N, H, W, C)).double()
    y, arg = maxpool_ref(x)
    Ho, Wo = y.shape[1:3]
    dy = draw(g, (N, Ho, Wo, C), 64, 0.9, 0)
    dx = maxpool_bwd_ref(arg, dy, H, W)
    for t in (x, dy, dx):
        need_repr(t, dt, "maxpool")
    return dict(x=x, y=y, arg=arg, dy=dy, dx=dx, N=N, H=H, W=W, C=C)


# stem pair: (N, H, W, cvecs, views, regime)
STEM_CASES = [(2, 9, 7, 1, 1, "repr"), (2, 8, 8, 3, 2, "round"), (3, 5, 11, 5, 1, "round"), (2, 12, 6, 24, 2, "repr"),
              (1, 4, 3, 256, 1, "round"), (2, 1, 1, 3, 2, "repr"), (2, 182, 182, 1, 1, "round")]  # the last: > 1 024 rows


def stem_case(dt, N, H, W, cv, views, regime, seed):
    g = torch.Generator().manual_seed(seed)
    C = cv * E[dt]
    x = draw(g, (N, H, W, C), 8, 0.9, -1)
    sc = pick(g, torch.tensor([0.5, 1.0, 2.0, -1.0]).double(), (views, C))
    sh = draw(g, (views, C), 6, 0.7, -1)
    if dt == F16:  # the underflow probe in channel 1: stored +0 where v > 0
        x[..., 1] = pick(g, torch.tensor([1.0, 2.0, 3.0, -1.0]).double(), (N, H, W))
        sc[:, 1] = 2.0 ** -26
        sh[:, 1] = 0.0
    vimg = torch.arange(N) // (N // views)
    pre = x * sc[vimg][:, None, None] + sh[vimg][:, None, None]
    f32_exact(x * sc[vimg][:, None, None], "stem x*scale")
    f32_exact(pre, "stem pre")
    act = stored(pre.clamp_min(0), dt)
    y, arg = maxpool_ref(act)
    Ho, Wo = y.shape[1:3]
    if regime == "repr":
        dy = draw(g, (N, Ho, Wo, C), 8, 0.9, -1)
    else:  # window sums that round in T (exact in fp32)
        e = {F32: -6, BF16: -6, F16: -9}[dt]
        dy = draw(g, (N, Ho, Wo, C), 7, 0.9, 0) * torch.pow(2.0, (torch.randint(0, 2, (N, Ho, Wo, C), generator=g) * e).double())
    gsum = maxpool_bwd_ref(arg, dy, H, W)
    f32_exact(gsum, "stem window sums")
    dz = torch.where(act > 0, stored(gsum, dt), 0.0)
    mean = draw(g, (views, C), 4, 0.9, 0)
    invstd = pick(g, torch.tensor([0.5, 1.0, 2.0]).double(), (views, C))
    xhat = (x - mean[vimg][:, None, None]) * invstd[vimg][:, None, None]
    rows = N // views * H * W
    gy = max(1, min(1024, (rows + 63) // 64))
    blk = row_block(rows, stem_tby(cv), gy)
    r_dz, r_t = dz.reshape(views, rows, C), (dz * xhat).reshape(views, rows, C)
    f32_exact(dz * (x - mean[vimg][:, None, None]), "stem dz*(x-mu)")
    for vi in range(views):
        need_exact_cols(r_dz[vi], blk, gy, "stem partial dz")
        need_exact_cols(r_t[vi], blk, gy, "stem partial dz*xhat")
    need_repr(dy, dt, "stem dy")
    return dict(x=x, sc=sc, sh=sh, pre=pre, act=act, y=y, arg=arg, dy=dy, gsum=gsum, dz=dz, mean=mean, invstd=invstd,
                sums=torch.stack([r_dz.sum(1), r_t.sum(1)], 1), N=N, H=H, W=W, C=C, views=views, regime=regime)


AVG_CASES = [(3, 64, 8), (2, 49, 24), (5, 49, 256), (1, 64, 2048)]  # (N, HW, cvecs)


def avg_case(dt, N, HW, cv, seed):
    g = torch.Generator().manual_seed(seed)
    C = cv * E[dt]
    x = draw(g, (N, HW, C), 60, 0.9, -2)
    s = x.sum(1)
    f32_exact(s, "avgpool sum")
    need_exact(x.abs().sum(1).reshape(-1), 0.25, "avgpool sum")
    df = draw(g, (N, C), 255 if dt == BF16 else 1000, 0.9, -3)
    need_repr(df, dt, "avgpool dfeat")
    return dict(x=x, s=s, df=df, N=N, HW=HW, C=C)


# ------------------------------------------------------------------------------------------------------------------------
# slab reductions (linbn.hip)
# ------------------------------------------------------------------------------------------------------------------------
def linbn_plan():
    for nslabs in (1, 47, 48, 49, 300):
        for views in (1, 2):
            yield nslabs, 4 * 257, views, (nslabs + views) % 2 == 0


def linbn_case(nslabs, n, views, with_colsum):
    g = torch.Generator().manual_seed(nslabs * 10 + views)
    slabs = draw(g, (views, nslabs, n), 5000, 0.9, 0)
    need_exact(slabs.abs().sum(1).reshape(-1), 1.0, "slab sum")
    p, crow = 72, 37
    cs = draw(g, (views, crow, p), 1 << 20, 0.9, -3)
    ws = draw(g, (views, 11, n), 1 << 30, 0.9, -7)
    return dict(slabs=slabs, G=slabs.sum(1), cs=cs, s=cs.sum(1), p=p, crow=crow, ws=ws, fold=ws.sum(1),
                with_colsum=with_colsum)


# ------------------------------------------------------------------------------------------------------------------------
# the CPU self-check
# ------------------------------------------------------------------------------------------------------------------------
def all_preconditions():
    n = 0
    for rows, C, views in stats_plan():
        stats_case(rows, C, views)
        n += 1
    for kind in ("exact", "const", "general"):
        for views in (1, 2, 3):
            finalize_case(kind, views, 200, 50 + views)
            n += 1
    for dt in DTYPES:
        for rows, C, views, regime, seed in act_plan(dt):
            act_case(dt, rows, C, views, regime, seed)
            n += 1
        for rows, C, views, seed in red_plan(dt):
            red_case(dt, rows, C, views, seed)
            n += 1
        for rows, C, views, kind, seed in apply_plan(dt):
            apply_case(dt, rows, C, views, kind, seed)
            n += 1
        for args in pool_plan(dt):
            pool_case(dt, *args)
            n += 1
        for args in colsum_plan(dt):
            colsum_case(dt, *args)
            n += 1
        for i, geo in enumerate(SUB_CASES):
            sub_case(dt, *geo, 300 + i)
            n += 1
        for i, geo in enumerate(STEM_CASES):
            stem_case(dt, *geo, 70 + i)
            n += 1
        for i, geo in enumerate(AVG_CASES):
            avg_case(dt, *geo, 90 + i)
            n += 1
    for args in linbn_plan():
        linbn_case(*args)
        n += 1
    return n


def test_case_table_preconditions():
    """CPU self-check: every case of the tables satisfies the exactness preconditions it is run under."""
    assert all_preconditions() > 300
    # the rounding regime really rounds, f16 overflows and underflows
    c = act_case(BF16, 100, 64, 1, "round", 5)
    assert not torch.equal(stored(c["pre"], BF16), c["pre"])
    c = act_case(F16, 100, 64, 1, "round", 6)
    y = stored(c["pre"], F16)
    assert bool(torch.isinf(y[:, 0]).any()) and bool(((c["pre"][:, 1] > 0) & (y[:, 1] == 0)).any())
    c = act_case(BF16, 100, 64, 2, "repr", 7)
    need_repr(c["pre"], BF16, "repr regime")
    assert int((c["pre"] == 0).sum()) > 50  # exact zeros exercise the strict ReLU bit
    c = stem_case(BF16, 2, 8, 8, 3, 2, "round", 71)
    assert not torch.equal(stored(c["gsum"], BF16), c["gsum"])
    c = stem_case(F16, 2, 8, 8, 3, 2, "round", 71)
    assert not torch.equal(stored(c["gsum"], F16), c["gsum"])
    c = pool_case(BF16, 2, 5, 8, 16, 1)
    assert int((c["arg"] > 0).sum()) > 20
    c = finalize_case("const", 1, 200, 3)
    assert torch.equal(c["ref"]["save_invstd"], torch.full_like(c["ref"]["save_invstd"], 256.0))
    # the cap-bound cases really reach the caps
    assert walk(6144 + 773, 256)[3] == 768 and walk(196608 + 77, 8)[3] == 768
    assert max(1, min(1024, (65536 + 64 * 3 + 5 + 63) // 64)) == 1024


# ------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------
def _g(t, dt):
    return t.to(dt).reshape(-1).to(_dev()).contiguous()


def ops():
    from sm3hip import ops as o
    return o


def lib():
    from sm3hip import _lib
    return _lib.load()


def launch(fn, *a, **k):
    LAUNCHES[0] += 1
    return fn(*a, **k)


def code(dt):
    return ops().dtype_code(dt)


def bits_equal(a, b, what):
    assert a.dtype == b.dtype and a.numel() == b.numel(), what
    ia = a.reshape(-1).view({4: torch.int32, 2: torch.int16}[a.element_size()])
    ib = b.reshape(-1).view({4: torch.int32, 2: torch.int16}[b.element_size()])
    eq = ia == ib
    if not bool(eq.all()):
        i = int((~eq).nonzero()[0, 0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {a.numel()} differ in their bits; first at {i}: "
                             f"{float(a.reshape(-1)[i])!r} vs {float(b.reshape(-1)[i])!r}")


def mask_of(bits, dt):
    return mask_bytes(bits, E[dt]).to(_dev())


# ------------------------------------------------------------------------------------------------------------------------
# statistics
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stats_reduce_sums_are_the_exact_totals_in_both_forms():
    """sm3_bn_stats_reduce with sums, and the workspace-only form folded into sm3_bn_finalize: exact totals, equal bits."""
    o = ops()
    LAUNCHES[0] = 0
    for rows, C, views in stats_plan():
        c = stats_case(rows, C, views)
        tag = f"stats rows={rows} C={C} views={views}"
        part = _g(c["p"], F32)
        sums = Guarded(views * 2 * C, torch.float64)
        launch(o.bn_stats_reduce, part, rows, C, sums.t, views=views)
        torch.cuda.synchronize()
        same(sums.t, c["sums"], tag + " sums")
        assert sums.guards(), tag + ": sums guard band written"
        # the two forms of the finalize: from the sums (groups = 1), from the stage-A workspace (groups = G)
        outs = []
        for form in ("sums", "ws"):
            if form == "sums":
                src, groups = sums.t, 1
            else:
                src, groups = launch(o.bn_stats_reduce, part, rows, C, None, views=views)
                assert groups == min(64, (rows + 31) // 32)
            r = [Guarded(views * C, F32) for _ in range(4)]
            rm, rv = _g(torch.zeros(C), F32), _g(torch.ones(C), F32)
            nbt = torch.zeros(1, dtype=torch.int64, device=_dev())
            launch(o.bn_finalize, src, float(rows * 8), C, None, None, 1e-5, 0.1, rm, rv, nbt, r[0].t, r[1].t, r[2].t,
                   r[3].t, groups=groups, views=views)
            torch.cuda.synchronize()
            outs.append([t.t.clone() for t in r] + [rm, rv])
            assert all(t.guards() for t in r), tag + f" {form}: finalize guard band written"
            assert int(nbt) == views, tag + ": num_batches_tracked"
        for a, b in zip(*outs):
            bits_equal(a, b, tag + " finalize from sums vs workspace")
    print(f"stats: {LAUNCHES[0]} launches checked")


def run_finalize(c, views, C, nulls=()):
    o = ops()
    gam = None if "gamma" in nulls else _g(c["gamma"], F32)
    bet = None if "beta" in nulls else _g(c["beta"], F32)
    rm = None if "running" in nulls else Guarded(C, F32, c["rm0"].float())
    rv = None if "running" in nulls else Guarded(C, F32, c["rv0"].float())
    nbt = torch.full((1,), 5, dtype=torch.int64, device=_dev())
    out = {k: Guarded(views * C, F32) for k in ("scale", "shift", "save_mean", "save_invstd")}
    save = not ("save" in nulls)
    launch(o.bn_finalize, _g(c["sums"], torch.float64), c["count"], C, gam, bet, c["eps"], c["mom"],
           rm.t if rm else None, rv.t if rv else None, nbt, out["scale"].t, out["shift"].t,
           out["save_mean"].t if save else None, out["save_invstd"].t if save else None, views=views)
    torch.cuda.synchronize()
    assert int(nbt) == 5 + views
    return out, rm, rv, save


@pytest.mark.gpu
def test_finalize_exact_general_and_null_forms():
    o = ops()
    LAUNCHES[0] = 0
    C = 200
    for kind in ("exact", "const", "general"):
        for views in (1, 2, 3):
            c = finalize_case(kind, views, C, 50 + views)
            tag = f"finalize {kind} views={views}"
            for nulls in ((), ("gamma",), ("beta",), ("running",), ("save",), ("gamma", "beta", "running", "save")):
                cc = dict(c)
                if "gamma" in nulls or "beta" in nulls:
                    g = torch.ones(C, dtype=torch.float64) if "gamma" in nulls else c["gamma"]
                    b = torch.zeros(C, dtype=torch.float64) if "beta" in nulls else c["beta"]
                    m, inv = c["ref"]["save_mean"], c["ref"]["save_invstd"]
                    cc["ref"] = dict(c["ref"], scale=g * inv, shift=b - m * g * inv)
                out, rm, rv, save = run_finalize(c, views, C, nulls)
                t2 = f"{tag} nulls={nulls}"
                for k in ("scale", "shift", "save_mean", "save_invstd"):
                    if k.startswith("save") and not save:
                        assert out[k].untouched(), t2 + f": {k} written with a null pointer"
                        continue
                    want = cc["ref"][k].reshape(-1)
                    if kind == "general":
                        got = out[k].t.double().cpu()
                        bad = (got - want).abs() > ulp32(want)
                        assert not bool(bad.any()), t2 + f" {k}: {int(bad.sum())} beyond 1 ulp"
                    else:
                        same(out[k].t, want, t2 + " " + k)
                    assert out[k].guards(), t2 + f": {k} guard band written"
                if rm is not None:
                    for got, want, tol, nm in ((rm, c["rm"], c["tol_m"], "running_mean"),
                                               (rv, c["rv"], c["tol_v"], "running_var")):
                        d = (got.t.double().cpu() - want).abs()
                        assert bool((d <= tol).all()), t2 + f" {nm}: max diff {float(d.max())!r}"
                        assert got.guards(), t2 + f": {nm} guard band written"
    # eval-mode scale / shift in the exact regime: running_var a power of 4, eps 0, dyadic gamma / beta / mean
    g = torch.Generator().manual_seed(9)
    rvar = torch.pow(4.0, torch.randint(-3, 4, (C,), generator=g).double())
    rmean, gam, bet = draw(g, (C,), 40, 0.9, -2), pick(g, torch.tensor([0.5, 1.0, -1.5]).double(), (C,)), draw(g, (C,), 9, 0.9, -2)
    inv = 1.0 / torch.sqrt(rvar)
    sc, sh = Guarded(C, F32), Guarded(C, F32)
    launch(o.bn_eval_scale_shift, _g(gam, F32), _g(bet, F32), _g(rmean, F32), _g(rvar, F32), 0.0, C, sc.t, sh.t)
    torch.cuda.synchronize()
    same(sc.t, gam * inv, "eval scale")
    same(sh.t, bet - rmean * gam * inv, "eval shift")
    assert sc.guards() and sh.guards()
    print(f"finalize: {LAUNCHES[0]} launches checked")


# ------------------------------------------------------------------------------------------------------------------------
# forward row walks
# ------------------------------------------------------------------------------------------------------------------------
def colsum_expect(ystored, rows, C, views, dt, gy):
    """[views][gy][C]: the block sums of the stored outputs in the view-independent cut of sm3_bn_act_colsum."""
    tby = walk(rows, C // E[dt], 2)[1]
    blk = row_block(rows, tby, gy)
    return torch.stack([block_sums(ystored[v * rows:(v + 1) * rows], blk, gy) for v in range(views)])


def check_act(y, mk, want, dt, tag, out_dt=None):
    same(y.t, want, tag + " y")
    assert y.guards(), tag + ": y guard band written"
    if mk is not None:
        assert torch.equal(mk.t, mask_of(want > 0, dt)), tag + ": mask bits != (stored y > 0)"
        assert mk.guards(), tag + ": mask guard band written"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bn_act_row_walk(dt):
    """sm3_bn_act: ReLU on / off, residual on / off, out_f32, mask, views 1 and 2, over the row-walk edge shapes."""
    o, cd = ops(), code(dt)
    LAUNCHES[0] = 0
    t0 = time.time()
    for rows, C, views, regime, seed in act_plan(dt):
        c = act_case(dt, rows, C, views, regime, seed)
        n = views * rows * C
        x, res = _g(c["x"], dt), _g(c["res"], dt)
        sc, sh = _g(c["sc"], F32), _g(c["sh"], F32)
        big = n > 1 << 22
        for relu, residual, out_f32, with_mask in ((True, True, False, True), (False, False, False, False),
                                                   (True, False, True, True), (False, True, True, False)):
            if big and not (relu and with_mask):
                continue
            if out_f32 and dt == F32:
                continue
            tag = f"bn_act {dt} rows={rows} C={C} v={views} {regime} relu={relu} res={residual} f32={out_f32}"
            pre = c["pre"] if residual else c["pre"] - c["res"]
            v = pre.clamp_min(0) if relu else pre
            want = v if out_f32 else stored(v, dt)
            y = Guarded(n, F32 if out_f32 else dt)
            mk = Guarded(n // E[dt], torch.uint8) if (relu and with_mask) else None
            launch(o.bn_act, cd, x, sc, sh, res if residual else None, relu, y.t, rows, C, out_f32=out_f32,
                   mask=mk.t if mk else None, views=views)
            torch.cuda.synchronize()
            check_act(y, mk, want, dt, tag)
    print(f"bn_act {dt}: {LAUNCHES[0]} launches checked in {time.time() - t0:.1f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bn_act_colsum_and_add_bn_act_row_walk(dt):
    """sm3_bn_act_colsum: the colsum rows are the block sums of the STORED outputs, exactly sm3_bn_act_colsum_rows of them
    per view, and a view's rows are bit-equal alone and in a 2-view launch.  sm3_bn_add_bn_act: both normalisations."""
    o, cd = ops(), code(dt)
    LAUNCHES[0] = 0
    for rows, C, regime, seed in colsum_plan(dt):
        c = colsum_case(dt, rows, C, regime, seed)
        n = 2 * rows * C
        x, res, sc, sh = _g(c["x"], dt), _g(c["res"], dt), _g(c["sc"], F32), _g(c["sh"], F32)
        gy = o.bn_act_colsum_rows(cd, rows, C)
        assert gy == walk(rows, C // E[dt], 2)[3]
        want = c["want"]
        cs_want = colsum_expect(want, rows, C, 2, dt, gy)
        tag = f"colsum {dt} rows={rows} C={C} {regime}"
        y, mk, cs = Guarded(n, dt), Guarded(n // E[dt], torch.uint8), Guarded(2 * gy * C, F32)
        launch(o.bn_act, cd, x, sc, sh, res, True, y.t, rows, C, mask=mk.t, views=2, colsum=cs.t)
        torch.cuda.synchronize()
        check_act(y, mk, want, dt, tag + " 2 views")
        same(cs.t, cs_want, tag + " colsum (2 views)")
        assert cs.guards(), tag + ": colsum rows beyond sm3_bn_act_colsum_rows written"
        # view 1 alone: the same colsum bits
        y1, cs1 = Guarded(rows * C, dt), Guarded(gy * C, F32)
        launch(o.bn_act, cd, x[rows * C:], sc[C:], sh[C:], res[rows * C:], True, y1.t, rows, C, views=1, colsum=cs1.t)
        torch.cuda.synchronize()
        bits_equal(cs1.t, cs.t[gy * C:], tag + " colsum of view 1 alone vs in the 2-view launch")
        same(y1.t, want[rows:], tag + " view 1 alone y")
        assert cs1.guards() and y1.guards()
        # add form: y = relu(x*scale + shift + x2*scale2 + shift2)
        want2 = stored(c["pre2"].clamp_min(0), dt)
        y2, mk2 = Guarded(n, dt), Guarded(n // E[dt], torch.uint8)
        launch(o.bn_add_bn_act, cd, x, sc, sh, res, _g(c["sc2"], F32), _g(c["sh2"], F32), True, y2.t, rows, C,
               mask=mk2.t, views=2)
        torch.cuda.synchronize()
        check_act(y2, mk2, want2, dt, tag + " add_bn_act")
    print(f"colsum / add {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_subsample_colsum(dt):
    """sm3_subsample_colsum: stride 1 and 2, odd H and W, y null; views 1 and 2."""
    o, cd = ops(), code(dt)
    LAUNCHES[0] = 0
    for i, (N, H, W, cv, stride, views) in enumerate(SUB_CASES):
        c = sub_case(dt, N, H, W, cv, stride, views, 300 + i)
        x, sub, C, Hs, Ws, rows = c["x"], c["sub"], c["C"], c["Hs"], c["Ws"], c["rows"]
        gy = o.subsample_colsum_rows(cd, rows, C)
        cs_want = colsum_expect(sub, rows, C, views, dt, gy)
        for with_y in (True, False):
            tag = f"subsample {dt} {N}x{H}x{W}x{C} s={stride} v={views} y={with_y}"
            y = Guarded(N * Hs * Ws * C, dt) if with_y else None
            cs = Guarded(views * gy * C, F32)
            launch(o.subsample_colsum, cd, _g(x, dt), y.t if y else None, cs.t, N, H, W, C, stride, views=views)
            torch.cuda.synchronize()
            same(cs.t, cs_want, tag + " colsum")
            assert cs.guards(), tag + ": colsum guard band written"
            if y is not None:
                same(y.t, sub, tag + " y")
                assert y.guards(), tag + ": y guard band written"
    print(f"subsample {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
def test_relu_bit_f16_underflow_probe():
    """f16: v in {2^-26, 2^-25} stores +0 and its bit is 0; 3 2^-26 stores 2^-24 (bit 1); -2^-26 stores 0.  bf16 / f32 at the
    same v store it exactly (bit 1)."""
    o = ops()
    vals = torch.tensor([1.0, 2.0, 3.0, -1.0, 0.0, 4.0, 1.0, 2.0]).double()
    for dt in DTYPES:
        C = 8
        rows = 33
        x = vals.repeat(rows, 1)[:, :C].contiguous()
        sc = torch.full((1, C), 2.0 ** -26, dtype=torch.float64)
        sh = torch.zeros(1, C, dtype=torch.float64)
        want = stored((x * sc).clamp_min(0), dt)
        y, mk = Guarded(rows * C, dt), Guarded(rows * C // E[dt], torch.uint8)
        launch(o.bn_act, code(dt), _g(x, dt), _g(sc, F32), _g(sh, F32), None, True, y.t, rows, C, mask=mk.t)
        torch.cuda.synchronize()
        check_act(y, mk, want, dt, f"probe {dt}")
        if dt == F16:
            assert int((want == 0).sum()) > int((x <= 0).sum()), "the probe must reach stored zeros with v > 0"


# ------------------------------------------------------------------------------------------------------------------------
# backward row walks
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bn_bwd_reduce_row_walk(dt):
    """sm3_bn_bwd_reduce with mask / y / neither, x null (second slot 0), dz in place / separate / null: dz and exactly
    sm3_bn_bwd_partial_rows partial rows per view, each the exact block sum."""
    o, cd = ops(), code(dt)
    LAUNCHES[0] = 0
    for rows, C, views, seed in red_plan(dt):
        c = red_case(dt, rows, C, views, seed)
        n = views * rows * C
        gy = o.bn_bwd_partial_rows(rows, C)
        assert gy == c["gy"], (gy, c["gy"])
        dy, x = _g(c["dy"], dt), _g(c["x"], dt)
        mean, invstd = _g(c["mean"], F32), _g(c["invstd"], F32)
        yv, mbits = _g(c["y"], dt), mask_of(c["bits"], dt)
        forms = [("mask", "sep", True), ("y", "inplace", True), ("none", "null", True), ("mask", "null", False),
                 ("y", "sep", False), ("none", "sep", True)]
        for gate, dzmode, with_x in forms:
            tag = f"bwd_reduce {dt} rows={rows} C={C} v={views} gate={gate} dz={dzmode} x={with_x}"
            dzw = {"mask": torch.where(c["bits"], c["dy"], 0.0), "y": torch.where(c["y"] > 0, c["dy"], 0.0),
                   "none": c["dy"]}[gate]
            dyb = Guarded(n, dt, dy) if dzmode == "inplace" else None
            dzb = Guarded(n, dt) if dzmode == "sep" else None
            part = Guarded(views * gy * 2 * C, F32)
            launch(o.bn_bwd_reduce, cd, dyb.t if dyb else dy, yv if gate == "y" else None, x if with_x else None,
                   mean, invstd, dyb.t if dyb else (dzb.t if dzb else None), rows, C, part.t,
                   mask=mbits if gate == "mask" else None, views=views)
            torch.cuda.synchronize()
            for b in (dyb, dzb):
                if b is not None:
                    same(b.t, dzw, tag + " dz")
                    assert b.guards(), tag + ": dz guard band written"
            pr = part.t.view(views, gy, 2, C)
            for vi in range(views):
                sl = slice(vi * rows, (vi + 1) * rows)
                same(pr[vi, :, 0], block_sums(dzw[sl], c["blk"], gy), tag + f" view {vi} partial sum(dz)")
                t2 = block_sums(dzw[sl] * c["xhat"][sl], c["blk"], gy) if with_x else torch.zeros(gy, C, dtype=torch.float64)
                same(pr[vi, :, 1], t2, tag + f" view {vi} partial sum(dz*xhat)")
            assert part.guards(), tag + ": partial rows beyond sm3_bn_bwd_partial_rows written"
    print(f"bwd_reduce {dt}: {LAUNCHES[0]} launches checked")


def check_apply(got, s, dt, tag):
    if s["tol"] is None:
        same(got.t, stored(s["ref"], dt), tag + " dx")
    else:
        d = (got.t.double().cpu() - s["ref"].reshape(-1)).abs()
        bad = d > s["tol"].reshape(-1)
        assert not bool(bad.any()), tag + f" dx: {int(bad.sum())} beyond the fp64-derived bound"
    assert got.guards(), tag + ": dx guard band written"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bn_bwd_apply_and_apply2_row_walk(dt):
    """sm3_bn_bwd_apply / _apply2, views 1 and 2: dx exact for a power-of-two count, within the fp64-derived bound
    otherwise; dgamma / dbeta grow by the fp32 sum of the local sums in view order, once per launch, from a nonzero start;
    with lsums null they stay untouched."""
    o, cd = ops(), code(dt)
    LAUNCHES[0] = 0
    for rows, C, views, kind, seed in apply_plan(dt):
        c = apply_case(dt, rows, C, views, kind, seed)
        n = views * rows * C
        dz = _g(c["dz"], dt)
        a, b = c["a"], c["b"]
        tag = f"apply {dt} rows={rows} C={C} v={views} {kind}"
        dev = {}
        for s, nm in ((a, "a"), (b, "b")):
            dev[nm] = dict(x=_g(s["x"], dt), mean=_g(s["mean"], F32), invstd=_g(s["invstd"], F32), gamma=_g(s["gamma"], F32),
                           gsums=_g(s["gs"], torch.float64), lsums=_g(s["ls"], torch.float64))
        # single form, lsums given
        d = dev["a"]
        dx, dg, db = Guarded(n, dt), Guarded(C, F32, a["dg0"].float()), Guarded(C, F32, a["db0"].float())
        launch(o.bn_bwd_apply, cd, dz, d["x"], d["mean"], d["invstd"], d["gamma"], d["gsums"], a["count"], d["lsums"],
               dg.t, db.t, dx.t, rows, C, views=views)
        torch.cuda.synchronize()
        check_apply(dx, a, dt, tag + " single")
        same(db.t, a["dbeta"], tag + " dbeta")
        same(dg.t, a["dgamma"], tag + " dgamma")
        assert dg.guards() and db.guards()
        # lsums null: dgamma / dbeta untouched
        dx2, dg2, db2 = Guarded(n, dt), Guarded(C, F32, a["dg0"].float()), Guarded(C, F32, a["db0"].float())
        launch(o.bn_bwd_apply, cd, dz, d["x"], d["mean"], d["invstd"], d["gamma"], d["gsums"], a["count"], None,
               dg2.t, db2.t, dx2.t, rows, C, views=views)
        torch.cuda.synchronize()
        bits_equal(dx2.t, dx.t, tag + " dx without lsums")
        same(dg2.t, a["dg0"], tag + " dgamma untouched")
        same(db2.t, a["db0"], tag + " dbeta untouched")
        # dual form: each side as the single form
        bufs = {}
        sides = []
        for s, nm in ((a, "a"), (b, "b")):
            bufs[nm] = (Guarded(n, dt), Guarded(C, F32, s["dg0"].float()), Guarded(C, F32, s["db0"].float()))
            sd = dict(dev[nm], dx=bufs[nm][0].t, dgamma=bufs[nm][1].t, dbeta=bufs[nm][2].t)
            if nm == "b" and views == 1:
                sd["lsums"] = None
            sides.append(sd)
        assert a["count"] == b["count"]
        launch(o.bn_bwd_apply2, cd, dz, a["count"], sides[0], sides[1], rows, C, views=views)
        torch.cuda.synchronize()
        for s, nm in ((a, "a"), (b, "b")):
            dxs, dgs, dbs = bufs[nm]
            check_apply(dxs, s, dt, tag + f" dual side {nm}")
            if nm == "b" and views == 1:
                same(dgs.t, s["dg0"], tag + " dual: dgamma untouched without lsums")
                same(dbs.t, s["db0"], tag + " dual: dbeta untouched without lsums")
            else:
                same(dbs.t, s["dbeta"], tag + f" dual side {nm} dbeta")
                same(dgs.t, s["dgamma"], tag + f" dual side {nm} dgamma")
            assert dgs.guards() and dbs.guards()
    print(f"apply {dt}: {LAUNCHES[0]} launches checked")


# ------------------------------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_maxpool_first_maximum_and_exact_gradient(dt):
    o, cd = ops(), code(dt)
    for N, H, W, C, seed in pool_plan(dt):
        c = pool_case(dt, N, H, W, C, seed)
        tag = f"maxpool {dt} {N}x{H}x{W}x{C}"
        y, am = Guarded(c["y"].numel(), dt), Guarded(c["y"].numel(), torch.uint8)
        launch(o.maxpool_fwd, cd, _g(c["x"], dt), y.t, N, H, W, C, argmax=am.t)
        torch.cuda.synchronize()
        same(y.t, c["y"], tag + " y")
        assert torch.equal(am.t.cpu(), c["arg"].reshape(-1).to(torch.uint8)), tag + ": argmax != first maximum"
        assert y.guards() and am.guards(), tag + ": guard band written"
        dx = Guarded(c["dx"].numel(), dt)
        launch(o.maxpool_bwd, cd, am.t, _g(c["dy"], dt), dx.t, N, H, W, C)
        torch.cuda.synchronize()
        same(dx.t, c["dx"], tag + " dx")
        assert dx.guards(), tag + ": dx guard band written"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stem_pair_equals_the_separate_kernels_bit_for_bit(dt):
    """sm3_bn_relu_maxpool_fwd == sm3_bn_act + sm3_maxpool3x3s2_fwd; sm3_maxpool_bn_bwd == sm3_maxpool3x3s2_bwd +
    sm3_bn_bwd_reduce(y = stored) in dz, and its partial rows (as many as sm3_maxpool_bn_bwd_partial_rows) hold the exact
    totals of the ROUNDED dz."""
    o, cd = ops(), code(dt)
    LAUNCHES[0] = 0
    for i, (N, H, W, cv, views, regime) in enumerate(STEM_CASES):
        c = stem_case(dt, N, H, W, cv, views, regime, 70 + i)
        C = c["C"]
        tag = f"stem {dt} {N}x{H}x{W}x{C} v={views} {regime}"
        rows = N // views * H * W
        x, sc, sh = _g(c["x"], dt), _g(c["sc"], F32), _g(c["sh"], F32)
        ny = c["y"].numel()
        # forward: fused vs separate
        yf, af = Guarded(ny, dt), Guarded(ny, torch.uint8)
        launch(o.bn_relu_maxpool_fwd, cd, x, sc, sh, yf.t, N, H, W, C, argmax=af.t, views=views)
        act = Guarded(x.numel(), dt)
        launch(o.bn_act, cd, x, sc, sh, None, True, act.t, rows, C, views=views)
        ys, as_ = Guarded(ny, dt), Guarded(ny, torch.uint8)
        launch(o.maxpool_fwd, cd, act.t, ys.t, N, H, W, C, argmax=as_.t)
        torch.cuda.synchronize()
        same(act.t, c["act"], tag + " bn_act")
        same(yf.t, c["y"], tag + " fused y")
        bits_equal(yf.t, ys.t, tag + " fused y vs separate")
        assert torch.equal(af.t, as_.t), tag + ": fused argmax vs separate"
        assert torch.equal(af.t.cpu(), c["arg"].reshape(-1).to(torch.uint8)), tag + ": argmax != first maximum"
        assert all(b.guards() for b in (yf, af, act, ys, as_)), tag + ": forward guard band written"
        # backward: fused vs maxpool_bwd + bn_bwd_reduce(y = stored)
        dy, mean, invstd = _g(c["dy"], dt), _g(c["mean"], F32), _g(c["invstd"], F32)
        gyf = o.maxpool_bn_bwd_partial_rows(N, H, W, views)
        assert gyf == max(1, min(1024, (rows + 63) // 64))
        dzf, pf = Guarded(x.numel(), dt), Guarded(views * gyf * 2 * C, F32)
        launch(o.maxpool_bn_bwd, cd, af.t, dy, x, sc, sh, mean, invstd, dzf.t, pf.t, N, H, W, C, views=views)
        gx = Guarded(x.numel(), dt)
        launch(o.maxpool_bwd, cd, as_.t, dy, gx.t, N, H, W, C)
        gyr = o.bn_bwd_partial_rows(rows, C)
        dzs, ps = Guarded(x.numel(), dt), Guarded(views * gyr * 2 * C, F32)
        launch(o.bn_bwd_reduce, cd, gx.t, act.t, x, mean, invstd, dzs.t, rows, C, ps.t, views=views)
        torch.cuda.synchronize()
        same(dzf.t, c["dz"], tag + " fused dz vs fp64")
        bits_equal(dzf.t, dzs.t, tag + " fused dz vs separate")
        tot_f = pf.t.view(views, gyf, 2, C).double().sum(1)
        tot_s = ps.t.view(views, gyr, 2, C).double().sum(1)
        same(tot_f, c["sums"], tag + " fused partial totals")
        same(tot_s, c["sums"], tag + " separate partial totals")
        assert all(b.guards() for b in (dzf, pf, gx, dzs, ps)), tag + ": backward guard band written"
    print(f"stem {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_avgpool_forward_backward(dt):
    """HW = 64: exact.  HW = 49: the f32 mean is the fp32 product sum * fl(1/49), within 1 ulp of fp64; the T output is
    the rounding of the kernel's own f32 output; the gradient is fl(dfeat * fl(1/HW)) rounded to T."""
    o, cd = ops(), code(dt)
    for i, (N, HW, cv) in enumerate(AVG_CASES):
        c = avg_case(dt, N, HW, cv, 90 + i)
        C = c["C"]
        tag = f"avgpool {dt} N={N} HW={HW} C={C}"
        f32o, ft = Guarded(N * C, F32), Guarded(N * C, dt)
        launch(o.avgpool_fwd, cd, _g(c["x"], dt), f32o.t, ft.t, N, HW, C)
        torch.cuda.synchronize()
        inv = torch.tensor(1.0 / HW, dtype=torch.float32)
        want32 = (c["s"].float() * inv).double()
        same(f32o.t, want32, tag + " f32 mean")
        ref = (c["s"] / HW).reshape(-1)
        assert bool(((f32o.t.double().cpu() - ref).abs() <= ulp32(ref)).all()), tag + ": f32 mean beyond 1 ulp"
        bits_equal(ft.t, f32o.t.to(dt), tag + " T mean vs the rounded f32 mean")
        if HW == 64:
            same(f32o.t, ref, tag + " exact mean")
        assert f32o.guards() and ft.guards()
        dx = Guarded(N * HW * C, dt)
        launch(o.avgpool_bwd, cd, _g(c["df"], dt), dx.t, N, HW, C)
        torch.cuda.synchronize()
        wantdx = (c["df"].float() * inv).to(dt)[:, None, :].expand(N, HW, C)
        bits_equal(dx.t, wantdx.to(_dev()).contiguous(), tag + " dx")
        if HW == 64:
            same(dx.t, (c["df"] / 64)[:, None, :].expand(N, HW, C), tag + " exact dx")
        assert dx.guards()


# ------------------------------------------------------------------------------------------------------------------------
# slab reductions
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_linbn_moments_and_fold_exact():
    o = ops()
    for nslabs, n, views, with_colsum in linbn_plan():
        c = linbn_case(nslabs, n, views, with_colsum)
        tag = f"linbn_moments nslabs={nslabs} views={views} colsum={with_colsum}"
        out = Guarded(views * n, F32)
        s_out = Guarded(views * c["p"], torch.float64) if with_colsum else None
        launch(o.linbn_moments, _g(c["slabs"], F32), nslabs, n, out.t, views=views,
               colsum=_g(c["cs"], F32) if with_colsum else None, colsum_rows=c["crow"],
               s_out=s_out.t if s_out else None, p=c["p"])
        torch.cuda.synchronize()
        same(out.t, c["G"], tag + " G")
        assert out.guards(), tag + ": G guard band written"
        if s_out is not None:
            same(s_out.t, c["s"], tag + " s")
            assert s_out.guards(), tag + ": s guard band written"
        fo = Guarded(views * n, torch.float64)
        launch(o.linbn_fold, _g(c["ws"], torch.float64), 11, n, fo.t, views=views)
        torch.cuda.synchronize()
        same(fo.t, c["fold"], f"linbn_fold views={views}")
        assert fo.guards()


# ------------------------------------------------------------------------------------------------------------------------
# rejections
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rejected_launches_leave_outputs_untouched():
    """C % E and C/E > 256 (maxpool_bn_bwd) -> SM3_EALIGN; N % views -> SM3_EINVAL; nothing written."""
    L = lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cd = code(BF16)
    x = torch.zeros(4096 * 8, dtype=BF16, device=_dev())
    f = torch.zeros(8192, dtype=F32, device=_dev())
    for C, want in ((12, -2), (2056, None)):
        y, mk, p = Guarded(4096 * 8, BF16), Guarded(4096, torch.uint8), Guarded(8192, F32)
        if want is not None:
            assert L.sm3_bn_act(cd, P(x), P(f), P(f), None, 1, 0, P(y.t), P(mk.t), 4, C, 1, st) == want
            assert L.sm3_bn_bwd_reduce(cd, P(x), None, None, None, None, None, P(y.t), 4, C, P(p.t), 1, st) == want
            assert L.sm3_bn_bwd_apply(cd, P(x), P(x), P(f), P(f), None, P(f.view(torch.float64)), 4.0, None, None, None,
                                      P(y.t), 4, C, 1, st) == want
            assert L.sm3_maxpool3x3s2_fwd(cd, P(x), P(y.t), P(mk.t), 1, 2, 2, C, st) == want
        # maxpool_bn_bwd: C = 12 (C % 8) and C = 2056 (C/E = 257 > 256)
        assert L.sm3_maxpool_bn_bwd(cd, P(mk.t), P(x), P(x), P(f), P(f), P(f), P(f), P(y.t), P(p.t), 1, 2, 2, C, 1, st) == -2
        torch.cuda.synchronize()
        assert y.untouched() and mk.untouched() and p.untouched(), f"C={C}: a rejected launch wrote"
    y, p = Guarded(4096 * 8, BF16), Guarded(8192, F32)
    assert L.sm3_maxpool_bn_bwd(cd, P(x), P(x), P(x), P(f), P(f), P(f), P(f), P(y.t), P(p.t), 3, 2, 2, 8, 2, st) == -1
    assert L.sm3_bn_relu_maxpool_fwd(cd, P(x), P(f), P(f), P(y.t), None, 3, 2, 2, 8, 2, st) == -1
    assert L.sm3_subsample_colsum(cd, P(x), P(y.t), P(p.t), 3, 2, 2, 8, 1, 2, st) == -1
    torch.cuda.synchronize()
    assert y.untouched() and p.untouched(), "N % views: a rejected launch wrote"


# ------------------------------------------------------------------------------------------------------------------------
# the process-wide row-walk knobs
# ------------------------------------------------------------------------------------------------------------------------
ROW_WALK_TESTS = ["test_bn_act_row_walk", "test_bn_act_colsum_and_add_bn_act_row_walk", "test_bn_bwd_reduce_row_walk",
                  "test_bn_bwd_apply_and_apply2_row_walk", "test_relu_bit_f16_underflow_probe"]
KNOBS = [{"SM3_BN_UNROLL": "1", "SM3_BN_NT": "0"}, {"SM3_BN_UNROLL": "2"}, {"SM3_BN_UNROLL": "8"}, {"SM3_BN_GRID_CAP": "1"}]


@pytest.mark.gpu
def test_row_walk_knobs_in_child_processes():
    """Each knob setting reruns the row-walk tests in a fresh process (the knobs are read once per process), one child at
    a time; the first failure ends the test."""
    if os.environ.get(CHILD_MARK):
        pytest.skip("inside a knob child process")
    me = os.path.relpath(os.path.abspath(__file__), ROOT)
    ids = [f"{me}::{t}" for t in ROW_WALK_TESTS]
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    for knobs in KNOBS:
        child_env = dict(os.environ, **knobs, **{CHILD_MARK: "1"})
        for k in ("SM3_BN_UNROLL_ACT", "SM3_BN_UNROLL_RED", "SM3_BN_UNROLL_APP"):
            child_env.pop(k, None)
        t0 = time.time()
        r = subprocess.run(py + ["-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", *ids], cwd=ROOT,
                           env=child_env, capture_output=True, text=True, timeout=600)
        tail = (r.stdout + r.stderr)[-3000:]
        assert r.returncode == 0, f"row walks under {knobs} failed (exit {r.returncode}):\n{tail}"
        print(f"knobs {knobs}: passed in {time.time() - t0:.1f} s")
