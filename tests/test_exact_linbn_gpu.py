"""Bit-exact checks of the BatchNorm-by-linearity kernels (csrc/linbn.hip) on integer inputs: sm3_linbn_fwd_stats, _stats,
_coef, _banks, _post, _banks_post and _scale_banks, and the composed backward unit through sm3_conv_dgrad_seg_bnfuse.
Also the `only_if` argument of the three conditional weight preparations.

The method is test_exact_gemm_gpu.py's and test_exact_bn_gpu.py's: every operand is a small integer times a power of
two, the generators below check in fp64 on the CPU that every fp32 operation a kernel performs is exact (need_f32), that
every fp32 sum stays under 2^24 quanta in any order (need_exact) and every fp64 sum under 2^53 (need_exact64).  Then a launch
must return exactly the fp64 value of the DEFINITION,

    x = y_v W^T,   dx = a (dz - m1) - b (x - mu),   dy = dx W,   dW = sum_v sum_m dx^T y,

not of a restatement of the kernel: G = y^T y, s = sum_m y, P = dz^T y and the partial rows of sum_m dz are computed in fp64
on the CPU and handed to the kernels; only the kernel under test runs on the GPU.  Two regimes:
  repr:   every stored 16-bit value is exact in the storage type T;
  round:  a product (wa, wbn, the scaled banks) or a sum (Hn) exceeds T, and the stored value is the fp64 result rounded
          once, nearest even.
Every output is a slice of a sentinel-filled buffer whose guard bytes must survive, +0 and -0 are identified, and there is
no tolerance anywhere.  The shapes are the smallest at which each loop structure of the kernels changes (idle and
unevenly loaded waves of the 4-wave K splits, block tails, the second trip of the strided loops); every view of a launch
has coefficients and moments of its own, so that a value taken from the wrong view is a wrong value."""
import pytest
import torch

from exact_inputs import (Guarded, _dev, draw, need_exact, need_exact64, need_f32, need_repr, pick, quantum, same,
                          stored)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
F64 = torch.float64
DTS = [BF16, F16]
IDS = ["bf16", "f16"]
ALL_DTS = [F32, BF16, F16]
ALL_IDS = ["f32", "bf16", "f16"]
NB = {BF16: 9, F16: 12}       # bits of a rounding-regime coefficient: one more than T's significand


def finite_in(t, dt, what):
    assert bool(torch.isfinite(t.to(dt)).all()), f"{what}: out of range in {dt}"


# ------------------------------------------------------------------------------------------------------------------------
# the operands of one conv3 -> bn3 unit and its coefficients (CPU, fp64)
# ------------------------------------------------------------------------------------------------------------------------
def unit(g, V, Mv, C, p, y_amp=3, y_den=0.6, dz_amp=3, dz_den=0.7, w_amp=2, w_den=0.8, shape_dz=None):
    y = draw(g, (V, Mv, p), y_amp, y_den).abs()
    dz = draw(g, (V, Mv, C), dz_amp, dz_den)
    if shape_dz is not None:
        dz = shape_dz(dz)
    W = draw(g, (C, p), w_amp, w_den)
    u = dict(y=y, dz=dz, W=W, wd=W.t().contiguous(), x=y @ W.t(), G=torch.einsum("vmk,vmj->vkj", y, y), s=y.sum(1),
             P=torch.einsum("vmc,vmk->vck", dz, y), V=V, Mv=Mv, C=C, p=p)
    need_exact64(torch.einsum("vmc,vmk->vck", dz.abs(), y) + u["G"].max(), 1.0, "moments")
    for k in ("G", "s", "P"):
        need_f32(u[k], k)
    return u


def coefs(g, V, C, kind, dt):
    """(a, b, m1, mu), each [V][C], different per view."""
    if kind == "repr":      # dyadic, a few bits
        a = pick(g, torch.tensor([1.0, -1.0, 2.0, 0.5], dtype=F64), (V, C))
        b = pick(g, torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0, 1.0], dtype=F64), (V, C))
        m1, mu = draw(g, (V, C), 4, 0.8, -1), draw(g, (V, C), 4, 0.8, -1)
    elif kind == "int":     # the composed unit: dy has to be exact in T
        a = pick(g, torch.tensor([1.0, -1.0, 2.0], dtype=F64), (V, C))
        b = pick(g, torch.tensor([0.0, 1.0, -1.0], dtype=F64), (V, C))
        m1, mu = draw(g, (V, C), 1, 0.5, 0), draw(g, (V, C), 1, 0.5, 0)
    else:                   # round: one bit more than T holds, so a w and b w round in T
        a = draw(g, (V, C), 2 ** NB[dt] - 1, 1.0, 2 - NB[dt])
        b = draw(g, (V, C), 2 ** NB[dt] - 1, 1.0, 2 - NB[dt])
        m1, mu = draw(g, (V, C), 2, 0.8, 0), draw(g, (V, C), 2, 0.8, 0)
    return a, b, m1, mu


def coef4(cf):
    return torch.stack(cf, -1)  # [V][C][4]


# ------------------------------------------------------------------------------------------------------------------------
# sm3_linbn_fwd_stats
# ------------------------------------------------------------------------------------------------------------------------
FWD_P = [32, 64, 96, 160]   # K-steps p/2 over 4 waves in batches of 8: two waves idle / one batch each / uneven / 2 rounds + part
FWD_C = [32, 96, 128]       # one 32-channel tile; ct = 3 not a power of two; (C 32, p 96): p > C; (C 128, p 64): C = 2p


def fwd_plan():
    for i, C in enumerate(FWD_C):
        for j, p in enumerate(FWD_P):
            yield C, p, 1 + (i + j) % 3, 100 + 10 * i + j


def wg_exact(u, what):
    """The exact-f32 MFMA tile of W G: every partial sum of a K split is exact."""
    need_exact(torch.einsum("ck,vkj->vcj", u["W"].abs(), u["G"].abs()).reshape(-1), 1.0, what)
    return torch.einsum("ck,vkj->vcj", u["W"], u["G"])


def fwd_case(dt, C, p, V, seed):
    g = torch.Generator().manual_seed(seed)
    u = unit(g, V, 48, C, p)
    need_repr(u["W"], dt, "W")
    Tm = wg_exact(u, "Tm = W G")
    need_f32(Tm, "Tm")
    pt = p // 32
    t1 = u["W"][None] * u["s"][:, None, :]                       # [V][C][p]
    t2 = Tm * u["W"][None]
    for t in (t1, t2):
        need_exact64(t.abs().sum(-1).reshape(-1), 1.0, "fwd_stats rows")
    ws = torch.cat([t.reshape(V, C, pt, 32).sum(-1).permute(0, 2, 1) for t in (t1, t2)], -1)  # [V][pt][2C]
    # the rows add up to the batch sums of the explicit x
    assert torch.equal(ws.sum(1), torch.cat([u["x"].sum(1), (u["x"] * u["x"]).sum(1)], -1)), "rows vs sum x, sum x^2"
    return dict(u, Tm=Tm, ws=ws)


# ------------------------------------------------------------------------------------------------------------------------
# sm3_linbn_stats / sm3_linbn_coef
# ------------------------------------------------------------------------------------------------------------------------
def stats_plan():
    """(C, p, groups, V, gamma, grads, count)"""
    yield 1, 1, 1, 1, True, True, 64.0
    yield 3, 63, 63, 2, True, True, 32.0
    yield 4, 64, 64, 3, True, True, 64.0
    yield 5, 65, 65, 2, True, True, 128.0
    yield 130, 200, 1, 3, True, True, 64.0          # coef: views * C = 3 * 130
    yield 130, 64, 65, 1, False, True, 64.0         # gamma = None
    yield 5, 200, 63, 2, True, False, 64.0          # dgamma = dbeta = None
    yield 4, 65, 64, 3, False, False, 0.0           # count = 0: coef untouched
    yield 3, 1, 65, 1, True, True, 0.0
    for C, V in ((255, 1), (256, 1), (128, 2), (257, 1)):   # coef: the block tail at views * C = 255, 256, 257
        yield C, 8, 3, V, True, True, 64.0


def stats_case(dt, C, p, groups, V, with_gamma, with_grads, count, seed):
    g = torch.Generator().manual_seed(seed)
    Mv = max(40, 2 * groups)
    grp = torch.arange(Mv) % groups          # row m of dz belongs to group m % groups; row g < groups is group g's first

    def rows_of(dz):
        return torch.zeros(V, groups, C, dtype=F64).index_add_(1, grp, dz)

    def every_group_counts(dz):
        """Adjust the first row of each group so that no entry of a partial row is 0 and, in channel 0, group g of view v
        holds +-(g + 1 + v): every lane and every trip of the kernel's loop over `groups` carries a value of its own."""
        part = rows_of(dz)
        want = torch.where(part == 0, torch.ones_like(part), part)
        sign = 1.0 - 2.0 * (torch.arange(groups) % 2)
        want[:, :, 0] = sign[None] * (torch.arange(groups)[None] + 1.0 + torch.arange(V)[:, None])
        dz = dz.clone()
        dz[:, :groups] += want - part
        return dz

    u = unit(g, V, Mv, C, p, shape_dz=every_group_counts)
    need_repr(u["W"], dt, "W")
    mean = draw(g, (V, C), 8, 0.9, -2)
    invstd = pick(g, torch.tensor([0.25, 0.5, 1.0, 2.0], dtype=F64), (V, C))
    gamma = pick(g, torch.tensor([0.5, 1.0, 1.5, -2.0, 0.25], dtype=F64), (C,))
    part = rows_of(u["dz"])                                                 # partial rows of sum_m dz
    assert bool((part != 0).all()), "a partial row of sum dz has a zero: that group would not count"
    assert all(len(set(part[v, :, 0].tolist())) == groups for v in range(V)), "two groups hold the same value in channel 0"
    # a loop over `groups` that stops after lane 39, after one trip of 64, or before the last row gives another S1
    for cut in {min(40, groups - 1), min(64, groups - 1), groups - 1} - {0}:
        assert bool((part[:, cut:].sum(1) != 0).any(-1).all()), f"the groups from {cut} on add up to 0 in every channel"
    ws = torch.cat([part, torch.full_like(part, float("nan"))], -1)         # [V][groups][2C]; second half never read
    S1 = u["dz"].sum(1)
    assert torch.equal(S1, part.sum(1)), "the partial rows do not add up to sum_m dz"
    S2 = invstd * (u["dz"] * (u["x"] - mean[:, None])).sum(1)
    need_exact64((u["dz"].abs() * (u["x"].abs() + mean.abs()[:, None])).sum(1).reshape(-1), 0.25, "S2")
    need_exact64(torch.einsum("vck,ck->vc", u["P"].abs(), u["W"].abs()).reshape(-1), 1.0, "rowdot(W, P)")
    dg0, db0 = draw(g, (C,), 50, 1.0, 0), draw(g, (C,), 50, 1.0, 0)
    dg, db = dg0.clone(), db0.clone()
    for v in range(V):      # one fp32 add per view, in view order
        need_f32(S1[v], "S1")
        need_f32(S2[v], "S2")
        dg, db = dg + S2[v], db + S1[v]
        need_f32(dg, "dgamma")
        need_f32(db, "dbeta")
    c = dict(u, mean=mean, invstd=invstd, gamma=gamma if with_gamma else None, groups=groups, ws=ws, S1=S1, S2=S2,
             lsums=torch.cat([S1, S2], -1), dg0=dg0, db0=db0, dg=dg, db=db, with_grads=with_grads, count=count, coef=None)
    if count > 0:
        gm = gamma if with_gamma else torch.ones(C, dtype=F64)
        a = gm * invstd
        m2, m1 = S2 / count, S1 / count
        for t, nm in ((a, "a"), (m2, "S2 / count"), (m1, "S1 / count"), (a * invstd, "a invstd"), (a * invstd * m2, "b")):
            need_f32(t, "coef " + nm)
        c["coef"] = coef4((a, a * invstd * m2, m1, mean))
    return c


# ------------------------------------------------------------------------------------------------------------------------
# sm3_linbn_banks
# ------------------------------------------------------------------------------------------------------------------------
def banks_plan():
    """(C, p, V, regime): C 8 -> one thread; 136 -> 17 threads, three waves add 0; 2176 -> second trip of the stride."""
    i = 0
    for C in (8, 136, 2176):
        for p in (1, 3, 32):
            for regime in ("repr", "round"):
                if C == 2176 and regime == "round" and p != 3:
                    continue
                yield C, p, 1 + i % 3, regime
                i += 1


def banks_of(wd, cf, dt, regime, what):
    """wa = T(a wd), wbn = T(-b wd) [V][p][C] and the centring constant of the ROUNDED banks; also that of the products."""
    a, b, m1, mu = cf
    pa, pb = a[:, None, :] * wd[None], -b[:, None, :] * wd[None]
    for t in (pa, pb):
        need_f32(t, what + " a wd / b wd")
        finite_in(t, dt, what)
        if regime != "round":
            need_repr(t, dt, what + " bank")
    fa, fb = stored(pa, dt), stored(pb, dt)
    t1 = m1[:, None, :] * fa
    terms = mu[:, None, :] * fb + t1
    need_f32(t1, what + " m1 f(wa)")
    need_f32(mu[:, None, :] * fb, what + " mu f(wbn)")
    need_f32(terms, what + " mu f(wbn) + m1 f(wa)")
    need_exact(terms.abs().sum(-1).reshape(-1), quantum(terms), what + " col_const")
    const_products = -(mu[:, None, :] * pb + m1[:, None, :] * pa).sum(-1)
    return fa, fb, -terms.sum(-1), const_products


def banks_case(dt, C, p, V, regime, seed):
    g = torch.Generator().manual_seed(seed)
    big = C > 2000
    wd = draw(g, (p, C), 3, 0.3 if big else 0.8)
    need_repr(wd, dt, "wd")
    cf = coefs(g, V, C, regime, dt)
    wa, wbn, const, const_p = banks_of(wd, cf, dt, regime, f"banks C={C} p={p} {regime}")
    return dict(wd=wd, cf=cf, wa=wa, wbn=wbn, const=const, const_p=const_p, C=C, p=p, V=V)


# ------------------------------------------------------------------------------------------------------------------------
# sm3_linbn_post / sm3_linbn_banks_post
# ------------------------------------------------------------------------------------------------------------------------
def post_plan():
    """(C, p, V, regime); every case runs with Tm given and with Tm = None.
    C 128 / 384 / 640: one / three / all four waves of the H-tile K loop, wave 0 twice; p 32 / 96: pt = 1 / 3."""
    i = 0
    for C in (128, 384, 640):
        for p in (32, 96):
            for regime in ("repr", "round"):
                yield C, p, 1 + i % 3, regime
                i += 1
    yield 128, 64, 2, "repr"        # tile_wg at p 64 and 160 (Tm = None)
    yield 128, 160, 3, "round"
    yield 2176, 32, 2, "repr"       # the bank rows behind the tiles: second trip of the 2048-element stride


W_DEN = {128: 0.5, 384: 0.3, 640: 0.25, 2176: 0.12}


def dw_steps(u, cf, dw0, what):
    """Every fp32 operation of the weight-gradient tile is exact; returns dw0 + the formula."""
    a, b, m1, mu = (t[:, :, None] for t in cf)
    s = u["s"][:, None, :]
    Tm = wg_exact(u, what + " W G")
    need_f32(Tm, what + " Tm")
    tot = torch.zeros_like(dw0)
    for v in range(u["V"]):
        st = [m1[v] * s[v], u["P"][v] - m1[v] * s[v], a[v] * (u["P"][v] - m1[v] * s[v]), mu[v] * s[v], Tm[v] - mu[v] * s[v],
              b[v] * (Tm[v] - mu[v] * s[v])]
        st.append(st[2] - st[5])
        tot = tot + st[-1]
        for t in st + [tot, st[2] - b[v] * Tm[v], b[v] * Tm[v], b[v] * mu[v] * s[v]]:   # contracted forms included
            need_f32(t, what + " dw step")
    need_f32(dw0 + tot, what + " dw")
    return dw0 + tot, Tm


def post_case(dt, C, p, V, regime, seed, Mv=None):
    g = torch.Generator().manual_seed(seed)
    rnd = regime == "round"
    if Mv is None:
        Mv = 8 if rnd else 24
    u = unit(g, V, Mv, C, p, y_amp=1 if rnd else 3, y_den=0.5, dz_amp=2 if rnd else 3,
             w_amp=3 if rnd else 2, w_den=0.8 if rnd else W_DEN[C])
    need_repr(u["W"], dt, "W")
    cf = coefs(g, V, C, regime, dt)
    what = f"post C={C} p={p} V={V} {regime} {dt}"
    wa, wbn, const, _ = banks_of(u["wd"], cf, dt, regime, what)
    hn_x = torch.einsum("vkc,ic->vki", wbn, u["wd"])
    need_exact(torch.einsum("vkc,ic->vki", wbn.abs(), u["wd"].abs()).reshape(-1), quantum(wbn), what + " Hn")
    need_f32(hn_x, what + " Hn")
    finite_in(hn_x, dt, what + " Hn")
    if not rnd:
        need_repr(hn_x, dt, what + " Hn")
    dw0 = draw(g, (C, p), 40, 1.0, 0)
    dw_formula, Tm = dw_steps(u, cf, dw0, what)
    # the definition: dW = dw0 + sum_v sum_m dx^T y
    a, b, m1, mu = (t[:, None, :] for t in cf)
    dx = a * (u["dz"] - m1) - b * (u["x"] - mu)
    dw = dw0 + torch.einsum("vmc,vmk->ck", dx, u["y"])
    assert torch.equal(dw, dw_formula), what + ": the formula in moments is not the definition"
    return dict(u, cf=cf, wa=wa, wbn=wbn, const=const, hn_x=hn_x, hn=stored(hn_x, dt), dw0=dw0, dw=dw, Tm=Tm, dx=dx)


# composed backward unit: (V, Mv, C, p)
UNIT_CASES = [(1, 40, 128, 64), (2, 128, 384, 192)]   # p a multiple of the GEMM's 64-element K chunk


def unit_case(dt, V, Mv, C, p, seed):
    g = torch.Generator().manual_seed(seed)
    u = unit(g, V, Mv, C, p, y_amp=2, y_den=0.4, dz_amp=2, dz_den=0.6, w_amp=1, w_den=0.35 if C == 128 else 0.2)
    cf = coefs(g, V, C, "int", dt)
    what = f"unit V={V} Mv={Mv} C={C} p={p} {dt}"
    wa, wbn, const, _ = banks_of(u["wd"], cf, dt, "repr", what)
    hn = torch.einsum("vkc,ic->vki", wbn, u["wd"])
    need_exact(torch.einsum("vkc,ic->vki", wbn.abs(), u["wd"].abs()).reshape(-1), 1.0, what + " Hn")
    need_repr(hn, dt, what + " Hn")
    dw0 = draw(g, (C, p), 40, 1.0, 0)
    dw, Tm = dw_steps(u, cf, dw0, what)
    a, b, m1, mu = (t[:, None, :] for t in cf)
    dx = a * (u["dz"] - m1) - b * (u["x"] - mu)
    dy = dx @ u["W"]                                                  # [V][Mv][p]: the definition
    need_repr(dy, dt, what + " dy")
    need_repr(u["dz"], dt, "dz")
    need_repr(u["y"], dt, "y")
    # the two-segment GEMM: |dz| |wa| + |y| |Hn| + |const| stays exact in fp32 in any order
    tot = torch.einsum("vmc,vkc->vmk", u["dz"].abs(), wa.abs()) + torch.einsum("vmj,vkj->vmk", u["y"], hn.abs()) + \
        const.abs()[:, None]
    need_exact(tot.reshape(-1), quantum(wa, hn, const), what + " GEMM")
    assert torch.equal(dw, dw0 + torch.einsum("vmc,vmk->ck", dx, u["y"]))
    return dict(u, cf=cf, wa=wa, wbn=wbn, const=const, hn=hn, dw0=dw0, dw=dw, Tm=Tm, dy=dy)


# ------------------------------------------------------------------------------------------------------------------------
# sm3_linbn_scale_banks
# ------------------------------------------------------------------------------------------------------------------------
SCALE_K = [(8, 8), (2040, 16), (16, 2040), (2048, 8), (64, 128)]   # the segment switch at thread 255 / second trip of k0


def scale_plan():
    i = 0
    for K3, Kd in SCALE_K:
        for C in (1, 3):
            yield K3, Kd, C, 1 + i % 3, "round" if i % 2 else "repr"
            i += 1


def scale_case(dt, K3, Kd, C, V, regime, seed):
    g = torch.Generator().manual_seed(seed)
    w3, wd = draw(g, (C, K3), 3, 0.9), draw(g, (C, Kd), 3, 0.9)
    if regime == "repr":
        vals = torch.tensor([0.5, 1.0, 2.0, -1.0, -0.25, 1.5], dtype=F64)
        sc3, scd = pick(g, vals, (V, C)), pick(g, vals, (V, C))
    else:
        def wide():     # odd, with the top bit set: all NB bits in use, so every product with w = +-1 or +-2 rounds in T
            mag = 2 ** (NB[dt] - 1) + 2 * torch.randint(0, 2 ** (NB[dt] - 2), (V, C), generator=g) + 1
            return (mag * (torch.randint(0, 2, (V, C), generator=g) * 2 - 1)).double() * 2.0 ** (2 - NB[dt])
        sc3, scd = wide(), wide()
    o3, od = sc3[:, :, None] * w3[None], scd[:, :, None] * wd[None]
    for t in (o3, od):
        need_f32(t, "scale_banks product")
        finite_in(t, dt, "scale_banks")
        if regime == "repr":
            need_repr(t, dt, "scale_banks product")
    sh3, shd = torch.randn(V, C, generator=g), torch.randn(V, C, generator=g) * 3   # fp32: bias is ONE fp32 add
    return dict(w3=w3, wd=wd, sc3=sc3, scd=scd, o3=stored(o3, dt), od=stored(od, dt), o3x=o3, odx=od, sh3=sh3, shd=shd,
                bias=(sh3 + shd).double(), K3=K3, Kd=Kd, C=C, V=V)


# ------------------------------------------------------------------------------------------------------------------------
# the CPU self-check
# ------------------------------------------------------------------------------------------------------------------------
def all_preconditions():
    """Runs every case of every table through its generator (which asserts the exactness preconditions) and checks, on
    those same cases, that the rounding regime rounds, the representable one does not, and the views differ."""
    n = {"fwd_stats": 0, "stats": 0, "banks": 0, "post": 0, "unit": 0, "scale_banks": 0}
    const_differs = set()
    for dt in DTS:
        for args in fwd_plan():
            fwd_case(dt, *args)
            n["fwd_stats"] += 1
        for i, args in enumerate(stats_plan()):
            stats_case(dt, *args, 200 + i)
            n["stats"] += 1
        for i, (C, p, V, regime) in enumerate(banks_plan()):
            c = banks_case(dt, C, p, V, regime, 300 + i)
            a, b = c["cf"][0][:, None, :] * c["wd"][None], -c["cf"][1][:, None, :] * c["wd"][None]
            tag = f"banks {dt} C={C} p={p} V={V} {regime}"
            if regime == "round":
                assert not torch.equal(c["wa"], a) and not torch.equal(c["wbn"], b), tag + ": nothing rounds"
                if not torch.equal(c["const"], c["const_p"]):
                    const_differs.add((dt, C, p))
            else:
                assert torch.equal(c["wa"], a) and torch.equal(c["wbn"], b) and torch.equal(c["const"], c["const_p"]), tag
            n["banks"] += 1
        for i, (C, p, V, regime) in enumerate(post_plan()):
            c = post_case(dt, C, p, V, regime, 400 + i)
            tag = f"post {dt} C={C} p={p} V={V} {regime}"
            rounds = not torch.equal(c["hn"], c["hn_x"]) and \
                not torch.equal(c["wbn"], -c["cf"][1][:, None, :] * c["wd"][None])
            assert rounds == (regime == "round"), tag + ": Hn and wbn round in the rounding regime only"
            for v in range(1, V):   # a value taken from another view is a wrong value
                assert all(not torch.equal(t[v], t[0]) for t in c["cf"]) and not torch.equal(c["G"][v], c["G"][0]) and \
                    not torch.equal(c["P"][v], c["P"][0]) and not torch.equal(c["s"][v], c["s"][0]), tag + ": equal views"
            n["post"] += 1
        for i, geo in enumerate(UNIT_CASES):
            unit_case(dt, *geo, 500 + i)
            n["unit"] += 1
        for i, (K3, Kd, C, V, regime) in enumerate(scale_plan()):
            c = scale_case(dt, K3, Kd, C, V, regime, 600 + i)
            tag = f"scale_banks {dt} K3={K3} Kd={Kd} C={C} V={V} {regime}"
            for got, exact in ((c["o3"], c["o3x"]), (c["od"], c["odx"])):
                assert torch.equal(got, exact) == (regime == "repr"), tag + ": the scaled banks round in the rounding regime only"
            n["scale_banks"] += 1
    return n, const_differs


def test_case_table_preconditions():
    """CPU self-check: every case of every table satisfies the exactness preconditions it is run under, the rounding
    regime really rounds in every rounding case of the tables, and the tables hold the shapes the loop structures change at."""
    n, const_differs = all_preconditions()
    print("cases per entry point (both dtypes):", n)
    assert n == {"fwd_stats": 24, "stats": 26, "banks": 32, "post": 30, "unit": 4, "scale_banks": 20}
    # sm3_linbn_banks: in every rounding case of the table the centring constant of the rounded banks is not that of the
    # unrounded products
    assert const_differs == {(dt, C, p) for dt in DTS for C, p, _, regime in banks_plan() if regime == "round"}
    assert sorted({p for _, p, _, _ in fwd_plan()}) == FWD_P and sorted({C for C, _, _, _ in fwd_plan()}) == FWD_C
    assert {C for C, *_ in stats_plan()} >= {1, 3, 4, 5, 130} and {a[1] for a in stats_plan()} >= {1, 63, 64, 65, 200}
    assert {a[2] for a in stats_plan()} >= {1, 63, 64, 65}
    assert {a[3] * a[0] for a in stats_plan() if a[6] > 0} >= {1, 255, 256, 257, 390}
    assert {(C, p) for C, p, *_ in post_plan()} >= {(C, p) for C in (128, 384, 640) for p in (32, 96)} | {(2176, 32)}
    assert {(C, p) for C, p, *_ in banks_plan()} == {(C, p) for C in (8, 136, 2176) for p in (1, 3, 32)}
    for plan in (fwd_plan, banks_plan, post_plan, scale_plan):
        assert {a[2] if plan is not scale_plan else a[3] for a in plan()} == {1, 2, 3}


# ------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------
def _g(t, dt):
    return t.to(dt).reshape(-1).to(_dev()).contiguous()


def ops():
    from sm3hip import ops as o
    return o


def refusal():
    from sm3hip._lib import SM3LibraryError
    return (SM3LibraryError, ValueError)


def code(dt):
    return ops().dtype_code(dt)


def bits_equal(a, b, what):
    assert a.dtype == b.dtype and a.numel() == b.numel(), what
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[a.element_size()]
    eq = a.reshape(-1).view(it) == b.reshape(-1).view(it)
    assert bool(eq.all()), f"{what}: {int((~eq).sum())} of {a.numel()} differ in their bits"


def check(out, ref, what):
    same(out.t, ref, what)
    assert out.guards(), what + ": guard band written"


# ------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_fwd_stats_tiles_and_every_partial_row(dt):
    """sm3_linbn_fwd_stats: Tm = W G exactly and EVERY partial row of the batch sums, at the wave loads of tile_wg."""
    o, cd = ops(), code(dt)
    for C, p, V, seed in fwd_plan():
        c = fwd_case(dt, C, p, V, seed)
        tag = f"fwd_stats {dt} C={C} p={p} V={V}"
        Tm, ws = Guarded(V * C * p, F32), Guarded(V * (p // 32) * 2 * C, F64)
        assert o.linbn_fwd_stats(cd, _g(c["G"], F32), _g(c["wd"], dt), _g(c["W"], dt), _g(c["s"], F64), Tm.t, ws.t,
                               C, p, V) == p // 32
        torch.cuda.synchronize()
        check(Tm, c["Tm"], tag + " Tm")
        check(ws, c["ws"], tag + " partial rows")


def run_stats(o, cd, dt, c, tag):
    C, p, V = c["C"], c["p"], c["V"]
    ls = Guarded(V * 2 * C, F64)
    dg = Guarded(C, F32, c["dg0"].float()) if c["with_grads"] else None
    db = Guarded(C, F32, c["db0"].float()) if c["with_grads"] else None
    cf = Guarded(V * 4 * C, F32)
    o.linbn_stats(cd, _g(c["P"], F32), _g(c["W"], dt), _g(c["mean"], F32), _g(c["invstd"], F32),
                  _g(c["gamma"], F32) if c["gamma"] is not None else None, _g(c["ws"], F64), c["groups"], ls.t,
                  dg.t if dg else None, db.t if db else None, c["count"], cf.t, C, p, V)
    torch.cuda.synchronize()
    check(ls, c["lsums"], tag + " lsums = (S1 | S2)")
    if dg:
        check(dg, c["dg"], tag + " dgamma = start + S2")
        check(db, c["db"], tag + " dbeta = start + S1")
    return cf


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_stats_sums_gradients_and_coefficients(dt):
    """sm3_linbn_stats against the sums of the explicit x (the NaN half of reduce_ws is never read), and sm3_linbn_coef
    from the summed lsums: the same four numbers, the same bits."""
    o, cd = ops(), code(dt)
    for i, args in enumerate(stats_plan()):
        c = stats_case(dt, *args, 200 + i)
        C, V = c["C"], c["V"]
        tag = f"stats {dt} C={C} p={c['p']} groups={c['groups']} V={V} gamma={c['gamma'] is not None} count={c['count']}"
        cf = run_stats(o, cd, dt, c, tag)
        if c["count"] > 0:
            check(cf, c["coef"], tag + " coef")
            cf2 = Guarded(V * 4 * C, F32)
            o.linbn_coef(_g(c["lsums"], F64), c["count"], _g(c["gamma"], F32) if c["gamma"] is not None else None,
                         _g(c["mean"], F32), _g(c["invstd"], F32), cf2.t, C, V)
            torch.cuda.synchronize()
            check(cf2, c["coef"], tag + " linbn_coef")
            bits_equal(cf2.t, cf.t, tag + " coef of stats vs linbn_coef")
        else:
            assert cf.untouched(), tag + ": coef written with count = 0"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_banks_round_once_and_centre_on_the_rounded_products(dt):
    """sm3_linbn_banks: wa = T(a wd), wbn = T(-b wd), col_const from the ROUNDED banks."""
    o, cd = ops(), code(dt)
    for i, (C, p, V, regime) in enumerate(banks_plan()):
        c = banks_case(dt, C, p, V, regime, 300 + i)
        tag = f"banks {dt} C={C} p={p} V={V} {regime}"
        wa, wbn, cc = Guarded(V * p * C, dt), Guarded(V * p * C, dt), Guarded(V * p, F32)
        o.linbn_banks(cd, _g(c["wd"], dt), _g(coef4(c["cf"]), F32), wa.t, wbn.t, cc.t, C, p, V)
        torch.cuda.synchronize()
        check(wa, c["wa"], tag + " wa")
        check(wbn, c["wbn"], tag + " wbn")
        check(cc, c["const"], tag + " col_const")


def run_post(o, cd, dt, c, tag):
    """banks, post and banks_post on one case; every output against the definition, and the launch forms against each
    other bit for bit.  Returns the GPU's (wa, hn, col_const)."""
    C, p, V = c["C"], c["p"], c["V"]
    wd, cf = _g(c["wd"], dt), _g(coef4(c["cf"]), F32)
    P, G, Tm, s = _g(c["P"], F32), _g(c["G"], F32), _g(c["Tm"], F32), _g(c["s"], F64)
    wbn_in = _g(c["wbn"], dt)
    first = None
    for fused in (False, True):
        for tm in (Tm, None):
            form = ("banks_post" if fused else "post") + (" Tm" if tm is not None else " Tm=None")
            hn, dw = Guarded(V * p * p, dt), Guarded(C * p, F32, c["dw0"].float())
            if fused:
                wa, cc = Guarded(V * p * C, dt), Guarded(V * p, F32)
                o.linbn_banks_post(cd, wd, cf, wa.t, cc.t, hn.t, P, G, tm, s, dw.t, C, p, V)
            else:
                o.linbn_post(cd, wbn_in, wd, hn.t, P, G, tm, s, cf, dw.t, C, p, V)
            torch.cuda.synchronize()
            check(hn, c["hn"], f"{tag} {form} Hn")
            check(dw, c["dw"], f"{tag} {form} dw")
            if fused:
                check(wa, c["wa"], f"{tag} {form} wa")
                check(cc, c["const"], f"{tag} {form} col_const")
            if first is None:
                first = (hn, dw)
            else:
                bits_equal(hn.t, first[0].t, f"{tag} {form} Hn vs the first form")
                bits_equal(dw.t, first[1].t, f"{tag} {form} dw vs the first form")
    wa_b, wbn_b, cc_b = Guarded(V * p * C, dt), Guarded(V * p * C, dt), Guarded(V * p, F32)
    o.linbn_banks(cd, wd, cf, wa_b.t, wbn_b.t, cc_b.t, C, p, V)
    torch.cuda.synchronize()
    check(wbn_b, c["wbn"], tag + " banks wbn")
    bits_equal(wa_b.t, wa.t, tag + " wa of banks vs banks_post")
    bits_equal(cc_b.t, cc.t, tag + " col_const of banks vs banks_post")
    return wa, hn, cc


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_post_and_banks_post_against_the_definition(dt):
    """sm3_linbn_post (Tm given and recomputed) and sm3_linbn_banks_post: Hn = T(wbn wd^T) and dW = dw0 + sum dx^T y of the
    explicit dx; wa and col_const of the one-launch form as sm3_linbn_banks leaves them; all forms the same bits."""
    o, cd = ops(), code(dt)
    for i, (C, p, V, regime) in enumerate(post_plan()):
        c = post_case(dt, C, p, V, regime, 400 + i)
        run_post(o, cd, dt, c, f"{dt} C={C} p={p} V={V} {regime}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_scale_banks(dt):
    """sm3_linbn_scale_banks: both banks rounded once from the fp32 product, bias = shift3 + shiftd in one fp32 add."""
    o, cd = ops(), code(dt)
    for i, (K3, Kd, C, V, regime) in enumerate(scale_plan()):
        c = scale_case(dt, K3, Kd, C, V, regime, 600 + i)
        tag = f"scale_banks {dt} K3={K3} Kd={Kd} C={C} V={V} {regime}"
        o3, od, bias = Guarded(V * C * K3, dt), Guarded(V * C * Kd, dt), Guarded(V * C, F32)
        o.linbn_scale_banks(cd, _g(c["w3"], dt), _g(c["sc3"], F32), _g(c["sh3"], F32), o3.t, _g(c["wd"], dt),
                            _g(c["scd"], F32), _g(c["shd"], F32), od.t, bias.t, C, V)
        torch.cuda.synchronize()
        check(o3, c["o3"], tag + " out3")
        check(od, c["od"], tag + " outd")
        check(bias, c["bias"], tag + " bias")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("geo", UNIT_CASES, ids=[f"V{g[0]}-C{g[2]}-p{g[3]}" for g in UNIT_CASES])
def test_composed_backward_unit_gives_dx_W_exactly(geo, dt):
    """The GPU's wa, Hn and col_const through sm3_conv_dgrad_seg_bnfuse, wired as the engine wires it: dy = dx W of the
    definition, exactly (representable regime)."""
    o, cd = ops(), code(dt)
    V, Mv, C, p = geo
    c = unit_case(dt, V, Mv, C, p, 500 + UNIT_CASES.index(geo))
    wa, hn, cc = run_post(o, cd, dt, c, f"unit {dt} V={V} C={C} p={p}")
    M = V * Mv
    dd = o.dgrad_descs(cd, V, Mv, 1, p, C, 1, 1, 0)[0][0]
    prow = o.conv_partial_rows(dd)
    dy, part = Guarded(M * p, dt), torch.empty(prow * 2 * p, device=_dev())
    o.conv_dgrad_seg_bnfuse(dd, _g(c["dz"], dt), wa.t, _g(c["y"], dt), hn.t, cc.t, dy.t, None, None, None, None, part, 0,
                            views=V, row_offset_view1=prow // V, w_view_stride=p * C, w1_view_stride=p * p)
    torch.cuda.synchronize()
    check(dy, c["dy"], f"unit {dt} V={V} C={C} p={p}: dy = dx W")


# ------------------------------------------------------------------------------------------------------------------------
# refused calls
# ------------------------------------------------------------------------------------------------------------------------
class Outs:
    """Sentinel-filled outputs of every entry point for a launch of (C, p, V, K) that is going to be refused."""

    def __init__(self, dt, n=8192):
        self.all = {k: Guarded(n, d) for k, d in (("wa", dt), ("wbn", dt), ("hn", dt), ("o3", dt), ("od", dt), ("cc", F32),
                                                   ("dw", F32), ("Tm", F32), ("cf", F32), ("bias", F32), ("ws", F64),
                                                   ("ls", F64))}

    def __getattr__(self, k):
        return self.all[k].t

    def touched(self):
        return [k for k, g in self.all.items() if not g.untouched()]


def refused_calls(o, cd, dt, out, C, p, V, K3=8, Kd=8, count=64.0, G_given=True):
    """One lambda per entry point at (C, p, V); the inputs are generously sized zeros."""
    z = lambda d: torch.zeros(16384, dtype=d, device=_dev())  # noqa: E731
    f, d, w = z(F32), z(F64), z(dt)
    wn = lambda n: w[:max(n, 0)]  # noqa: E731
    G = f if G_given else None
    return {
        "fwd_stats": lambda: o.linbn_fwd_stats(cd, f, wn(p * C), wn(C * p), d, out.Tm, out.ws, C, p, V),
        "stats": lambda: o.linbn_stats(cd, f, wn(C * p), f, f, f, d, 1, out.ls, None, None, 0.0, out.cf, C, p, V),
        "coef": lambda: o.linbn_coef(d, count, f, f, f, out.cf, C, V),
        "banks": lambda: o.linbn_banks(cd, wn(p * C), f, out.wa, out.wbn, out.cc, C, p, V),
        "post": lambda: o.linbn_post(cd, w, wn(p * C), out.hn, f, G, None, d, f, out.dw[:max(C * p, 0)], C, p, V),
        "banks_post": lambda: o.linbn_banks_post(cd, wn(p * C), f, out.wa, out.cc, out.hn, f, G, None, d,
                                                 out.dw[:max(C * p, 0)], C, p, V),
        "scale_banks": lambda: o.linbn_scale_banks(cd, wn(C * K3), f, f, out.o3, w[8192:8192 + C * Kd], f, f, out.od,
                                                   out.bias, C, V),
    }


REFUSED = [  # (entry points, C, p, V, extra)
    (("post", "banks_post"), 64, 32, 1, {}), (("post", "banks_post"), 192, 32, 2, {}),       # C % 128
    (("post", "banks_post", "fwd_stats"), 128, 16, 1, {}), (("post", "banks_post", "fwd_stats"), 128, 48, 1, {}),  # p % 32
    (("fwd_stats",), 48, 32, 1, {}), (("fwd_stats",), 16, 32, 2, {}),                         # C % 32
    (("banks",), 12, 3, 1, {}), (("banks",), 4, 1, 2, {}), (("banks",), 130, 2, 1, {}),       # C % 8
    (("scale_banks",), 3, 32, 1, dict(K3=12, Kd=8)), (("scale_banks",), 3, 32, 1, dict(K3=8, Kd=4)),
    (("fwd_stats", "stats", "coef", "banks", "post", "banks_post", "scale_banks"), 128, 32, 0, {}),   # views = 0
    (("coef",), 8, 32, 1, dict(count=0.0)), (("coef",), 8, 32, 1, dict(count=-4.0)),
    (("post", "banks_post"), 128, 32, 1, dict(G_given=False)),                                # G and Tm both None
]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_refused_calls_write_nothing(dt):
    o, cd = ops(), code(dt)
    n = 0
    for names, C, p, V, extra in REFUSED:
        out = Outs(dt)
        calls = refused_calls(o, cd, dt, out, C, p, V, **extra)
        for nm in names:
            with pytest.raises(refusal()):
                calls[nm]()
            n += 1
        torch.cuda.synchronize()
        assert not out.touched(), f"C={C} p={p} V={V} {extra}: a refused call wrote {out.touched()}"
    assert n == 28


@pytest.mark.gpu
def test_f32_is_refused_with_edtype():
    """The kernels are 16-bit only: every dtype-taking entry point answers SM3_EDTYPE for f32 and writes nothing."""
    o = ops()
    from sm3hip._lib import SM3LibraryError
    out = Outs(F32)
    calls = refused_calls(o, code(F32), F32, out, 128, 32, 1)
    for nm in ("fwd_stats", "stats", "banks", "post", "banks_post", "scale_banks"):
        with pytest.raises(SM3LibraryError, match="SM3_EDTYPE"):
            calls[nm]()
    torch.cuda.synchronize()
    assert not out.touched(), f"an f32 launch wrote {out.touched()}"


# ------------------------------------------------------------------------------------------------------------------------
# only_if of the conditional weight preparations
# ------------------------------------------------------------------------------------------------------------------------
PREP_SHAPES = [(64, 9, 64), (33, 1, 48)]   # (Co, taps, Ci): on the 16-bit vector path / refused by it (odd Co)


def flag_of(v):
    return torch.full((1,), v, dtype=torch.int32, device=_dev())


class Prep:
    """One of the three conditional launches with sentinel-filled banks."""

    def __init__(self, kind, dt, masters=None):
        o = ops()
        self.kind, self.dt, self.cd = kind, dt, o.dtype_code(dt)
        g = torch.Generator().manual_seed(17)
        if kind == "batch":
            self.masters = masters or [torch.randn(Co * t * Ci, generator=g).to(_dev()) for Co, t, Ci in PREP_SHAPES]
            self.banks = [Guarded(m.numel(), dt) for m in self.masters for _ in range(2)]
            items = [(m, self.banks[2 * i].t, self.banks[2 * i + 1].t, Co, t, Ci, t * Ci)
                     for i, (m, (Co, t, Ci)) in enumerate(zip(self.masters, PREP_SHAPES))]
            self.table = o.weight_prep_table(items, _dev())
        elif kind == "stem":
            self.masters = [torch.randn(64 * 147, generator=g).to(_dev())]
            self.banks = [Guarded(64 * o.STEM_KDIRECT, dt)]
        else:
            self.masters = [torch.randn(128 * 9 * 4, generator=g).to(_dev())]
            self.banks = [Guarded(128 * 9 * 4, dt), Guarded(128 * 9 * 4, dt)]

    def run(self, only_if):
        o = ops()
        if self.kind == "batch":
            o.weight_prep_batch(self.cd, self.table, only_if=only_if)
        elif self.kind == "stem":
            o.stem_weight_prep(self.cd, self.masters[0], self.banks[0].t, only_if=only_if)
        else:
            o.gconv_weight_prep(self.cd, self.masters[0], 128, 32, self.banks[0].t, self.banks[1].t, only_if=only_if)
        torch.cuda.synchronize()
        return self


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ALL_DTS, ids=ALL_IDS)
@pytest.mark.parametrize("kind", ["batch", "stem", "gconv"])
def test_only_if_zero_skips_and_nonzero_prepares(kind, dt):
    """only_if holding 0: the banks stay untouched; 1, -1 or 2: the bits of the unconditional launch; the flag is only read."""
    want = Prep(kind, dt).run(None)
    assert all(b.guards() and not b.untouched() for b in want.banks)
    flag = flag_of(0)
    got = Prep(kind, dt).run(flag)
    assert all(b.untouched() for b in got.banks), f"{kind} {dt}: only_if = 0 wrote a bank"
    assert int(flag) == 0
    for v in (1, -1, 2):
        flag = flag_of(v)
        got = Prep(kind, dt).run(flag)
        for i, (a, b) in enumerate(zip(got.banks, want.banks)):
            bits_equal(a.t, b.t, f"{kind} {dt} only_if={v} bank {i}")
            assert a.guards()
        assert int(flag) == v, "the flag was written"


@pytest.mark.gpu
def test_only_if_chained_to_weights_changed():
    """sm3_weights_changed on a flat master sets the flag: the first call prepares, an unchanged master does not, one changed
    word prepares again."""
    o = ops()
    sizes = [Co * t * Ci for Co, t, Ci in PREP_SHAPES]
    flat = torch.randn(sum(sizes), generator=torch.Generator().manual_seed(23)).to(_dev())
    masters = [flat[:sizes[0]], flat[sizes[0]:]]
    state = torch.zeros(2, dtype=torch.int64, device=_dev())
    flag = flag_of(-7)
    pr = Prep("batch", BF16, masters)

    def step():
        o.weights_changed(flat, state, flag)
        pr.run(flag)
        return int(flag)

    def banks_are_current():
        return all(torch.equal(pr.banks[2 * i].t, m.to(BF16)) for i, m in enumerate(masters))

    assert step() == 1 and banks_are_current()
    for b in pr.banks:                       # wipe the banks: an unchanged master must leave them wiped
        b.buf.view(torch.uint8).fill_(0xA5)
    assert step() == 0 and all(b.untouched() for b in pr.banks)
    flat.view(torch.int32)[sizes[0] + 5] ^= 1   # one word of the second master
    assert step() == 1 and banks_are_current() and all(b.guards() for b in pr.banks)
    for b in pr.banks:
        b.buf.view(torch.uint8).fill_(0xA5)
    assert step() == 0 and all(b.untouched() for b in pr.banks)
