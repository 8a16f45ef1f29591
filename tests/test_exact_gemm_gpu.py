"""Bit-exact checks of the gather-GEMM family on integer inputs.

Every operand is a small integer times a power of two.  Every product is then exact in fp32, and so is every partial sum
whose magnitude stays below 2^24 quanta, whatever the summation order.  So every kernel variant, K order, tiling and split
must return exactly what torch gives when it rounds the exact fp64 result to the storage type (round to nearest even):
no tolerance.  That makes the atomic, fixed-order, nine-tap, halo and lean paths comparable to fp64 bit for bit.

The generator below checks those exactness preconditions in fp64 before a case runs (test_case_table_preconditions does it
for the whole table without a GPU).  Two regimes:
  representable: every output and every intermediate that is stored or rounded is exact in the storage type;
  rounding:      the outputs of a plain sum exceed it, and the final store must equal ref_fp64.to(dtype).
The epilogues with an affine step or an addend round the GEMM result to 16 bits BEFORE the addend on the lean path
(csrc/conv_igemm.hip, EPI 2 / 3): those cases stay in the representable regime, where one and two roundings agree.

Contracts pinned here besides the values: the ReLU bits are `stored y > 0` (strict, as threshold_backward); the BatchNorm partial
rows of a forward launch are the sums of the rounded GEMM result (before an addend); a fused BN-backward launch without x
writes 0 into the sum(dz * xhat) slot; outputs are compared with +0 and -0 identified.  Every output is a slice of a larger
buffer filled with a sentinel, and the bytes around it must come back unchanged.

sm3_conv_bn_eval -- the one launch of every frozen-encoder forward, scale / shift derived per output channel in the epilogue
(ep_affine, csrc/conv_common.h) -- runs the whole forward table next to sm3_conv_bn_act_eval: BatchNorm tensors with
running_var a power of four and eps = 0 make every step of the derivation exact (bn_operands), so its outputs equal fp64
and the other entry point's bits; on real values the two are compared bit for bit over the same table.
"""
import pytest
import torch
import torch.nn.functional as F

from exact_inputs import (SENTINEL, Guarded, _dev, draw, env, ep_affine_exact, mask_bytes, need_exact, need_repr, pick,
                          quantum, same, stem_wgrad_case)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IDS = ["f32", "bf16", "f16"]
KCH = {F32: 32, BF16: 64, F16: 64}  # elements per 128-byte K chunk
EPC = {F32: 4, BF16: 8, F16: 8}     # elements per ReLU-mask byte (one 16-byte vector)
LAUNCHES = [0]


# ------------------------------------------------------------------------------------------------------------------------
# exact-input generator and its preconditions (CPU only)
# ------------------------------------------------------------------------------------------------------------------------
def tile_sums(rows, tiles=None):
    """[M, C] -> per-128-row sums [tiles, C] (fp64)."""
    M, C = rows.shape
    tiles = tiles or (M + 127) // 128
    pad = torch.zeros(tiles * 128, C, dtype=torch.float64)
    pad[:M] = rows
    return pad.view(tiles, 128, C).sum(1)


def conv_ref(x, w, s, p):
    """x NHWC, w OHWI (fp64) -> NHWC."""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=s, padding=p).permute(0, 2, 3, 1).contiguous()


def dgrad_ref(dy, w, x_shape, s, p):
    """Data gradient of conv_ref: dy NHWC [N, Ho, Wo, Co], w OHWI -> NHWC [N, H, W, Ci]."""
    N, H, W, Ci = x_shape
    g = torch.nn.grad.conv2d_input((N, Ci, H, W), w.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), stride=s, padding=p)
    return g.permute(0, 2, 3, 1).contiguous()


def wgrad_ref(x, dy, w_shape, s, p, groups=1):
    """dW (OHWI) of conv_ref."""
    Co, k, _, Ci = w_shape
    g = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (Co, Ci, k, k), dy.permute(0, 3, 1, 2), stride=s, padding=p,
                                    groups=groups)
    return g.permute(0, 2, 3, 1).contiguous()


def ci_for(dt, ci16):
    """The edge-table Ci of the 16-bit types (odd K-chunk counts) and its f32 twin."""
    return ci16 if dt != F32 else ci16 // 2


def pick_density(K, nnz):
    """Operand density giving about `nnz` nonzero products per output."""
    return min(0.9, (nnz / max(K, 1)) ** 0.5)


# Edge-shape table of the forward / data-gradient / weight-gradient sections (16-bit Ci; f32 uses half of it):
#   name, N, H, W, Ci, Co, k, stride, pad
FWD_CASES = [
    ("M1", 1, 1, 1, 64, 8, 1, 1, 0),                 # M = 1
    ("M127_Wo1", 1, 127, 1, 192, 24, 1, 1, 0),       # M = 127, Wo = 1
    ("M128", 1, 8, 16, 320, 72, 1, 1, 0),            # M = 128, Co tail in a 64-column tile
    ("M129", 3, 43, 1, 64, 136, 1, 1, 0),            # M = 129, Co tail in a 128-column tile
    ("1x1s2_odd", 2, 13, 11, 192, 200, 1, 2, 0),
    ("1x1s2_even", 2, 16, 18, 64, 128, 1, 2, 0),     # 64-multiple control
    ("3x3_H1", 2, 1, 37, 64, 72, 3, 1, 1),
    ("3x3_W1", 2, 29, 1, 192, 24, 3, 1, 1),          # Wo = 1
    ("3x3_2x3", 5, 2, 3, 64, 200, 3, 1, 1),
    ("3x3_7x7", 3, 7, 7, 320, 136, 3, 1, 1),
    ("3x3_13x11", 2, 13, 11, 64, 64, 3, 1, 1),
    ("3x3_61x59", 1, 61, 59, 64, 8, 3, 1, 1),        # halo image of the 64-column tile at its width limit
    ("3x3_29_wide", 9, 29, 29, 64, 136, 3, 1, 1),    # > 96 tiles of 128 columns: wide; 120 blocks, halo with DEEP=0
    ("3x3_59_wide", 2, 59, 59, 64, 200, 3, 1, 1),    # wide, chunk-outer order without the halo image (DEEP=0)
    ("3x3_29_264blk", 20, 29, 29, 64, 136, 3, 1, 1),  # wide, 264 blocks: not deep, the 128-column halo kernel by default
    ("3x3s2_odd", 2, 13, 11, 192, 24, 3, 2, 1),
    ("3x3s2_even", 2, 14, 16, 64, 72, 3, 2, 1),
    ("3x3s2_Wo1", 3, 9, 2, 64, 136, 3, 2, 1),        # Wo = 1
]
# grids of t = 1 .. 17 tiles of 128 x 64 (the XCD remap with nwg % 8 != 0): 1x1, Co = 64
GRID_CASES = [(f"grid{t}", t, 8, 16, 64, 64, 1, 1, 0) for t in range(1, 18)]
# two views in one launch (M / 2 a multiple of 128, dense output)
VIEW2_CASES = [("v2_1x1", 2, 8, 16, 192, 24, 1, 1, 0), ("v2_3x3", 4, 8, 8, 64, 136, 3, 1, 1),
               ("v2_3x3_72", 2, 16, 16, 320, 72, 3, 1, 1)]
# the deep K loop's threshold: 256 and 257 blocks of 128 x 64
DEEP_CASES = [("deep256", 2, 128, 128, 64, 64, 3, 1, 1), ("deep257", 1, 257, 128, 64, 64, 3, 1, 1)]
# the case on which sm3_conv_bn_eval's gamma-alone and beta-alone forms are pinned (Co tail in a 128-column tile, M = 30)
HALF_AFFINE_CASE = FWD_CASES[8]
# weight-gradient channel counts (multiples of 8)
WGRAD_CH = [(8, 8), (24, 40), (40, 24), (8, 136)]


def fwd_case(dt, case, regime, seed, views=1):
    """Operands and exact references of one forward case.  regime 'repr': outputs, the affine/addend forms and partial
    sums exact in dt; 'round': the plain sum only, rounded once (partials checked where exact)."""
    name, N, H, W, ci16, Co, k, s, p = case
    Ci = ci_for(dt, ci16)
    g = torch.Generator().manual_seed(seed)
    K = k * k * Ci
    if regime == "repr":
        d = pick_density(K, 6)
        x = draw(g, (N, H, W, Ci), 2, d, -1)
        w = draw(g, (Co, k, k, Ci), 1, d, 1)
    else:
        nnz = 400 if dt == F16 else 3
        d = pick_density(K, nnz)
        x = draw(g, (N, H, W, Ci), 15, d, -2)
        w = draw(g, (Co, k, k, Ci), 15, d, 1 if dt == F16 else 0)
    y = conv_ref(x, w, s, p)
    Ho, Wo = y.shape[1:3]
    ya = conv_ref(x.abs(), w.abs(), s, p)
    c = dict(name=name, dt=dt, N=N, H=H, W=W, Ci=Ci, Co=Co, k=k, s=s, p=p, Ho=Ho, Wo=Wo, M=N * Ho * Wo, x=x, w=w, y=y,
             regime=regime)
    need_exact(ya, quantum(x) * quantum(w), f"{name}: conv sum")
    yr = y.to(dt).double()
    rows = yr.reshape(-1, Co)
    qy = quantum(rows)
    c["check_partials"] = regime == "repr" or dt == BF16
    if c["check_partials"]:
        need_exact(tile_sums(rows.abs()), qy, f"{name}: partial sum(y)")
        need_exact(tile_sums(rows * rows), qy * qy, f"{name}: partial sum(y^2)")
    if regime == "round":
        return c
    need_repr(y, dt, f"{name}: y")
    # affine / addend / residual forms, dyadic scale and shift per view
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0, -0.5])[torch.randint(0, 5, (views, Co), generator=g)].double()
    shift = draw(g, (views, Co), 4, 0.8, -1)
    res = draw(g, (N, Ho, Wo, Co), 3, 0.5, -1)
    vrows = torch.zeros(c["M"], dtype=torch.long)
    if views == 2:
        vrows[c["M"] // 2:] = 1
    aff = (y.reshape(-1, Co) * scale[vrows] + shift[vrows]).reshape(y.shape)
    c.update(scale=scale, shift=shift, res=res, aff=aff, vrows=vrows)
    for t, nm in ((y + res, "y + addend"), (aff, "affine"), (aff + res, "affine + residual")):
        need_repr(t, dt, f"{name}: {nm}")
        need_repr(t, F32, f"{name}: {nm} (fp32)")
    if views == 1:  # (drawn last: the operands above are those of the earlier forms, value for value)
        bn_operands(c, g)
    return c


RV_VALUES = (0.25, 1.0, 4.0, 16.0)  # powers of four: sqrtf and the reciprocal are exact


def bn_operands(c, g):
    """BatchNorm tensors of sm3_conv_bn_eval for the forward case c (one view, eps = 0), in two sets.
    Affine: gamma, beta, rm, rv from which ep_affine derives exactly the case's dyadic scale / shift (so `aff` is its reference
    too): rv a power of four, gamma = scale * sqrt(rv), rm a small integer, beta = shift + rm * scale.
    No affine (gamma = beta = NULL): scale_na = 1 / sqrt(rv), shift_na = -rm / sqrt(rv), reference aff_na.
    gamma alone / beta alone (the header: the missing one is 1 / 0): references aff_g / aff_b, checked where a test uses them
    (half_affine_refs)."""
    name, dt, Co, y = c["name"], c["dt"], c["Co"], c["y"]
    scale, shift = c["scale"][0], c["shift"][0]
    rv = pick(g, torch.tensor(RV_VALUES, dtype=torch.float64), (Co,))
    rm = draw(g, (Co,), 3, 0.8, 0)
    gamma = scale * rv.sqrt()
    beta = shift + rm * scale
    sc, sh = ep_affine_exact(gamma, beta, rm, rv, 0.0, f"{name}: BatchNorm operands")
    assert torch.equal(sc, scale) and torch.equal(sh, shift), f"{name}: the BatchNorm operands do not give scale / shift back"
    scale_na, shift_na = ep_affine_exact(None, None, rm, rv, 0.0, f"{name}: BatchNorm operands, no affine")
    assert torch.equal(scale_na, 1.0 / rv.sqrt()) and torch.equal(shift_na, -rm / rv.sqrt())
    aff_na = (y.reshape(-1, Co) * scale_na + shift_na).reshape(y.shape)
    for t, nm in ((aff_na, "no-affine BatchNorm"), (aff_na + c["res"], "no-affine BatchNorm + residual")):
        need_repr(t, dt, f"{name}: {nm}")
        need_repr(t, F32, f"{name}: {nm} (fp32)")
    c.update(gamma=gamma, beta=beta, rm=rm, rv=rv, scale_na=scale_na, shift_na=shift_na, aff_na=aff_na)


def half_affine_refs(c):
    """gamma given with beta NULL, and the reverse, on the operands of bn_operands: (aff_g, aff_b), each representable with and
    without the residual."""
    Co, y = c["Co"], c["y"]
    out = []
    for gam, bet, nm in ((c["gamma"], None, "gamma alone"), (None, c["beta"], "beta alone")):
        sc, sh = ep_affine_exact(gam, bet, c["rm"], c["rv"], 0.0, f"{c['name']}: {nm}")
        a = (y.reshape(-1, Co) * sc + sh).reshape(y.shape)
        for t in (a, a + c["res"]):
            need_repr(t, c["dt"], f"{c['name']}: {nm}")
            need_repr(t, F32, f"{c['name']}: {nm} (fp32)")
        out.append(a)
    return out


def seg_case(dt, M, Ci, Ci1, Co, views, seed):
    """Two K segments over the same pixels with a per-view column bias (16-bit only), representable regime."""
    g = torch.Generator().manual_seed(seed)
    d = pick_density(Ci + Ci1, 6)
    x0, x1 = draw(g, (M, Ci), 2, d, -1), draw(g, (M, Ci1), 2, d, 0)
    w0, w1 = draw(g, (views, Co, Ci), 1, d, 1), draw(g, (views, Co, Ci1), 1, d, -1)
    cb = draw(g, (views, Co), 6, 0.8, -1)
    add = draw(g, (M, Co), 3, 0.5, -1)
    vr = torch.zeros(M, dtype=torch.long)
    if views == 2:
        vr[M // 2:] = 1
    y = torch.einsum("mk,mnk->mn", x0, w0[vr]) + torch.einsum("mk,mnk->mn", x1, w1[vr]) + cb[vr]
    ya = torch.einsum("mk,mnk->mn", x0.abs(), w0[vr].abs()) + torch.einsum("mk,mnk->mn", x1.abs(), w1[vr].abs())
    need_exact(ya + cb[vr].abs(), min(quantum(x0) * quantum(w0), quantum(x1) * quantum(w1), quantum(cb)), "seg sum")
    for t, nm in ((y, "y"), (y + add, "y + addend")):
        need_repr(t, dt, f"seg {nm}")
    return dict(x0=x0, x1=x1, w0=w0, w1=w1, cb=cb, add=add, y=y, vr=vr)


def dgrad_case(dt, case, with_x, seed, views=1):
    """Data gradient of a forward case: dz = mask ? conv^T(dy) + addend : 0, with the producer BatchNorm's phase-1 sums
    (sum dz, sum dz * xhat) per 128-row tile of each parity-class launch.  Representable regime."""
    name, N, H, W, ci16, co16, k, s, p = case
    Cf = ci_for(dt, ci16)      # the forward conv's output channels = the data gradient's K (a K-chunk multiple)
    Cout = co16                # the data gradient's output channels (the forward Ci: any multiple of 8 / 4)
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = pick_density(k * k * Cf, 6)
    dy = draw(g, (N, Ho, Wo, Cf), 2, d, -1)
    w = draw(g, (Cf, k, k, Cout), 1, d, 1)  # forward OHWI weight: [Co_fwd = Cf][k][k][Ci_fwd = Cout]
    dx = dgrad_ref(dy, w, (N, H, W, Cout), s, p)
    dxa = dgrad_ref(dy.abs(), w.abs(), (N, H, W, Cout), s, p)
    need_exact(dxa, quantum(dy) * quantum(w), f"{name}: dgrad sum")
    add = draw(g, (N, H, W, Cout), 3, 0.5, -1)
    mask = torch.rand(N, H, W, Cout, generator=g) < 0.7
    mean = draw(g, (views, Cout), 6, 0.9, -2)                                   # on a 1/4 grid
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (views, Cout), generator=g)].double()
    bx = draw(g, (N, H, W, Cout), 8, 0.9, 0) if with_x else None
    c = dict(name=name, dt=dt, N=N, H=H, W=W, Cf=Cf, Cout=Cout, k=k, s=s, p=p, Ho=Ho, Wo=Wo, dy=dy, w=w, dx=dx, add=add,
             mask=mask, mean=mean, invstd=invstd, bx=bx)
    for t, nm in ((dx, "dx"), (dx + add, "dx + addend")):
        need_repr(t, dt, f"{name}: {nm}")
    if bx is not None:
        need_repr(bx, dt, f"{name}: x")
    return c


def dgrad_expect(c, add_mode, views=1):
    """Per parity-class launch: (dz over the full output, {class: (rows m -> output pixel index, partial rows)})."""
    N, H, W, C, s = c["N"], c["H"], c["W"], c["Cout"], c["s"]
    v = c["dx"].clone()
    if add_mode == "dense":
        v = v + c["add"]
    elif add_mode == "compact":  # present at the even pixels only
        ev = torch.zeros_like(v)
        ev[:, ::2, ::2] = c["add"][:, ::2, ::2]
        v = v + ev
    dz = torch.where(c["mask"], v, torch.zeros_like(v))
    pix_view = torch.zeros(N, H, W, dtype=torch.long)
    if views == 2:
        pix_view[N // 2:] = 1
    if c["bx"] is not None:
        xhat = (c["bx"] - c["mean"][pix_view]) * c["invstd"][pix_view]
    else:
        xhat = torch.zeros_like(dz)
    classes = {}
    for py in range(s):
        for px in range(s):
            sub_dz = dz[:, py::s, px::s]
            if sub_dz.shape[1] == 0 or sub_dz.shape[2] == 0:
                continue
            rows_dz = sub_dz.reshape(-1, C)
            rows_t = (sub_dz * xhat[:, py::s, px::s]).reshape(-1, C)
            if views == 2:
                half = rows_dz.shape[0] // 2
                parts = [(tile_sums(rows_dz[:half]), tile_sums(rows_t[:half])),
                         (tile_sums(rows_dz[half:]), tile_sums(rows_t[half:]))]
                ta = [(tile_sums(rows_dz[:half].abs()), tile_sums(rows_t[:half].abs())),
                      (tile_sums(rows_dz[half:].abs()), tile_sums(rows_t[half:].abs()))]
            else:
                parts = [(tile_sums(rows_dz), tile_sums(rows_t))]
                ta = [(tile_sums(rows_dz.abs()), tile_sums(rows_t.abs()))]
            for (a1, a2) in ta:
                need_exact(a1, quantum(dz), f"{c['name']}: sum dz")
                need_exact(a2, quantum(dz) * quantum(xhat) if c["bx"] is not None else 1.0, f"{c['name']}: sum dz*xhat")
            classes[(py, px)] = parts
    return dz, classes


def wgrad_case(dt, N, H, W, Ci, Co, k, s, p, seed, prior=True):
    """dW (fp32, OHWI) += the weight gradient; integer prior value in dw."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = pick_density(N * Ho * Wo, 40)
    x = draw(g, (N, H, W, Ci), 7, d, -1)
    dy = draw(g, (N, Ho, Wo, Co), 7, d, 1)
    dw0 = draw(g, (Co, k, k, Ci), 5, 0.5, 0) if prior else torch.zeros(Co, k, k, Ci, dtype=torch.float64)
    ref = wgrad_ref(x, dy, (Co, k, k, Ci), s, p)
    refa = wgrad_ref(x.abs(), dy.abs(), (Co, k, k, Ci), s, p)
    q = min(quantum(x) * quantum(dy), quantum(dw0))
    need_exact(refa + dw0.abs(), q, "wgrad sum")
    need_repr(x, dt, "wgrad x")
    need_repr(dy, dt, "wgrad dy")
    return dict(N=N, H=H, W=W, Ci=Ci, Co=Co, k=k, s=s, p=p, Ho=Ho, Wo=Wo, x=x, dy=dy, dw0=dw0, ref=ref)


def wgrad_cases(dt):
    out = []
    for i, (_, N, H, W, ci16, Co, k, s, p) in enumerate(FWD_CASES):
        if H * W * N > 4000:
            continue
        out.append(("tab_" + FWD_CASES[i][0], (N, H, W, ci_for(dt, ci16), Co, k, s, p)))
    for Ci, Co in WGRAD_CH:  # channel counts only the weight gradient accepts
        if dt == F32 or Ci % 8 == 0:
            out.append((f"ch{Ci}x{Co}_3x3", (2, 9, 7, Ci, Co, 3, 1, 1)))
            out.append((f"ch{Ci}x{Co}_1x1s2", (3, 10, 9, Ci, Co, 1, 2, 0)))
    # nine-tap owner geometries (16-bit, Co and Ci multiples of 64, maps whose rows fill 16-pixel K blocks)
    out.append(("nine_16x16", (2, 16, 16, 64, 128, 3, 1, 1)))
    out.append(("nine_8x8", (4, 8, 8, 128, 64, 3, 1, 1)))
    out.append(("nine_28x28", (2, 28, 28, 64, 64, 3, 1, 1)))
    return out


def dgrad_seg_case(dt, M, Ci, Ci1, Co, views, seed):
    """conv_dgrad_seg_bnfuse: dz = mask(two-segment product + col_bias) and its phase-1 sums per 128-row tile."""
    c = seg_case(dt, M, Ci, Ci1, Co, views, seed)
    g = torch.Generator().manual_seed(M)
    c["mbits"] = torch.rand(M, Co, generator=g) < 0.6
    c["bx"] = draw(g, (M, Co), 8, 0.9, 0)
    c["mean"] = draw(g, (views, Co), 6, 0.9, -2)
    c["invstd"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (views, Co), generator=g)].double()
    dz = torch.where(c["mbits"], c["y"], torch.zeros_like(c["y"]))
    xhat = (c["bx"] - c["mean"][c["vr"]]) * c["invstd"][c["vr"]]
    need_repr(c["bx"], dt, "dgrad seg x")
    need_exact(tile_sums(dz.abs()), quantum(dz), "dgrad seg sum dz")
    need_exact(tile_sums((dz * xhat).abs()), quantum(dz) * quantum(xhat), "dgrad seg sum dz*xhat")
    c.update(dz=dz, xhat=xhat)
    return c


def wgrad_cat2_case(dt):
    """conv_wgrad_cat with a second output (Co a multiple of 128), two views."""
    g = torch.Generator().manual_seed(41)
    N, H, W, Ci, Co, Co1 = 4, 6, 5, KCH[dt], 128, 72
    x = draw(g, (N, H, W, Ci), 7, 0.5, 0)
    dy0, dy1 = draw(g, (N, H, W, Co), 7, 0.5, 0), draw(g, (N, H, W, Co1), 7, 0.5, -1)
    refs = []
    for vi in range(2):
        sl = slice(2 * vi, 2 * vi + 2)
        for dy, C in ((dy0, Co), (dy1, Co1)):
            need_exact(wgrad_ref(x[sl].abs(), dy[sl].abs(), (C, 1, 1, Ci), 1, 0), quantum(x) * quantum(dy), "cat sum")
        refs.append((wgrad_ref(x[sl], dy0[sl], (Co, 1, 1, Ci), 1, 0), wgrad_ref(x[sl], dy1[sl], (Co1, 1, 1, Ci), 1, 0)))
    return dict(N=N, H=H, W=W, Ci=Ci, Co=Co, Co1=Co1, x=x, dy0=dy0, dy1=dy1, refs=refs)


def grouped_case(rows, G, K, N):
    g = torch.Generator().manual_seed(rows + G)
    x = draw(g, (rows, G * K), 3, pick_density(K, 6), -1)
    w = draw(g, (G, N, K), 2, pick_density(K, 6), 1)
    dy = draw(g, (rows, G * N), 5, 0.5, 0)
    xg = x.view(rows, G, K)
    y = torch.einsum("rgk,gnk->rgn", xg, w).reshape(rows, G * N)
    dw = torch.einsum("rgn,rgk->gnk", dy.view(rows, G, N), xg)
    need_exact(torch.einsum("rgk,gnk->rgn", xg.abs(), w.abs()), quantum(x) * quantum(w), "grouped y")
    need_exact(tile_sums(y.abs()), quantum(y), "grouped partial sum")
    need_exact(tile_sums(y * y), quantum(y) ** 2, "grouped partial sum sq")
    need_exact(torch.einsum("rgn,rgk->gnk", dy.abs().view(rows, G, N), xg.abs()), quantum(x) * quantum(dy), "grouped dw")
    return dict(x=x, w=w, dy=dy, y=y, dw=dw)


def gconv_case(dt, C, G, H, s, N):
    g = torch.Generator().manual_seed(C + H)
    cg = C // G
    Ho = (H - 1) // s + 1
    x = draw(g, (N, H, H, C), 2, pick_density(9 * cg, 6), -1)
    master = draw(g, (C, 3, 3, cg), 1, pick_density(9 * cg, 6), 1)
    dy = draw(g, (N, Ho, Ho, C), 2, pick_density(9 * cg, 6), 0)
    xn, wn, dyn = x.permute(0, 3, 1, 2), master.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    y = F.conv2d(xn, wn, stride=s, padding=1, groups=G).permute(0, 2, 3, 1).reshape(-1, C)
    dx = torch.nn.grad.conv2d_input(xn.shape, wn, dyn, stride=s, padding=1, groups=G).permute(0, 2, 3, 1).reshape(-1, C)
    dw = wgrad_ref(x, dy, (C, 3, 3, cg), s, 1, groups=G).reshape(C, -1)
    ya = F.conv2d(xn.abs(), wn.abs(), stride=s, padding=1, groups=G)
    dxa = torch.nn.grad.conv2d_input(xn.shape, wn.abs(), dyn.abs(), stride=s, padding=1, groups=G)
    dwa = wgrad_ref(x.abs(), dy.abs(), (C, 3, 3, cg), s, 1, groups=G)
    need_exact(ya, quantum(x) * quantum(master), "gconv y")
    need_exact(dxa, quantum(dy) * quantum(master), "gconv dx")
    need_exact(dwa, quantum(x) * quantum(dy), "gconv dw")
    need_exact(tile_sums(y.abs()), quantum(y), "gconv partial sum")
    need_exact(tile_sums(y * y), quantum(y) ** 2, "gconv partial sum sq")
    for t, nm in ((y, "y"), (dx, "dx")):
        need_repr(t, dt, f"gconv {nm}")
    return dict(x=x, master=master, dy=dy, y=y, dx=dx, dw=dw, Ho=Ho)


# per-launch switches of conv_igemm.hip: each value of each switch at least once
CONV_ENVS = [
    {},
    {"SM3_CONV_LEAN": 0},
    {"SM3_CONV_DEEP": 0},
    {"SM3_CONV_HALO": 0},
    {"SM3_CONV_PW": 0},
    {"SM3_CONV_PW": 1},
    {"SM3_CONV_PW": 2},
    {"SM3_CONV_FORCE_NARROW": 1},
    {"SM3_CONV_LEAN": 0, "SM3_CONV_DEEP": 0, "SM3_CONV_FORCE_NARROW": 1},
    {"SM3_CONV_HALO": 0, "SM3_CONV_PW": 0, "SM3_CONV_DEEP": 0, "SM3_CONV_FORCE_NARROW": 1},
]


def fwd_envs(case):
    """The small cases run every switch setting.  The large ones run the defaults, the general epilogue, DEEP=0 (halo on,
    128-column tiles: the one-stage wide kernels, halo or chunk-outer, that the deep loop replaces at up to 256 blocks)
    and the combined setting."""
    return CONV_ENVS if case[1] * case[2] * case[3] <= 4000 else [CONV_ENVS[i] for i in (0, 1, 2, 8)]


# What each GPU test runs: (case, regime, seed, views, envs, parts), parts "all" = plain + every epilogue form, "plain" or
# "epi" one of them.  The CPU self-check walks the same plans with the same seeds.
def fwd_plan(dt):
    i = DTYPES.index(dt)
    for case in FWD_CASES:
        yield case, "repr", 100 + i, 1, fwd_envs(case), "all"
        if dt != F32:
            yield case, "round", 200 + i, 1, fwd_envs(case), "plain"
    for case in VIEW2_CASES:
        yield case, "repr", 600, 2, CONV_ENVS, "epi"


def grid_plan(dt):
    seed = 110 + DTYPES.index(dt)
    for case in GRID_CASES:
        yield case, "repr", seed, 1, [CONV_ENVS[0], CONV_ENVS[1], CONV_ENVS[4]], "plain"
        if case[1] % 2 == 0:
            yield case, "repr", 600, 2, [CONV_ENVS[0]], "epi"
    for case in DEEP_CASES:
        yield case, "repr", seed, 1, [CONV_ENVS[0], CONV_ENVS[2], CONV_ENVS[3]], "plain"
        if case[0] == "deep256":
            yield case, "repr", 600, 2, [CONV_ENVS[0], CONV_ENVS[2]], "epi"


SEG_FWD = [(256, 64, 128, 136, 2), (384, 192, 64, 24, 1), (129, 64, 128, 136, 1), (1, 64, 64, 8, 1), (512, 320, 64, 200, 2)]
SEG_DGRAD = [(256, 64, 128, 136, 2), (384, 192, 64, 24, 1), (129, 64, 128, 72, 1), (512, 64, 64, 8, 2)]


def dgrad_plan(dt):
    """(case, with_x, seed, views, [(addend mode, envs)])"""
    seed = 300 + DTYPES.index(dt)
    for case in FWD_CASES:
        envs = fwd_envs(case)
        for with_x in (True, False):
            modes = [("dense", envs), ("compact", envs[:3])] if with_x else [("none", envs)]
            yield case, with_x, seed, 1, modes
    for case in VIEW2_CASES:
        for with_x in (True, False):
            yield case, with_x, seed + 7, 2, [("dense" if with_x else "none", CONV_ENVS)]


def wgrad_plan(dt):
    for i, (name, geo) in enumerate(wgrad_cases(dt)):
        yield name, geo, 400 + DTYPES.index(dt) + i


GROUPED = [(129, 4, 32, 8), (1, 3, 64, 24), (384, 2, 96, 136), (2176, 8, 32, 64), (300, 5, 160, 200)]
GCONV = [(128, 32, 16, 1, 2), (256, 32, 16, 2, 2), (256, 64, 3, 1, 2), (1024, 32, 4, 2, 1),  # ResNeXt shapes
         (128, 32, 13, 2, 3), (64, 16, 7, 1, 1)]                                            # + odd-map tails


def all_preconditions():
    """Every case the GPU tests below draw, through the same plans, seeds and generator (and its asserts)."""
    n = 0
    for dt in DTYPES:
        for plan in (fwd_plan, grid_plan):
            for case, regime, seed, views, _, _ in plan(dt):
                fwd_case(dt, case, regime, seed, views=views)
                n += 1
        for case, with_x, seed, views, modes in dgrad_plan(dt):
            c = dgrad_case(dt, case, with_x, seed, views=views)
            for mode, _ in modes:
                dgrad_expect(c, mode, views)
                n += 1
        for name, geo, seed in wgrad_plan(dt):
            wgrad_case(dt, *geo, seed=seed)
            n += 1
        wgrad_cat2_case(dt)
        if dt != F32:
            for M, Ci, Ci1, Co, views in SEG_FWD:
                seg_case(dt, M, Ci, Ci1, Co, views, 500 + M)
            for M, Ci, Ci1, Co, views in SEG_DGRAD:
                dgrad_seg_case(dt, M, Ci, Ci1, Co, views, 700 + M)
            n += len(SEG_FWD) + len(SEG_DGRAD)
        for geo in GCONV:
            gconv_case(dt, *geo)
            n += 1
        for i, geo in enumerate(STEM_GEOMS):
            stem_case(*geo[:3], 800 + i)
            stem_wgrad_case(dt, *geo, 900 + i)
            n += 2
    for geo in GROUPED:
        grouped_case(*geo)
        n += 1
    return n


def test_case_table_preconditions():
    """CPU self-check: every case of the tables satisfies the exactness preconditions it is run under."""
    assert all_preconditions() > 300
    # the rounding regime really rounds (the check is not vacuous)
    c = fwd_case(BF16, FWD_CASES[12], "round", 201)
    assert not torch.equal(c["y"].to(BF16).double(), c["y"])
    c = fwd_case(F16, FWD_CASES[12], "round", 202)
    assert not torch.equal(c["y"].to(F16).double(), c["y"])
    # zeros are common enough to exercise the strict ReLU bit
    c = fwd_case(BF16, FWD_CASES[10], "repr", 101)
    assert int((c["aff"] + c["res"] == 0).sum()) > 100
    # the BatchNorm operand sets of sm3_conv_bn_eval: built (and checked, bn_operands) for every case of the table in every
    # dtype, through the plan the GPU test walks; every variance value and both signs of the mean occur, and the no-affine
    # form is another function than the affine one
    n_bn, seen_rv = 0, set()
    for dt in DTYPES:
        planned = {case[0]: (case, seed) for case, regime, seed, views, _, parts in fwd_plan(dt)
                   if regime == "repr" and views == 1 and parts == "all"}
        assert list(planned) == [case[0] for case in FWD_CASES]
        for case, seed in planned.values():
            c = fwd_case(dt, case, "repr", seed)
            assert all(c[k].shape == (c["Co"],) for k in ("gamma", "beta", "rm", "rv")), case[0]
            assert bool((c["rv"] > 0).all()) and not torch.equal(c["aff_na"], c["aff"]), case[0]
            assert bool((c["rm"] != 0).any()), case[0]
            seen_rv |= set(c["rv"].tolist())
            n_bn += 1
        half_affine_refs(fwd_case(dt, HALF_AFFINE_CASE, "repr", 100 + DTYPES.index(dt)))
    assert n_bn == 3 * len(FWD_CASES) and seen_rv == set(RV_VALUES)
    # a neighbouring channel's statistics give another result in every case: a launch that derived its scale / shift from
    # channel c ^ 1 cannot pass
    for case in FWD_CASES:
        c = fwd_case(F16, case, "repr", 102)
        sw = torch.arange(c["Co"]) ^ 1
        wrong = c["y"].reshape(-1, c["Co"]) * c["scale_na"][sw] + c["shift_na"][sw]
        assert not torch.equal(wrong.reshape(c["y"].shape).clamp_min(0), c["aff_na"].clamp_min(0)), case[0]


# ------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------
def _g(t, dt):
    return t.to(dt).to(_dev()).contiguous()


def launch(fn, *a, **k):
    LAUNCHES[0] += 1
    return fn(*a, **k)


def ops():
    from sm3hip import ops as o
    return o


def desc_of(c):
    o = ops()
    return o.fwd_desc(o.dtype_code(c["dt"]), c["N"], c["H"], c["W"], c["Ci"], c["Co"], c["k"], c["s"], c["p"])


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
def run_plain(c, envs, with_partials):
    o, dt = ops(), c["dt"]
    d = desc_of(c)
    x, w = _g(c["x"], dt), _g(c["w"], dt)
    want = c["y"].to(dt).double()
    rows = want.reshape(-1, c["Co"])
    prow = o.conv_partial_rows(d)
    for e in envs:
        with env(e):
            y = Guarded(want.numel(), dt)
            part = Guarded(prow * 2 * c["Co"], F32) if with_partials else None
            launch(o.conv_gemm, d, x, w, y.t, None, part.t if part else None)
            torch.cuda.synchronize()
            tag = f"{c['name']} {dt} {c['regime']} plain {e}"
            same(y.t, want, tag + " y")
            assert y.guards(), tag + ": y guard band written"
            if part is not None:
                pr = part.t.view(prow, 2, c["Co"])
                same(pr[:, 0], tile_sums(rows), tag + " partial sum(y)")
                same(pr[:, 1], tile_sums(rows * rows), tag + " partial sum(y^2)")
                assert part.guards(), tag + ": partials guard band written"


def run_fwd_epilogues(c, envs, views=1):
    """Addend with partials; conv_bn_act_fused (views); conv_bn_act_eval (with / without residual, relu) and, next to each
    of its launches, conv_bn_eval on BatchNorm tensors that derive the same scale / shift (same bits wanted) and with
    gamma = beta = NULL."""
    o, dt, Co = ops(), c["dt"], c["Co"]
    d = desc_of(c)
    x, w = _g(c["x"], dt), _g(c["w"], dt)
    res = _g(c["res"], dt)
    sc, sh = _g(c["scale"], F32), _g(c["shift"], F32)
    bn = [_g(c[k], F32) for k in ("gamma", "beta", "rm", "rv")] if views == 1 else None
    y_rows = c["y"].reshape(-1, Co)
    prow = o.conv_partial_rows(d)
    n = c["y"].numel()
    for e in envs:
        with env(e):
            tag = f"{c['name']} {dt} views{views} {e}"
            if views == 1:
                # general / lean epilogue with an addend; partial rows = sums of the rounded GEMM result (before the addend)
                y = Guarded(n, dt)
                part = Guarded(prow * 2 * Co, F32)
                launch(o.conv_gemm, d, x, w, y.t, res, part.t)
                torch.cuda.synchronize()
                same(y.t, c["y"] + c["res"], tag + " y + addend")
                pr = part.t.view(prow, 2, Co)
                same(pr[:, 0], tile_sums(y_rows), tag + " addend launch partial sum")
                same(pr[:, 1], tile_sums(y_rows * y_rows), tag + " addend launch partial sum sq")
                assert y.guards() and part.guards(), tag + ": addend launch wrote outside its outputs"
            for residual in (True, False):
                pre = c["aff"] + (c["res"] if residual else 0)
                y = Guarded(n, dt)
                mk = Guarded(n // EPC[dt], torch.uint8)
                launch(o.conv_bn_act_fused, d, x, w, sc, sh, res if residual else None, True, y.t, mk.t, views=views)
                torch.cuda.synchronize()
                same(y.t, pre.clamp_min(0), tag + f" fused y res={residual}")
                assert torch.equal(mk.t.cpu(), mask_bytes(pre > 0, EPC[dt])), tag + f" fused mask res={residual}"
                assert y.guards() and mk.guards(), tag + ": fused launch wrote outside its outputs"
                if views == 1:
                    pre_na = c["aff_na"] + (c["res"] if residual else 0)
                    for relu in (True, False):
                        y = Guarded(n, dt)
                        launch(o.conv_bn_act_eval, d, x, w, sc, sh, res if residual else None, relu, y.t)
                        torch.cuda.synchronize()
                        same(y.t, pre.clamp_min(0) if relu else pre, tag + f" eval res={residual} relu={relu}")
                        assert y.guards(), tag + ": eval launch wrote outside y"
                        # the same launch with scale / shift derived in the epilogue from the BatchNorm's tensors, and its
                        # gamma = beta = NULL form
                        yb = Guarded(n, dt)
                        launch(o.conv_bn_eval, d, x, w, bn[0], bn[1], bn[2], bn[3], 0.0, res if residual else None, relu, yb.t)
                        torch.cuda.synchronize()
                        same(yb.t, pre.clamp_min(0) if relu else pre, tag + f" bn_eval res={residual} relu={relu}")
                        assert yb.guards(), tag + ": bn_eval launch wrote outside y"
                        assert torch.equal(yb.t, y.t), tag + f" bn_eval != conv_bn_act_eval res={residual} relu={relu}"
                        yb = Guarded(n, dt)
                        launch(o.conv_bn_eval, d, x, w, None, None, bn[2], bn[3], 0.0, res if residual else None, relu, yb.t)
                        torch.cuda.synchronize()
                        same(yb.t, pre_na.clamp_min(0) if relu else pre_na, tag + f" bn_eval no affine res={residual} relu={relu}")
                        assert yb.guards(), tag + ": bn_eval launch (no affine) wrote outside y"


def run_fwd_plan(dt, plan):
    for case, regime, seed, views, envs, parts in plan(dt):
        c = fwd_case(dt, case, regime, seed, views=views)
        if parts in ("all", "plain"):
            run_plain(c, envs, c["check_partials"])
        if parts in ("all", "epi"):
            run_fwd_epilogues(c, envs, views=views)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_forward_bit_exact(dt):
    LAUNCHES[0] = 0
    run_fwd_plan(dt, fwd_plan)
    print(f"forward {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_forward_grids_and_deep_threshold(dt):
    """Grids of 1 .. 17 tiles (XCD remap with nwg % 8 != 0) and the 256-block threshold of the deep K loop."""
    LAUNCHES[0] = 0
    run_fwd_plan(dt, grid_plan)
    print(f"grids {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_conv_bn_eval_same_bits_as_scale_shift_then_conv_bn_act_eval(dt):
    """The identity include/sm3_hip.h states for sm3_conv_bn_eval, on real values (random x, w, BatchNorm tensors, eps = 1e-5)
    over the whole edge table under the default switches: the same bits as sm3_bn_eval_scale_shift followed by
    sm3_conv_bn_act_eval, with and without a residual, gamma / beta, and the ReLU.  (Two entry points of the code under test:
    the identity is the documented contract, and sm3_bn_eval_scale_shift is held to fp64 in test_exact_bn_gpu.py.)"""
    o = ops()
    LAUNCHES[0] = 0
    bits = torch.int32 if dt == F32 else torch.int16
    for i, case in enumerate(FWD_CASES):
        name, N, H, W, ci16, Co, k, s, p = case
        Ci = ci_for(dt, ci16)
        g = torch.Generator().manual_seed(1000 + i)
        d = o.fwd_desc(o.dtype_code(dt), N, H, W, Ci, Co, k, s, p)
        n = N * d.Ho * d.Wo * Co
        x = _g(torch.randn(N, H, W, Ci, generator=g), dt)
        w = _g(torch.randn(Co, k, k, Ci, generator=g) / (k * k * Ci) ** 0.5, dt)
        res = _g(torch.randn(n, generator=g), dt)
        gamma, beta = _g(torch.rand(Co, generator=g) + 0.5, F32), _g(torch.randn(Co, generator=g), F32)
        rm, rv = _g(torch.randn(Co, generator=g), F32), _g(torch.rand(Co, generator=g) + 0.1, F32)
        for affine in (True, False):
            ga, be = (gamma, beta) if affine else (None, None)
            sc, sh = Guarded(Co, F32), Guarded(Co, F32)
            launch(o.bn_eval_scale_shift, ga, be, rm, rv, 1e-5, Co, sc.t, sh.t)
            for residual in (True, False):
                for relu in (True, False):
                    tag = f"{name} {dt} affine={affine} res={residual} relu={relu}"
                    y0, y1 = Guarded(n, dt), Guarded(n, dt)
                    launch(o.conv_bn_act_eval, d, x, w, sc.t, sh.t, res if residual else None, relu, y0.t)
                    launch(o.conv_bn_eval, d, x, w, ga, be, rm, rv, 1e-5, res if residual else None, relu, y1.t)
                    torch.cuda.synchronize()
                    assert bool(torch.isfinite(y0.t).all()), tag + ": the two-launch form is not finite"
                    assert torch.equal(y1.t.view(bits), y0.t.view(bits)), tag + ": bits differ"
                    assert y0.guards() and y1.guards(), tag + ": wrote outside y"
            assert sc.guards() and sh.guards(), f"{name}: bn_eval_scale_shift wrote outside scale / shift"
    print(f"bn_eval identity {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_conv_bn_eval_with_gamma_or_beta_alone(dt):
    """gamma given with beta NULL takes beta = 0, beta given with gamma NULL takes gamma = 1 (include/sm3_hip.h): fp64 on one
    small case, every switch setting, with and without the residual and the ReLU."""
    o = ops()
    c = fwd_case(dt, HALF_AFFINE_CASE, "repr", 100 + DTYPES.index(dt))
    aff_g, aff_b = half_affine_refs(c)
    d = desc_of(c)
    x, w, res = _g(c["x"], dt), _g(c["w"], dt), _g(c["res"], dt)
    gamma, beta, rm, rv = (_g(c[k], F32) for k in ("gamma", "beta", "rm", "rv"))
    for e in CONV_ENVS:
        with env(e):
            for ga, be, ref, nm in ((gamma, None, aff_g, "gamma alone"), (None, beta, aff_b, "beta alone")):
                for residual in (True, False):
                    pre = ref + (c["res"] if residual else 0)
                    for relu in (True, False):
                        y = Guarded(pre.numel(), dt)
                        o.conv_bn_eval(d, x, w, ga, be, rm, rv, 0.0, res if residual else None, relu, y.t)
                        torch.cuda.synchronize()
                        tag = f"{c['name']} {dt} {nm} res={residual} relu={relu} {e}"
                        same(y.t, pre.clamp_min(0) if relu else pre, tag)
                        assert y.guards(), tag + ": wrote outside y"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16], ids=IDS[1:])
def test_two_segment_forms_bit_exact(dt):
    """conv_gemm_seg (+addend) and conv_seg_act (ReLU bits) with col_bias, views 1 and 2."""
    o = ops()
    LAUNCHES[0] = 0
    code = o.dtype_code(dt)
    for M, Ci, Ci1, Co, views in SEG_FWD:
        c = seg_case(dt, M, Ci, Ci1, Co, views, 500 + M)
        d = o.make_desc(code, M, 1, 1, Ci, 1, 1, Co, 1, 1, [(0, 0, 0)], Ci)
        x0, x1, w0, w1 = (_g(c[k], dt) for k in ("x0", "x1", "w0", "w1"))
        cb, add = _g(c["cb"], F32), _g(c["add"], dt)
        for e in CONV_ENVS:
            with env(e):
                tag = f"seg M{M} Co{Co} v{views} {dt} {e}"
                for with_add in (False, True):
                    y = Guarded(M * Co, dt)
                    launch(o.conv_gemm_seg, d, x0, w0, x1, w1, cb, y.t, add if with_add else None, views=views,
                           w_view_stride=Co * Ci, w1_view_stride=Co * Ci1)
                    torch.cuda.synchronize()
                    same(y.t, c["y"] + (c["add"] if with_add else 0), tag + f" seg add={with_add}")
                    assert y.guards(), tag + ": seg wrote outside y"
                y = Guarded(M * Co, dt)
                mk = Guarded(M * Co // 8, torch.uint8)
                launch(o.conv_seg_act, d, x0, w0, x1, w1, cb, y.t, mk.t, True, views=views, w_view_stride=Co * Ci,
                       w1_view_stride=Co * Ci1)
                torch.cuda.synchronize()
                same(y.t, c["y"].clamp_min(0), tag + " seg_act y")
                assert torch.equal(mk.t.cpu(), mask_bytes(c["y"] > 0, 8)), tag + " seg_act mask"
                assert y.guards() and mk.guards(), tag + ": seg_act wrote outside its outputs"
    print(f"segments {dt}: {LAUNCHES[0]} launches checked")


# ------------------------------------------------------------------------------------------------------------------------
# data gradient
# ------------------------------------------------------------------------------------------------------------------------
def run_dgrad(c, envs, add_mode, views=1):
    o, dt, C = ops(), c["dt"], c["Cout"]
    code = o.dtype_code(dt)
    descs, full = o.dgrad_descs(code, c["N"], c["H"], c["W"], C, c["Cf"], c["k"], c["s"], c["p"])
    dz_ref, classes = dgrad_expect(c, add_mode, views)
    # pixels of the parity classes no tap reaches (1x1 / stride 2) belong to no launch: they must keep the sentinel
    covered = torch.zeros(c["N"], c["H"], c["W"], C, dtype=torch.bool)
    for d in descs:
        covered[:, d.ooy::d.osy, d.oox::d.osx] = True
    assert full == bool(covered.all())
    covered = covered.reshape(-1).to(_dev())
    dy = _g(c["dy"], dt)
    wd = _g(c["w"].permute(3, 1, 2, 0), dt)  # [Ci_fwd][k][k][Co_fwd]
    mask = _g(mask_bytes(c["mask"], EPC[dt]), torch.uint8)
    bx = _g(c["bx"], dt) if c["bx"] is not None else None
    mean, invstd = _g(c["mean"], F32), _g(c["invstd"], F32)
    n = dz_ref.numel()
    for e in envs:
        with env(e):
            tag = f"{c['name']} {dt} dgrad add={add_mode} x={bx is not None} v{views} {e}"
            dz = Guarded(n, dt)
            prows = [o.conv_partial_rows(d) for d in descs]
            # two rows before the first launch's rows, one between launches and two after the last: nothing may land there
            offs, off, gap = [], 2, torch.ones(sum(prows) + len(descs) + 3, dtype=torch.bool)
            for d, pr in zip(descs, prows):
                offs.append(off)
                gap[off:off + pr] = False
                off += pr + 1
            total = gap.numel()
            part = Guarded(total * 2 * C, F32)
            for d, ro in zip(descs, offs):
                cls = (d.ooy, d.oox)
                addend, sp = None, None
                if add_mode == "dense":
                    addend = _g(c["add"], dt)
                elif add_mode == "compact":
                    if c["s"] == 1:
                        addend = _g(c["add"][:, ::2, ::2], dt)
                        sp = ((c["H"] + 1) // 2, (c["W"] + 1) // 2)
                    elif cls == (0, 0):
                        addend = _g(c["add"][:, ::2, ::2], dt)
                        sp = (d.Ho, d.Wo)
                if views == 2:
                    launch(o.conv_dgrad_bnfuse, d, dy, wd, dz.t, addend, mask, bx, mean, invstd, part.t, ro, views=2,
                           row_offset_view1=ro + o.conv_partial_rows(d) // 2, addend_sparse=sp)
                else:
                    launch(o.conv_dgrad_bnfuse, d, dy, wd, dz.t, addend, mask, bx, mean, invstd, part.t, ro,
                           addend_sparse=sp)
            torch.cuda.synchronize()
            same(dz.t[covered], dz_ref.reshape(-1)[covered.cpu()], tag + " dz")
            if not full:
                assert bool((dz.t[~covered].view(torch.uint8) == SENTINEL).all()), tag + ": uncovered pixels written"
            assert dz.guards() and part.guards(), tag + ": wrote outside dz / partials"
            pall = part.t.view(total, 2, C)
            assert bool((pall[gap.to(_dev())].view(torch.uint8) == SENTINEL).all()), \
                tag + ": partial rows outside the launches' rows written"
            for d, ro, pr in zip(descs, offs, prows):
                parts = classes[(d.ooy, d.oox)]
                got = pall[ro:ro + pr]
                want_s = torch.cat([p_[0] for p_ in parts])
                want_t = torch.cat([p_[1] for p_ in parts])
                same(got[:, 0], want_s, tag + f" class {d.ooy, d.oox} sum dz")
                same(got[:, 1], want_t, tag + f" class {d.ooy, d.oox} sum dz*xhat")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_data_gradient_bit_exact(dt):
    LAUNCHES[0] = 0
    for case, with_x, seed, views, modes in dgrad_plan(dt):
        c = dgrad_case(dt, case, with_x, seed, views=views)
        for mode, envs in modes:
            run_dgrad(c, envs, mode, views=views)
    print(f"data gradient {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16], ids=IDS[1:])
def test_data_gradient_two_segments_bit_exact(dt):
    """conv_dgrad_seg_bnfuse with and without x, views 1 and 2."""
    o = ops()
    LAUNCHES[0] = 0
    code = o.dtype_code(dt)
    for M, Ci, Ci1, Co, views in SEG_DGRAD:
        c = dgrad_seg_case(dt, M, Ci, Ci1, Co, views, 700 + M)
        mbits, bx, mean, invstd, dz, xhat = (c[k] for k in ("mbits", "bx", "mean", "invstd", "dz", "xhat"))
        d = o.make_desc(code, M, 1, 1, Ci, 1, 1, Co, 1, 1, [(0, 0, 0)], Ci)
        x0, x1, w0, w1 = (_g(c[k], dt) for k in ("x0", "x1", "w0", "w1"))
        cb = _g(c["cb"], F32)
        mask = _g(mask_bytes(mbits, 8), torch.uint8)
        prow = o.conv_partial_rows(d)
        for e in CONV_ENVS:
            for with_x in (True, False):
                with env(e):
                    tag = f"dgrad seg M{M} Co{Co} v{views} x={with_x} {dt} {e}"
                    y = Guarded(M * Co, dt)
                    part = Guarded((prow + 1) * 2 * Co, F32)
                    kw = dict(views=2, row_offset_view1=1 + prow // 2) if views == 2 else {}
                    launch(o.conv_dgrad_seg_bnfuse, d, x0, w0, x1, w1, cb, y.t, mask, _g(bx, dt) if with_x else None,
                           _g(mean, F32), _g(invstd, F32), part.t, 1, w_view_stride=Co * Ci, w1_view_stride=Co * Ci1, **kw)
                    torch.cuda.synchronize()
                    same(y.t, dz, tag + " dz")
                    assert y.guards() and part.guards(), tag + ": wrote outside dz / partials"
                    pr = part.t.view(prow + 1, 2, Co)[1:]
                    if views == 2:
                        h = M // 2
                        ws = torch.cat([tile_sums(dz[:h]), tile_sums(dz[h:])])
                        wt = torch.cat([tile_sums((dz * xhat)[:h]), tile_sums((dz * xhat)[h:])])
                    else:
                        ws, wt = tile_sums(dz), tile_sums(dz * xhat)
                    same(pr[:, 0], ws, tag + " sum dz")
                    same(pr[:, 1], wt if with_x else torch.zeros_like(wt), tag + " sum dz*xhat")
    print(f"data gradient segments {dt}: {LAUNCHES[0]} launches checked")


# ------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_weight_gradients_bit_exact(dt):
    """conv_wgrad (atomic), conv_wgrad_det over slab caps 1..9, conv_wgrad_slabs + slab_reduce (views 1, 2), conv_wgrad_cat
    (views, second output), and the nine-tap owner against the tap-shifted kernel: all equal to fp64."""
    o = ops()
    LAUNCHES[0] = 0
    code = o.dtype_code(dt)
    for name, geo, seed in wgrad_plan(dt):
        c = wgrad_case(dt, *geo, seed=seed)
        N, H, W, Ci, Co, k, s, p = geo
        d = o.fwd_desc(code, N, H, W, Ci, Co, k, s, p)
        x, dy = _g(c["x"], dt), _g(c["dy"], dt)
        want = c["ref"] + c["dw0"]
        n = Co * k * k * Ci
        nine = [{"SM3_WGRAD9": 1}, {"SM3_WGRAD9": 0}] if dt != F32 and k == 3 and s == 1 else [{}]
        for e in nine:
            with env(e):
                tag = f"wgrad {name} {dt} {e}"
                dw = Guarded(n, F32, c["dw0"])
                launch(o.conv_wgrad, d, x, dy, dw.t)
                torch.cuda.synchronize()
                same(dw.t, want, tag + " atomic")
                assert dw.guards(), tag + ": atomic wrote outside dw"
                for cap in range(1, 10):
                    dw = Guarded(n, F32, c["dw0"])
                    sl = Guarded(cap * n, F32)
                    launch(o.conv_wgrad_det, d, x, dy, dw.t, sl.t, cap)
                    torch.cuda.synchronize()
                    same(dw.t, want, tag + f" det cap {cap}")
                    assert dw.guards() and sl.guards(), tag + f": det cap {cap} wrote outside dw / slabs"
                views = 2 if N % 2 == 0 else 1
                for v in sorted({1, views}):
                    sl = Guarded(v * 8 * n, F32)
                    used = launch(o.conv_wgrad_slabs, d, x, dy, sl.t, views=v, cap=8)
                    outs = []
                    for vi in range(v):
                        out = Guarded(n, F32, c["dw0"])
                        launch(o.slab_reduce, sl.t[vi * used * n:(vi + 1) * used * n], used, n, out.t, accumulate=True)
                        outs.append(out)
                    torch.cuda.synchronize()
                    assert sl.guards(), tag + f": slabs v{v} wrote outside its buffer"
                    Nv = N // v
                    for vi, out in enumerate(outs):
                        ref_v = wgrad_ref(c["x"][vi * Nv:(vi + 1) * Nv], c["dy"][vi * Nv:(vi + 1) * Nv], (Co, k, k, Ci), s, p)
                        same(out.t, ref_v + c["dw0"], tag + f" slabs v{v} view {vi}")
                        assert out.guards(), tag + ": slab_reduce wrote outside out"
                    if v == 2 or views == 1:
                        dwc = Guarded(v * n, F32)
                        dwc.t.zero_()
                        launch(o.conv_wgrad_cat, d, x, dy, dwc.t, views=v)
                        torch.cuda.synchronize()
                        for vi in range(v):
                            ref_v = wgrad_ref(c["x"][vi * Nv:(vi + 1) * Nv], c["dy"][vi * Nv:(vi + 1) * Nv],
                                              (Co, k, k, Ci), s, p)
                            same(dwc.t[vi * n:(vi + 1) * n], ref_v, tag + f" cat v{v} view {vi}")
                        assert dwc.guards(), tag + ": cat wrote outside dw"
    # conv_wgrad_cat with a second output (Co a multiple of 128), two views
    c = wgrad_cat2_case(dt)
    N, H, W, Ci, Co, Co1, x, dy0, dy1 = (c[k] for k in ("N", "H", "W", "Ci", "Co", "Co1", "x", "dy0", "dy1"))
    d = o.fwd_desc(code, N, H, W, Ci, Co, 1, 1, 0)
    dw, dw1 = Guarded(2 * Co * Ci, F32), Guarded(2 * Co1 * Ci, F32)
    dw.t.zero_(); dw1.t.zero_()
    launch(o.conv_wgrad_cat, d, _g(x, dt), _g(dy0, dt), dw.t, _g(dy1, dt), dw1.t, views=2)
    torch.cuda.synchronize()
    for vi in range(2):
        sl = slice(2 * vi, 2 * vi + 2)
        same(dw.t.view(2, -1)[vi], c["refs"][vi][0], f"cat {dt} view {vi} dw")
        same(dw1.t.view(2, -1)[vi], c["refs"][vi][1], f"cat {dt} view {vi} dw1")
    assert dw.guards() and dw1.guards(), f"cat {dt}: wrote outside dw / dw1"
    print(f"weight gradients {dt}: {LAUNCHES[0]} launches checked")


# ------------------------------------------------------------------------------------------------------------------------
# related families: grouped GEMM, grouped 3x3 conv
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_grouped_gemm_and_wgrad_bit_exact():
    o = ops()
    LAUNCHES[0] = 0
    for rows, G, K, N in GROUPED:
        c = grouped_case(rows, G, K, N)
        x, w, dy, y, dw_ref = (c[k] for k in ("x", "w", "dy", "y", "dw"))
        for e in (CONV_ENVS[0], CONV_ENVS[2]):
            with env(e):
                tag = f"grouped rows{rows} G{G} K{K} N{N} {e}"
                yo = Guarded(rows * G * N, F32)
                tiles = (rows + 127) // 128
                part = Guarded(tiles * 2 * G * N, F32)
                launch(o.grouped_gemm, _g(x, F32), _g(w, F32), yo.t.view(rows, G * N), G, part.t)
                dw = Guarded(G * N * K, F32)
                dw.t.zero_()
                launch(o.grouped_wgrad_det, _g(x, F32), _g(dy, F32), dw.t, G)
                torch.cuda.synchronize()
                same(yo.t, y, tag + " y")
                pr = part.t.view(tiles, 2, G * N)
                same(pr[:, 0], tile_sums(y), tag + " partial sum")
                same(pr[:, 1], tile_sums(y * y), tag + " partial sum sq")
                same(dw.t, dw_ref, tag + " dw")
                assert yo.guards() and part.guards() and dw.guards(), tag + ": wrote outside its outputs"
    print(f"grouped: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_grouped_conv_bit_exact(dt):
    o = ops()
    LAUNCHES[0] = 0
    code = o.dtype_code(dt)
    for C, G, H, s, N in GCONV:
        c = gconv_case(dt, C, G, H, s, N)
        x, master, dy, y, dx, dwr, Ho = (c[k] for k in ("x", "master", "dy", "y", "dx", "dw", "Ho"))
        n = master.numel()
        wf, wd = torch.empty(n, dtype=dt, device=_dev()), torch.empty(n, dtype=dt, device=_dev())
        o.gconv_weight_prep(code, _g(master, F32), C, G, wf, wd)
        tag = f"gconv C{C} G{G} H{H} s{s} {dt}"
        M = N * Ho * Ho
        prow = (M + 127) // 128
        yo, part = Guarded(M * C, dt), Guarded(prow * 2 * C, F32)
        launch(o.gconv_fwd, code, _g(x.reshape(-1, C), dt), wf, yo.t, part.t, N, H, H, C, G, s)
        dxo = Guarded(N * H * H * C, dt)
        launch(o.gconv_dgrad, code, _g(dy.reshape(-1, C), dt), wd, dxo.t, N, H, H, C, G, s)
        torch.cuda.synchronize()
        same(yo.t, y, tag + " y")
        same(part.t.view(prow, 2, C)[:, 0], tile_sums(y), tag + " partial sum")
        same(part.t.view(prow, 2, C)[:, 1], tile_sums(y * y), tag + " partial sum sq")
        same(dxo.t, dx, tag + " dx")
        assert yo.guards() and part.guards() and dxo.guards(), tag + ": wrote outside its outputs"
        for cap in (1, 3, 8, o.wgrad_det_cap(n)):
            ns = o.gconv_wgrad_slabs(N, H, H, s, cap)
            dw, sl = Guarded(n, F32), Guarded(max(ns, 1) * n, F32)
            dw.t.zero_()
            launch(o.gconv_wgrad_det, code, _g(x.reshape(-1, C), dt), _g(dy.reshape(-1, C), dt), dw.t, sl.t, cap,
                   N, H, H, C, G, s)
            torch.cuda.synchronize()
            same(dw.t, dwr, tag + f" dw cap {cap}")
            assert dw.guards() and sl.guards(), tag + f": wgrad cap {cap} wrote outside dw / slabs"
    print(f"grouped conv {dt}: {LAUNCHES[0]} launches checked")


# ------------------------------------------------------------------------------------------------------------------------
# rejections and f16 overflow
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rejected_shapes_leave_outputs_untouched():
    from sm3hip import _lib
    o = ops()
    errors = (ValueError, _lib.SM3LibraryError)
    for dt in (BF16, F16):
        code = o.dtype_code(dt)
        # 16-bit Ci % 64 != 0
        d = o.fwd_desc(code, 1, 4, 4, 32, 64, 1, 1, 0)
        y = Guarded(16 * 64, dt)
        with pytest.raises(errors):
            o.conv_gemm(d, torch.zeros(16 * 32, dtype=dt, device=_dev()), torch.zeros(64 * 32, dtype=dt, device=_dev()), y.t)
        torch.cuda.synchronize()
        assert y.untouched()
        # Co * sz % 16 != 0
        d = o.fwd_desc(code, 1, 4, 4, 64, 4, 1, 1, 0)
        y = Guarded(16 * 4, dt)
        with pytest.raises(errors):
            o.conv_gemm(d, torch.zeros(16 * 64, dtype=dt, device=_dev()), torch.zeros(4 * 64, dtype=dt, device=_dev()), y.t)
        torch.cuda.synchronize()
        assert y.untouched()
        # views = 2 with M / 2 % 128 != 0
        d = o.fwd_desc(code, 2, 8, 12, 64, 64, 1, 1, 0)  # M = 192
        y, mk = Guarded(192 * 64, dt), Guarded(192 * 8, torch.uint8)
        one = torch.ones(128, device=_dev())
        with pytest.raises(errors):
            o.conv_bn_act_fused(d, torch.zeros(192 * 64, dtype=dt, device=_dev()), torch.zeros(64 * 64, dtype=dt, device=_dev()),
                                one, one, None, True, y.t, mk.t, views=2)
        torch.cuda.synchronize()
        assert y.untouched() and mk.untouched()
    # the C ABI refuses them too when the wrapper is bypassed
    code = o.dtype_code(BF16)
    d = o.fwd_desc(code, 1, 4, 4, 64, 4, 1, 1, 0)
    y = Guarded(16 * 4, BF16)
    rc = _lib.load().sm3_conv_gather_gemm(__import__("ctypes").byref(d), o._ptr(torch.zeros(16 * 64, dtype=BF16, device=_dev())),
                                          o._ptr(torch.zeros(4 * 64, dtype=BF16, device=_dev())), o._ptr(y.t), None, None,
                                          o._stream())
    torch.cuda.synchronize()
    assert rc != 0 and y.untouched()
    # sm3_conv_bn_eval needs both running statistics and an eps that is a number >= 0: through the wrapper, and through the
    # C ABI when the wrapper is bypassed
    byref, lib = __import__("ctypes").byref, _lib.load()
    for dt in DTYPES:
        code = o.dtype_code(dt)
        d = o.fwd_desc(code, 1, 4, 4, KCH[dt], 64, 1, 1, 0)
        x = torch.ones(16 * KCH[dt], dtype=dt, device=_dev())
        w = torch.ones(64 * KCH[dt], dtype=dt, device=_dev())
        v = torch.ones(64, device=_dev())
        for rm, rv, eps, what in ((None, v, 0.0, "NULL running_mean"), (v, None, 0.0, "NULL running_var"),
                                  (v, v, -1e-5, "eps < 0"), (v, v, float("nan"), "eps = NaN")):
            y = Guarded(16 * 64, dt)
            with pytest.raises(errors):
                o.conv_bn_eval(d, x, w, v, v, rm, rv, eps, None, True, y.t)
            torch.cuda.synchronize()
            assert y.untouched(), f"{dt} {what}: the wrapper's refusal wrote y"
            rc = lib.sm3_conv_bn_eval(byref(d), o._ptr(x), o._ptr(w), o._ptr(v), o._ptr(v), o._ptr(rm), o._ptr(rv), eps,
                                      o._ptr(None), 1, o._ptr(y.t), o._stream())
            torch.cuda.synchronize()
            assert rc != 0 and y.untouched(), f"{dt} {what}: rc {rc}"
        # (the same call with every operand in place is accepted: the refusals above are those of the operands named)
        y = Guarded(16 * 64, dt)
        o.conv_bn_eval(d, x, w, v, v, v, v, 0.0, None, True, y.t)
        torch.cuda.synchronize()
        same(y.t, torch.full((16 * 64,), float(KCH[dt])), f"{dt}: accepted control launch")
        assert y.guards()


@pytest.mark.gpu
def test_f16_data_gradient_overflow_stores_inf():
    """Exact sums 65519, 65520 and -65520 store as 65504, +inf and -inf (round to nearest even, overflow -> inf), on every
    epilogue path of the fused data-gradient launch and of the plain forward launch."""
    o = ops()
    code = o.dtype_code(F16)
    M, K, C = 128, 64, 8
    dy = torch.zeros(M, K, dtype=torch.float64)
    w = torch.zeros(C, K, dtype=torch.float64)  # w_dgrad [C][K]
    dy[:, 0], dy[:, 1], dy[:, 2] = 2048.0, 1.0, 1.0
    w[0, 0], w[0, 1], w[0, 2] = 31.0, 2016.0, 15.0    # 63488 + 2016 + 15 = 65519
    w[1, 0], w[1, 1], w[1, 2] = 31.0, 2032.0, 0.0     # 65520
    w[2, 0], w[2, 1], w[2, 2] = -31.0, -2032.0, 0.0   # -65520
    w[3, 0], w[3, 1] = 31.0, 2000.0                   # 65488: the tie between 65472 and 65504 goes to the even 65472
    w[4, 0], w[4, 1] = 31.0, 1984.0                   # 65472: exact
    want = torch.zeros(M, C, dtype=torch.float64)
    want[:, 0], want[:, 1], want[:, 2], want[:, 3], want[:, 4] = 65504.0, float("inf"), float("-inf"), 65472.0, 65472.0
    d = o.make_desc(code, M, 1, 1, K, 1, 1, C, 1, 1, [(0, 0, 0)], K)
    mask = torch.full((M * C // 8,), 255, dtype=torch.uint8, device=_dev())
    for e in CONV_ENVS:
        with env(e):
            dz = Guarded(M * C, F16)
            part = torch.zeros(2 * C, device=_dev())
            o.conv_dgrad_bnfuse(d, _g(dy, F16), _g(w, F16), dz.t, None, mask, None, None, None, part, 0)
            y = Guarded(M * C, F16)
            o.conv_gemm(d, _g(dy, F16), _g(w, F16), y.t)
            torch.cuda.synchronize()
            same(dz.t, want, f"f16 overflow dgrad {e}")
            same(y.t, want, f"f16 overflow forward {e}")
            assert dz.guards() and y.guards()


@pytest.mark.gpu
def test_f16_relu_bits_at_the_underflow_threshold():
    """Affine outputs 2^-26, 2^-25, 3 2^-26 and -2^-26 store as +0, +0 (the tie goes to the even 0), 2^-24 and 0: their
    ReLU bits are 0, 0, 1, 0 -- the stored y > 0 -- on every epilogue path of the fused forward launch."""
    o = ops()
    code = o.dtype_code(F16)
    M, K, C = 128, 64, 8
    x = torch.zeros(M, K, dtype=torch.float64)
    w = torch.zeros(C, K, dtype=torch.float64)
    x[:, 0] = torch.tensor([1.0, 2.0, 3.0, -1.0, 4.0, 0.0, 1.0, 3.0]).repeat(M // 8)
    w[:, 0] = 1.0
    sc = torch.full((C,), 2.0 ** -26, dtype=torch.float64)
    pre = (x[:, :1] * sc).expand(M, C)
    want = pre.clamp_min(0).to(F16).double()
    assert int(((pre > 0) & (want == 0)).sum()) == M // 8 * 3 * C
    d = o.make_desc(code, M, 1, 1, K, 1, 1, C, 1, 1, [(0, 0, 0)], K)
    for e in CONV_ENVS:
        with env(e):
            y = Guarded(M * C, F16)
            mk = Guarded(M * C // 8, torch.uint8)
            o.conv_bn_act_fused(d, _g(x, F16), _g(w, F16), _g(sc, F32), _g(torch.zeros(C), F32), None, True, y.t, mk.t)
            torch.cuda.synchronize()
            same(y.t, want, f"f16 underflow y {e}")
            assert torch.equal(mk.t.cpu(), mask_bytes(want > 0, 8)), f"f16 underflow: ReLU bits != (stored y > 0) {e}"
            assert y.guards() and mk.guards()


# ------------------------------------------------------------------------------------------------------------------------
# direct stem (7x7 / 2 / 3, 64 output channels)
# ------------------------------------------------------------------------------------------------------------------------
# N, H, W, BatchNorm views: odd sizes, an image wider than one 128-pixel tile, two views; the last has 1040 tiles, more than
# any grid cap of these persistent kernels (768, and 512 for stem_conv_fwd16): every workgroup runs a second tile
STEM_GEOMS = [(2, 32, 32, 2), (1, 13, 7, 1), (3, 9, 70, 1), (1, 1, 1, 1), (4, 10, 12, 2), (1040, 2, 2, 2)]


def stem_case(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = draw(g, (N, 3, H, W), 3, 0.6, -1)
    w = draw(g, (64, 3, 7, 7), 2, 0.5, 0)
    y = F.conv2d(x, w, stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    ya = F.conv2d(x.abs(), w.abs(), stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    need_exact(ya, quantum(x) * quantum(w), "stem sum")
    need_exact(y.abs().sum(0), quantum(y), "stem partial sum")  # any partial row is a subset of these sums
    need_exact((y * y).sum(0), quantum(y) ** 2, "stem partial sum sq")
    return x, w, y


def test_stem_preconditions():
    for i, (N, H, W, views) in enumerate(STEM_GEOMS):
        _, _, y = stem_case(N, H, W, 800 + i)
        for dt in DTYPES:
            need_repr(y, dt, "stem y")
            stem_wgrad_case(dt, N, H, W, views, 900 + i)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stem_forward_bit_exact(dt):
    """stem_conv_fwd (fp32 NCHW images) and stem_conv_fwd16 (16-bit padded image): y bit-exact, the partial rows adding up
    to the exact column sums."""
    o = ops()
    code = o.dtype_code(dt)
    LAUNCHES[0] = 0
    for i, (N, H, W, _) in enumerate(STEM_GEOMS):
        x, w, y = stem_case(N, H, W, 800 + i)
        ws = torch.empty(64, o.STEM_KDIRECT, dtype=dt, device=_dev())
        o.stem_weight_prep(code, _g(w.permute(0, 2, 3, 1).reshape(64, 147), F32), ws)
        prow = o.stem_partial_rows(N, H, W)
        forms = [("fwd", lambda yo, po: o.stem_conv_fwd(code, _g(x, F32), ws, yo, po))]
        if dt != F32:
            img = o.stem_image_prep(code, [_g(x, F32)])
            forms.append(("fwd16", lambda yo, po: o.stem_conv_fwd16(code, img, ws, yo, po)))
        for nm, fn in forms:
            yo, part = Guarded(y.numel(), dt), Guarded(prow * 2 * 64, F32)
            launch(fn, yo.t, part.t)
            torch.cuda.synchronize()
            tag = f"stem {nm} N{N} H{H} W{W} {dt}"
            same(yo.t, y, tag + " y")
            ps = part.t.view(prow, 2, 64).double().sum(0)
            same(ps[0], y.sum(0), tag + " partial sum")
            same(ps[1], (y * y).sum(0), tag + " partial sum sq")
            assert yo.guards() and part.guards(), tag + ": wrote outside y / partials"
    print(f"stem {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stem_weight_gradient_bit_exact(dt):
    """stem_wgrad_bn (fp32 NCHW images) and stem_wgrad_bn16 (16-bit padded image), float atomics and the fixed-order slab
    sum, with dyadic BatchNorm inputs: dw, dgamma and dbeta equal to fp64."""
    o = ops()
    code = o.dtype_code(dt)
    LAUNCHES[0] = 0
    for i, (N, H, W, views) in enumerate(STEM_GEOMS):
        c = stem_wgrad_case(dt, N, H, W, views, 900 + i)
        xg = _g(c["x"], F32)
        args = (_g(c["dz"], dt), _g(c["xo"], dt), _g(c["mean"], F32), _g(c["invstd"], F32), _g(c["gamma"], F32),
                _g(c["gs"], torch.float64), c["count"], _g(c["ls"], torch.float64))
        forms = [("bn", lambda *a, **k: o.stem_wgrad_bn(code, xg, *a, **k))]
        if dt != F32:
            img = o.stem_image_prep(code, [xg])
            forms.append(("bn16", lambda *a, **k: o.stem_wgrad_bn16(code, img, *a, **k)))
        for nm, fn in forms:
            for use_slabs in (False, True):
                tag = f"stem wgrad {nm} N{N} H{H} W{W} v{views} slabs={use_slabs} {dt}"
                dw, dg, db = Guarded(64 * 147, F32), Guarded(64, F32), Guarded(64, F32)
                for t in (dw, dg, db):
                    t.t.zero_()
                sl = Guarded(o.STEM_WGRAD_SLABS * 64 * 147, F32) if use_slabs else None
                launch(fn, *args, dg.t, db.t, dw.t, views=views, slabs=sl.t if sl else None)
                torch.cuda.synchronize()
                same(dw.t, c["dw"], tag + " dw")
                same(dg.t, c["dgamma"], tag + " dgamma")
                same(db.t, c["dbeta"], tag + " dbeta")
                assert dw.guards() and dg.guards() and db.guards() and (sl is None or sl.guards()), \
                    tag + ": wrote outside its outputs"
    print(f"stem weight gradient {dt}: {LAUNCHES[0]} launches checked")
