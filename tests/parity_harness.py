"""Test helper of the teacher-forced block-parity suites (test_block_parity_gpu.py, test_basicblock_gpu.py,
test_geometry_parity_gpu.py, test_parity_harness_cpu.py): every unit of an encoder -- the stem, each Bottleneck or BasicBlock
-- recomputed in fp64 from the unit's OWN input and OWN upstream gradient, at any image size H x W.

  * maps_of(H, W): the five map sizes of an encoder; taps are reshaped with these explicit sizes (hwc asserts
    rows == N * h * w) -- nothing assumes a square map;
  * engine_run(): one train-mode forward + backward of a bare encoder on the HIP engine with block-boundary taps;
    standin_run(): the same record from the reference alone (the mode restatement chained into a whole encoder, CPU or GPU);
  * Conv / bn / stem_ref / block_ref / basic_ref: the fp64 units (Conv takes groups: ResNeXt's conv2);
  * the MODE RESTATEMENT of a unit -- reference code only -- is the rounding floor of an ideal implementation of a mode: for
    bf16 / f16 the fp64 unit with every stored tensor rounded to the type, forward and in the gradient (Round: straight
    through, x.to(dt).double() forward, g.to(dt).double() backward) after every convolution, after every BatchNorm(+ReLU),
    after the join, after the max-pool, and on the unit's input (forward a no-op: the input is stored in the type; backward
    the rounding of the stored input gradient); for f32 the same unit executed by torch in float32;
  * check_run(): per unit, the engine's (or stand-in's) tensors against fp64 with
        limit = max(BOUNDS[mode][metric], 3 x the restatement's value on that same unit, same inputs, same upstream gradient)
    (cosine: min(BOUNDS cos, 1 - 3 (1 - cos_restated))).  BOUNDS is test_block_parity_gpu.py's table, measured at the
    benchmarked shapes; the second term comes from the reference alone.  No limit is derived from what the engine returned.

Not a conftest; changes no pytest setting.  SM3_GEOMETRY_MEASURE=<file>: check_run appends one JSON line per case with the
worst engine and restatement value of every metric (profiles/geometry_parity_measure.md is made from such a run)."""
import json
import os

import torch
import torch.nn.functional as F

MARGIN = 3.0
DTNAME = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
DTYPE = {v: k for k, v in DTNAME.items()}

# (H, W) -> maps (stem, pool, layer2, layer3, layer4)
GEOMETRIES = {
    "A": (73, 37),    # 37x19, 19x10, 10x5, 5x3, 3x2: an odd side into every stride-2 operation
    "B": (33, 301),   # 17x151, 9x76, 5x38, 3x19, 2x10: a stem output row wider than 128
    "C": (17, 9),     # 9x5, 5x3, 3x2, 2x1, 1x1
    "224": (224, 224),
}
# the teacher-forced train-mode cases of test_geometry_parity_gpu.py: arch, mode, images (all views), views, geometry
TRAIN_CASES = [
    ("resnet50", "bf16", 16, 1, "A"), ("resnet50", "f16", 16, 1, "C"), ("resnet50", "f32", 16, 1, "A"),
    ("resnet50", "bf16", 4, 1, "B"), ("resnet50", "bf16", 256, 2, "A"),
    ("resnet18", "bf16", 16, 1, "A"), ("resnet18", "f32", 16, 1, "C"), ("resnet18", "f16", 256, 2, "A"),
    ("resnext50_32x4d", "bf16", 16, 1, "A"), ("resnext50_32x4d", "f16", 16, 1, "C"), ("resnext50_32x4d", "f32", 4, 1, "B"),
    ("resnext50_32x4d", "bf16", 256, 2, "224"),
]


def case_id(c):
    arch, mode, N, V, geo = c
    return f"{arch}-{mode}-{N if V == 1 else f'{V}x{N // V}'}-{geo}"


def bounds(mode):
    from test_block_parity_gpu import BOUNDS  # the project's table stays where it was measured
    return BOUNDS[mode]


# ---- geometry -------------------------------------------------------------------------------------------------------
def maps_of(H, W):
    """[(h, w)] of the stem output, the max-pool output (= layer1), layer2, layer3, layer4: each (x - 1) // 2 + 1."""
    out = []
    for _ in range(5):
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out.append((H, W))
    return out


def stage_map(maps, prefix):
    """The output map of the unit `prefix` ("" = the stem + max-pool, "layer3.1." ...)."""
    return maps[int(prefix.split(".")[0][len("layer"):])] if prefix else maps[1]


def hwc(t, n_img, hw):
    """The engine's [N*h*w, C] rows -> fp64 [N, h, w, C], with the explicit map size."""
    h, w = hw
    assert t.dim() == 2 and t.shape[0] == n_img * h * w, (tuple(t.shape), n_img, h, w)
    return t.double().view(n_img, h, w, t.shape[1])


# ---- convolution on NHWC maps -----------------------------------------------------------------------------------------
def _tap_slices(k, s, Ho, Wo):
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, (slice(None), slice(ky, ky + s * (Ho - 1) + 1, s), slice(kx, kx + s * (Wo - 1) + 1, s))


class Conv(torch.autograd.Function):
    """conv2d without bias, x [N, H, W, Ci], w [Co, Ci / groups, k, k] (OIHW) -> [N, Ho, Wo, Co], in x's dtype: one GEMM per
    tap (groups > 1: one batched GEMM over the groups per tap)."""

    @staticmethod
    def forward(ctx, x, w, stride, pad, groups=1):
        N, H, W, Ci = x.shape
        Co, cg, k = w.shape[0], w.shape[1], w.shape[2]
        assert cg * groups == Ci and Co % groups == 0
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        xp = F.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x
        out = None
        for ky, kx, sl in _tap_slices(k, stride, Ho, Wo):
            if groups == 1:
                t = xp[sl].reshape(-1, Ci) @ w[:, :, ky, kx].t()
            else:
                xg = xp[sl].reshape(-1, groups, cg).transpose(0, 1)                      # [G, rows, cg]
                wg = w[:, :, ky, kx].reshape(groups, Co // groups, cg).transpose(1, 2)   # [G, cg, Co / G]
                t = torch.bmm(xg, wg).transpose(0, 1).reshape(-1, Co)
            out = t if out is None else out.add_(t)
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.pad, ctx.groups = stride, pad, groups
        return out.view(N, Ho, Wo, Co)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        s, p, G = ctx.stride, ctx.pad, ctx.groups
        N, H, W, Ci = x.shape
        Co, cg, k = w.shape[0], w.shape[1], w.shape[2]
        Ho, Wo = g.shape[1], g.shape[2]
        g = g.contiguous()
        xp = F.pad(x, (0, 0, p, p, p, p)) if p else x
        gi = g.view(N, Ho * Wo, Co).transpose(1, 2)  # [N, Co, pixels]: the weight gradient as a batch of per-image GEMMs
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        dxp = torch.zeros_like(xp) if ctx.needs_input_grad[0] else None
        for ky, kx, sl in _tap_slices(k, s, Ho, Wo):
            if dw is not None:
                if G == 1:
                    dw[:, :, ky, kx] = torch.bmm(gi, xp[sl].reshape(N, Ho * Wo, Ci)).sum(0)
                else:
                    gg = gi.reshape(N, G, Co // G, Ho * Wo)
                    xg = xp[sl].reshape(N, Ho * Wo, G, cg).permute(0, 2, 1, 3)           # [N, G, pixels, cg]
                    dw[:, :, ky, kx] = torch.matmul(gg, xg).sum(0).reshape(Co, cg)
            if dxp is not None:
                if G == 1:
                    dxp[sl] += (g.view(-1, Co) @ w[:, :, ky, kx]).view(N, Ho, Wo, Ci)
                else:
                    gg = g.view(-1, G, Co // G).transpose(0, 1)                          # [G, rows, Co / G]
                    dxp[sl] += torch.bmm(gg, w[:, :, ky, kx].reshape(G, Co // G, cg)).transpose(0, 1).reshape(N, Ho, Wo, Ci)
        dx = dxp[:, p:p + H, p:p + W] if (dxp is not None and p) else dxp
        return dx, dw, None, None, None


def bn(t, P, B, name, V):
    """Train-mode BatchNorm of an NHWC map whose V views lie back to back: the oracle once per view, in view order."""
    from oracle import sm3_oracle as O
    outs = [O.batchnorm(c.permute(0, 3, 1, 2), P, B, name, True).permute(0, 2, 3, 1) for c in t.chunk(V, 0)]
    return outs[0] if V == 1 else torch.cat(outs, 0)


# ---- the roundings of a mode, and seeded defects (stand-in only) --------------------------------------------------------
class Round(torch.autograd.Function):
    """A tensor stored in `dt`: rounded forward, and its gradient rounded backward (straight through)."""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None


class _GradTimes(torch.autograd.Function):
    """Identity forward; the gradient times `m` (a number or a broadcastable mask).  Seeds a defect into the stand-in."""

    @staticmethod
    def forward(ctx, x, m):
        ctx.m = m
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.m, None


def _ident(x):
    return x


def rounder(dt):
    """The store of a mode: Round for the 16-bit types, nothing for fp64 / float32 execution."""
    return (lambda x: Round.apply(x, dt)) if dt in (torch.bfloat16, torch.float16) else _ident


# ---- the units: fp64 with q = identity, the 16-bit restatement with q = rounder(dt), f32 by float32 tensors ------------
def block_ref(x, P, B, p, stride, V, groups=1, q=_ident, defect=None):
    """Bottleneck.forward (src/models/resnet.py:154-174) -> (pre-ReLU sum out + identity, block output)."""
    d = defect or {}
    x = q(x)
    out = Conv.apply(x, P[p + "conv1.weight"], 1, 0)
    out = q(F.relu(bn(d.get("bn1", _ident)(q(out)), P, B, p + "bn1", V)))
    out = q(F.relu(bn(q(Conv.apply(out, P[p + "conv2.weight"], stride, 1, groups)), P, B, p + "bn2", V)))
    out = q(bn(q(Conv.apply(out, P[p + "conv3.weight"], 1, 0)), P, B, p + "bn3", V))
    if p + "downsample.0.weight" in P:
        idn = q(bn(q(Conv.apply(d.get("idn", _ident)(x), P[p + "downsample.0.weight"], stride, 0)), P, B, p + "downsample.1", V))
    else:
        idn = d.get("idn", _ident)(x)
    pre = q(out + idn)
    return pre, F.relu(pre)


def basic_ref(x, P, B, p, stride, V, q=_ident, defect=None):
    """BasicBlock.forward (src/models/resnet.py:91-106) on NHWC maps -> (pre-ReLU sum, block output)."""
    d = defect or {}
    x = q(x)
    out = Conv.apply(x, P[p + "conv1.weight"], stride, 1)
    out = q(F.relu(bn(d.get("bn1", _ident)(q(out)), P, B, p + "bn1", V)))
    out = q(bn(q(Conv.apply(out, P[p + "conv2.weight"], 1, 1)), P, B, p + "bn2", V))
    if p + "downsample.0.weight" in P:
        idn = q(bn(q(Conv.apply(d.get("idn", _ident)(x), P[p + "downsample.0.weight"], stride, 0)), P, B, p + "downsample.1", V))
    else:
        idn = d.get("idn", _ident)(x)
    pre = q(out + idn)
    return pre, F.relu(pre)


def stem_ref(img, P, B, V, q=_ident):
    """conv1 7x7/2 -> bn1 -> ReLU -> max-pool 3x3/2 (src/models/resnet.py:292-297) on NCHW images -> NHWC map."""
    x = img.permute(0, 2, 3, 1)
    y = q(F.relu(bn(q(Conv.apply(x, P["conv1.weight"], 2, 3)), P, B, "bn1", V)))
    return q(F.max_pool2d(y.permute(0, 3, 1, 2), kernel_size=3, stride=2, padding=1).permute(0, 2, 3, 1))


def unit_ref(x, P, B, blk, V, q=_ident, defect=None):
    """The block `blk` of a run's unit list -> (pre, out)."""
    if blk["basic"]:
        return basic_ref(x, P, B, blk["prefix"], blk["stride"], V, q, defect)
    return block_ref(x, P, B, blk["prefix"], blk["stride"], V, blk["groups"], q, defect)


# ---- metrics ----------------------------------------------------------------------------------------------------------
def cos(a, b):
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-300))


def rel(got, ref):
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def maxrel(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def record(rep, stage, kind, name, value, worse):
    """rep[stage][kind] = (worst value, tensor name); worse(a, b): a is worse than b."""
    cur = rep.setdefault(stage, {}).get(kind)
    if cur is None or worse(value, cur[0]):
        rep[stage][kind] = (value, name)


def ref_params(run, prefix, names, dtype=torch.float64):
    """Leaf copies of the unit's parameters, and copies of its BatchNorms' buffers as they were before the step."""
    P = {n: run["P"][n].to(dtype).clone().requires_grad_(True) for n in names}
    B = {k: (v.to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in run["buf0"].items()
         if k.startswith(prefix)}
    return P, B


def compare_unit(run, dt, prefix, stage, names, out_ref, got_out, dx_ref, got_dx, P, B, V, rep, fails, lim):
    """Compare one unit's output, running statistics, parameter gradients and input gradient against the fp64 ones."""
    lo, hi = (lambda a, b: a < b), (lambda a, b: a > b)
    fr, fm = rel(got_out, out_ref), maxrel(got_out, out_ref)
    record(rep, stage, "out_rel", prefix or "stem", fr, hi)
    record(rep, stage, "out_max", prefix or "stem", fm, hi)
    if fr > lim["out_rel"] or fm > lim["out_max"]:
        fails.append((prefix or "stem", "output", fr, fm))
    for k, ref in B.items():
        got = run["bufs"][k]
        if k.endswith("num_batches_tracked"):
            if int(got) != int(ref) or int(ref) != int(run["buf0"][k]) + V:
                fails.append((k, int(got), int(ref)))
            continue
        r = rel(got.double(), ref)
        record(rep, stage, "stat_rel", k, r, hi)
        if r > lim["stat_rel"]:
            fails.append((k, "running statistic", r))
    for n in names:
        ref, got = P[n].grad, run["grads"][n].double()
        c, r = cos(got, ref), rel(got, ref)
        record(rep, stage, "g_cos", n, c, lo)
        record(rep, stage, "g_rel", n, r, hi)
        cat = "conv" if got.dim() == 4 else "bn"
        q = abs(float(got.norm() / ref.norm()) - 1)
        record(rep, stage, cat + "_rel", n, r, hi)
        record(rep, stage, cat + "_ratio", n, q, hi)
        if c < lim["cos"] or r > lim["rel"] or q > lim[cat + "_ratio"]:
            fails.append((n, "gradient", c, r, q))
    if dx_ref is not None:
        c, r = cos(got_dx, dx_ref), rel(got_dx, dx_ref)
        record(rep, stage, "g_cos", prefix + "<input>", c, lo)
        record(rep, stage, "g_rel", prefix + "<input>", r, hi)
        q = abs(float(got_dx.norm() / dx_ref.norm()) - 1)
        record(rep, stage, "in_rel", prefix + "<input>", r, hi)
        record(rep, stage, "in_ratio", prefix + "<input>", q, hi)
        if c < lim["cos"] or r > lim["rel"] or q > lim["in_ratio"]:
            fails.append((prefix + "<input>", "input gradient", c, r, q))


def stage_of(prefix):
    return prefix.split(".")[0] if prefix else "stem"


# ---- the limit rule ---------------------------------------------------------------------------------------------------
_NO_LIMIT = {"out_rel": float("inf"), "out_max": float("inf"), "stat_rel": float("inf"), "cos": -float("inf"),
             "rel": float("inf"), "in_ratio": float("inf"), "conv_ratio": float("inf"), "bn_ratio": float("inf")}
_REP_KEY = {"out_rel": "out_rel", "out_max": "out_max", "stat_rel": "stat_rel", "cos": "g_cos", "rel": "g_rel",
            "in_ratio": "in_ratio", "conv_ratio": "conv_ratio", "bn_ratio": "bn_ratio"}
METRICS = tuple(_REP_KEY)


def unit_values(rep_unit):
    """{metric: the unit's worst value} from one unit's record (metrics the unit does not have are absent)."""
    return {m: rep_unit[k][0] for m, k in _REP_KEY.items() if k in rep_unit}


def limits(base, restated):
    """max(bound, MARGIN x the restatement's value), the cosine min(bound, 1 - MARGIN (1 - restated))."""
    lim = dict(base)
    for m, v in restated.items():
        lim[m] = min(base[m], 1.0 - MARGIN * (1.0 - v)) if m == "cos" else max(base[m], MARGIN * v)
    return lim


# ---- runs: the engine, and the reference-only stand-in -----------------------------------------------------------------
def images(B, H, W, tag):
    """One view's batch [B, 3, H, W] from oracle/procedural.py; non-square: the top-left H x W of the max(H, W) square."""
    from oracle import procedural
    return torch.from_numpy(procedural.make_images(B, max(H, W), 23, tag)[..., :H, :W]).contiguous()


def _encoder(arch):
    from src.models import resnet
    torch.manual_seed(5)
    m = getattr(resnet, arch)()
    m.fc = torch.nn.Identity()
    return m


def _units(names):
    """The unit list of an encoder from its parameter names: prefix, stride, groups, BasicBlock or Bottleneck."""
    out = []
    for n in names:
        if n.startswith("layer") and n.endswith(".conv1.weight"):
            out.append(n[: -len("conv1.weight")])
    return out


def describe_units(P, prefixes):
    units = []
    for p in prefixes:
        basic = p + "conv3.weight" not in P
        stride = 2 if (p.endswith(".0.") and not p.startswith("layer1.")) else 1
        w2 = P[p + "conv2.weight"]
        units.append(dict(prefix=p, basic=basic, stride=stride, groups=w2.shape[0] // w2.shape[1] if not basic else 1))
    return units


def engine_run(arch, dt, N, V, H, W, dev="cuda:0"):
    """One train-mode forward + backward of an encoder-only engine with taps.  Returns what the reference needs."""
    from sm3hip.engine import SM3Engine
    m = _encoder(arch)
    m.to(dev).train()
    eng = SM3Engine(m, dtype=dt, kind="encoder")
    eng.prepare(torch.device(dev))
    eng.refresh_weights()
    plan = eng.branches["main"][0]
    B = N // V
    imgs = [images(B, H, W, f"view{v}").to(dev) for v in range(V)]
    g = torch.Generator().manual_seed(29)
    dfeat = torch.randn(N, plan.out_dim, generator=g).to(dev)
    buf0 = {k: b.detach().clone() for k, b in m.named_buffers()}  # the running statistics before the step
    feats = torch.empty(N, plan.out_dim, device=dev)
    ctx, taps = [], {}
    eng.encoder_forward(plan, imgs if V > 1 else imgs[0], True, feats, None, ctx, views=V, taps=taps)
    eng.store.flat_g.zero_()
    eng.encoder_backward(ctx[0], dfeat.to(eng.tdt), taps=taps)
    torch.cuda.synchronize()
    forms, views_ran = [br.form for br in ctx[0].blocks], ctx[0].stem.V
    del ctx, feats
    st = eng.store
    wdt = dt if dt != torch.float32 else torch.float64  # the filter banks: fp32 masters rounded to the mode's dtype
    weights = {n: st._view(st.flat_p, n).detach() for n in st.names}
    P = {n: (w.to(wdt).double() if w.dim() == 4 else w.double()) for n, w in weights.items()}
    grads = {n: st._view(st.flat_g, n) for n in st.names}
    bufs = dict(m.named_buffers())
    img = torch.cat(imgs, 0)
    if dt != torch.float32:  # the 16-bit stem kernels read the images rounded once to the mode's dtype
        img = img.to(dt)
    prefixes = [blk["c1"].name[: -len("conv1")] for blk in plan.blocks]
    units = describe_units(P, prefixes)
    for u, blk in zip(units, plan.blocks):  # the plan's own strides and groups, not the names'
        assert (u["stride"], u["groups"], u["basic"]) == ((blk["c1"] if plan.basic else blk["c2"]).stride,
                                                          blk.get("c2").groups if not plan.basic else 1, plan.basic)
    return dict(eng=eng, P=P, grads=grads, bufs=bufs, buf0=buf0, taps=taps, img=img, plan=plan, units=units, forms=forms,
                views_ran=views_ran, N=N, V=V, maps=maps_of(H, W), dt=dt)


def standin_run(arch, dt, N, V, H, W, dev="cpu", defects=None):
    """The record engine_run returns, from the reference alone: the mode restatement of every unit chained into a whole
    encoder, one train-mode forward + backward under autograd.  Every boundary gradient is with respect to the block's
    output (g_pre_relu False).  defects: {unit prefix: {"bn1" | "idn": function}} seeded into those units."""
    m = _encoder(arch).train()
    edt = torch.float32 if dt == torch.float32 else torch.float64
    q = rounder(dt)
    wdt = dt if dt != torch.float32 else torch.float64
    P = {n: (w.detach().to(wdt).double() if w.dim() == 4 else w.detach().double()).to(dev) for n, w in m.named_parameters()}
    buf0 = {k: b.detach().clone().to(dev) for k, b in m.named_buffers()}
    units = describe_units(P, _units(P))
    Pl = {n: w.to(edt).clone().requires_grad_(True) for n, w in P.items()}
    Bl = {k: (v.to(edt).clone() if v.is_floating_point() else v.clone()) for k, v in buf0.items()}
    B = N // V
    img = torch.cat([images(B, H, W, f"view{v}") for v in range(V)], 0).to(dev)
    if dt != torch.float32:
        img = img.to(dt)
    xs = [stem_ref(img.to(edt), Pl, Bl, V, q)]
    for u in units:
        x = xs[-1]
        x.retain_grad()
        xs.append(unit_ref(x, Pl, Bl, u, V, q, (defects or {}).get(u["prefix"]))[1])
    xs[-1].retain_grad()
    out_dim = xs[-1].shape[-1]
    dfeat = torch.randn(N, out_dim, generator=torch.Generator().manual_seed(29)).to(dev)
    if dt != torch.float32:
        dfeat = dfeat.to(dt)
    xs[-1].mean(dim=(1, 2)).backward(dfeat.to(edt))
    flat = lambda t: t.detach().reshape(-1, t.shape[-1])
    taps = dict(x=[flat(x) for x in xs], g=[flat(x.grad) for x in xs], g_pre_relu=[False] * len(xs))
    return dict(P=P, grads={n: w.grad for n, w in Pl.items()}, bufs=Bl, buf0=buf0, taps=taps, img=img, units=units,
                N=N, V=V, maps=maps_of(H, W), dt=dt)


# ---- every unit of a run against fp64, limits by the rule ------------------------------------------------------------
def _unit_pass(run, ui, dtype, q):
    """Unit ui (0: the stem) recomputed from the run's own input and upstream gradient, in `dtype` with the stores `q`.
    -> (names, P, B, output, input gradient or None), the gradient masked as the run's boundary gradient is."""
    N, V, maps, taps = run["N"], run["V"], run["maps"], run["taps"]
    if ui == 0:
        names = ["conv1.weight", "bn1.weight", "bn1.bias"]
        P, B = ref_params(run, "bn1.", names, dtype)
        out = stem_ref(run["img"].to(dtype), P, B, V, q)
        out.backward(hwc(taps["g"][0], N, maps[1]).to(dtype))
        return names, P, B, out.detach(), None
    blk = run["units"][ui - 1]
    prefix = blk["prefix"]
    names = [n for n in run["P"] if n.startswith(prefix)]
    P, B = ref_params(run, prefix, names, dtype)
    x = hwc(taps["x"][ui - 1], N, stage_map(maps, run["units"][ui - 2]["prefix"] if ui > 1 else "")).to(dtype)
    x.requires_grad_(True)
    pre, out = unit_ref(x, P, B, blk, V, q)
    gup = hwc(taps["g"][ui], N, stage_map(maps, prefix)).to(dtype)
    (pre if taps["g_pre_relu"][ui] else out).backward(gup)
    dx = x.grad
    if taps["g_pre_relu"][ui - 1]:  # the run's gradient at this boundary is already masked by the producer's ReLU
        dx = dx * (x.detach() > 0)
    return names, P, B, out.detach(), dx


def check_run(run, case, base=None, restate=True):
    """Teacher forcing over every unit of `run`.  -> (rep, rest, fails): the per-stage record of the run against fp64, the
    same record of the mode restatement against fp64, and the tensors over their limit.
    base: the mode's bounds (default: BOUNDS of the run's dtype); restate=False: those bounds alone (the cases that
    test_block_parity_gpu.py holds at the benchmarked shapes)."""
    dt, N, V, maps, taps = run["dt"], run["N"], run["V"], run["maps"], run["taps"]
    base = base or bounds(DTNAME[dt])
    assert len(taps["x"]) == len(taps["g"]) == len(run["units"]) + 1
    rep, rest, fails = {}, {}, []
    rdt, q = (torch.float32, _ident) if dt == torch.float32 else (torch.float64, rounder(dt))
    for ui in range(len(run["units"]) + 1):
        prefix = run["units"][ui - 1]["prefix"] if ui else ""
        stage = stage_of(prefix)
        names, P, B, out, dx = _unit_pass(run, ui, torch.float64, _ident)
        lim = base
        if restate:
            _, Pq, Bq, outq, dxq = _unit_pass(run, ui, rdt, q)
            mine = dict(bufs=Bq, buf0=run["buf0"], grads={n: Pq[n].grad for n in names})
            one, bad = {}, []
            compare_unit(mine, dt, prefix, "u", names, out, outq.double(), dx, None if dxq is None else dxq.double(),
                         P, B, V, one, bad, _NO_LIMIT)
            assert not bad, bad  # only num_batches_tracked can land here
            lim = limits(base, unit_values(one["u"]))
            for kind, (v, n) in one["u"].items():
                record(rest, stage, kind, n, v, (lambda a, b: a < b) if kind == "g_cos" else (lambda a, b: a > b))
            del Pq, Bq, outq, dxq
        got_dx = hwc(taps["g"][ui - 1], N, stage_map(maps, run["units"][ui - 2]["prefix"] if ui > 1 else "")) if ui else None
        compare_unit(run, dt, prefix, stage, names, out, hwc(taps["x"][ui], N, stage_map(maps, prefix)), dx, got_dx,
                     P, B, V, rep, fails, lim)
        del P, B, out, dx
    _measure(case, rep, rest)
    return rep, rest, fails


class Kinks:
    """The decisions of an fp64 eval-mode pass that float32 cannot resolve: a ReLU input within tau x the tensor's largest
    magnitude of 0, a max-pool window whose two largest entries lie within tau x the map's maximum of each other.  There the
    gradient is set-valued at float32 resolution: an exact-f32 implementation may take either side, and whole receptive
    fields of x.grad move with it (one stem max-pool tie of 1.3e-8 moves the x.grad of resnet18 at 73 x 37 by 7.8e-3).
    found: [("relu", site, flat index) | ("pool", flat window index, the runner-up's tap)], filled by a pass; flip: the
    decisions a pass takes the other way."""
    TAU = 8 * 2.0 ** -23

    def __init__(self, flip=()):
        self.flip, self.found, self._site = set(flip), [], 0

    def relu(self, z):
        site, self._site = self._site, self._site + 1
        zd = z.detach()
        near = (zd.abs() <= self.TAU * zd.abs().max()).view(-1).nonzero().view(-1).tolist()
        self.found += [("relu", site, i) for i in near]
        mask = zd > 0
        for kind, s_, i in self.flip:
            if kind == "relu" and s_ == site:
                mask.view(-1)[i] ^= True
        return z * mask

    def max_pool(self, y):
        """max_pool2d(y, 3, 2, 1) of a post-ReLU NCHW map (zero padding is neutral), as a gather over unfolded windows."""
        N, C, H, W = y.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        u = F.unfold(y, 3, padding=1, stride=2).view(N, C, 9, Ho * Wo)
        top = u.detach().topk(2, dim=2)
        pick = top.indices[:, :, 0].clone()
        near = ((top.values[:, :, 0] > 0) & (top.values[:, :, 0] - top.values[:, :, 1] <= self.TAU * y.detach().max()))
        flat = near.view(-1).nonzero().view(-1).tolist()
        second = top.indices[:, :, 1].reshape(-1)
        self.found += [("pool", i, int(second[i])) for i in flat]
        for kind, i, tap in self.flip:
            if kind == "pool":
                pick.view(-1)[i] = tap
        return u.gather(2, pick.unsqueeze(2)).view(N, C, Ho, Wo)


def restated_features(m, x, dt=None, kinks=None):
    """fp64 eval-mode forward of a torchvision-layout ResNet / ResNeXt from its own modules' tensors, any H x W.
    dt (a 16-bit type): the restatement of that mode -- filter banks and images rounded to dt, and every stored tensor
    (after each convolution, BatchNorm(+ReLU), join and the max-pool) rounded forward and in the gradient.
    kinks (fp64 only): a Kinks that records the decisions float32 cannot resolve and takes kinks.flip the other way."""
    q = rounder(dt) if dt is not None else _ident
    wq = (lambda w: w.to(dt).double()) if dt is not None else (lambda w: w.double())
    relu = kinks.relu if kinks is not None else F.relu
    pool = kinks.max_pool if kinks is not None else (lambda t: F.max_pool2d(t, 3, 2, 1))

    def bn64(t, b):
        return F.batch_norm(t, b.running_mean.double(), b.running_var.double(), b.weight.double(), b.bias.double(),
                            False, 0.0, b.eps)

    def conv64(t, c):
        return q(F.conv2d(t, wq(c.weight), None, c.stride, c.padding, c.dilation, c.groups))

    if dt is not None:
        x = x + (x.to(dt).double() - x).detach()  # the images are read rounded; their gradient is not
    y = q(relu(bn64(conv64(x, m.conv1), m.bn1)))
    y = q(pool(y))
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for blk in layer:
            idn = y
            out = q(relu(bn64(conv64(y, blk.conv1), blk.bn1)))
            if hasattr(blk, "conv3"):
                out = q(relu(bn64(conv64(out, blk.conv2), blk.bn2)))
                out = q(bn64(conv64(out, blk.conv3), blk.bn3))
            else:
                out = q(bn64(conv64(out, blk.conv2), blk.bn2))
            if blk.downsample is not None:
                idn = q(bn64(conv64(y, blk.downsample[0]), blk.downsample[1]))
            y = relu(q(out + idn))
    return y.mean(dim=(2, 3))


def nearest_branch(grad_of, found, got, g0, cap=24):
    """The fp64 gradient on the branch nearest to `got` among those that differ from g0 = grad_of(()) only in decisions of
    `found` (Kinks.found: what float32 cannot resolve).  The flip patterns are local (one receptive field each), so every
    decision is judged on its own -- taken the other way when `got` contains more than half of its pattern -- and the
    chosen ones are then flipped together in ONE exact fp64 pass, whose gradient is returned with the flips."""
    d = (got - g0).reshape(-1)
    take = []
    for dec in found[:cap]:
        p = (grad_of((dec,)) - g0).reshape(-1)
        if float(p.norm()) > 0 and float(d @ p) / float(p @ p) > 0.5:
            take.append(dec)
    return (grad_of(tuple(take)) if take else g0), take


def worst(rep):
    """{metric: worst value over the stages} of a check_run record."""
    out = {}
    for m, k in _REP_KEY.items():
        vals = [r[k][0] for r in rep.values() if k in r]
        if vals:
            out[m] = min(vals) if m == "cos" else max(vals)
    return out


def measure_line(rec):
    """Appends one JSON line to the file SM3_GEOMETRY_MEASURE names, when a measurement run asks for it."""
    path = os.environ.get("SM3_GEOMETRY_MEASURE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _measure(case, rep, rest):
    measure_line({"case": case, "engine": worst(rep), "restated": worst(rest)})


def report(case, rep):
    """The two lines test_block_parity_gpu.py prints per case."""
    print(f"\n{case}: per stage, worst tensor: "
          + "; ".join(f"{s}: out rel {r['out_rel'][0]:.2e} max {r['out_max'][0]:.2e}, stats {r['stat_rel'][0]:.2e} "
                      f"({r['stat_rel'][1]}), grad cos {r['g_cos'][0]:.6f} ({r['g_cos'][1]}), "
                      f"rel {r['g_rel'][0]:.2e} ({r['g_rel'][1]})" for s, r in rep.items()))
    print(f"{case}: by class, worst rel / worst |norm ratio - 1|: "
          + "; ".join(f"{s}: " + ", ".join(f"{c} {r[c + '_rel'][0]:.2e} ({r[c + '_rel'][1]}) / {r[c + '_ratio'][0]:.2e} ({r[c + '_ratio'][1]})"
                                         for c in ("conv", "bn", "in") if c + "_rel" in r) for s, r in rep.items()))
