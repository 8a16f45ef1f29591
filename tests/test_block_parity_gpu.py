"""Every block of the 16-bit TRAINING step against fp64, at the benchmarked shapes, by teacher forcing.

The whole-encoder comparisons (tests/test_round5_gpu.py, tests/test_config_gpu.py) cannot pin a train-mode gradient: 53
train-mode BatchNorms amplify rounding to O(1) direction errors at random init, so their bf16 floors pass almost anything.
Here each unit -- the stem (7x7/2 conv, BatchNorm, ReLU, max-pool) and each of the 16 Bottlenecks -- is checked ON ITS
OWN: the engine runs one train-mode forward and backward with block-boundary taps (SM3Engine.encoder_forward /
encoder_backward, taps=), and each unit is recomputed in fp64 on the GPU from the engine's OWN input to that unit and the
engine's OWN upstream gradient.  Every unit is then well conditioned, and per tensor it is compared:

  * the output (relative L2 error, max error over the tensor's max),
  * running_mean / running_var of every BatchNorm (relative L2) and num_batches_tracked (exactly),
  * the gradient of every parameter tensor -- conv weights, BatchNorm gamma / beta -- (cosine, relative L2),
  * the gradient at the unit's input, i.e. the engine's next tap down (cosine, relative L2).

At 224 x 224 and B = 256 pairs, layer 1 has 1.6 M rows per view: the size-selected paths (slab counts of the fixed-order
weight gradients, the eight-lane linbn_moments, view tiles, the stride-2 join, bn3's statistics by linearity from fp32
Gram matrices) run exactly as bench.py runs them.

The fp64 reference is oracle/sm3_oracle.py's `batchnorm` (one call per view half, in view order: statistics per view and
the two running-statistic updates) around fp64 convolutions written as one matmul per filter tap over NHWC rows (_Conv):
no unfold matrix, and weight gradients split over images so that no GEMM has a 1.6 M-long K loop on a handful of tiles.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- fp64 convolution on NHWC maps ----------------------------------------------------------------------------------
def _tap_slices(k, s, Ho, Wo):
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, (slice(None), slice(ky, ky + s * (Ho - 1) + 1, s), slice(kx, kx + s * (Wo - 1) + 1, s))


class _Conv(torch.autograd.Function):
    """conv2d without bias, x [N, H, W, Ci], w [Co, Ci, k, k] (OIHW) -> [N, Ho, Wo, Co], fp64: one GEMM per tap."""

    @staticmethod
    def forward(ctx, x, w, stride, pad):
        N, H, W, Ci = x.shape
        k = w.shape[2]
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        xp = F.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x
        out = None
        for ky, kx, sl in _tap_slices(k, stride, Ho, Wo):
            t = xp[sl].reshape(-1, Ci) @ w[:, :, ky, kx].t()
            out = t if out is None else out.add_(t)
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.pad = stride, pad
        return out.view(N, Ho, Wo, w.shape[0])

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        s, p = ctx.stride, ctx.pad
        N, H, W, Ci = x.shape
        Co, k = w.shape[0], w.shape[2]
        Ho, Wo = g.shape[1], g.shape[2]
        g = g.contiguous()
        xp = F.pad(x, (0, 0, p, p, p, p)) if p else x
        gi = g.view(N, Ho * Wo, Co).transpose(1, 2)  # [N, Co, pixels]: the weight gradient as a batch of per-image GEMMs
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        dxp = torch.zeros_like(xp) if ctx.needs_input_grad[0] else None
        for ky, kx, sl in _tap_slices(k, s, Ho, Wo):
            if dw is not None:
                dw[:, :, ky, kx] = torch.bmm(gi, xp[sl].reshape(N, Ho * Wo, Ci)).sum(0)
            if dxp is not None:
                dxp[sl] += (g.view(-1, Co) @ w[:, :, ky, kx]).view(N, Ho, Wo, Ci)
        dx = dxp[:, p:p + H, p:p + W] if (dxp is not None and p) else dxp
        return dx, dw, None, None


def _bn(t, P, B, name, V):
    """Train-mode BatchNorm of an NHWC map whose V views lie back to back: the oracle once per view, in view order."""
    from oracle import sm3_oracle as O
    outs = [O.batchnorm(c.permute(0, 3, 1, 2), P, B, name, True).permute(0, 2, 3, 1) for c in t.chunk(V, 0)]
    return outs[0] if V == 1 else torch.cat(outs, 0)


def _block_ref(x, P, B, p, stride, V):
    """Bottleneck.forward (src/models/resnet.py:154-174) -> (pre-ReLU sum out + identity, block output)."""
    out = F.relu(_bn(_Conv.apply(x, P[p + "conv1.weight"], 1, 0), P, B, p + "bn1", V))
    out = F.relu(_bn(_Conv.apply(out, P[p + "conv2.weight"], stride, 1), P, B, p + "bn2", V))
    out = _bn(_Conv.apply(out, P[p + "conv3.weight"], 1, 0), P, B, p + "bn3", V)
    if p + "downsample.0.weight" in P:
        idn = _bn(_Conv.apply(x, P[p + "downsample.0.weight"], stride, 0), P, B, p + "downsample.1", V)
    else:
        idn = x
    pre = out + idn
    return pre, F.relu(pre)


def _stem_ref(img, P, B, V):
    """conv1 7x7/2 -> bn1 -> ReLU -> max-pool 3x3/2 (src/models/resnet.py:292-297) on NCHW images -> NHWC map."""
    x = img.permute(0, 2, 3, 1)
    y = F.relu(_bn(_Conv.apply(x, P["conv1.weight"], 2, 3), P, B, "bn1", V))
    return F.max_pool2d(y.permute(0, 3, 1, 2), kernel_size=3, stride=2, padding=1).permute(0, 2, 3, 1)


# ---- metrics --------------------------------------------------------------------------------------------------------
def _cos(a, b):
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-300))


def _rel(got, ref):
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def _maxrel(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


# ---- the engine run -------------------------------------------------------------------------------------------------
def _engine_run(dt, N, V, size):
    """One train-mode forward + backward of an encoder-only engine with taps.  Returns what the reference needs."""
    from oracle import procedural
    from src.models import resnet
    from sm3hip.engine import SM3Engine
    torch.manual_seed(5)
    m = resnet.resnet50()
    m.fc = torch.nn.Identity()
    m.to(DEV).train()
    eng = SM3Engine(m, dtype=dt, kind="encoder")
    D = torch.device(DEV)
    eng.prepare(D)
    eng.refresh_weights()
    plan = eng.branches["main"][0]
    B = N // V
    imgs = [torch.from_numpy(procedural.make_images(B, size, 23, f"view{v}")).to(DEV) for v in range(V)]
    g = torch.Generator().manual_seed(29)
    dfeat = torch.randn(N, 2048, generator=g).to(DEV)
    buf0 = {k: b.detach().clone() for k, b in m.named_buffers()}  # the running statistics before the step
    feats = torch.empty(N, 2048, device=DEV)
    ctx, taps = [], {}
    eng.encoder_forward(plan, imgs if V > 1 else imgs[0], True, feats, None, ctx, views=V, taps=taps)
    eng.store.flat_g.zero_()
    eng.encoder_backward(ctx[0], dfeat.to(eng.tdt), taps=taps)
    torch.cuda.synchronize()
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
    return dict(eng=eng, P=P, grads=grads, bufs=bufs, buf0=buf0, taps=taps, img=img, plan=plan)


def _ref_params(run, prefix, names):
    """Leaf fp64 copies of the unit's parameters, and fp64 copies of its BatchNorms' buffers as they were before the step."""
    P = {n: run["P"][n].clone().requires_grad_(True) for n in names}
    B = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in run["buf0"].items()
         if k.startswith(prefix)}
    return P, B


def _record(rep, stage, kind, name, value, worse):
    """rep[stage][kind] = (worst value, tensor name); worse(a, b): a is worse than b."""
    cur = rep.setdefault(stage, {}).get(kind)
    if cur is None or worse(value, cur[0]):
        rep[stage][kind] = (value, name)


def _compare_unit(run, dt, prefix, stage, names, out_ref, got_out, dx_ref, got_dx, P, B, V, rep, fails, lim):
    """Compare one unit's output, running statistics, parameter gradients and input gradient against the fp64 ones."""
    lo, hi = (lambda a, b: a < b), (lambda a, b: a > b)
    fr, fm = _rel(got_out, out_ref), _maxrel(got_out, out_ref)
    _record(rep, stage, "out_rel", prefix or "stem", fr, hi)
    _record(rep, stage, "out_max", prefix or "stem", fm, hi)
    if fr > lim["out_rel"] or fm > lim["out_max"]:
        fails.append((prefix or "stem", "output", fr, fm))
    for k, ref in B.items():
        got = run["bufs"][k]
        if k.endswith("num_batches_tracked"):
            if int(got) != int(ref) or int(ref) != int(run["buf0"][k]) + V:
                fails.append((k, int(got), int(ref)))
            continue
        r = _rel(got.double(), ref)
        _record(rep, stage, "stat_rel", k, r, hi)
        if r > lim["stat_rel"]:
            fails.append((k, "running statistic", r))
    for n in names:
        ref, got = P[n].grad, run["grads"][n].double()
        c, r = _cos(got, ref), _rel(got, ref)
        _record(rep, stage, "g_cos", n, c, lo)
        _record(rep, stage, "g_rel", n, r, hi)
        cat = "conv" if got.dim() == 4 else "bn"
        q = abs(float(got.norm() / ref.norm()) - 1)
        _record(rep, stage, cat + "_rel", n, r, hi)
        _record(rep, stage, cat + "_ratio", n, q, hi)
        if c < lim["cos"] or r > lim["rel"] or q > lim[cat + "_ratio"]:
            fails.append((n, "gradient", c, r, q))
    if dx_ref is not None:
        c, r = _cos(got_dx, dx_ref), _rel(got_dx, dx_ref)
        _record(rep, stage, "g_cos", prefix + "<input>", c, lo)
        _record(rep, stage, "g_rel", prefix + "<input>", r, hi)
        q = abs(float(got_dx.norm() / dx_ref.norm()) - 1)
        _record(rep, stage, "in_rel", prefix + "<input>", r, hi)
        _record(rep, stage, "in_ratio", prefix + "<input>", q, hi)
        if c < lim["cos"] or r > lim["rel"] or q > lim["in_ratio"]:
            fails.append((prefix + "<input>", "input gradient", c, r, q))


def _stage(prefix):
    return prefix.split(".")[0] if prefix else "stem"


CASES = {  # dtype, images (both views), views, size
    "bf16-2x256-224": (torch.bfloat16, 512, 2, 224),   # exactly what bench.py times
    "f16-2x256-224": (torch.float16, 512, 2, 224),     # the --amp recipe, same kernel templates
    "bf16-16-224": (torch.bfloat16, 16, 1, 224),       # unpaired: no view tiles, stride-2 join without the 256 multiple
    "f32-16-224": (torch.float32, 16, 1, 224),         # exact-f32 mode: two-pass BatchNorms, f32 MFMA
    "f16-2x128-448": (torch.float16, 256, 2, 448),     # BASELINE config 5: the largest tensors
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_block_of_the_train_step_against_fp64_by_teacher_forcing(case):
    dt, N, V, size = CASES[case]
    dtname = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[dt]
    lim = BOUNDS[dtname]
    run = _engine_run(dt, N, V, size)
    taps, plan = run["taps"], run["plan"]
    rep, fails = {}, []
    assert len(taps["x"]) == len(taps["g"]) == len(plan.blocks) + 1

    def hwc(t, n_img):  # the engine's [N*H*W, C] rows -> fp64 [N, H, W, C]
        hw = t.shape[0] // n_img
        h = int(round(hw ** 0.5))
        return t.double().view(n_img, h, hw // h, t.shape[1])

    # the stem: conv 7x7/2 + bn1 + ReLU + max-pool on the images as the engine saw them; no input gradient
    names = ["conv1.weight", "bn1.weight", "bn1.bias"]
    P, B = _ref_params(run, "bn1.", names)
    out = _stem_ref(run["img"].double(), P, B, V)
    out.backward(hwc(taps["g"][0], N))
    _compare_unit(run, dt, "", "stem", names, out.detach(), hwc(taps["x"][0], N), None, None, P, B, V, rep, fails, lim)
    del out, P, B
    # the Bottlenecks, each from the engine's own input and upstream gradient
    for bi, blk in enumerate(plan.blocks):
        prefix = blk["c1"].name[: -len("conv1")]
        stride = blk["c2"].stride
        names = [n for n in run["P"] if n.startswith(prefix)]
        P, B = _ref_params(run, prefix, names)
        x = hwc(taps["x"][bi], N).requires_grad_(True)
        pre, out = _block_ref(x, P, B, prefix, stride, V)
        gup = hwc(taps["g"][bi + 1], N)
        (pre if taps["g_pre_relu"][bi + 1] else out).backward(gup)
        dx = x.grad
        if taps["g_pre_relu"][bi]:  # the engine's gradient at this boundary is already masked by the producer's ReLU
            dx = dx * (x.detach() > 0)
        _compare_unit(run, dt, prefix, _stage(prefix), names, out.detach(), hwc(taps["x"][bi + 1], N), dx,
                      hwc(taps["g"][bi], N), P, B, V, rep, fails, lim)
        del x, pre, out, gup, dx, P, B
    print(f"\n{case}: per stage, worst tensor: "
          + "; ".join(f"{s}: out rel {r['out_rel'][0]:.2e} max {r['out_max'][0]:.2e}, stats {r['stat_rel'][0]:.2e} "
                      f"({r['stat_rel'][1]}), grad cos {r['g_cos'][0]:.6f} ({r['g_cos'][1]}), "
                      f"rel {r['g_rel'][0]:.2e} ({r['g_rel'][1]})" for s, r in rep.items()))
    print(f"{case}: by class, worst rel / worst |norm ratio - 1|: "
          + "; ".join(f"{s}: " + ", ".join(f"{c} {r[c + '_rel'][0]:.2e} ({r[c + '_rel'][1]}) / {r[c + '_ratio'][0]:.2e} ({r[c + '_ratio'][1]})"
                                         for c in ("conv", "bn", "in") if c + "_rel" in r) for s, r in rep.items()))
    assert not fails, fails[:8]


# Measured (MI355X, det mode: the same bits on every run), worst tensor over all units and the cases of a mode:
#   bf16 (2x256 and 16 images at 224): output rel 5.7e-3, max 7.5e-3; running statistics 2.5e-4; gradient cosine 0.99463,
#        rel 0.104; |norm ratio - 1| of the unit's input gradient 3.0e-4, of a conv weight gradient 8.1e-3, of a BatchNorm
#        parameter gradient 1.4e-2
#   f16 (2x256 at 224, 2x128 at 448): output 7.2e-4, max 8.9e-4; statistics 1.2e-5; cosine 0.99953, rel 3.1e-2; ratios 1.7e-5
#        (input), 1.2e-3 (conv), 9.4e-3 (BatchNorm)
#   f32 (16 images at 224): output 1.2e-6, max 1.4e-6; statistics 1.1e-7; cosine 0.999996, rel 2.8e-3; ratios 1.9e-6, 2.0e-5,
#        2.2e-4
# The 16-bit gradient errors are far above 2^-8: the engine's saved activations and gradients are 16-bit, and a gradient
# behind a train-mode BatchNorm is a cancellation -- d(beta) = sum(dz) of a dz whose mean the next BatchNorm removed,
# d(W) of a conv feeding a BatchNorm orthogonal to W row by row -- which turns per-element rounding into a relative error
# of 1e-2 .. 1e-1 in the tensor (bf16 / f16 = 3.3 in every stage, the same for paired and unpaired batches: no single block
# stands out).  That noise is nearly orthogonal to the gradient, so a gradient's NORM stays within 3e-4 (bf16) of fp64:
# the norm ratio of the input gradient is the sharp check of the backward pass -- one linbn coefficient scaled by 1 + 1e-2
# moves it to 1.0e-2 in every block while the cosines do not move; a dropped stride-2 join addend drops the cosine of the
# stage's input gradient to 0.82; view-1 tiles of the fused conv3 epilogue using view 0's BatchNorm triple the max output
# error (2.8e-2 .. 3.8e-2).  In f32 every tensor is at 1e-6 except a few in three blocks (layer2.1, layer2.3, layer4.2:
# conv1 / conv2 weights and bn1 / bn2 bias at 4e-4 .. 2.8e-3, their gamma at 1e-6): a bn1 / bn2 output within rounding of 0
# takes the other side of the ReLU than in fp64 -- beta = 0, so it moves sum(dz) and not sum(dz * xhat) -- and over the
# 784 .. 12 544 rows of those maps one element is 1e-3 of a cancelled sum.  Bounds: 3 - 7x the measured values.
BOUNDS = {
    "bf16": {"out_rel": 1.5e-2, "out_max": 2e-2, "stat_rel": 1e-3, "cos": 0.97, "rel": 0.3,
             "in_ratio": 2e-3, "conv_ratio": 3e-2, "bn_ratio": 5e-2},
    "f16": {"out_rel": 3e-3, "out_max": 3e-3, "stat_rel": 6e-5, "cos": 0.9975, "rel": 0.1,
            "in_ratio": 1e-4, "conv_ratio": 6e-3, "bn_ratio": 3e-2},
    "f32": {"out_rel": 5e-6, "out_max": 6e-6, "stat_rel": 5e-7, "cos": 0.99998, "rel": 1e-2,
            "in_ratio": 1e-5, "conv_ratio": 1e-4, "bn_ratio": 1e-3},
}
