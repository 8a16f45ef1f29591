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
  * ranks (test_dp_parity_gpu.py, test_dp_parity_cpu.py): engine_run / standin_run as rank r of a data-parallel step with
    synchronised BatchNorm, check_run(stat_reduce=all_reduce_sum) as its fp64 reference, seeded defects of the exchange.

The second half of the file does the same for the HEAD of a training step -- everything past the layer4 tap: pool, projectors,
NT-Xent terms and dz, projector backward, the joins of the pooled-feature gradient, the metadata branch
(test_head_parity_gpu.py, test_head_parity_cpu.py; see the comment above HEAD_CASES).

Not a conftest; changes no pytest setting.  SM3_GEOMETRY_MEASURE=<file>: check_run and check_head append one JSON line per
case with the worst engine and restatement value of every metric (profiles/geometry_parity_measure.md and
profiles/head_parity_measure.md are made from such runs)."""
import json
import os
import sys

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


def bn(t, P, B, name, V, stat_reduce=None):
    """Train-mode BatchNorm of an NHWC map whose V views lie back to back: the oracle once per view, in view order.
    stat_reduce (SyncBatchNorm): sums the oracle's packed [sum x, sum x^2, count] over the ranks (all_reduce_sum).
    The float32 restatement hands the oracle its map in fp64 then and takes the result back in float32: the packed sums are
    the one-pass form (sum x^2 / n - mean^2), which in float32 cancels where ATen's two-pass form of the single-rank call
    does not, and the exchange format of the project is fp64 sums.  Measured on resnet50 f32, 2 ranks x 16 at 73 x 37: the
    restatement's running statistics at 3.7e-7 with float32 sums (limit 1.1e-6, above BOUNDS' 5e-7), 8.6e-8 with fp64 ones."""
    from oracle import sm3_oracle as O
    up = stat_reduce is not None and t.dtype == torch.float32
    outs = [O.batchnorm((c.double() if up else c).permute(0, 3, 1, 2), P, B, name, True, True, stat_reduce).permute(0, 2, 3, 1)
            for c in t.chunk(V, 0)]
    out = outs[0] if V == 1 else torch.cat(outs, 0)
    return out.to(t.dtype) if up else out


# ---- ranks: the exchange of SyncBatchNorm, and seeded defects of it (stand-in only) ---------------------------------------
class AllReduceSum(torch.autograd.Function):
    """Sum over the ranks of the default process group, forward and of the gradient backward: with it as a BatchNorm's
    stat_reduce the fp64 gradient on a rank is SyncBatchNorm's -- the global sums of dz and dz * xhat over the global count.
    Works on fp64 CUDA tensors over gloo (through host memory, as the engine's own stat_sync does)."""

    @staticmethod
    def forward(ctx, x):
        import torch.distributed as dist
        y = x.clone()
        dist.all_reduce(y)
        return y

    @staticmethod
    def backward(ctx, g):
        import torch.distributed as dist
        g = g.clone()
        dist.all_reduce(g)
        return g


all_reduce_sum = AllReduceSum.apply


class _ForwardOnlyReduce(torch.autograd.Function):
    """Seeded defect: the backward exchange dropped.  Forward the sum over ranks; backward the same collective, its result
    discarded (the ranks stay in step) and the gradient of the packed sums kept local."""

    @staticmethod
    def forward(ctx, x):
        return AllReduceSum.forward(ctx, x)

    @staticmethod
    def backward(ctx, g):
        AllReduceSum.backward(ctx, g)
        return g


class _NoReduce(torch.autograd.Function):
    """Seeded defect: statistics left local.  Both collectives of a clean reducer are issued and their results discarded."""

    @staticmethod
    def forward(ctx, x):
        AllReduceSum.forward(ctx, x)
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        AllReduceSum.backward(ctx, g)
        return g


def reduce_local_count(t):
    """Seeded defect: the summed sums over the LOCAL count (the last element of the oracle's packed vector)."""
    return torch.cat([all_reduce_sum(t)[:-1], t[-1:]])


reduce_forward_only = _ForwardOnlyReduce.apply
reduce_nothing = _NoReduce.apply


def _reducer(defect, name, stat_reduce):
    """The reducer of the BatchNorm `name` ("bn1" ... "downsample.1") of a unit: the run's, unless a defect names that
    BatchNorm under "reduce" ({BatchNorm name: reducer}).  A single-rank run has none, seeded or not."""
    if stat_reduce is None:
        return None
    return (defect or {}).get("reduce", {}).get(name, stat_reduce)


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
def block_ref(x, P, B, p, stride, V, groups=1, q=_ident, defect=None, stat_reduce=None):
    """Bottleneck.forward (src/models/resnet.py:154-174) -> (pre-ReLU sum out + identity, block output)."""
    d = defect or {}
    sr = lambda name: _reducer(d, name, stat_reduce)
    x = q(x)
    out = Conv.apply(x, P[p + "conv1.weight"], 1, 0)
    out = q(F.relu(bn(d.get("bn1", _ident)(q(out)), P, B, p + "bn1", V, sr("bn1"))))
    out = q(F.relu(bn(q(Conv.apply(out, P[p + "conv2.weight"], stride, 1, groups)), P, B, p + "bn2", V, sr("bn2"))))
    out = q(bn(q(Conv.apply(out, P[p + "conv3.weight"], 1, 0)), P, B, p + "bn3", V, sr("bn3")))
    if p + "downsample.0.weight" in P:
        idn = q(bn(q(Conv.apply(d.get("idn", _ident)(x), P[p + "downsample.0.weight"], stride, 0)), P, B, p + "downsample.1", V,
                   sr("downsample.1")))
    else:
        idn = d.get("idn", _ident)(x)
    pre = q(out + idn)
    return pre, F.relu(pre)


def basic_ref(x, P, B, p, stride, V, q=_ident, defect=None, stat_reduce=None):
    """BasicBlock.forward (src/models/resnet.py:91-106) on NHWC maps -> (pre-ReLU sum, block output)."""
    d = defect or {}
    sr = lambda name: _reducer(d, name, stat_reduce)
    x = q(x)
    out = Conv.apply(x, P[p + "conv1.weight"], stride, 1)
    out = q(F.relu(bn(d.get("bn1", _ident)(q(out)), P, B, p + "bn1", V, sr("bn1"))))
    out = q(bn(q(Conv.apply(out, P[p + "conv2.weight"], 1, 1)), P, B, p + "bn2", V, sr("bn2")))
    if p + "downsample.0.weight" in P:
        idn = q(bn(q(Conv.apply(d.get("idn", _ident)(x), P[p + "downsample.0.weight"], stride, 0)), P, B, p + "downsample.1", V,
                   sr("downsample.1")))
    else:
        idn = d.get("idn", _ident)(x)
    pre = q(out + idn)
    return pre, F.relu(pre)


def stem_ref(img, P, B, V, q=_ident, stat_reduce=None):
    """conv1 7x7/2 -> bn1 -> ReLU -> max-pool 3x3/2 (src/models/resnet.py:292-297) on NCHW images -> NHWC map."""
    x = img.permute(0, 2, 3, 1)
    y = q(F.relu(bn(q(Conv.apply(x, P["conv1.weight"], 2, 3)), P, B, "bn1", V, stat_reduce)))
    return q(F.max_pool2d(y.permute(0, 3, 1, 2), kernel_size=3, stride=2, padding=1).permute(0, 2, 3, 1))


def unit_ref(x, P, B, blk, V, q=_ident, defect=None, stat_reduce=None):
    """The block `blk` of a run's unit list -> (pre, out)."""
    if blk["basic"]:
        return basic_ref(x, P, B, blk["prefix"], blk["stride"], V, q, defect, stat_reduce)
    return block_ref(x, P, B, blk["prefix"], blk["stride"], V, blk["groups"], q, defect, stat_reduce)


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


def rank_inputs(N, V, H, W, out_dim, rank=0):
    """What rank `rank` feeds a run: ([one batch of N // V images per view], the gradient of the pooled features [N, out_dim]).
    The ranks' shards differ clearly -- other procedural images (a rank suffix on the tag), another seed of the gradient --
    and rank 0 gets the tensors a single-rank run always got."""
    sfx = f"-rank{rank}" if rank else ""
    imgs = [images(N // V, H, W, f"view{v}{sfx}") for v in range(V)]
    return imgs, torch.randn(N, out_dim, generator=torch.Generator().manual_seed(29 + rank))


def engine_run(arch, dt, N, V, H, W, dev="cuda:0", rank=0, world=1, stat_sync=None):
    """One train-mode forward + backward of an encoder-only engine with taps.  Returns what the reference needs.
    world > 1: the step of rank `rank` of a data-parallel run over N images PER RANK -- the same weights on every rank,
    rank_inputs' shard, and stat_sync (a callable that sums an fp64 CUDA tensor over the ranks in place) installed as a
    trainer installs it."""
    from sm3hip.engine import SM3Engine
    m = _encoder(arch)
    m.to(dev).train()
    eng = SM3Engine(m, dtype=dt, kind="encoder")
    if world > 1:
        assert stat_sync is not None
        eng.stat_sync, eng.world_size, eng._explicit_sync = stat_sync, world, True
    eng.prepare(torch.device(dev))
    eng.refresh_weights()
    plan = eng.branches["main"][0]
    imgs, dfeat = rank_inputs(N, V, H, W, plan.out_dim, rank)
    imgs, dfeat = [t.to(dev) for t in imgs], dfeat.to(dev)
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


def standin_run(arch, dt, N, V, H, W, dev="cpu", defects=None, rank=0, world=1, stat_reduce=None, shards=None):
    """The record engine_run returns, from the reference alone: the mode restatement of every unit chained into a whole
    encoder, one train-mode forward + backward under autograd.  Every boundary gradient is with respect to the block's
    output (g_pre_relu False).  defects: {unit prefix: {"bn1" | "idn": function, "reduce": {BatchNorm name: reducer}}}
    seeded into those units.
    world > 1: rank `rank` of a data-parallel run over N images per rank; stat_reduce (all_reduce_sum) goes to every
    BatchNorm.  shards (one view): the ranks whose inputs, back to back, make up this run's batch of N images -- the
    single-process full batch that a sharded run is compared with."""
    assert world == 1 or stat_reduce is not None
    m = _encoder(arch).train()
    edt = torch.float32 if dt == torch.float32 else torch.float64
    q = rounder(dt)
    wdt = dt if dt != torch.float32 else torch.float64
    P = {n: (w.detach().to(wdt).double() if w.dim() == 4 else w.detach().double()).to(dev) for n, w in m.named_parameters()}
    buf0 = {k: b.detach().clone().to(dev) for k, b in m.named_buffers()}
    units = describe_units(P, _units(P))
    Pl = {n: w.to(edt).clone().requires_grad_(True) for n, w in P.items()}
    Bl = {k: (v.to(edt).clone() if v.is_floating_point() else v.clone()) for k, v in buf0.items()}
    out_dim = P[units[-1]["prefix"] + ("bn2" if units[-1]["basic"] else "bn3") + ".weight"].shape[0]
    if shards is None:
        imgs, dfeat = rank_inputs(N, V, H, W, out_dim, rank)
    else:
        assert V == 1 and N % len(shards) == 0
        parts = [rank_inputs(N // len(shards), 1, H, W, out_dim, r) for r in shards]
        imgs, dfeat = [torch.cat([p[0][0] for p in parts], 0)], torch.cat([p[1] for p in parts], 0)
    img, dfeat = torch.cat(imgs, 0).to(dev), dfeat.to(dev)
    if dt != torch.float32:
        img = img.to(dt)
    xs = [stem_ref(img.to(edt), Pl, Bl, V, q, stat_reduce)]
    for u in units:
        x = xs[-1]
        x.retain_grad()
        xs.append(unit_ref(x, Pl, Bl, u, V, q, (defects or {}).get(u["prefix"]), stat_reduce)[1])
    xs[-1].retain_grad()
    assert xs[-1].shape[-1] == out_dim
    if dt != torch.float32:
        dfeat = dfeat.to(dt)
    xs[-1].mean(dim=(1, 2)).backward(dfeat.to(edt))
    flat = lambda t: t.detach().reshape(-1, t.shape[-1])
    taps = dict(x=[flat(x) for x in xs], g=[flat(x.grad) for x in xs], g_pre_relu=[False] * len(xs))
    return dict(P=P, grads={n: w.grad for n, w in Pl.items()}, bufs=Bl, buf0=buf0, taps=taps, img=img, units=units,
                N=N, V=V, maps=maps_of(H, W), dt=dt)


# ---- every unit of a run against fp64, limits by the rule ------------------------------------------------------------
def _unit_pass(run, ui, dtype, q, stat_reduce=None):
    """Unit ui (0: the stem) recomputed from the run's own input and upstream gradient, in `dtype` with the stores `q`.
    -> (names, P, B, output, input gradient or None), the gradient masked as the run's boundary gradient is."""
    N, V, maps, taps = run["N"], run["V"], run["maps"], run["taps"]
    if ui == 0:
        names = ["conv1.weight", "bn1.weight", "bn1.bias"]
        P, B = ref_params(run, "bn1.", names, dtype)
        out = stem_ref(run["img"].to(dtype), P, B, V, q, stat_reduce)
        out.backward(hwc(taps["g"][0], N, maps[1]).to(dtype))
        return names, P, B, out.detach(), None
    blk = run["units"][ui - 1]
    prefix = blk["prefix"]
    names = [n for n in run["P"] if n.startswith(prefix)]
    P, B = ref_params(run, prefix, names, dtype)
    x = hwc(taps["x"][ui - 1], N, stage_map(maps, run["units"][ui - 2]["prefix"] if ui > 1 else "")).to(dtype)
    x.requires_grad_(True)
    pre, out = unit_ref(x, P, B, blk, V, q, None, stat_reduce)
    gup = hwc(taps["g"][ui], N, stage_map(maps, prefix)).to(dtype)
    (pre if taps["g_pre_relu"][ui] else out).backward(gup)
    dx = x.grad
    if taps["g_pre_relu"][ui - 1]:  # the run's gradient at this boundary is already masked by the producer's ReLU
        dx = dx * (x.detach() > 0)
    return names, P, B, out.detach(), dx


def check_run(run, case, base=None, restate=True, stat_reduce=None):
    """Teacher forcing over every unit of `run`.  -> (rep, rest, fails): the per-stage record of the run against fp64, the
    same record of the mode restatement against fp64, and the tensors over their limit.
    base: the mode's bounds (default: BOUNDS of the run's dtype); restate=False: those bounds alone (the cases that
    test_block_parity_gpu.py holds at the benchmarked shapes).
    stat_reduce (the run is one rank of a data-parallel step): handed to every BatchNorm of the fp64 pass and of the
    restatement, so a unit's reference is SyncBatchNorm's on this rank's shard: global batch statistics and running
    statistics, local parameter gradients.  Every rank must call this with the same unit list: each BatchNorm is a
    collective, so the loop below never skips a unit or ends early on one rank."""
    dt, N, V, maps, taps = run["dt"], run["N"], run["V"], run["maps"], run["taps"]
    base = base or bounds(DTNAME[dt])
    assert len(taps["x"]) == len(taps["g"]) == len(run["units"]) + 1
    rep, rest, fails = {}, {}, []
    rdt, q = (torch.float32, _ident) if dt == torch.float32 else (torch.float64, rounder(dt))
    for ui in range(len(run["units"]) + 1):
        prefix = run["units"][ui - 1]["prefix"] if ui else ""
        stage = stage_of(prefix)
        names, P, B, out, dx = _unit_pass(run, ui, torch.float64, _ident, stat_reduce)
        lim = base
        if restate:
            _, Pq, Bq, outq, dxq = _unit_pass(run, ui, rdt, q, stat_reduce)
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


# ---- ranks as processes: one gloo group per world size, its cases one after the other -----------------------------------
def _rank_entry(fn, rank, world, port, q, cases, collective_s, threads):
    """Process `rank` of a group: fn(rank, world, case) for every case, in order -> q.put((rank, case index, True, payload));
    an exception ends the process with (rank, None, False, traceback).  Payloads are plain Python values."""
    import datetime
    import traceback
    import torch.distributed as dist
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        for p in (root, os.path.join(root, "skin-sm3_amd"), os.path.join(root, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        torch.set_num_threads(threads)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=collective_s))
        for i, case in enumerate(cases):
            q.put((rank, i, True, fn(rank, world, case)))
        dist.all_reduce(torch.zeros(1))  # (not barrier(): on a CPU-only group it would open the GPU, see test_dp_gloo.py)
        dist.destroy_process_group()
    except Exception:
        q.put((rank, None, False, traceback.format_exc()))


def run_rank_group(fn, world, cases, start_s, case_s, collective_s=120, threads=4):
    """`world` processes over gloo, spawned ONCE; each runs fn(rank, world, case) over `cases`.  fn must be a module-level
    function.  -> {"results": [{rank: payload} per case, complete ones only], "error": None or the report every remaining
    case fails with}.  Every wait has a limit: a collective collective_s, the first result start_s + case_s, each later one
    case_s.  After a reported exception or a result that does not come, nothing more is fetched, the group is terminated,
    and nothing is retried."""
    import queue
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_entry, args=(fn, r, world, port, q, cases, collective_s, threads)) for r in range(world)]
    for p in procs:
        p.start()
    results, error = [dict() for _ in cases], None
    wait = start_s + case_s
    for _ in range(world * len(cases)):
        try:
            rank, i, ok, payload = q.get(timeout=wait)
        except queue.Empty:
            error = f"no result within {wait} s; complete cases so far: {[len(r) == world for r in results]}"
            break
        if not ok:
            error = f"rank {rank} failed:\n{payload}"
            break
        results[i][rank] = payload
        wait = case_s
    for p in procs:
        if error is None:
            p.join(timeout=30)
        if p.is_alive():
            p.terminate()
            p.join(timeout=10)
    return {"results": [r if len(r) == world else None for r in results], "error": error}


def group_case(group, i):
    """{rank: payload} of case i of a run_rank_group record; fails with the group's report when the case did not complete."""
    res = group["results"][i]
    assert res is not None, group["error"]
    return res


# ======================================================================================================================
# The head: everything past the layer4 tap of a training step, pinned to fp64 by teacher forcing
# ======================================================================================================================
# average pool -> in-modal projector over 2B rows -> cross-modal projectors over B rows, one pass per pair -> NT-Xent terms
# with the weights 1 / 0.5 / 0.25 and the loss scale inside dz -> projector backward -> the into= / addend= accumulations
# that make up the pooled-feature gradient -> the pool's backward; and the metadata branch.
#
#   * head_engine_run(): one train-mode step through SM3Trainer.step with the engine's bound methods wrapped on the
#     instance (nothing of the engine changes): the return of forward, the dz handed to backward, the dfeat of every
#     encoder_backward call, the layer4 taps.  kind "simclr" has no trainer (SM3Trainer drives the two-branch models): its
#     step is forward -> sm3_ntxent_fused (the trainer's per-term launch) -> backward, without AdamW;
#   * head_standin_run(): the same record from the reference alone on synthetic layer4 maps, with seeded defects;
#   * head_tensors(): every compared tensor recomputed from the run's own INPUT to that step, in fp64 (q = _ident), as the
#     mode restatement (q = rounder(dt)), or in float32.  The restatement's rounding points are read off the engine's code:
#       - conv_bn: `xo` (the Linear output before its BatchNorm) is stored in the type and the batch statistics are those
#         of the stored tensor; `y_out` (BatchNorm + ReLU) is stored in the type; bn7 writes fp32 (out_f32): not rounded;
#       - the NT-Xent kernel stores dz in the type AFTER the multiplication by the loss scale (csrc/ntxent.hip, k = weight *
#         dz_scale / (T R)); the trainer's `dz["cross0"][rows] += dd[:Bm]` is one more store per addend;
#       - bn_backward writes the Linear-output gradient in the type (dxo = dy, in place); conv_backward writes the data
#         gradient in the type, masked by the previous unit's ReLU in its epilogue (fuse=);
#       - conv_backward(into=) is conv_gemm(..., into, into): accumulator + addend, ONE store per addend;
#       - the pool writes its fp32 and 16-bit features from one accumulator, and dfeat / (h w) in the type;
#       - weight gradients are fp32 sums in the flat buffer: not rounded;
#   * check_head(): per tensor, limit = limits(BOUNDS[mode], the restatement's value on the same inputs) -- the rule of
#     check_run, nothing else.  The loss is held to the tolerance tests/test_ntxent_edges_gpu.py holds the fused kernel to
#     (edge_inputs.loss_limit, per term), the 16-bit pooled features to equality with the rounded fp32 ones, and
#     num_batches_tracked to equality.
#   * the pooled-feature gradient is compared per branch, over the rows of both views (the dfeat of every encoder_backward
#     call, put back in view order): its norm ratio is a sum over elements and is sharper on 2B rows than on B.
HEAD_T = 0.1
META_PAD = 64
# Both f16 cases carry the loss scale 1024.  (The trainer's default, GradScaler's 65536, is a starting point the scaler backs
# off from whenever a step overflows; whether the first step at these shapes does was not measured, and a skipped step has
# no gradient to compare.)
HEAD_CASES = [  # id, kind, arch, style, mode, B, image side, proj_dim, metadata_dim, initial loss scale (f16)
    dict(id="1-r18-v32s0-bf16-B64", kind="v32", arch="resnet18", style=0, mode="bf16", B=64, size=32, proj=128, meta=None,
         scale=None),
    dict(id="2-r18-v32s2-f16-B72", kind="v32", arch="resnet18", style=2, mode="f16", B=72, size=32, proj=128, meta=None,
         scale=1024.0),
    dict(id="3-r18-v32s1-p64-bf16-B40", kind="v32", arch="resnet18", style=1, mode="bf16", B=40, size=32, proj=64, meta=None,
         scale=None, seed=1),
    dict(id="4-r50-v32s0-bf16-B256", kind="v32", arch="resnet50", style=0, mode="bf16", B=256, size=32, proj=128, meta=None,
         scale=None),
    dict(id="5-r50-v3s2-f16-B64", kind="v3", arch="resnet50", style=2, mode="f16", B=64, size=32, proj=128, meta=None,
         scale=1024.0),
    dict(id="6-r18-v32s0-f32-B8", kind="v32", arch="resnet18", style=0, mode="f32", B=8, size=32, proj=128, meta=None,
         scale=None, seed=1),
    dict(id="7-r18-v32s0-meta20-bf16-B64", kind="v32", arch="resnet18", style=0, mode="bf16", B=64, size=32, proj=128,
         meta=20, scale=None),
    dict(id="8-r18-simclr-64px-bf16-B64", kind="simclr", arch="resnet18", style=0, mode="bf16", B=64, size=64, proj=128,
         meta=None, scale=None),
]
# seed: of the stand-in's synthetic maps alone (head_standin_run; default 0).  Cases 3 and 6 take 1: the restatement's own norm
# ratio of the pooled-feature gradient in bf16 -- 80 x 512 and 16 x 512 elements -- is 1.9e-4 .. 1.2e-3 over the seeds 0 .. 5
# of case 3 and 8.1e-4 .. 2.3e-3 of case 6 (which no GPU case runs in 16 bit), and tests/test_head_parity_cpu.py keeps 3 x
# that value <= 3e-3 so that the limit rule stays sharp.
DEFAULT_INIT_SCALE = 65536.0  # SM3Trainer's (GradScaler's) default
FEAT_DIM = {"resnet18": 512, "resnet50": 2048}


def head_scale(case, dt):
    """The loss scale of a case in the type dt: the case's own, or the trainer's default, in f16; none otherwise."""
    return (case["scale"] or DEFAULT_INIT_SCALE) if dt == torch.float16 else 1.0


def cross_pairs(style):
    """The pair table of oracle.sm3_oracle.sm3_v32_projections (tests/test_head_parity_cpu.py holds it to that function)."""
    return {0: [(0, 0), (1, 1)], 1: [(0, 1), (1, 0)], 2: [(0, 0), (0, 1), (1, 0), (1, 1)]}[style]


def cross_weight(style):
    """The weight of a cross term in oracle.sm3_oracle.sm3_loss (held to it by the same test)."""
    return 0.25 if style == 2 else 0.5


def valround(dt):
    """A VALUE stored in the type (no autograd): the accumulations the engine does outside a differentiated chain."""
    return (lambda x: x.to(dt).to(x.dtype)) if dt in (torch.bfloat16, torch.float16) else _ident


def head_calls(kind, style, B, meta, pairs=None):
    """The projector passes of a step in the reference's order (SimCLR.forward per branch, then _cal_logits per pair: derm
    projector, clinic projector; then the metadata projector): dicts with the name of the z they write and its rows, the
    parameter prefix, the branch whose pooled features they read and the rows of those."""
    full, out = slice(0, 2 * B), []
    if kind == "simclr":
        return [dict(z="main", zrows=full, prefix="projector.", key="main", frows=full)]
    for key in ("derm", "clinic"):
        out.append(dict(z=key, zrows=full, prefix=f"{key}_backbone.projector.", key=key, frows=full))
    cp = ("cross_proj.", "cross_proj.") if kind == "v3" else ("cross_proj.0.", "cross_proj.1.")
    for ci, ab in enumerate(cross_pairs(style) if pairs is None else pairs):
        for side, key in enumerate(("derm", "clinic")):
            out.append(dict(z=f"cross{ci}", zrows=slice(side * B, (side + 1) * B), prefix=cp[side], key=key,
                            frows=slice(ab[side] * B, (ab[side] + 1) * B)))
    if meta:
        out.append(dict(z="meta", zrows=slice(0, B), prefix="meta_proj.", key=None, frows=slice(0, B)))
    return out


def proj_ref(x, P, B, prefix, q=_ident, bn7=None):
    """oracle.sm3_oracle.projector with the stores of a mode: q after every Linear and every BatchNorm + ReLU; the last
    BatchNorm (affine=False) writes fp32.  bn7 (a seeded defect): (gamma, beta) of an affine it does not have."""
    from oracle import sm3_oracle as O
    h = q(F.linear(x, P[prefix + "0.weight"]))
    h = q(F.relu(O.batchnorm(h, P, B, prefix + "1", True)))
    h = q(F.linear(h, P[prefix + "3.weight"]))
    h = q(F.relu(O.batchnorm(h, P, B, prefix + "4", True)))
    h = q(F.linear(h, P[prefix + "6.weight"]))
    if bn7 is not None:
        Pd = {prefix + "7.weight": bn7[0].to(h.dtype), prefix + "7.bias": bn7[1].to(h.dtype)}
        return O.batchnorm(h, Pd, B, prefix + "7", True, True)
    return O.batchnorm(h, P, B, prefix + "7", True, False)


def _proj_forward(calls, feats, meta_x, P, B, q, order=None, widen=False, once=False, bn7=None):
    """Every projector pass of `calls` on the rows it reads -> [(call, leaf input, rows of the leaf the pass is about, z)],
    the buffers B advancing in the order `order` (default: the order of calls).
    Seeded defects: widen -- a cross pass normalises over all 2B rows of its modality; once -- a cross projector's running
    statistics advance on its first pass only; bn7 -- {prefix: (gamma, beta)}."""
    out = [None] * len(calls)
    seen = set()
    for i in (range(len(calls)) if order is None else order):
        c = calls[i]
        src = meta_x if c["key"] is None else feats[c["key"]]
        cross = c["z"].startswith("cross")
        rows = slice(0, src.shape[0]) if (widen and cross) else c["frows"]
        x = src[rows].detach().clone().requires_grad_(True)
        Bc = B
        if once and cross and c["prefix"] in seen:
            Bc = {k: v.clone() for k, v in B.items()}
        seen.add(c["prefix"])
        z = proj_ref(x, P, Bc, c["prefix"], q, (bn7 or {}).get(c["prefix"]))
        take = c["frows"] if (widen and cross) else slice(0, x.shape[0])
        out[i] = (c, x, take, z[take])
    return out


def _assemble_z(fw, B, proj):
    zs = {}
    for c, _, _, z in fw:
        n = B if c["z"] == "meta" else 2 * B
        zs.setdefault(c["z"], torch.zeros(n, proj, dtype=z.dtype, device=z.device))[c["zrows"]] = z.detach()
    return zs


def _head_loss(zs, style, B, T, wc=None):
    """fp64 (or float32) NT-Xent of the projections with the weights of sm3_loss, and the trainer's two metadata terms.
    -> (terms [(name, weighted loss)], pieces [(name, rows, d(term) / d(z[name][rows]), first)] in the order the trainer
    stores / adds them: the first piece of a name is the kernel's store of the whole tensor, the others are `+=`)."""
    from oracle import sm3_oracle as O
    wc = cross_weight(style) if wc is None else wc
    dev = next(iter(zs.values())).device  # the oracle's closed form builds its masks on the CPU: a few hundred rows, run there
    leaf = {n: z.detach().cpu().clone().requires_grad_(True) for n, z in zs.items()}
    terms, pieces = [], []
    for n in leaf:
        if n == "meta":
            continue
        t = (wc if n.startswith("cross") else 1.0) * O.ntxent_loss_closed_form(leaf[n], T)
        terms.append((n, t.detach().to(dev)))
        pieces.append((n, slice(0, 2 * B), torch.autograd.grad(t, leaf[n])[0].to(dev), True))
    if "meta" in leaf:
        for half in (0, 1):
            rows = slice(half * B, (half + 1) * B)
            t = 0.5 * O.ntxent_loss_closed_form(torch.cat([leaf["cross0"][rows], leaf["meta"]], 0), T)
            gc, gm = torch.autograd.grad(t, [leaf["cross0"], leaf["meta"]])
            terms.append((f"meta{half}", t.detach().to(dev)))
            pieces.append(("cross0", rows, gc[rows].to(dev), False))
            pieces.append(("meta", slice(0, B), gm.to(dev), half == 0))
    return terms, pieces


def _assemble_dz(pieces, scale, qv, skip=()):
    """dz as the step leaves it: the kernel's store qv(scale * g) of every piece, `+=` pieces added in the type."""
    dz = {}
    for name, rows, g, first in pieces:
        s = qv(scale * g)
        if first:
            dz[name] = s.clone()
        elif name not in skip:
            dz[name][rows] = qv(dz[name][rows] + s)
    return dz


def _proj_backward(fw, dz, dtype):
    """Backward of every pass from its rows of dz: parameter gradients accumulate in the leaves of P, the input gradient of
    a pass is its x.grad."""
    for c, x, take, z in fw:
        z.backward(dz[c["z"]][c["zrows"]].to(dtype))


def _join(fw, B, qv, drop=None, view0_only=False):
    """The pooled-feature gradient of every branch as _backward assembles it: the in-modal projector's data gradient
    (conv_backward(addend=None): one store), then one conv_backward(into=) per cross pass in pair order: a store per addend.
    Seeded defects: drop -- (branch, index of the addend left out); view0_only -- the in-modal gradient reaches view 0 only."""
    dfe, n_add = {}, {}
    for c, x, take, _ in fw:
        key, g = c["key"], x.grad[take]
        if key is None:
            continue
        if not c["z"].startswith("cross"):
            dfe[key] = qv(g.clone())
            if view0_only:
                dfe[key][B:] = 0
            continue
        i = n_add[key] = n_add.get(key, -1) + 1
        if drop == (key, i):
            continue
        dfe[key][c["frows"]] = qv(dfe[key][c["frows"]] + g)
    return dfe


def _pool_expand(df, hw, qv):
    """avgpool_bwd: dfeat / (h w) at every pixel, stored in the type -> [N * hw, C]."""
    return qv(df / hw).unsqueeze(1).expand(-1, hw, -1).reshape(df.shape[0] * hw, df.shape[1])


def head_names(P):
    return [n for n in P if "projector." in n or n.startswith(("cross_proj.", "meta_proj."))]


def head_tensors(run, dtype, q, qv):
    """Every compared tensor of the head, each from the run's own input to its step, in `dtype` with the stores q / qv.
    Reads of the run: tap_x (-> pool), ft and meta_x (-> projectors, buffers), zs (-> loss, dz), dz and ft (-> projector
    backward, joins, parameter gradients), dfeat (-> pool gradient); never f32, tap_g, bufs, grads or loss.
    -> {name: (class, tensor)}; classes: out, stat, count, loss, dz, in, w, bn."""
    B, hw, style, scale, kind = run["B"], run["hw"], run["style"], run["scale"], run["kind"]
    out = {}
    for key in run["branches"]:
        x = run["tap_x"][key].to(dtype)
        out[f"pool:{key}"] = ("out", x.view(2 * B, hw, -1).mean(1))
        g = _pool_expand(run["dfeat"][key].to(dtype), hw, qv)
        if run["g_pre_relu"][key]:
            g = g * (run["tap_x"][key] > 0)
        out[f"poolgrad:{key}"] = ("in", g / scale)
    # projectors forward, the buffers' update sequence, and the backward from the run's own dz
    names = head_names(run["P"])
    P = {n: run["P"][n].to(dtype).clone().requires_grad_(True) for n in names}
    Bf = {k: (v.to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in run["buf0"].items()
          if any(k.startswith(c["prefix"]) for c in run["calls"])}
    feats = {k: run["ft"][k].to(dtype) for k in run["branches"]}
    meta_x = run["meta_x"].to(dtype) if run["meta_x"] is not None else None
    fw = _proj_forward(run["calls"], feats, meta_x, P, Bf, q)
    for n, z in _assemble_z(fw, B, run["proj"]).items():
        out[f"z:{n}"] = ("out", z)
    for k, v in Bf.items():
        out[f"buf:{k}"] = ("count" if k.endswith("num_batches_tracked") else "stat", v)
    _proj_backward(fw, {n: d.to(dtype) for n, d in run["dz"].items()}, dtype)
    for key, d in _join(fw, B, qv).items():  # both views' rows: the norm concentrates better on 2B rows than on B
        out[f"dfeat:{key}"] = ("in", d / scale)
    for n in names:
        out[f"grad:{n}"] = ("w" if P[n].dim() == 2 else "bn", P[n].grad / scale)
    # loss and dz from the run's own projections
    terms, pieces = _head_loss({n: z.to(dtype) for n, z in run["zs"].items()}, style, B, run["T"])
    out["loss"] = ("loss", torch.stack([t for _, t in terms]))
    for n, d in _assemble_dz(pieces, scale, qv).items():
        out[f"dz:{n}"] = ("dz", d / scale)
    return {k: (c, t.detach()) for k, (c, t) in out.items()}


def head_got(run):
    """The run's own tensors under the names of head_tensors."""
    s, B, out = run["scale"], run["B"], {}
    for key in run["branches"]:
        out[f"pool:{key}"] = run["f32"][key]
        out[f"poolgrad:{key}"] = run["tap_g"][key].double() / s
        out[f"dfeat:{key}"] = run["dfeat"][key].double() / s
    for n, z in run["zs"].items():
        out[f"z:{n}"] = z
    for k, v in run["bufs"].items():
        out[f"buf:{k}"] = v
    for n, d in run["dz"].items():
        out[f"dz:{n}"] = d.double() / s
    for n in head_names(run["P"]):
        out[f"grad:{n}"] = run["grads"][n].double() / s
    return out


_CLASS_METRICS = {"out": ("out_rel", "out_max"), "stat": ("stat_rel",), "dz": ("cos", "rel"), "in": ("cos", "rel", "in_ratio"),
                  "w": ("cos", "rel", "conv_ratio"), "bn": ("cos", "rel", "bn_ratio")}


def head_metrics(cls, got, ref):
    got, ref = got.double(), ref.double()
    ratio = abs(float(got.norm() / (ref.norm() + 1e-300)) - 1)
    vals = {"out_rel": rel(got, ref), "out_max": maxrel(got, ref), "stat_rel": rel(got, ref), "cos": cos(got, ref),
            "rel": rel(got, ref), "in_ratio": ratio, "conv_ratio": ratio, "bn_ratio": ratio}
    return {m: vals[m] for m in _CLASS_METRICS[cls]}


def within(m, v, lim):
    """NaN is outside every limit."""
    return (v >= lim[m]) if m == "cos" else (v <= lim[m])


def head_limits(run, base=None):
    """-> (ref, restated values, limits) per tensor name: the fp64 tensors, the mode restatement's metrics against them, and
    limits(BOUNDS[mode], those).  A function of the inputs head_tensors reads, and of nothing the run returned for that
    step."""
    dt = run["dt"]
    base = base or bounds(DTNAME[dt])
    rdt, q, qv = (torch.float32, _ident, _ident) if dt == torch.float32 else (torch.float64, rounder(dt), valround(dt))
    ref = head_tensors(run, torch.float64, _ident, _ident)
    rst = head_tensors(run, rdt, q, qv)
    vals, lims = {}, {}
    for name, (cls, t) in ref.items():
        if cls in _CLASS_METRICS:
            vals[name] = head_metrics(cls, rst[name][1], t)
            lims[name] = limits({m: base[m] for m in _CLASS_METRICS[cls]}, vals[name])
    return ref, vals, lims


def nbt_expected(run):
    """num_batches_tracked after the step: the pre-step count + the passes of that projector (+1 in-modal and metadata,
    +len(pairs) per cross projector, +2 len(pairs) for v3's shared one)."""
    out = {}
    for c in run["calls"]:
        for i in (1, 4, 7):
            k = f"{c['prefix']}{i}.num_batches_tracked"
            out[k] = out.get(k, int(run["buf0"][k])) + 1
    return out


def check_head(run, case, base=None):
    """Teacher forcing over the head of `run` -> (rep, rest, fails, lims): the worst value per stage and metric of the run and
    of the restatement against fp64, the tensors over their limit (name first), and the limits applied per tensor."""
    from edge_inputs import loss_limit
    dt = run["dt"]
    ref, vals, lims = head_limits(run, base)
    got = head_got(run)
    rep, rest, fails = {}, {}, []
    worse = lambda m: (lambda a, b: a < b) if m == "cos" else (lambda a, b: a > b)
    for name, (cls, t) in ref.items():
        stage = name.split(":")[0]
        if cls == "count":
            k = name[len("buf:"):]
            if not (int(got[name]) == int(t) == nbt_expected(run)[k]):
                fails.append((name, "num_batches_tracked", int(got[name]), int(t), nbt_expected(run)[k]))
            continue
        if cls == "loss":
            lim = sum(loss_limit(float(x)) for x in t)
            err = abs(run["loss"] - float(t.sum()))
            record(rep, stage, "loss_err", name, err, lambda a, b: a > b)
            record(rep, stage, "loss_lim", name, lim, lambda a, b: a > b)
            if not err <= lim:
                fails.append((name, "loss", run["loss"], float(t.sum()), lim))
            continue
        mine = head_metrics(cls, got[name], t)
        for m, v in mine.items():
            record(rep, stage, _REP_KEY[m], name, v, worse(m))
            record(rest, stage, _REP_KEY[m], name, vals[name][m], worse(m))
        bad = [m for m, v in mine.items() if not within(m, v, lims[name])]
        if bad:
            fails.append((name, cls, {m: (mine[m], lims[name][m]) for m in bad}))
    for key in run["branches"]:  # one rounding of the pool's accumulator: the 16-bit features ARE the fp32 ones, rounded
        if not torch.equal(run["ft"][key], run["f32"][key].to(dt)):
            fails.append((f"pool:{key}:ft", "is not the fp32 feature rounded to the type",
                          int((run["ft"][key] != run["f32"][key].to(dt)).sum())))
    applied = {}
    for name, lim in lims.items():
        for m, v in lim.items():
            applied[m] = min(applied.get(m, v), v) if m == "cos" else max(applied.get(m, v), v)
    measure_line({"case": case, "engine": worst(rep), "restated": worst(rest), "limit": applied,
                  "loss": {"err": rep["loss"]["loss_err"][0], "limit": rep["loss"]["loss_lim"][0]}})
    return rep, rest, fails, lims


def head_report(case, rep, rest, lims):
    we, wr = worst(rep), worst(rest)
    print(f"\n{case}: worst over the head's tensors, run / restatement: "
          + ", ".join(f"{m} {we[m]:.3g} / {wr[m]:.3g}" for m in METRICS if m in we)
          + f"; loss error {rep['loss']['loss_err'][0]:.2e} (limit {rep['loss']['loss_lim'][0]:.2e})")
    print(f"{case}: per stage, worst tensor: "
          + "; ".join(f"{s}: " + ", ".join(f"{k} {v:.3g} ({n})" for k, (v, n) in r.items()) for s, r in rep.items()))


# ---- the runs -------------------------------------------------------------------------------------------------------
def _perturb_head(named_modules, seed=13):
    """Seeded, non-trivial affine parameters and running statistics for the projectors' BatchNorms (the fresh-module state
    -- gamma 1, beta 0, mean 0, var 1 -- hides a wrong gamma or a skipped update)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda t, a, b: t.copy_(torch.rand(t.shape, generator=g) * (b - a) + a)
    with torch.no_grad():
        for name, mod in named_modules:
            if isinstance(mod, torch.nn.BatchNorm1d):
                u(mod.running_mean, -0.1, 0.1)
                u(mod.running_var, 0.5, 1.5)
                if mod.affine:
                    u(mod.weight, 0.5, 1.5)
                    u(mod.bias, -0.2, 0.2)


def head_metadata(B, d):
    return torch.randn(B, d, generator=torch.Generator().manual_seed(41))


def _meta_input(B, d, dt):
    """The metadata projector's input as forward() makes it: zero-padded to META_PAD columns, cast to the type."""
    x = torch.zeros(B, META_PAD)
    x[:, :d] = head_metadata(B, d)
    return x.to(dt)


def head_setup(case, dt, dev, lanes=None):
    """A fresh model, trainer (None for kind "simclr") and engine for a case, and the step's inputs."""
    from sm3hip.bridge import sm3_engine_for
    from sm3hip.trainer import SM3Trainer
    from src.models.simclr import SimCLR, SimCLRSkinV3, SimCLRSkinV32
    kind, B, size = case["kind"], case["B"], case["size"]
    torch.manual_seed(5)
    if kind == "v32":
        model = SimCLRSkinV32(case["arch"], None, case["proj"], HEAD_T, metadata_dim=case["meta"])
    elif kind == "v3":
        model = SimCLRSkinV3(case["arch"], None, case["proj"], HEAD_T)
    else:
        model = SimCLR(case["arch"], None, case["proj"], HEAD_T)
    _perturb_head([(n, m) for n, m in model.named_modules() if "projector" in n or n.startswith(("cross_proj", "meta_proj"))])
    model.sm3_dtype = dt
    model.to(dev).train()
    tr = None
    if kind != "simclr":
        tr = SM3Trainer(model, lr=1e-3, weight_decay=5e-2, eps=1e-5, style=case["style"], init_scale=head_scale(case, dt))
    eng = sm3_engine_for(model, kind)
    if lanes is not None:
        eng.two_streams, eng.lane_cross = lanes[0], lanes[1] and eng.lane_cross  # v3 keeps its lane_cross off
    eng.prepare(torch.device(dev))
    if kind == "simclr":
        imgs = {"main": [images(B, size, size, f"main{v}").to(dev) for v in (0, 1)]}
    else:
        imgs = {k: [images(B, size, size, f"{k}{v}").to(dev) for v in (0, 1)] for k in ("derm", "clinic")}
    meta = head_metadata(B, case["meta"]).to(dev) if case["meta"] else None
    return model, tr, eng, imgs, meta


def head_step(case, tr, eng, imgs, meta):
    """One step -> the loss (a float).  kind "simclr": forward, the trainer's per-term NT-Xent launch, backward."""
    from sm3hip import ops
    if tr is not None:
        return float(tr.step(imgs["derm"], imgs["clinic"], metadata=meta))
    eng.store.flat_g.zero_()
    zs, _, saved = eng.forward(imgs, 0, True, True)
    z = zs["main"]
    loss = torch.zeros(1, dtype=torch.float32, device=z.device)
    dz = torch.empty(z.shape, dtype=eng.tdt, device=z.device)
    ws = eng._work("ntxent_ws", ops.ntxent_workspace_floats(*z.shape))
    ops.ntxent_fused(eng.dtype, z, HEAD_T, 1.0, ws, loss, dz, dz_scale=None)
    eng.backward(saved, {"main": dz})
    return float(loss)


def head_engine_run(case, dt=None, dev="cuda:0", lanes=None):
    """One train-mode step of a HEAD_CASES entry on the engine -> the record check_head reads."""
    dt = dt or DTYPE[case["mode"]]
    B, size = case["B"], case["size"]
    model, tr, eng, imgs, meta = head_setup(case, dt, dev, lanes)
    st = eng.store
    wdt = dt if dt != torch.float32 else torch.float64
    P = {n: st._view(st.flat_p, n).detach().clone() for n in st.names}
    P = {n: (w.to(wdt).double() if w.dim() >= 2 else w.double()) for n, w in P.items()}  # Linear weights are filter banks
    buf0 = {k: b.detach().clone() for k, b in model.named_buffers()}
    cap = dict(taps={}, order=[], dfeat=[], scale=1.0)
    real = dict(forward=eng.forward, backward=eng.backward, ef=eng.encoder_forward, eb=eng.encoder_backward)

    def encoder_forward(plan, x, train, feat_f32, feat_t, save=None, **kw):
        taps = {}
        real["ef"](plan, x, train, feat_f32, feat_t, save, taps=taps, **kw)
        cap["taps"][id(save[-1])] = (plan.prefix, kw.get("views", 1), taps, save[-1])

    def encoder_backward(ctx, dfeat, *a, **kw):
        taps = cap["taps"][id(ctx)][2]
        cap["dfeat"].append((id(ctx), dfeat.clone()))
        return real["eb"](ctx, dfeat, *a, taps=taps, **kw)

    def forward(*a, **kw):
        out = real["forward"](*a, **kw)
        cap["fwd"] = (dict(out[0]), out[1])  # a copy of the dict: the trainer pops "meta" from its own
        return out

    def backward(saved, dz, *a, **kw):
        cap["dz"] = {n: d.clone() for n, d in dz.items()}
        if tr is not None and tr._scaler is not None:
            cap["scale"] = tr._scaler["scale"].clone()  # no host read inside the step
        out = real["backward"](saved, dz, *a, **kw)
        cap["grads"] = st.flat_g.clone()  # as the backward pass left them (an AdamW launch may follow)
        return out

    eng.forward, eng.backward, eng.encoder_forward, eng.encoder_backward = forward, backward, encoder_forward, encoder_backward
    try:
        loss = head_step(case, tr, eng, imgs, meta)
        torch.cuda.synchronize()
    finally:
        for k in ("forward", "backward", "encoder_forward", "encoder_backward"):
            delattr(eng, k)
    zs, feats = cap["fwd"]
    branches = list(eng.branches)
    hw_ = maps_of(size, size)[4]
    hw = hw_[0] * hw_[1]
    # the encoder passes of a branch, in forward order: one pair pass, or view 0 then view 1
    passes = {k: [] for k in branches}
    for cid, (prefix, views, taps, ctx) in cap["taps"].items():
        key = next(k for k in branches if eng.branches[k][0].prefix == prefix)
        passes[key].append((cid, views, taps))
    dfe = dict(cap["dfeat"])
    tap_x, tap_g, pre, dfeat = {}, {}, {}, {}
    for key, ps in passes.items():
        assert [v for _, v, _ in ps] in ([2], [1, 1]), ps
        tap_x[key] = torch.cat([t["x"][-1] for _, _, t in ps], 0)
        tap_g[key] = torch.cat([t["g"][-1] for _, _, t in ps], 0)
        pre[key] = any(t["g_pre_relu"][-1] for _, _, t in ps)
        dfeat[key] = torch.cat([dfe[cid] for cid, _, _ in ps], 0)
        assert tap_x[key].shape[0] == 2 * B * hw
    grads = {n: st._view(cap["grads"], n) for n in st.names}
    meta_x = _meta_input(B, case["meta"], dt).to(dev) if case["meta"] else None
    return dict(kind=case["kind"], style=case["style"], dt=dt, B=B, hw=hw, proj=case["proj"], T=HEAD_T,
                scale=float(cap["scale"]), branches=branches, calls=head_calls(case["kind"], case["style"], B, case["meta"]),
                P=P, buf0=buf0, bufs=dict(model.named_buffers()), tap_x=tap_x, tap_g=tap_g, g_pre_relu=pre,
                f32={k: feats[k][0] for k in branches}, ft={k: feats[k][1] for k in branches}, zs=dict(zs), dz=cap["dz"],
                dfeat=dfeat, grads=grads, loss=loss, meta_x=meta_x,
                paired={k: len(ps) == 1 for k, ps in passes.items()}, eng=eng, trainer=tr, model=model)


def _head_modules(case):
    """The projectors of a case's model alone (no encoders), under the names the model gives them."""
    from src.models.simclr import make_projector
    C, proj = FEAT_DIM[case["arch"]], case["proj"]
    torch.manual_seed(5)
    if case["kind"] == "simclr":
        return {"projector.": make_projector(C, proj)}
    mods = {f"{k}_backbone.projector.": make_projector(C, proj) for k in ("derm", "clinic")}
    if case["kind"] == "v3":
        mods["cross_proj."] = make_projector(C, proj)
    else:
        mods["cross_proj.0."], mods["cross_proj.1."] = make_projector(C, proj), make_projector(C, proj)
    if case["meta"]:
        mods["meta_proj."] = make_projector(META_PAD, proj)
    return mods


HEAD_DEFECTS = ("pairs_style0", "cross_weight_half", "cross_bn_2B", "cross_stats_once", "v3_order", "bn7_affine", "drop_into",
                "addend_view0", "dz_scaled", "meta_not_added", "pool_twice")


def head_standin_run(case, dt, defects=(), dev="cpu"):
    """The record head_engine_run returns, from the reference alone: the mode restatement of the head chained from seeded
    synthetic layer4 maps (ReLU of a Gaussian with per-channel scales, stored in the type) through the pool, the projectors,
    the loss, dz, the projector backward, the joins and the pool's backward, with autograd inside every piece.
    defects: names of HEAD_DEFECTS seeded into the chain (never into the record's description of the step)."""
    defects = set(defects)
    assert defects <= set(HEAD_DEFECTS), defects
    kind, style, B, proj = case["kind"], case["style"], case["B"], case["proj"]
    C = FEAT_DIM[case["arch"]]
    hw_ = maps_of(case["size"], case["size"])[4]
    hw = hw_[0] * hw_[1]
    edt = torch.float32 if dt == torch.float32 else torch.float64
    q, qv = rounder(dt), valround(dt)
    wdt = dt if dt != torch.float32 else torch.float64
    scale = head_scale(case, dt)
    mods = _head_modules(case)
    _perturb_head([(p, m) for p, seq in mods.items() for m in seq])
    P, buf0 = {}, {}
    for p, seq in mods.items():
        for n, w in seq.named_parameters():
            P[p + n] = (w.detach().to(wdt).double() if w.dim() >= 2 else w.detach().double()).to(dev)
        for n, b in seq.named_buffers():
            buf0[p + n] = b.detach().clone().to(dev)
    Pl = {n: w.to(edt).clone().requires_grad_(True) for n, w in P.items()}
    Bl = {k: (v.to(edt).clone() if v.is_floating_point() else v.clone()) for k, v in buf0.items()}
    branches = ["main"] if kind == "simclr" else ["derm", "clinic"]
    tap_x, f32, ft = {}, {}, {}
    for i, key in enumerate(branches):
        g = torch.Generator().manual_seed(101 + i + 1000 * case.get("seed", 0))
        scales = torch.exp(0.5 * torch.randn(C, generator=g))
        tap_x[key] = F.relu(torch.randn(2 * B * hw, C, generator=g) * scales).to(dt).to(dev)
        f32[key] = tap_x[key].to(edt).view(2 * B, hw, C).mean(1).float()
        ft[key] = f32[key].to(dt)
    meta_x = _meta_input(B, case["meta"], dt).to(dev) if case["meta"] else None
    calls = head_calls(kind, style, B, case["meta"])
    mine = head_calls(kind, style, B, case["meta"], pairs=cross_pairs(0)) if "pairs_style0" in defects else calls
    order = None
    if "v3_order" in defects:  # all derm passes of the shared projector, then all clinic ones
        cross = [i for i, c in enumerate(mine) if c["z"].startswith("cross")]
        rest = [i for i in range(len(mine)) if i not in cross]
        order = [i for i in rest if mine[i]["key"] is not None] + [i for i in cross if mine[i]["key"] == "derm"] \
            + [i for i in cross if mine[i]["key"] == "clinic"] + [i for i in rest if mine[i]["key"] is None]
    bn7 = None
    if "bn7_affine" in defects:
        g = torch.Generator().manual_seed(3)
        bn7 = {p: (1 + 0.1 * torch.randn(proj, generator=g), 0.1 * torch.randn(proj, generator=g)) for p in mods}
    fw = _proj_forward(mine, {k: ft[k].to(edt) for k in branches}, None if meta_x is None else meta_x.to(edt), Pl, Bl, q,
                       order=order, widen="cross_bn_2B" in defects, once="cross_stats_once" in defects, bn7=bn7)
    zs = {n: z.float() for n, z in _assemble_z(fw, B, proj).items()}
    terms, pieces = _head_loss({n: z.to(edt) for n, z in zs.items()}, style, B, HEAD_T,
                               wc=0.5 if "cross_weight_half" in defects else None)
    loss = float(sum(float(t) for _, t in terms))
    dz = _assemble_dz(pieces, scale * (scale if "dz_scaled" in defects else 1.0), qv,
                      skip=("cross0",) if "meta_not_added" in defects else ())
    dz = {n: d.to(dt) for n, d in dz.items()}
    _proj_backward(fw, dz, edt)
    dfe = _join(fw, B, qv, drop=("derm", len(cross_pairs(style)) - 1) if "drop_into" in defects else None,
                view0_only="addend_view0" in defects)
    dfeat = {k: d.to(dt) for k, d in dfe.items()}
    tap_g = {k: _pool_expand(dfeat[k].to(edt) / (hw if "pool_twice" in defects else 1), hw, qv).to(dt) for k in branches}
    grads = {n: (w.grad if w.grad is not None else torch.zeros_like(w)) for n, w in Pl.items()}
    return dict(kind=kind, style=style, dt=dt, B=B, hw=hw, proj=proj, T=HEAD_T, scale=scale, branches=branches, calls=calls,
                P=P, buf0=buf0, bufs=Bl, tap_x=tap_x, tap_g=tap_g, g_pre_relu={k: False for k in branches}, f32=f32, ft=ft,
                zs=zs, dz=dz, dfeat=dfeat, grads=grads, loss=loss, meta_x=meta_x)
