"""Test helper of test_trainer_schedule_gpu.py: models and batches of its matrix, and checked_step(), which takes one
SM3Trainer step and replays it from its own before / after state.

The gradients of a step are a function of their inputs (SM3Engine.det_wgrad), sm3_adamw / sm3_ema_update are per-element
functions whose bits do not depend on the position or the length of a launch (test_optimizer_edges_gpu.py), and the
trainer keeps flat_g until the next step.  So whatever schedule applied the update -- one launch, one per bucket from
inside backward, one behind every all-reduce, the dynamic-loss-scale triple -- one sm3_adamw launch over the state before
the step with the retained gradient must give the state after it bit for bit, padding between the parameters included.
The fp64 bounds are those of edge_inputs.py, unchanged; every trainer is built with its hyper-parameters (make_trainer)."""
import copy

import torch

import edge_inputs as E
from test_config_gpu import DEV, _batch, _build

WD = 0.05
EMA_RTOL = 1e-5  # the rtol of _canonical("ema") in test_optimizer_edges_gpu.py
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# id -> model class, encoder, style, pairs per step, image size, arithmetic, metadata_dim, target momentum
ROWS = {
    "rn50-b4-f32": ("v32", "resnet50", 0, 4, (64, 64), F32, None, None),
    "rn50-b4-bf16": ("v32", "resnet50", 0, 4, (64, 64), BF16, None, None),
    "rn50-b32-bf16": ("v32", "resnet50", 0, 32, (64, 64), BF16, None, None),
    "rn18-style1-bf16": ("v32", "resnet18", 1, 4, (64, 64), BF16, None, None),
    "rn18-style2-33x47-bf16": ("v32", "resnet18", 2, 4, (33, 47), BF16, None, None),
    "v3-rn18-bf16": ("v3", "resnet18", 0, 4, (64, 64), BF16, None, None),
    "rn18-meta-f32": ("v32", "resnet18", 0, 4, (64, 64), F32, 20, None),
    "rx50-bf16": ("v32", "resnext50_32x4d", 0, 4, (64, 64), BF16, None, None),
    "rn18-target-bf16": ("v32", "resnet18", 0, 4, (64, 64), BF16, None, 0.9),
}
SEED = 17


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


_template = {}


def fresh_model(cls, arch, dtype, metadata_dim=None, seed=SEED):
    """A new model on the GPU with procedural weights (oracle/procedural.py); the last template is kept, so the variants
    of one row do not pay for the initialisation again."""
    from oracle import procedural
    from src.models.simclr import SimCLRSkinV3, SimCLRSkinV32
    key = (cls, arch, metadata_dim, seed)
    if key not in _template:
        _template.clear()
        if cls == "v32" and arch == "resnet50" and metadata_dim is None:
            tpl = _build(seed, dtype)
        else:
            tpl = (SimCLRSkinV3(arch, None, 128, 0.1) if cls == "v3" else
                   SimCLRSkinV32(arch, None, 128, 0.1, metadata_dim=metadata_dim))
            spec = [(k, tuple(v.shape)) for k, v in tpl.state_dict().items()]
            state = procedural.make_state_dict(spec, seed=seed)
            tpl.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
            tpl.to(DEV)
        _template[key] = tpl
    model = copy.deepcopy(_template[key])  # the template never steps: it holds no engine and its parameters stay its own
    model.sm3_dtype = dtype
    return model


def row_model(row):
    cls, arch, _style, _B, _hw, dtype, meta, _mom = ROWS[row]
    return fresh_model(cls, arch, dtype, meta)


def make_trainer(model, **kw):
    """Every trainer of the schedule tests: edge_inputs.ADAM and weight decay 0.05, so that one step moves bits and
    edge_inputs.adamw_ref_step applies as it stands."""
    from sm3hip.trainer import SM3Trainer
    return SM3Trainer(model, lr=E.ADAM["lr"], weight_decay=WD, eps=E.ADAM["eps"], betas=(E.ADAM["beta1"], E.ADAM["beta2"]),
                      **kw)


def row_trainer(row, model, **kw):
    _cls, _arch, style, _B, _hw, _dtype, _meta, mom = ROWS[row]
    return make_trainer(model, style=style, target_momentum=mom, **kw)


def make_batches(B, hw, steps, seed=60, metadata_dim=None):
    """`steps` different batches: (derm views, clinic views, metadata or None).  A non-square size is cut out of the
    procedural square images."""
    H, W = hw
    out = []
    for i in range(steps):
        derm, clinic = _batch(B, max(H, W), seed + i)
        if H != W:
            derm, clinic = ([t[:, :, :H, :W].contiguous() for t in v] for v in (derm, clinic))
        meta = None
        if metadata_dim is not None:
            meta = torch.randn(B, metadata_dim, generator=torch.Generator().manual_seed(seed + i)).to(DEV)
        out.append((derm, clinic, meta))
    return out


def row_batches(row, steps=4):
    _cls, _arch, _style, B, hw, _dtype, meta, _mom = ROWS[row]
    return make_batches(B, hw, steps, metadata_dim=meta)


def first_diff(store, a, b):
    """Where two flat buffers differ first: (parameter name or 'padding after <name>', index in it, count of differing
    elements) -- the name maps to a bucket, a stream and a step."""
    ne = (bits(a) != bits(b)).nonzero().flatten()
    if ne.numel() == 0:
        return None
    i = int(ne[0])
    name = max((n for n in store.names if store.offsets[n] <= i), key=lambda n: store.offsets[n])
    k = i - store.offsets[name]
    n = 1
    for s in store.shapes[name]:
        n *= s
    return (name if k < n else f"padding after {name}", k, int(ne.numel()))


def buffers_of(model):
    return {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


def check_banks(eng, p_before):
    """The filter banks the engine holds after a step are those of the masters the step's last forward read."""
    from sm3hip import ops
    st = eng.store
    n = 0
    for cu in eng._all_conv_units():
        wname = cu.name + ".weight"
        if wname not in st.offsets:
            continue
        master = st.flat2d(p_before, wname)
        if cu.groups > 1:
            wf, wd = torch.full_like(cu.w_fwd, 7.0), torch.full_like(cu.w_dgrad, 7.0)
            ops.gconv_weight_prep(eng.dtype, master, cu.Co, cu.groups, wf, wd)
            assert torch.equal(wf, cu.w_fwd), ("grouped forward bank", wname)
            assert torch.equal(wd, cu.w_dgrad), ("grouped data-gradient bank", wname)
        elif cu.stem:
            w = torch.full_like(cu.w_fwd, 7.0)
            ops.stem_weight_prep(eng.dtype, master, w)
            assert torch.equal(w, cu.w_fwd), ("stem bank", wname)
        else:
            assert torch.equal(cu.w_fwd, master.to(eng.tdt)), ("forward bank", wname)
            ref = master.view(cu.Co, cu.taps, cu.Ci).permute(2, 1, 0).contiguous().to(eng.tdt)  # wd[ci][t][co] = w[co][t][ci]
            assert torch.equal(cu.w_dgrad.reshape(-1), ref.reshape(-1)), ("data-gradient bank", wname)
        n += 1
    assert n > 0
    return n


def checked_step(tr, batch, tag=""):
    """One tr.step on batch = (derm views, clinic views, metadata or None), replayed from its before / after state:
    bits (one sm3_adamw launch), fp64 (edge_inputs.adamw_ref_step / adamw_ratios), the momentum target (one sm3_ema_update
    launch and the fp64 expression) and the filter banks.  -> dict of clones: loss (bits), p, m, v, g, target, buffers."""
    from sm3hip import ops
    derm, clinic, meta = batch
    eng = tr._engine()
    eng.prepare(torch.device(DEV))
    st = eng.store
    p0 = st.flat_p.clone()
    m0 = tr.m.clone() if tr.m is not None else torch.zeros_like(p0)
    v0 = tr.v.clone() if tr.v is not None else torch.zeros_like(p0)
    t0 = None
    if tr.target_momentum is not None:  # before the first step the target is the online network
        t0 = tr.flat_target.clone() if tr.flat_target is not None else p0.clone()
    dyn = tr.loss_scale if tr.loss_scale is not None else eng.tdt == torch.float16
    scale0 = (float(tr._scaler["scale"]) if tr._scaler is not None else tr.scaler_cfg[0]) if dyn else 1.0
    taken0 = tr.steps_taken()

    loss = tr.step(derm, clinic) if meta is None else tr.step(derm, clinic, metadata=meta)
    torch.cuda.synchronize()

    t = tr.steps_taken()
    assert t == taken0 + 1, (tag, taken0, t)
    gs = 1.0 / tr.world / scale0  # fp16: exact, the scale is a power of two
    g = st.flat_g
    assert bool(torch.isfinite(g).all()), tag
    # ---- bits: the schedule, whichever it was, amounts to one launch over the flat buffer -------------------------------
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    ops.adamw(p1, g, m1, v1, tr.lr, tr.betas[0], tr.betas[1], tr.eps, tr.wd, t, gs)
    torch.cuda.synchronize()
    for name, got, want in (("p", st.flat_p, p1), ("exp_avg", tr.m, m1), ("exp_avg_sq", tr.v, v1)):
        assert same_bits(got, want), (tag, name, "step", t, first_diff(st, got, want))
    del p1, m1, v1
    # ---- fp64 -----------------------------------------------------------------------------------------------------------
    pr, mr, vr = p0.double(), m0.double(), v0.double()
    g64 = g.double()
    E.adamw_ref_step(pr, g64, mr, vr, t, tr.wd, gs)
    gsum = m0.double().abs() + (g64 * gs).abs()
    rp, rm, rv = E.adamw_ratios(f"trainer step {t} {tag}", st.flat_p, tr.m, tr.v, pr, mr, vr, gsum)
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (tag, t, rp, rm, rv)
    del pr, mr, vr, g64, gsum
    # ---- the momentum target ---------------------------------------------------------------------------------------------
    if t0 is not None:
        mom = tr.target_momentum
        t1 = t0.clone()
        if not dyn:
            ops.ema_update(t1, st.flat_p, mom)
        else:
            # under a loss scale the trainer gates the factor on the device by the step's overflow flag and applies it with
            # torch (no sm3_ema_update launch): the same expression with the flag clear gives the same bits
            w = (1.0 - mom) * torch.ones(1, dtype=torch.float32, device=t1.device)
            t1.add_((st.flat_p - t1) * w)
        torch.cuda.synchronize()
        assert same_bits(tr.flat_target, t1), (tag, "target", first_diff(st, tr.flat_target, t1))
        # rtol of the fp64 value, as _canonical("ema") has it, wherever the two terms do not cancel (|a + b| at least half
        # of |a| + |b|); where m t and (1 - m) p cancel (a small parameter that one update carried through zero) the
        # roundings of the terms are all that is left of the sum, and rtol is taken of the terms' magnitude, as gsum above
        a, b = E.f32(mom) * t0.double(), (1.0 - E.f32(mom)) * st.flat_p.double()
        mag = a.abs() + b.abs()
        limit = EMA_RTOL * torch.where((a + b).abs() >= 0.5 * mag, (a + b).abs(), mag) + 1e-30
        ratio = float(((tr.flat_target.double() - (a + b)).abs() / limit).max())
        assert E.record(f"ema target {tag}", ratio, 1.0) <= 1.0, (tag, "target against fp64", ratio)
        assert not same_bits(tr.flat_target, t0), (tag, "the target did not move")
    # ---- banks -----------------------------------------------------------------------------------------------------------
    check_banks(eng, p0)
    return {"loss": bits(loss.detach()).clone(), "p": st.flat_p.clone(), "m": tr.m.clone(), "v": tr.v.clone(),
            "g": g.clone(), "target": tr.flat_target.clone() if t0 is not None else None, "buffers": buffers_of(tr.model)}


def assert_same_step(a, b, store, tag):
    """Two records of checked_step are equal bit for bit."""
    assert torch.equal(a["loss"], b["loss"]), (tag, "loss", a["loss"].view(torch.float32).item(),
                                               b["loss"].view(torch.float32).item())
    for k in ("g", "p", "m", "v", "target"):
        if a[k] is None:
            assert b[k] is None, (tag, k)
            continue
        assert same_bits(a[k], b[k]), (tag, k, first_diff(store, a[k], b[k]))
    assert a["buffers"].keys() == b["buffers"].keys()
    for k, x in a["buffers"].items():
        assert same_bits(x, b["buffers"][k]), (tag, k)
