"""Every block family against fp64 at odd, non-square and tiny image sizes (GPU).

The whole-encoder tests elsewhere feed square images of side 64, 96, 224 or 448: every input of a stride-2 operation is even
and H == W, so the engine's size bookkeeping (ceil against floor in Rec.Ho / Wo, the unequal parity classes of
ops.dgrad_descs, the compact stride-2 addend grid, compact_dgrad_desc, subsample_colsum, maxpool_bn_bwd's clipped windows,
the total // V and per_view offsets of the partial rows) and any swapped (h, w) are invisible to them.  Here:

  A = 73 x 37    maps 37x19, 19x10, 10x5, 5x3, 3x2: an odd side into every stride-2 operation
  B = 33 x 301   maps 17x151, 9x76, 5x38, 3x19, 2x10: a stem output row wider than one stem tile
  C = 17 x 9     maps 9x5, 5x3, 3x2, 2x1, 1x1

  * train mode, teacher forcing (tests/parity_harness.py): ResNet-50, ResNet-18 and ResNeXt-50 in every mode, unpaired and
    paired (2 x 128 at A: pair_ok holds, so view tiles and the fused stride-2 join run on odd maps), and ResNeXt-50's first
    teacher-forced check at 224 x 224.  Per unit the output, the running statistics, every parameter gradient and the input
    gradient, each with limit = max(BOUNDS[mode], 3 x the mode restatement's own value on that unit);
  * eval mode, whole encoder: features and x.grad (which must have the image's shape) against an fp64 restatement; and the
    features of the same encoders under no_grad, where every dense unit is one sm3_conv_bn_eval launch (counted);
  * the whole SM3 model in f32 at A: logits and loss of the compat forward and of one fused trainer step against the oracle.
"""
import math

import numpy as np
import pytest
import torch

import parity_harness as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- train mode: every unit by teacher forcing ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.TRAIN_CASES, ids=[H.case_id(c) for c in H.TRAIN_CASES])
def test_every_unit_against_fp64_at_this_geometry_by_teacher_forcing(case):
    from sm3hip.engine import SM3Engine
    arch, mode, N, V, geo = case
    h, w = H.GEOMETRIES[geo]
    if V > 1:
        assert SM3Engine.pair_ok(N // V, h, w)
    run = H.engine_run(arch, H.DTYPE[mode], N, V, h, w, DEV)
    assert run["views_ran"] == V  # the paired cases really ran as one batch of two views
    taps, units = run["taps"], run["units"]
    # form facts: the gradient entering a stride-2 stage entry comes out of the fused launch (compact downsample addend,
    # previous block's BatchNorm-backward phase 1 in the epilogue) exactly where the block's form says so ...
    entries = [i for i, u in enumerate(units) if u["stride"] == 2]
    assert len(entries) == 3
    fused = [run["forms"][i].sparse_join for i in entries]
    assert [taps["g_pre_relu"][i] for i in entries] == fused, (fused, taps["g_pre_relu"])
    # ... and it does at every one of them: each launch set covers the odd maps, and with two views every parity class
    # splits into whole tiles per view
    assert fused == [True, True, True], fused
    rep, rest, fails = H.check_run(run, H.case_id(case))
    H.report(H.case_id(case), rep)
    we, wr = H.worst(rep), H.worst(rest)
    print(f"{H.case_id(case)}: worst over units, engine / restatement: "
          + ", ".join(f"{m} {we[m]:.3g} / {wr[m]:.3g}" for m in H.METRICS if m in we))
    assert not fails, fails[:8]


# ---- eval mode: the whole encoder ----------------------------------------------------------------------------------------
def _frozen_encoder(arch):
    from src.models import resnet
    torch.manual_seed(5)
    m = getattr(resnet, arch)(weights=None)
    m.fc = torch.nn.Identity()
    with torch.no_grad():  # non-trivial frozen statistics
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.1, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
    return m.to(DEV).eval()


def _ref_features_and_xgrad(m, x, dt=None, kinks=None):
    xd = x.double().requires_grad_()
    f = H.restated_features(m, xd, dt, kinks)
    (f ** 2).sum().backward()
    return f.detach(), xd.grad


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("geo", ["A", "B"])
@pytest.mark.parametrize("arch", ["resnet50", "resnet18", "resnext50_32x4d"])
def test_eval_mode_features_and_input_gradient_against_fp64(arch, geo, mode):
    h, w = H.GEOMETRIES[geo]
    m = _frozen_encoder(arch)
    x = H.images(3, h, w, "eval").to(DEV)
    kinks = H.Kinks() if mode == "f32" else None
    f_ref, g_ref = _ref_features_and_xgrad(m, x, kinks=kinks)
    if mode == "f32":
        lim_f = lim_g = 2e-3  # the bound test_other_block_families_input_gradient_against_fp64 holds
    else:  # 3 x the 16-bit restatement's own error on the same input
        f_q, g_q = _ref_features_and_xgrad(m, x, torch.bfloat16)
        lim_f, lim_g = H.MARGIN * H.rel(f_q, f_ref), H.MARGIN * H.rel(g_q, g_ref)
    m.sm3_dtype = H.DTYPE[mode]
    xg = x.clone().requires_grad_()
    f = m(xg)
    (f.double() ** 2).sum().backward()
    torch.cuda.synchronize()
    assert xg.grad is not None and xg.grad.shape == (3, 3, h, w) and xg.grad.dtype == torch.float32
    assert f.shape == f_ref.shape
    if kinks is not None and kinks.found:
        # ReLU inputs / max-pool ties below float32 resolution: the fp64 gradient on the nearest of the branches float32
        # cannot tell apart (same network, same input, same bound; H.Kinks)
        g_ref, took = H.nearest_branch(lambda fl: _ref_features_and_xgrad(m, x, kinks=H.Kinks(fl))[1], kinks.found,
                                       xg.grad.double(), g_ref)
        print(f"\n{arch} {geo}: {len(kinks.found)} decisions below float32 resolution, {len(took)} taken the other way: {took}")
    ef, eg = H.rel(f.detach().double(), f_ref), H.rel(xg.grad.double(), g_ref)
    print(f"\n{arch} {geo} {mode} eval: features {ef:.3e} (limit {lim_f:.3e}), x.grad {eg:.3e} (limit {lim_g:.3e})")
    H.measure_line({"case": f"eval-{arch}-{mode}-{geo}", "engine": {"feat_rel": ef, "xgrad_rel": eg},
                    "limit": {"feat_rel": lim_f, "xgrad_rel": lim_g}})
    assert ef <= lim_f and eg <= lim_g, (ef, lim_f, eg, lim_g)


# what every tool runs: the same encoders under no_grad, where conv_bn takes the one-launch form (sm3_conv_bn_eval); C for
# resnet18 alone, in f32: a final map of 1 x 1, M = N rows, the smallest launch an encoder hands to that kernel
NOGRAD_CASES = [(arch, geo, mode) for arch in ("resnet50", "resnet18", "resnext50_32x4d") for geo in ("A", "B")
                for mode in ("f32", "bf16", "f16")] + [("resnet18", "C", "f32")]


def _count_calls(monkeypatch, names):
    """{name: calls of sm3hip.ops.<name> from now on}, through wrappers that pass every call on."""
    from sm3hip import ops
    counts = {n: 0 for n in names}

    def wrap(n, real):
        def counted(*a, **k):
            counts[n] += 1
            return real(*a, **k)
        return counted
    for n in names:
        monkeypatch.setattr(ops, n, wrap(n, getattr(ops, n)))
    return counts


@pytest.mark.parametrize("arch,geo,mode", NOGRAD_CASES, ids=["-".join(c) for c in NOGRAD_CASES])
def test_eval_mode_features_without_autograd_against_fp64(arch, geo, mode, monkeypatch):
    """The frozen encoder under torch.no_grad(): every non-grouped unit is ONE launch (convolution, running-statistics
    BatchNorm, residual, ReLU; scale / shift derived in the epilogue), where the test above -- an image that requires a
    gradient -- runs the two-pass form.  Features against the fp64 restatement; f32: 2e-3, the bound of the test above; 16-bit:
    3 x the 16-bit restatement's own error on the same input (it rounds the pre-BatchNorm tensor, which this form never
    stores).  In f32 the distance to the two-pass form's features is recorded as well."""
    h, w = H.GEOMETRIES[geo]
    dt = H.DTYPE[mode]
    m = _frozen_encoder(arch)
    x = H.images(3, h, w, "eval").to(DEV)
    with torch.no_grad():
        f_ref = H.restated_features(m, x.double())
        lim = 2e-3 if mode == "f32" else H.MARGIN * H.rel(H.restated_features(m, x.double(), dt), f_ref)
    m.sm3_dtype = dt
    counts = _count_calls(monkeypatch, ("conv_bn_eval", "bn_eval_scale_shift"))
    with torch.no_grad():
        f = m(x)
    torch.cuda.synchronize()
    ran = dict(counts)
    # the one-launch branch ran for every dense unit but the stem (whose BatchNorm is applied inside the pooling pass); the
    # stem and a ResNeXt's grouped 3x3 units computed their scale / shift first: counted on the plan's own unit list
    units = list(m.__dict__["_sm3_engine"].branches["main"][0].conv_units())
    two_pass = [u for u in units if u.stem or u.groups > 1]
    assert len(two_pass) == 1 + (sum(u.k == 3 for u in units) if arch.startswith("resnext") else 0), len(two_pass)
    assert ran == {"conv_bn_eval": len(units) - len(two_pass), "bn_eval_scale_shift": len(two_pass)}, (ran, len(units))
    assert ran["conv_bn_eval"] > 0 and not f.requires_grad and f.dtype == torch.float32 and f.shape == f_ref.shape
    ef = H.rel(f.double(), f_ref)
    rec = {"case": f"eval-nograd-{arch}-{mode}-{geo}", "engine": {"feat_rel": ef}, "limit": {"feat_rel": lim},
           "launches": ran}
    line = f"\n{arch} {geo} {mode} eval, no_grad: features {ef:.3e} (limit {lim:.3e}), launches {ran}"
    if mode == "f32":  # how far the one-launch and the two-pass form are apart (recorded, not bounded beyond the limit above)
        f2 = m(x.clone().requires_grad_())
        torch.cuda.synchronize()
        assert counts["conv_bn_eval"] == ran["conv_bn_eval"], "the autograd forward took the one-launch form"
        e2, ef2 = H.rel(f.double(), f2.detach().double()), H.rel(f2.detach().double(), f_ref)
        rec["engine"].update(two_pass_rel=e2, two_pass_feat_rel=ef2)
        line += f"; against the two-pass form {e2:.3e} (two-pass against fp64 {ef2:.3e})"
    print(line)
    H.measure_line(rec)
    assert ef <= lim, (ef, lim)


# ---- the whole model -----------------------------------------------------------------------------------------------------
def test_sm3_model_and_fused_trainer_at_a_nonsquare_odd_size_against_the_oracle():
    """SimCLRSkinV32("resnet50"), exact-f32 mode, 4 pairs at 73 x 37, style 0: model(derm, clinic, 0) and one SM3Trainer.step
    against oracle.sm3_oracle in fp64.  Limits: the tolerances tests/test_e2e_gpu.py holds (logits 2e-3, loss 1e-3) or
    3 x the oracle's own float32-against-float64 difference on this batch, whichever is larger."""
    from oracle import procedural, sm3_oracle as O
    from sm3hip.trainer import SM3Trainer
    from src.models.simclr import SimCLRSkinV32
    B, seed, style = 4, 7, 0
    h, w = H.GEOMETRIES["A"]
    state = procedural.make_state_dict(seed=seed)
    derm_np, clinic_np = procedural.make_pair_batch(B, max(h, w), seed)
    derm_np = [np.ascontiguousarray(a[..., :h, :w]) for a in derm_np]
    clinic_np = [np.ascontiguousarray(a[..., :h, :w]) for a in clinic_np]
    ref = {}
    for dt in (torch.float64, torch.float32):
        P, Bf = O.split_state(state, dt, requires_grad=False)
        with torch.no_grad():
            outs = O.sm3_v32_forward(P, Bf, [torch.from_numpy(a).to(dt) for a in derm_np],
                                     [torch.from_numpy(a).to(dt) for a in clinic_np], style, 0.1, training=True)
            logits = [outs[0][0], outs[1][0]] + [o[0] for o in outs[2]]
            ref[dt] = ([t.double() for t in logits], float(O.sm3_loss(outs, style)))
    own = max(float((a - b).abs().max()) for a, b in zip(ref[torch.float32][0], ref[torch.float64][0]))
    lim_logits = max(2e-3, H.MARGIN * own)
    lim_loss = max(1e-3, H.MARGIN * abs(ref[torch.float32][1] - ref[torch.float64][1]))
    want_logits, want_loss = ref[torch.float64]

    def build():
        model = SimCLRSkinV32("resnet50", None, 128, 0.1)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
        model.sm3_dtype = torch.float32
        return model.to(DEV).train()

    derm = [torch.from_numpy(a).to(DEV) for a in derm_np]
    clinic = [torch.from_numpy(a).to(DEV) for a in clinic_np]
    outputs = build()(derm, clinic, style)
    crit = torch.nn.CrossEntropyLoss()
    loss = float((crit(*outputs[0]) + crit(*outputs[1]) + sum(0.5 * crit(*o) for o in outputs[2])).detach())
    got = [outputs[0][0].detach(), outputs[1][0].detach()] + [o[0].detach() for o in outputs[2]]
    errs = [float((g.double().cpu() - r).abs().max()) for g, r in zip(got, want_logits)]
    tr = SM3Trainer(build(), lr=1e-3, weight_decay=5e-2, eps=1e-5, style=style)
    tloss = float(tr.step(derm, clinic))
    torch.cuda.synchronize()
    print(f"\nSM3 f32 4 pairs 73x37: logits max err {max(errs):.3e} (limit {lim_logits:.3e}, oracle f32-f64 {own:.3e}), "
          f"loss {loss:.6f} / trainer {tloss:.6f} / fp64 {want_loss:.6f} (limit {lim_loss:.3e})")
    H.measure_line({"case": "sm3-f32-4pairs-A", "engine": {"logits_max": max(errs), "loss": abs(loss - want_loss),
                                                           "trainer_loss": abs(tloss - want_loss)},
                    "limit": {"logits_max": lim_logits, "loss": lim_loss}})
    assert all(g.shape == r.shape for g, r in zip(got, want_logits))
    assert math.isfinite(loss) and math.isfinite(tloss)
    assert max(errs) <= lim_logits, errs
    assert abs(loss - want_loss) <= lim_loss and abs(tloss - want_loss) <= lim_loss, (loss, tloss, want_loss)
    assert abs(tloss - loss) < 1e-3, (tloss, loss)  # the tolerance of test_fused_trainer_matches_golden_and_compat
