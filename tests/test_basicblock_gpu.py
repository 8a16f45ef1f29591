"""ResNet-18 / ResNet-34 (BasicBlock encoders) on the HIP engine (GPU).

  * the kernel case BasicBlock networks add: the data gradient of a 3x3 / stride-2 conv1 (four parity-class launches) with
    the downsample's compact data gradient as the addend of the (0, 0) class and the previous block's BatchNorm-backward
    phase 1 in the epilogue -- against fp64, and bit for bit against the same launches with the addend scattered dense;
  * SimCLRSkinV32("resnet18") / ("resnet34") and Baseline("resnet18") against fp64 goldens of the reference itself
    (tests/golden/gen_resnet18_golden.py), with the tolerances tests/test_e2e_gpu.py holds ResNet-50 to;
  * every unit of a bf16 ResNet-18 training pass (two views as one batch, 224 x 224) against fp64 by teacher forcing,
    with the per-tensor bounds of tests/test_block_parity_gpu.py;
  * determinism and a checkpoint round trip of the fused trainer.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT_IDS = ["bf16", "f16", "f32"]


def _ops():
    from sm3hip import ops
    return ops


# ---- kernel: compact addend on the (0, 0) parity class of a stride-2 data gradient ----------------------------------
STAGE_ENTRIES = {  # forward conv1 Ci -> Co, 3x3 / stride 2, at the input size of a 224 x 224 network; images per view
    "layer2": (64, 128, 56, 8),
    "layer3": (128, 256, 28, 32),
    "layer4": (256, 512, 14, 128),
}


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("views", [1, 2])
@pytest.mark.parametrize("stage", list(STAGE_ENTRIES))
def test_stride2_dgrad_with_compact_addend_and_fused_bn_phase1(stage, views, dt):
    ops = _ops()
    Ci, Co, H, Nv = STAGE_ENTRIES[stage]
    N, W, V = Nv * views, H, views
    code = ops.dtype_code(dt)
    E = 4 if dt == torch.float32 else 8
    D = torch.device(DEV)
    g = torch.Generator().manual_seed(Ci + views)
    Hs, Ws = H // 2, W // 2
    rows = N * H * W
    dy = torch.randn(N, Hs, Ws, Co, generator=g).to(dt).to(D)
    w_dg = (torch.randn(Ci, 9, Co, generator=g) / math.sqrt(9 * Co)).to(dt).to(D)
    sp = torch.randn(N, Hs, Ws, Ci, generator=g).to(dt).to(D)        # the downsample's compact data gradient
    dense = torch.zeros(N, H, W, Ci, dtype=dt, device=D)
    dense[:, ::2, ::2] = sp
    bn_x = torch.randn(rows, Ci, generator=g).to(dt).to(D)            # the previous join's pre-BatchNorm tensor
    mean = (0.1 * torch.randn(V, Ci, generator=g)).to(D)
    invstd = (torch.rand(V, Ci, generator=g) + 0.5).to(D)
    descs, full = ops.dgrad_descs(code, N, H, W, Ci, Co, 3, 2, 1)
    assert full and len(descs) == 4
    assert [(d.osy, d.ooy, d.oox) for d in descs][0] == (2, 0, 0) and (descs[0].Ho, descs[0].Wo) == (Hs, Ws)
    total = sum(ops.conv_partial_rows(d) for d in descs)
    per_view = total // V

    def fused(mask, compact):
        out = torch.full((rows, Ci), float("nan"), dtype=dt, device=D)
        part = torch.full((total, 2, Ci), float("nan"), device=D)
        off = 0
        for d in descs:
            if compact:
                add, spk = (sp, (Hs, Ws)) if (d.ooy, d.oox) == (0, 0) else (None, None)
            else:
                add, spk = dense, None
            n = ops.conv_dgrad_bnfuse(d, dy, w_dg, out, add, mask, bn_x, mean, invstd, part, off, views=V,
                                      row_offset_view1=per_view + off, addend_sparse=spk)
            off += n // V
        assert off == per_view
        return out, part

    ones = torch.full((rows * Ci // E,), 0xFF if E == 8 else 0x0F, dtype=torch.uint8, device=D)
    rnd = torch.randint(0, 256, (rows * Ci // E,), generator=g, dtype=torch.uint8).to(D)
    if E == 4:
        rnd &= 0x0F
    for mask in (ones, rnd):
        out_c, part_c = fused(mask, True)
        out_d, part_d = fused(mask, False)
        torch.cuda.synchronize()
        # the same arithmetic (fp32 accumulator + the same rounded addend, same epilogue): the same bits
        assert torch.equal(out_c, out_d)
        assert torch.equal(part_c, part_d)
    # ... and the unfused two-launch form: the plain data gradient with the dense addend, then the phase-1 kernel
    ref = torch.empty(rows, Ci, dtype=dt, device=D)
    for d in descs:
        ops.conv_gemm(d, dy, w_dg, ref, dense, None)
    prow = ops.bn_bwd_partial_rows(rows // V, Ci)
    part_ref = torch.zeros(V * prow, 2, Ci, device=D)
    ops.bn_bwd_reduce(code, ref, None, bn_x, mean, invstd, ref, rows // V, Ci, part_ref, mask=rnd, views=V)
    torch.cuda.synchronize()
    assert torch.equal(out_c, ref)
    for v in range(V):
        a = part_c[v * per_view:(v + 1) * per_view].double().sum(0)
        b = part_ref[v * prow:(v + 1) * prow].double().sum(0)
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))
    # fp64 torch: conv2d autograd for the data gradient, plus the addend; BatchNorm-backward sums with the all-ones mask
    out1, part1 = fused(ones, True)
    torch.cuda.synchronize()
    w64 = w_dg.double().view(Ci, 3, 3, Co).permute(3, 0, 1, 2).contiguous()  # OIHW of the forward conv
    x64 = torch.zeros(N, Ci, H, W, dtype=torch.float64, device=D, requires_grad=True)
    F.conv2d(x64, w64, stride=2, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    dz = x64.grad.permute(0, 2, 3, 1).reshape(rows, Ci) + dense.double().reshape(rows, Ci)
    got = out1.double()
    tol = {torch.bfloat16: 2 ** -7, torch.float16: 2 ** -10, torch.float32: 1e-5}[dt]
    assert float((got - dz).abs().max()) <= tol * float(dz.abs().max()) * 2
    for v in range(V):
        sl = slice(v * rows // V, (v + 1) * rows // V)
        xh = (bn_x[sl].double() - mean[v].double()) * invstd[v].double()
        want = torch.stack([dz[sl].sum(0), (dz[sl] * xh).sum(0)])
        have = part1[v * per_view:(v + 1) * per_view].double().sum(0)
        # each dz element carries one rounding to the mode's dtype (fp32 accumulation in f32 mode)
        bound = torch.stack([dz[sl].abs().sum(0), (dz[sl] * xh).abs().sum(0)]) * (1e-5 if dt == torch.float32 else tol)
        assert bool(((have - want).abs() <= bound + 1e-9).all()), float(((have - want).abs() - bound).max())
    # the other three classes take no compact addend; a wrong grid is refused
    with pytest.raises(ValueError):
        ops.conv_dgrad_bnfuse(descs[1], dy, w_dg, out1, sp, rnd, bn_x, mean, invstd, part1, 0, views=V,
                              row_offset_view1=per_view, addend_sparse=(Hs, Ws))
    with pytest.raises(ValueError):
        ops.conv_dgrad_bnfuse(descs[0], dy, w_dg, out1, sp, rnd, bn_x, mean, invstd, part1, 0, views=V,
                              row_offset_view1=per_view, addend_sparse=((Hs + 1) // 2, (Ws + 1) // 2))


# ---- models against the reference's fp64 goldens ---------------------------------------------------------------------
def _procedural(model, seed):
    from oracle import procedural
    return {k: torch.from_numpy(np.asarray(procedural.fill_tensor(k, tuple(v.shape), seed)))
            for k, v in model.state_dict().items()}


def _sm3(arch, seed, dtype):
    from src.models.simclr import SimCLRSkinV32
    model = SimCLRSkinV32(arch, None, 128, 0.1)
    model.load_state_dict(_procedural(model, seed), strict=True)
    model.sm3_dtype = dtype
    return model.to(DEV)


def _pairs(batch, size, seed):
    from oracle import procedural
    derm_np, clinic_np = procedural.make_pair_batch(batch, size, seed)
    return [torch.from_numpy(a).to(DEV) for a in derm_np], [torch.from_numpy(a).to(DEV) for a in clinic_np]


def _golden(tag):
    return np.load(os.path.join(GOLDEN, f"sm3_v32_{tag}_b4_s64_f64.npz"))


def _compat_step(g, arch):
    batch, size, seed, style = [int(v) for v in g["meta"]]
    model = _sm3(arch, seed, torch.float32).train()
    derm, clinic = _pairs(batch, size, seed)
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.AdamW(model.parameters(), lr=float(g["lr"]), weight_decay=5e-2, eps=1e-5)
    outputs = model(derm, clinic, style)
    loss = crit(*outputs[0]) + crit(*outputs[1]) + sum(0.5 * crit(*o) for o in outputs[2])
    opt.zero_grad(set_to_none=True)
    loss.backward()
    gn = np.array([p.grad.double().norm().item() for _, p in model.named_parameters()])
    opt.step()
    torch.cuda.synchronize()
    return model, outputs, float(loss.detach()), gn


@pytest.mark.parametrize("arch,tag", [("resnet18", "r18"), ("resnet34", "r34")])
def test_compat_step_matches_the_reference_golden(arch, tag):
    """model(derm, clinic, 0) -> CrossEntropyLoss -> backward -> torch AdamW, exact-f32 mode, B = 4 pairs at 64 x 64."""
    g = _golden(tag)
    model, outputs, loss, gn = _compat_step(g, arch)
    assert math.isfinite(loss)
    np.testing.assert_allclose(outputs[0][0].detach().double().cpu().numpy(), g["derm_logits"], atol=2e-3, rtol=0)
    np.testing.assert_allclose(outputs[1][0].detach().double().cpu().numpy(), g["clinic_logits"], atol=2e-3, rtol=0)
    for i, o in enumerate(outputs[2]):
        np.testing.assert_allclose(o[0].detach().double().cpu().numpy(), g[f"cross_logits_{i}"], atol=2e-3, rtol=0)
    assert abs(loss - float(g["loss"])) < 1e-3, (loss, float(g["loss"]))
    np.testing.assert_allclose(gn, g["grad_norm"], rtol=5e-2, atol=1e-7)
    sd = model.state_dict()
    names = [k for k, _ in model.named_parameters()]
    pn = np.array([sd[k].double().norm().item() for k in names])
    np.testing.assert_allclose(pn, g["post_param_norm"], rtol=5e-3)


def test_fused_trainer_resnet18_matches_the_reference_golden():
    from sm3hip.trainer import SM3Trainer
    g = _golden("r18")
    batch, size, seed, style = [int(v) for v in g["meta"]]
    model = _sm3("resnet18", seed, torch.float32)
    derm, clinic = _pairs(batch, size, seed)
    tr = SM3Trainer(model, lr=float(g["lr"]), weight_decay=5e-2, eps=1e-5, style=style)
    loss = float(tr.step(derm, clinic))
    torch.cuda.synchronize()
    assert abs(loss - float(g["loss"])) < 1e-3, (loss, float(g["loss"]))
    names = [k for k, _ in model.named_parameters()]
    gv = dict(zip(tr._engine().store.names, tr._engine().store.grad_views()))
    gn = np.array([gv[k].double().norm().item() for k in names])
    np.testing.assert_allclose(gn, g["grad_norm"], rtol=5e-2, atol=1e-7)
    sd = model.state_dict()
    pn = np.array([sd[k].double().norm().item() for k in names])
    np.testing.assert_allclose(pn, g["post_param_norm"], rtol=5e-3)


def test_baseline_resnet18_linear_probe_matches_the_reference_golden():
    """--finetune fc: eval-mode encoders (one conv + BatchNorm (+residual) (+ReLU) kernel per unit), 2 x 512 features."""
    from src.models.baseline import Baseline
    g = np.load(os.path.join(GOLDEN, "baseline_r18_b4_s64_f64.npz"))
    batch, size, seed = [int(v) for v in g["meta"]]
    model = Baseline("resnet18", None)
    model.load_state_dict(_procedural(model, seed), strict=True)
    for bb in (model.derm_backbone, model.clinic_backbone):  # each encoder has its own engine
        bb.sm3_dtype = torch.float32
    model.to(DEV).eval()
    model.freeze_backbone()
    assert model.classifier[0].in_features == 1024
    derm, clinic = _pairs(batch, size, seed)
    labels = torch.from_numpy(g["labels"]).to(DEV)
    outputs = model([derm[0], clinic[0]])
    crit = torch.nn.CrossEntropyLoss()
    loss = sum(crit(o, labels[:, i]) for i, o in enumerate(outputs)) / 8
    loss.backward()
    torch.cuda.synchronize()
    # the bounds tests/test_linear_probe.py holds Baseline("resnet50") to
    scale = max(float(np.abs(g[f"logits_{i}"]).max()) for i in range(8))
    for i, o in enumerate(outputs):
        np.testing.assert_allclose(o.detach().double().cpu().numpy(), g[f"logits_{i}"], atol=2e-4 * scale, rtol=0)
        for key, got in ((f"grad_w_{i}", model.classifier[i].weight.grad), (f"grad_b_{i}", model.classifier[i].bias.grad)):
            want = g[key]
            np.testing.assert_allclose(got.double().cpu().numpy(), want, atol=2e-4 * float(np.abs(want).max()) + 1e-9, rtol=0)
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4 * float(g["loss"])
    assert int(model.derm_backbone.bn1.num_batches_tracked) == 0  # eval mode: running statistics untouched


# ---- determinism and checkpoints -------------------------------------------------------------------------------------
def _three_steps(batches):
    from sm3hip.trainer import SM3Trainer
    model = _sm3("resnet18", 11, torch.bfloat16)
    tr = SM3Trainer(model, lr=1e-3, weight_decay=5e-2, eps=1e-5, style=0)
    losses = [float(tr.step(*b)) for b in batches]
    torch.cuda.synchronize()
    return losses, tr._engine().store.flat_p.clone(), tr.m.clone()


def test_three_bf16_resnet18_steps_repeat_bit_for_bit():
    """Two runs of three bf16 training steps (B = 128 pairs at 224 x 224: both views as one batch, fused stage entries)
    give the same losses and parameters, bit for bit."""
    batches = [_pairs(128, 224, 40 + i) for i in range(3)]
    a = _three_steps(batches)
    b = _three_steps(batches)
    assert all(math.isfinite(x) for x in a[0])
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_resnet18_checkpoint_round_trip_in_the_reference_wire_format(tmp_path):
    from sm3hip.trainer import SM3Trainer
    from src.models.simclr import SimCLRSkinV32
    batches = [_pairs(8, 64, 60 + i) for i in range(2)]
    model = _sm3("resnet18", 13, torch.float32)
    tr = SM3Trainer(model, lr=1e-4, weight_decay=5e-2, eps=1e-5, style=0)
    tr.step(*batches[0])
    torch.cuda.synchronize()
    path = str(tmp_path / "checkpoint.pth.tar")
    torch.save({"epoch": 0, "state_dict": model.state_dict(), "optimizer": tr.optimizer_state_dict(), "scaler": {}}, path)
    loss2 = float(tr.step(*batches[1]))
    p2 = tr._engine().store.flat_p.clone()
    ck = torch.load(path, map_location="cpu", weights_only=False)
    keys = open(os.path.join(GOLDEN, "r18_state_dict_keys.txt")).read().split()
    assert list(ck["state_dict"].keys()) == keys
    fresh = SimCLRSkinV32("resnet18", None, 128, 0.1)
    fresh.sm3_dtype = torch.float32
    res = fresh.load_state_dict(ck["state_dict"], strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    fresh.to(DEV)
    tr2 = SM3Trainer(fresh, lr=1.0, weight_decay=0.0, eps=1.0, style=0)
    tr2.load_optimizer_state_dict(ck["optimizer"])
    assert (tr2.lr, tr2.wd, tr2.eps, tr2.step_count) == (1e-4, 5e-2, 1e-5, 1)
    loss2b = float(tr2.step(*batches[1]))
    torch.cuda.synchronize()
    assert abs(loss2 - loss2b) < 1e-5, (loss2, loss2b)
    assert float((tr2._engine().store.flat_p - p2).abs().max()) < 1e-6


# ---- every unit of a bf16 ResNet-18 training pass against fp64 --------------------------------------------------------
def test_every_unit_of_a_bf16_resnet18_pass_against_fp64():
    """Teacher forcing as in tests/test_block_parity_gpu.py (tests/parity_harness.py): the engine runs one train-mode forward
    + backward of a bare resnet18 with block-boundary taps (B = 128 per view, two views as one batch, 224 x 224); every unit
    is recomputed in fp64 from the engine's own input and upstream gradient and compared per tensor with that file's bf16
    bounds."""
    import parity_harness as H
    from test_block_parity_gpu import BOUNDS
    run = H.engine_run("resnet18", torch.bfloat16, 256, 2, 224, 224, DEV)
    plan, taps = run["plan"], run["taps"]
    assert plan.basic and plan.out_dim == 512 and run["views_ran"] == 2
    assert len(taps["x"]) == len(taps["g"]) == len(plan.blocks) + 1 == 9
    # the stage entries' data gradients came out of the fused (0, 0)-class launch: masked by the previous block's ReLU
    assert [taps["g_pre_relu"][i] for i in (2, 4, 6)] == [True, True, True]
    rep, _, fails = H.check_run(run, "resnet18-bf16-2x128-224", base=BOUNDS["bf16"], restate=False)
    print("\nresnet18 bf16 2x128 224: " + "; ".join(
        f"{s}: out rel {r['out_rel'][0]:.2e}, grad cos {r['g_cos'][0]:.6f} ({r['g_cos'][1]}), rel {r['g_rel'][0]:.2e}"
        for s, r in rep.items()))
    assert not fails, fails[:8]
