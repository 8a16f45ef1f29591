"""ResNeXt encoders (grouped 3x3 convolutions, csrc/gconv.hip) on the HIP engine (GPU).

  * the grouped kernels -- forward with its BatchNorm partial rows, data gradient (stride 1 and 2), weight gradient -- at every
    (width, groups, map, stride) of conv2 in resnext50_32x4d / resnext101_32x8d / resnext101_64x4d at 224 x 224, plus small
    maps, against fp64 torch.nn.functional.conv2d and its autograd;
  * the weight gradient is a function of its inputs: equal bit for bit across runs;
  * SimCLRSkinV32("resnext50_32x4d") compat and fused-trainer steps, and the pooled features of both 101 variants, against fp64
    goldens of the reference itself (tests/golden/gen_resnext_golden.py);
  * bit-reproducible bf16 trainer steps, a checkpoint round trip, and a short mlc_train run on a ResNeXt extractor.
"""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT_IDS = ["bf16", "f16", "f32"]
# relative-norm bounds of one grouped launch against fp64 on the same (rounded) inputs: f32 to about 1e-5; the 16-bit modes
# within the per-unit output bounds of tests/test_block_parity_gpu.py
REL = {torch.bfloat16: 1.5e-2, torch.float16: 3e-3, torch.float32: 1e-5}


def _conv2_shapes():
    """(C, groups, H, stride) of every conv2 of the three ResNeXt constructors at 224 x 224 (layer1..4 maps 56/28/14/7, the
    stride-2 unit of a stage reading the previous stage's map), and a few maps of the 64 x 64 goldens."""
    shapes = set()
    for groups, wpg in ((32, 4), (32, 8), (64, 4)):
        h = 56
        for li, planes in enumerate((64, 128, 256, 512)):
            width = int(planes * wpg / 64) * groups
            if li == 0:
                shapes.add((width, groups, h, 1))
            else:
                shapes.add((width, groups, h, 2))
                h //= 2
                shapes.add((width, groups, h, 1))
    shapes |= {(128, 32, 16, 1), (256, 32, 16, 2), (1024, 32, 4, 2), (2048, 32, 2, 1), (2048, 64, 4, 2), (256, 64, 3, 1)}
    return sorted(shapes)


SHAPES = _conv2_shapes()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _case(C, G, H, s, dt, N=2, seed=0):
    g = torch.Generator().manual_seed(seed + C + G + H + s)
    cg = C // G
    x = torch.randn(N, H, H, C, generator=g).to(dt)                              # NHWC
    w = (torch.randn(C, cg, 3, 3, generator=g) * math.sqrt(2.0 / (9 * C))).float()  # OIHW master
    return x, w


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C,G,H,s", SHAPES, ids=[f"C{c}_G{g}_H{h}_s{s}" for c, g, h, s in SHAPES])
def test_grouped_conv_kernels_against_fp64(C, G, H, s, dt):
    from sm3hip import ops
    code = ops.dtype_code(dt)
    N = 2
    x, w = _case(C, G, H, s, dt, N)
    Ho = (H - 1) // s + 1
    master = w.permute(0, 2, 3, 1).contiguous().to(DEV)                           # [C][3][3][cg] (OHWI)
    n = master.numel()
    wf = torch.empty(n, dtype=dt, device=DEV)
    wd = torch.empty(n, dtype=dt, device=DEV)
    ops.gconv_weight_prep(code, master, C, G, wf, wd)
    wr = w.to(dt).double()                                                        # the rounded weights the kernels see
    # forward + BatchNorm partial rows
    xd = x.to(DEV).reshape(-1, C).contiguous()
    y = torch.empty(N * Ho * Ho, C, dtype=dt, device=DEV)
    prow = (N * Ho * Ho + 127) // 128
    part = torch.full((prow * 2 * C,), float("nan"), device=DEV)
    ops.gconv_fwd(code, xd, wf, y, part, N, H, H, C, G, s)
    torch.cuda.synchronize()
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wq = wr.clone().requires_grad_(True)
    ref = F.conv2d(xr, wq, stride=s, padding=1, groups=G)                         # [N, C, Ho, Wo]
    ref_rows = ref.detach().permute(0, 2, 3, 1).reshape(-1, C)
    got = y.double().cpu()
    assert _rel(got, ref_rows) < REL[dt], _rel(got, ref_rows)
    rows = got.shape[0]
    pad = torch.zeros(prow * 128, C, dtype=torch.float64)
    pad[:rows] = got
    blocks = pad.view(prow, 128, C)
    p = part.view(prow, 2, C).double().cpu()
    np.testing.assert_allclose(p[:, 0], blocks.sum(1), rtol=1e-4, atol=1e-3)      # sums of the stored outputs
    np.testing.assert_allclose(p[:, 1], (blocks ** 2).sum(1), rtol=1e-4, atol=1e-3)
    # data gradient and weight gradient against fp64 autograd
    gy = torch.randn(N, Ho, Ho, C, generator=torch.Generator().manual_seed(C * 7 + H)).to(dt)
    ref.backward(gy.double().permute(0, 3, 1, 2))
    dx = torch.empty(N * H * H, C, dtype=dt, device=DEV)
    gyd = gy.to(DEV).reshape(-1, C).contiguous()
    ops.gconv_dgrad(code, gyd, wd, dx, N, H, H, C, G, s)
    dx_ref = xr.grad.permute(0, 2, 3, 1).reshape(-1, C)
    dw = torch.zeros(C, 9 * (C // G), device=DEV)
    cap = ops.wgrad_det_cap(n)
    ops.gconv_wgrad_det(code, xd, gyd, dw, torch.empty(cap * n, device=DEV), cap, N, H, H, C, G, s)
    torch.cuda.synchronize()
    assert _rel(dx.double().cpu(), dx_ref) < REL[dt], _rel(dx.double().cpu(), dx_ref)
    dw_ref = wq.grad.permute(0, 2, 3, 1).reshape(C, -1)
    assert _rel(dw.double().cpu(), dw_ref) < max(REL[dt] / 3, 1e-5), _rel(dw.double().cpu(), dw_ref)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_grouped_weight_gradient_repeats_bit_for_bit(dt):
    """Two runs give the same bits; two slab capacities (different pixel partitions) both match fp64."""
    from sm3hip import ops
    code = ops.dtype_code(dt)
    C, G, H, s, N = 256, 32, 28, 2, 8
    x, _ = _case(C, G, H, s, dt, N)
    Ho = (H - 1) // s + 1
    gy = torch.randn(N * Ho * Ho, C, generator=torch.Generator().manual_seed(3)).to(dt)
    xd, gyd = x.to(DEV).reshape(-1, C).contiguous(), gy.to(DEV)
    n = C * 9 * (C // G)
    outs = []
    for cap in (512, 512, 7):
        dw = torch.zeros(C, 9 * (C // G), device=DEV)
        ops.gconv_wgrad_det(code, xd, gyd, dw, torch.empty(cap * n, device=DEV), cap, N, H, H, C, G, s)
        outs.append(dw)
    torch.cuda.synchronize()
    assert ops.gconv_wgrad_slabs(N, H, H, s, 512) != ops.gconv_wgrad_slabs(N, H, H, s, 7)
    assert torch.equal(outs[0], outs[1])
    xr = x.double().permute(0, 3, 1, 2)
    wq = torch.zeros(C, C // G, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wq, stride=s, padding=1, groups=G).backward(gy.double().view(N, Ho, Ho, C).permute(0, 3, 1, 2))
    ref = wq.grad.permute(0, 2, 3, 1).reshape(C, -1)
    for dw in (outs[0], outs[2]):
        assert _rel(dw.double().cpu(), ref) < 1e-5


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


def _golden():
    return np.load(os.path.join(GOLDEN, "sm3_v32_rx50_b4_s64_f64.npz"))


def test_compat_step_resnext50_matches_the_reference_golden():
    """model(derm, clinic, 0) -> CrossEntropyLoss -> backward -> torch AdamW, exact-f32 mode, B = 4 pairs at 64 x 64, with the
    tolerances tests/test_e2e_gpu.py holds ResNet-50 to."""
    g = _golden()
    batch, size, seed, style = [int(v) for v in g["meta"]]
    model = _sm3("resnext50_32x4d", seed, torch.float32).train()
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
    loss = float(loss.detach())
    np.testing.assert_allclose(outputs[0][0].detach().double().cpu().numpy(), g["derm_logits"], atol=2e-3, rtol=0)
    np.testing.assert_allclose(outputs[1][0].detach().double().cpu().numpy(), g["clinic_logits"], atol=2e-3, rtol=0)
    for i, o in enumerate(outputs[2]):
        np.testing.assert_allclose(o[0].detach().double().cpu().numpy(), g[f"cross_logits_{i}"], atol=2e-3, rtol=0)
    assert abs(loss - float(g["loss"])) < 1e-3, (loss, float(g["loss"]))
    np.testing.assert_allclose(gn, g["grad_norm"], rtol=5e-2, atol=1e-7)
    params = dict(model.named_parameters())
    k = "clinic_backbone.encoder.layer3.1.conv2.weight"                          # a grouped conv's gradient, subsampled
    sub = params[k].grad.detach().contiguous().reshape(-1)                        # OIHW order, as the golden
    step = max(1, sub.numel() // 256)
    np.testing.assert_allclose(sub[::step][:256].double().cpu().numpy(), g["grad_sub." + k],
                               atol=5e-2 * float(np.abs(g["grad_sub." + k]).max()), rtol=0)
    sd = model.state_dict()
    pn = np.array([sd[n].double().norm().item() for n in params])
    np.testing.assert_allclose(pn, g["post_param_norm"], rtol=5e-3)


def test_fused_trainer_resnext50_matches_the_reference_golden():
    from sm3hip.trainer import SM3Trainer
    g = _golden()
    batch, size, seed, style = [int(v) for v in g["meta"]]
    model = _sm3("resnext50_32x4d", seed, torch.float32)
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


@pytest.mark.parametrize("arch,tag", [("resnext101_32x8d", "rx101_32x8d"), ("resnext101_64x4d", "rx101_64x4d")])
def test_resnext101_features_match_the_reference_golden(arch, tag):
    """Pooled features of a bare encoder (fc = Identity), exact-f32 mode, 2 images at 64 x 64: eval mode (running statistics;
    the frozen-extractor path of the multi-label tools) and train mode (batch statistics from the grouped partial rows)."""
    from oracle import procedural
    from src.models import resnet
    g = np.load(os.path.join(GOLDEN, f"{tag}_feat_b2_s64_f64.npz"))
    batch, size, seed = [int(v) for v in g["meta"]]
    x_np, _ = procedural.make_pair_batch(batch, size, seed)
    x = torch.from_numpy(x_np[0]).to(DEV)
    model = resnet.__dict__[arch](weights=None)
    model.load_state_dict(_procedural(model, 5), strict=True)  # the generator's SEED
    model.fc = torch.nn.Identity()
    model.sm3_dtype = torch.float32
    model.to(DEV)
    for mode in ("eval", "train"):
        model.train(mode == "train")
        with torch.no_grad():
            feat = model(x).double().cpu()
        want = torch.from_numpy(g["feat_" + mode])
        assert feat.shape == want.shape == (batch, 2048)
        assert _rel(feat, want) < 1e-3, (mode, _rel(feat, want))


# ---- determinism, checkpoints, tools -----------------------------------------------------------------------------------
def _three_steps(batches):
    from sm3hip.trainer import SM3Trainer
    model = _sm3("resnext50_32x4d", 11, torch.bfloat16)
    tr = SM3Trainer(model, lr=1e-3, weight_decay=5e-2, eps=1e-5, style=0)
    losses = [float(tr.step(*b)) for b in batches]
    torch.cuda.synchronize()
    return losses, tr._engine().store.flat_p.clone(), tr.m.clone()


def test_three_bf16_resnext50_steps_repeat_bit_for_bit():
    """Two runs of three bf16 training steps (B = 32 pairs at 128 x 128: both views as one batch) give the same losses and
    parameters, bit for bit."""
    batches = [_pairs(32, 128, 40 + i) for i in range(3)]
    a = _three_steps(batches)
    b = _three_steps(batches)
    assert all(math.isfinite(x) for x in a[0])
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_resnext50_checkpoint_round_trip(tmp_path):
    from sm3hip.trainer import SM3Trainer
    from src.models.simclr import SimCLRSkinV32
    batches = [_pairs(8, 64, 60 + i) for i in range(2)]
    model = _sm3("resnext50_32x4d", 13, torch.float32)
    tr = SM3Trainer(model, lr=1e-4, weight_decay=5e-2, eps=1e-5, style=0)
    tr.step(*batches[0])
    torch.cuda.synchronize()
    path = str(tmp_path / "checkpoint.pth.tar")
    torch.save({"epoch": 0, "state_dict": model.state_dict(), "optimizer": tr.optimizer_state_dict(), "scaler": {}}, path)
    loss2 = float(tr.step(*batches[1]))
    p2 = tr._engine().store.flat_p.clone()
    ck = torch.load(path, map_location="cpu", weights_only=False)
    keys = open(os.path.join(GOLDEN, "rx50_state_dict_keys.txt")).read().split()
    assert list(ck["state_dict"].keys()) == keys
    fresh = SimCLRSkinV32("resnext50_32x4d", None, 128, 0.1)
    fresh.sm3_dtype = torch.float32
    res = fresh.load_state_dict(ck["state_dict"], strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    fresh.to(DEV)
    tr2 = SM3Trainer(fresh, lr=1.0, weight_decay=0.0, eps=1.0, style=0)
    tr2.load_optimizer_state_dict(ck["optimizer"])
    loss2b = float(tr2.step(*batches[1]))
    torch.cuda.synchronize()
    assert abs(loss2 - loss2b) < 1e-5, (loss2, loss2b)
    assert float((tr2._engine().store.flat_p - p2).abs().max()) < 1e-6


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_rx_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mlc_train_runs_on_a_resnext50_extractor(tmp_path):
    mt = _tool("mlc_train")
    args = mt.get_parser().parse_args(["-a", "resnext50_32x4d", "--data-name", "synthetic", "--data-path", "-", "--epochs", "2",
                                       "-b", "32", "--num-samples", "96", "--img-sz", "64", "64", "--log-path", str(tmp_path),
                                       "--temperature", "1", "--mlc-proj-dim", "128", "--sa-dim-ff", "64", "-lr", "1e-3",
                                       "--save-freq", "1"])
    args.world_size = 1
    hist = mt.main(0, args)
    assert len(hist) == 2 and all(math.isfinite(v) and 0.0 < v < 20.0 for v in hist), hist
    sd = torch.load(os.path.join(str(tmp_path), "ckp_1.pth"), map_location="cpu", weights_only=False)["state_dict"]
    first = torch.load(os.path.join(str(tmp_path), "ckp_0.pth"), map_location="cpu", weights_only=False)["state_dict"]
    moved = [k for k in sd if k.startswith(("mlc_sa.", "prototypes.", "projectors.")) and sd[k].is_floating_point()
             and not torch.equal(first[k], sd[k])]
    assert len(moved) > 10
