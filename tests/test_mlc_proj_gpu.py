"""--mlc-proj v0..v3 on the HIP heads (sm3hip/mlc.py): the reference's BN-MLP and identity label projectors against fixtures
written from the reference's own modules (tests/golden/gen_mlc_proj_golden.py), v1 at ResNet-50 size against fp64 autograd,
the grouped GEMM kernels against per-label launches (bit for bit) and fp64, the 4096-wide LayerNorm rows, and the tools."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
BOUND_AT_SIZE = 1e-2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "skin-sm3_amd", "tools")


class _Heads(nn.Module):
    """The head part of the reference's Model (mlc_train.py:58-90) around a projector module, stock PyTorch."""

    def __init__(self, projectors, D, nhead, ff, dropout, l2_norm):
        super().__init__()
        self.projectors = projectors
        self.mlc_sa = nn.TransformerEncoderLayer(d_model=D, nhead=nhead, dim_feedforward=ff, dropout=dropout)
        self.prototypes = nn.ModuleList([nn.Linear(D, n, bias=False) for n in NUM_CLASSES])
        self.l2_norm = l2_norm

    def forward(self, feats):
        p = self.projectors(feats)
        sa = self.mlc_sa(torch.stack(p if isinstance(p, list) else [p], dim=0))
        if self.l2_norm:
            sa = nn.functional.normalize(sa, dim=-1, p=2)
        return sa, [self.prototypes[i](sa[i % len(sa)]) for i in range(len(self.prototypes))]


def _build(kind, in_dim, D, nhead, ff, l2=False):
    from src.models.projector import build_mlc_projectors
    return _Heads(build_mlc_projectors(kind, in_dim, D, 8), D, nhead, ff, 0.0, l2)


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30))


def _loss(preds, targets, T):
    crit = nn.CrossEntropyLoss(ignore_index=-100)
    return sum(crit(p / T, t) for p, t in zip(preds, targets)) / len(NUM_CLASSES)


@pytest.mark.parametrize("case", ["v0", "v1", "v2", "v3", "v2_l2"])
def test_fixture_parity(case):
    """One fp32 train-mode step of the HIP heads against the reference's fp64 step: loss, sa_feats, preds, every parameter
    gradient and the feature gradient, BatchNorm buffers and num_batches_tracked, then the eval-mode preds."""
    from sm3hip import mlc
    z = np.load(os.path.join(GOLDEN, f"mlc_proj_{case}_f64.npz"))
    kind, l2 = case[:2], bool(z["l2_norm"])
    feats = torch.from_numpy(z["feats"])
    D = z["init:mlc_sa.linear1.weight"].shape[1]
    model = _build(kind, feats.shape[1], D, 2, z["init:mlc_sa.linear1.weight"].shape[0], l2)
    model.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init:")})
    model.to(DEV).train()
    f = feats.to(DEV).requires_grad_(True)
    targets = torch.from_numpy(z["targets"]).to(DEV)
    sa, preds = mlc.heads_forward(model, f, seed=1)
    loss = _loss(preds, targets, float(z["temperature"]))
    assert abs(float(loss) - float(z["loss"])) < 1e-5, (float(loss), float(z["loss"]))
    assert _rel(sa, torch.from_numpy(z["sa_feats"])) < 2e-5
    assert _rel(torch.cat(preds, 1), torch.from_numpy(z["preds"])) < 2e-5
    if not l2:
        loss.backward()
        torch.cuda.synchronize()
        for name, p in model.named_parameters():
            err = _rel(p.grad, torch.from_numpy(z["grad:" + name]))
            assert err < 2e-4, (name, err)
        assert _rel(f.grad, torch.from_numpy(z["grad:feats"])) < 2e-4
    for name, t in model.named_buffers():
        want = torch.from_numpy(z["after:" + name])
        if name.endswith("num_batches_tracked"):
            assert int(t) == int(want), name
        else:
            assert _rel(t, want) < 1e-5, name
    model.eval()
    with torch.no_grad():
        _, pe = mlc.heads_forward(model, f.detach(), seed=1)
    assert _rel(torch.cat(pe, 1), torch.from_numpy(z["preds_eval"])) < 2e-5


def test_v1_at_resnet50_size_against_fp64():
    """v1 on 4096-wide features, D 512, B 256 (the reference's mlc_train batch): output, every gradient, the buffers."""
    from sm3hip import mlc
    torch.manual_seed(5)
    B, in_dim, D = 256, 4096, 512
    model = _build("v1", in_dim, D, 1, 128).to(DEV).train()
    ref = _build("v1", in_dim, D, 1, 128).to(DEV).double().train()
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    feats = torch.randn(B, in_dim, device=DEV)
    targets = torch.stack([torch.randint(0, n, (B,), device=DEV) for n in NUM_CLASSES])
    fr = feats.double().requires_grad_(True)
    sa_r, pr = ref(fr)
    lr = _loss(pr, targets, 0.1)
    lr.backward()
    f = feats.clone().requires_grad_(True)
    sa, p = mlc.heads_forward(model, f, seed=1)
    loss = _loss(p, targets, 0.1)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(lr)) < 1e-4 * max(1.0, abs(float(lr)))
    assert _rel(sa, sa_r.detach()) < 1e-4
    # Three train-mode BatchNorms behind every projector gradient: each is a cancelled sum that magnifies fp32 rounding (the
    # fixtures above hold 2e-4 at width 64).  Bound BOUND_AT_SIZE is set about 4x above the worst measured on an MI355X.
    errs = {name: _rel(q.grad, qr.grad) for (name, q), (_, qr) in zip(model.named_parameters(), ref.named_parameters())}
    errs["feats"] = _rel(f.grad, fr.grad)
    worst = max(errs, key=errs.get)
    print(f"v1 at size: worst gradient error {errs[worst]:.3e} ({worst})")
    assert errs[worst] < BOUND_AT_SIZE, (worst, errs[worst])
    for (name, t), (_, tr) in zip(model.named_buffers(), ref.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(t) == int(tr) == 1
        else:
            assert _rel(t, tr) < 1e-5, name


def test_fc_mode_freezes_projector_buffers_and_parameters():
    """mlc_eval --finetune fc: projectors in eval mode with requires_grad off -- their buffers do not move, their parameters
    get no gradient, and the forward uses the running statistics (equal to torch's eval-mode modules)."""
    from sm3hip import mlc
    torch.manual_seed(6)
    model = _build("v2", 256, 64, 2, 64).to(DEV)
    with torch.no_grad():
        for name, t in model.named_buffers():
            if name.endswith("running_var"):
                t.uniform_(0.5, 1.5)
            elif name.endswith("running_mean"):
                t.normal_(0, 0.1)
    model.train()
    model.projectors.eval()
    model.mlc_sa.eval()
    for q in model.projectors.parameters():
        q.requires_grad = False
    before = {k: v.clone() for k, v in model.projectors.state_dict().items()}
    feats = torch.randn(16, 256, device=DEV)
    _, preds = mlc.heads_forward(model, feats, seed=3)
    _loss(preds, torch.stack([torch.randint(0, n, (16,), device=DEV) for n in NUM_CLASSES]), 1.0).backward()
    torch.cuda.synchronize()
    for k, v in model.projectors.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(q.grad is None for q in model.projectors.parameters())
    assert all(q.grad is not None for q in model.prototypes.parameters())
    model.eval()
    with torch.no_grad():
        _, got = mlc.heads_forward(model, feats, seed=3)
        _, want = model(feats)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) < 2e-4 * (float(b.abs().max()) + 1.0)


def _per_label_gemm(x, w, G):
    from sm3hip import ops
    from sm3hip._lib import SM3_F32
    rows, GK = x.shape
    K, N = GK // G, w.shape[-2]
    out = []
    for g in range(G):
        xg = x[:, g * K:(g + 1) * K].contiguous()
        y = torch.empty(rows, N, device=DEV)
        part = torch.empty((rows + 127) // 128, 2, N, device=DEV)
        ops.conv_gemm(ops.fwd_desc(SM3_F32, rows, 1, 1, K, N, 1, 1, 0), xg, w[g].contiguous(), y, None, part)
        out.append((y, part))
    return torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 2)


def _per_label_wgrad(x, dy, G):
    from sm3hip import ops
    from sm3hip._lib import SM3_F32
    rows = x.shape[0]
    K, N = x.shape[1] // G, dy.shape[1] // G
    dws = []
    for g in range(G):
        dw = torch.zeros(N, K, device=DEV)
        cap = ops.wgrad_det_cap(N * K)
        slabs = torch.empty(cap * N * K, device=DEV) if (rows + 255) // 256 > 1 else dw
        ops.conv_wgrad_det(ops.fwd_desc(SM3_F32, rows, 1, 1, K, N, 1, 1, 0), x[:, g * K:(g + 1) * K].contiguous(),
                           dy[:, g * N:(g + 1) * N].contiguous(), dw, slabs, min(cap, max(1, (rows + 255) // 256)))
        dws.append(dw)
    return torch.stack(dws)


@pytest.mark.parametrize("G,K,N,rows", [(8, 4096, 4096, 256), (8, 4096, 512, 256), (8, 256, 64, 24), (8, 512, 256, 200),
                                        (3, 96, 160, 600)])
def test_grouped_kernels_equal_per_label_launches_and_fp64(G, K, N, rows):
    from sm3hip import ops
    torch.manual_seed(7)
    x = torch.randn(rows, G * K, device=DEV)
    w = torch.randn(G, N, K, device=DEV) / math.sqrt(K)
    y = torch.empty(rows, G * N, device=DEV)
    part = torch.empty((rows + 127) // 128, 2, G * N, device=DEV)
    ops.grouped_gemm(x, w, y, G, part)
    y_ref, part_ref = _per_label_gemm(x, w, G)
    assert torch.equal(y, y_ref) and torch.equal(part, part_ref)
    y64 = torch.einsum("rgk,gnk->rgn", x.double().view(rows, G, K), w.double()).reshape(rows, G * N)
    assert _rel(y, y64) < 1e-5
    # data gradient: the same launch with the transposed banks
    dy = torch.randn(rows, G * N, device=DEV)
    wt = w.transpose(1, 2).contiguous()
    dx = torch.empty(rows, G * K, device=DEV)
    ops.grouped_gemm(dy, wt, dx, G)
    dx_ref, _ = _per_label_gemm(dy, wt, G)
    assert torch.equal(dx, dx_ref)
    dx64 = torch.einsum("rgn,gnk->rgk", dy.double().view(rows, G, N), w.double()).reshape(rows, G * K)
    assert _rel(dx, dx64) < 1e-5
    # weight gradient, fixed order
    dw = torch.zeros(G, N, K, device=DEV)
    ops.grouped_wgrad_det(x, dy, dw, G)
    assert torch.equal(dw, _per_label_wgrad(x, dy, G))
    dw64 = torch.einsum("rgn,rgk->gnk", dy.double().view(rows, G, N), x.double().view(rows, G, K))
    assert _rel(dw, dw64) < 1e-5
    dw2 = torch.zeros(G, N, K, device=DEV)
    ops.grouped_wgrad_det(x, dy, dw2, G)
    assert torch.equal(dw, dw2)
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [1024, 2048, 4096])
def test_wide_layernorm_rows_against_fp64(D):
    from sm3hip import _lib, ops
    from sm3hip._lib import check
    lib, P = _lib.load(), ops._ptr
    torch.manual_seed(8)
    rows = 40
    a, b = torch.randn(rows, D, device=DEV), torch.randn(rows, D, device=DEV)
    gamma, beta = 1 + 0.1 * torch.randn(D, device=DEV), 0.1 * torch.randn(D, device=DEV)
    out, st = torch.empty(rows, D, device=DEV), torch.empty(rows, 2, device=DEV)
    check(lib.sm3_mlc_add_ln_fwd(P(a), P(b), P(gamma), P(beta), 1e-5, 0.0, 1, P(out), P(st), rows, D, None), "ln_fwd")
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    g64, be64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = nn.functional.layer_norm(a64 + b64, (D,), g64, be64, 1e-5)
    dout = torch.randn(rows, D, device=DEV)
    ref.backward(dout.double())
    da, db = torch.empty_like(a), torch.empty_like(a)
    dg, dbe = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    check(lib.sm3_mlc_add_ln_bwd(P(dout), P(a), P(b), P(st), P(gamma), 0.0, 1, P(da), P(db), P(dg), P(dbe), rows, D, None),
          "ln_bwd")
    torch.cuda.synchronize()
    assert _rel(out, ref.detach()) < 1e-6
    assert _rel(da, a64.grad) < 1e-5 and _rel(db, b64.grad) < 1e-5
    assert _rel(dg, g64.grad) < 1e-5 and _rel(dbe, be64.grad) < 1e-5
    assert lib.sm3_mlc_add_ln_fwd(P(a), P(b), P(gamma), P(beta), 1e-5, 0.0, 1, P(out), P(st), rows, 4100, None) < 0


def test_v1_steps_are_reproducible():
    """Two identical v1 forward / backward passes: loss, sa_feats, the projector gradients (fixed-order grouped and plain
    weight gradients), the feature gradient and the BatchNorm buffers are equal bit for bit."""
    from sm3hip import mlc
    torch.manual_seed(9)
    base = _build("v1", 1024, 256, 2, 128)
    feats = torch.randn(64, 1024, device=DEV)
    targets = torch.stack([torch.randint(0, n, (64,), device=DEV) for n in NUM_CLASSES])
    runs = []
    for _ in range(2):
        m = _build("v1", 1024, 256, 2, 128)
        m.load_state_dict(base.state_dict())
        m.to(DEV).train()
        f = feats.clone().requires_grad_(True)
        sa, p = mlc.heads_forward(m, f, seed=4)
        loss = _loss(p, targets, 0.1)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach(), sa, [q.grad for q in m.projectors.parameters()], f.grad,
                     [t.clone() for t in m.projectors.buffers()]))
    (l0, s0, g0, f0, b0), (l1, s1, g1, f1, b1) = runs
    assert torch.equal(l0, l1) and torch.equal(s0, s1) and torch.equal(f0, f1)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1)) and all(torch.equal(a, b) for a, b in zip(b0, b1))


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_gpu_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind", ["v0", "v1", "v2", "v3"])
def test_mlc_train_tool_runs_each_projector(tmp_path, kind):
    mt = _tool("mlc_train")
    dim = "4096" if kind == "v0" else "128"
    args = mt.get_parser().parse_args(["--data-name", "synthetic", "--data-path", "-", "--epochs", "2", "-b", "32",
                                       "--num-samples", "96", "--img-sz", "64", "64", "--log-path", str(tmp_path),
                                       "--temperature", "1", "--mlc-proj", kind, "--mlc-proj-dim", dim, "--sa-dim-ff", "64",
                                       "--sa-dropout", "0.1", "-lr", "1e-3", "--save-freq", "1"])
    args.world_size = 1
    hist = mt.main(0, args)
    assert len(hist) == 2 and all(math.isfinite(v) and 0.0 < v < 20.0 for v in hist), hist
    sd = torch.load(os.path.join(str(tmp_path), "ckp_1.pth"), map_location="cpu", weights_only=False)["state_dict"]
    first = torch.load(os.path.join(str(tmp_path), "ckp_0.pth"), map_location="cpu", weights_only=False)["state_dict"]
    from src.models.projector import build_mlc_projectors
    want = ["projectors." + k for k in build_mlc_projectors(kind, 4096, int(dim), 8).state_dict()]
    assert [k for k in sd if k.startswith("projectors.")] == want
    moved = [k for k in sd if k.startswith(("mlc_sa.", "prototypes.", "projectors.")) and sd[k].is_floating_point()
             and not torch.equal(first[k], sd[k])]
    assert len(moved) > 10
    if kind != "v0":
        assert int(sd["projectors.projectors.0.1.num_batches_tracked"]) == 2 * 3  # 3 steps per epoch, 2 epochs


@pytest.mark.parametrize("mode", ["fc", "projector", "all"])
def test_mlc_eval_finetunes_from_a_v2_checkpoint(tmp_path, mode, capsys):
    mt, me = _tool("mlc_train"), _tool("mlc_eval")
    common = ["--data-name", "synthetic", "--data-path", "-", "--img-sz", "64", "64", "--mlc-proj", "v2", "--mlc-proj-dim",
              "128", "--sa-dim-ff", "64"]
    targs = mt.get_parser().parse_args(common + ["--epochs", "1", "-b", "16", "--num-samples", "32",
                                                 "--log-path", str(tmp_path / "train")])
    targs.world_size = 1
    mt.main(0, targs)
    ck = torch.load(str(tmp_path / "train" / "ckp_0.pth"), map_location="cpu", weights_only=False)["state_dict"]
    hist = me.main(common + ["--epochs", "2", "-b", "16", "--steps-per-epoch", "3", "--val-steps", "2",
                             "--log-path", str(tmp_path / "eval"), "--finetune", mode,
                             "--pretrain-path", str(tmp_path / "train" / "ckp_0.pth")])
    out = capsys.readouterr().out
    missing = out.split("missing keys:")[1].split("\n")[0]
    assert "projectors" not in missing, missing
    assert len(hist) == 2 and all(math.isfinite(t["loss"]) and 0.0 <= v["AUC_AVG"] <= 1.0 for t, v in hist)
    sd = torch.load(str(tmp_path / "eval" / "best_finetune.pth"), map_location="cpu", weights_only=False)["state_dict"]
    proj = [k for k in sd if k.startswith("projectors.")]
    if mode == "fc":
        assert all(torch.equal(sd[k], ck[k]) for k in proj)
    else:
        assert any(not torch.equal(sd[k], ck[k]) for k in proj if sd[k].is_floating_point())
