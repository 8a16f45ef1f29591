"""CPU: Grad-CAM (sm3hip/cam.py, csrc/cam.hip) -- the entry points in the header, the binding and the library, their
host-side refusals, grad_cam's refusals, tools/backbone_cam.py's and tools/mlc_cam.py's parsers and refusals (each before
anything touches the GPU), and the float64 Grad-CAM restatement that tests/test_cam_gpu.py checks the HIP path against, itself
checked against a hand computation on a 2 x 2 case."""
import ctypes as C
import importlib.util
import os
import re
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]


# ---- the float64 restatement (used by tests/test_cam_gpu.py) ----------------------------------------------------------
def cam_from(A, G, H, W):
    """A, G [N, C, h, w] -> (low [N, h, w], maps [N, H, W]): alpha = mean_p G, cam = ReLU(sum_c alpha_c A_c), bilinear
    upsample (align_corners=False), (cam - min) / (1e-7 + max(cam - min)) per map."""
    alpha = G.mean(dim=(2, 3))
    low = F.relu((alpha[:, :, None, None] * A).sum(dim=1))
    up = F.interpolate(low[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    up = up - up.amin(dim=(1, 2), keepdim=True)
    return low, up / (1e-7 + up.amax(dim=(1, 2), keepdim=True))


def _stage_key(prefix, layer):
    """The taps key of a ResNet-50 stage's last block (oracle.sm3_oracle.bottleneck records block outputs by name)."""
    from oracle.procedural import RESNET50_LAYERS
    li = int(layer[-1])
    return f"{prefix}layer{li}.{RESNET50_LAYERS[li - 1][1] - 1}"


def ref_grad_cam(forward, P, Bf, derm, clinic, prefixes, layer, target_class):
    """Grad-CAM in float64 on the oracle: forward(P, Bf, derm, clinic) -> 8 logits (oracle.sm3_oracle.baseline_forward,
    inference_forward, or a head restatement on top of resnet50_features), run with resnet50_features' taps recording the
    block outputs; G = autograd of each label's target logit with respect to the stage output.  Returns maps
    [N, 8, 2, H, W], low_res [N, 8, 2, h, w] and the logits."""
    from oracle import sm3_oracle as O
    taps = {}
    orig = O.resnet50_features

    def tapped(x, P_, B_, prefix, training, stat_reduce=None, taps_=None):
        return orig(x, P_, B_, prefix, training, stat_reduce, taps)

    derm, clinic = derm.detach().requires_grad_(), clinic.detach().requires_grad_()  # a graph through the stage outputs
    with mock.patch.object(O, "resnet50_features", tapped):
        logits = forward(P, Bf, derm, clinic)
    A = [taps[_stage_key(p, layer)] for p in prefixes]
    H, W = derm.shape[2:]
    maps, low = [], []
    for i in range(len(NUM_CLASSES)):
        y = logits[i].gather(1, target_class[:, i:i + 1]).sum()  # eval mode: each logit depends on its own sample only
        G = torch.autograd.grad(y, A, retain_graph=True)
        per = [cam_from(a.detach(), g, H, W) for a, g in zip(A, G)]
        low.append(torch.stack([p[0] for p in per], 1))
        maps.append(torch.stack([p[1] for p in per], 1))
    return {"maps": torch.stack(maps, 1), "low_res": torch.stack(low, 1), "logits": [l.detach() for l in logits]}


def test_restatement_against_a_hand_computation_2x2():
    A = torch.tensor([[[[1., 0.], [0., 1.]], [[0., 2.], [0., 0.]]]], dtype=torch.float64)     # [1, 2, 2, 2]
    G = torch.tensor([[[[1., 1.], [1., 1.]], [[-4., 0.], [0., 0.]]]], dtype=torch.float64)    # alpha = (1, -1)
    # cam = ReLU(1 * A0 - 1 * A1) = ReLU([[1, -2], [0, 1]]) = [[1, 0], [0, 1]]
    low, same = cam_from(A, G, 2, 2)
    assert torch.equal(low, torch.tensor([[[1., 0.], [0., 1.]]], dtype=torch.float64))
    assert torch.allclose(same, low / (1 + 1e-7), rtol=0, atol=1e-15)
    # 2 -> 4: source positions (dst + 0.5) / 2 - 0.5 = 0 (clamped), 0.25, 0.75, 1.25 (its right neighbour clamped)
    _, up = cam_from(A, G, 4, 4)
    hand = {(0, 0): 1.0, (0, 1): 0.75, (1, 1): 0.75 * 0.75 + 0.25 * 0.25, (0, 3): 0.0, (1, 2): 2 * 0.75 * 0.25,
            (3, 3): 1.0}
    for (r, c), v in hand.items():
        assert abs(float(up[0, r, c]) - v / (1 + 1e-7)) < 1e-12, (r, c)
    # the gradient is taken with respect to the post-ReLU output: a logit of A through a ReLU-free head gives G = its
    # weights, also where A is 0
    a = torch.zeros(1, 2, 2, 2, dtype=torch.float64, requires_grad=True)
    w = torch.tensor([3.0, -1.0], dtype=torch.float64)
    (g,) = torch.autograd.grad((a.mean(dim=(2, 3)) * w).sum(), [a])
    assert torch.allclose(g.mean(dim=(2, 3)), w[None] / 4)


def test_restatement_layer4_alpha_is_the_pooled_gradient():
    """At layer4 the stage output feeds the average pool directly: alpha = dfeat / (h*w), the shortcut grad_cam takes."""
    from oracle import procedural, sm3_oracle as O
    state = procedural.make_state_dict(procedural.baseline_spec(), seed=3)
    P, Bf = O.split_state(state, torch.float64, requires_grad=False)
    derm, clinic = [torch.from_numpy(a[0]).double() for a in procedural.make_pair_batch(2, 64, 3)]
    tc = torch.tensor([[1, 0, 1, 2, 0, 1, 2, 0], [4, 2, 0, 1, 2, 0, 1, 1]])
    ref = ref_grad_cam(O.baseline_forward, P, Bf, derm, clinic, ("derm_backbone.", "clinic_backbone."), "layer4", tc)
    assert ref["maps"].shape == (2, 8, 2, 64, 64) and ref["low_res"].shape == (2, 8, 2, 2, 2)
    taps = {}
    A = O.resnet50_features(derm, P, Bf, "derm_backbone.", False, taps=taps)  # noqa: F841 (records the taps)
    A4 = taps[_stage_key("derm_backbone.", "layer4")]
    for i in range(8):
        w = P[f"classifier.{i}.weight"][tc[:, i], :2048]                           # dfeat of the derm half
        low = F.relu((w[:, :, None, None] / 4 * A4).sum(1))
        assert torch.allclose(low, ref["low_res"][:, i, 0], rtol=1e-10, atol=1e-12)
    assert float(ref["maps"].amin()) >= 0 and float(ref["maps"].amax()) <= 1


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def _lib():
    from sm3hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_points_are_declared_bound_and_exported():
    from sm3hip import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sm3_hip.h")).read(), flags=re.S)
    lib = _lib()
    for name in ("sm3_cam_alpha", "sm3_cam_maps"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
        assert name in L.SIGNATURES
        assert hasattr(lib, name)
    assert lib.sm3_abi_version() == 9


def _p(v):
    return C.c_void_p(v) if v else C.c_void_p(0)


def _alpha(lib, dtype=1, g=0x1000, alpha=0x2000, T=8, N=2, HW=49, Cn=64):
    return lib.sm3_cam_alpha(dtype, _p(g), _p(alpha), T, N, HW, Cn, C.c_void_p(0))


def _maps(lib, dtype=1, a=0x1000, alpha=0x2000, low=0x3000, maps=0x4000, N=2, T=8, h=7, w=7, Cn=64, H=224, W=224):
    return lib.sm3_cam_maps(dtype, _p(a), _p(alpha), _p(low), _p(maps), N, T, h, w, Cn, H, W, C.c_void_p(0))


@pytest.mark.parametrize("kw,code", [
    (dict(g=0), -1), (dict(alpha=0), -1), (dict(T=0), -1), (dict(N=0), -1), (dict(HW=0), -1), (dict(Cn=-1), -1),
    (dict(T=2 ** 20, N=2 ** 10, HW=2 ** 12), -1), (dict(dtype=5), -3)])
def test_alpha_rejects_bad_arguments_before_any_launch(kw, code):
    assert _alpha(_lib(), **kw) == code, kw


@pytest.mark.parametrize("kw,code", [
    (dict(a=0), -1), (dict(alpha=0), -1), (dict(low=0), -1), (dict(maps=0), -1), (dict(N=0), -1), (dict(T=0), -1),
    (dict(h=0), -1), (dict(w=-3), -1), (dict(H=0), -1), (dict(W=0), -1), (dict(Cn=0), -1),
    (dict(N=2 ** 16, h=2 ** 8, w=2 ** 8), -1), (dict(H=2 ** 16, W=2 ** 16), -1),
    (dict(dtype=3), -3), (dict(Cn=60), -2), (dict(a=0x1008), -2)])
def test_maps_rejects_bad_arguments_before_any_launch(kw, code):
    assert _maps(_lib(), **kw) == code, kw


# ---- grad_cam's refusals --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def baseline18():
    from src.models.baseline import Baseline
    return Baseline("resnet18", None).eval()


def test_grad_cam_refuses_train_mode_cpu_tensors_and_bad_arguments(baseline18):
    from sm3hip.cam import grad_cam
    x = torch.zeros(2, 3, 32, 32)
    m = baseline18
    with pytest.raises(ValueError, match="eval mode"):
        grad_cam(m.train(), x, x)
    m.eval()
    m.classifier[3].train()
    with pytest.raises(ValueError, match="classifier.3"):
        grad_cam(m, x, x)
    m.eval()
    with pytest.raises(ValueError, match="CUDA tensor"):
        grad_cam(m, x, x)
    with pytest.raises(ValueError, match="layer must be"):
        grad_cam(m, x, x, layer="layer5")
    with pytest.raises(TypeError, match="Baseline"):
        grad_cam(torch.nn.Linear(2, 2), x, x)


# ---- the tools ----------------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(f"sm3_{name}_cpu", os.path.join(TOOLS, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_backbone_cam_parser_takes_backbone_eval_line_and_the_cam_flags():
    bc = _tool("backbone_cam")
    a = bc.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.target, a.cam_layer, a.split, a.max_cases, a.linear_path, a.arch) == ("pred", "layer4", "test", 64, None,
                                                                                     "resnet50")
    a = bc.get_parser().parse_args(["--data-path", "x", "--data-name", "SevenPCBaseDataset", "--target", "cls",
                                    "--cam-layer", "layer2", "--split", "valid", "--max-cases", "5", "--linear-path", "p.pth",
                                    "-a", "resnet18", "--img-sz", "64", "96", "--amp", "--amp-dtype", "bf16"])
    assert (a.target, a.cam_layer, a.split, a.max_cases, a.linear_path, a.arch, a.img_sz) == (
        "cls", "layer2", "valid", 5, "p.pth", "resnet18", [64, 96])


def test_mlc_cam_parser_takes_mlc_eval_line_and_a_checkpoint():
    mc = _tool("mlc_cam")
    a = mc.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.checkpoint, a.target, a.cam_layer, a.mlc_proj, a.arch, a.test_sz) == (None, "pred", "layer4", "v4", "resnet50",
                                                                                      224)
    a = mc.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic", "--checkpoint", "c.pth", "--mlc-proj", "v2",
                                    "--mlc-proj-dim", "512", "--sa-dim-ff", "128", "--cam-layer", "layer3", "--test-sz", "96",
                                    "--target", "cls", "--l2-norm"])
    assert (a.checkpoint, a.mlc_proj, a.mlc_proj_dim, a.cam_layer, a.test_sz, a.target, a.l2_norm) == (
        "c.pth", "v2", 512, "layer3", 96, "cls", True)


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that reaches for the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("touched the GPU before refusing")
    monkeypatch.setattr(torch, "Generator", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    monkeypatch.setattr(torch.nn.Module, "to", boom)


@pytest.mark.parametrize("argv,msg", [
    (["--linear-path", "/nonexistent/best_linear.pth"], "does not exist"),
    (["-a", "resnext50_32x4d"], "not supported"),
    (["--max-cases", "0"], "max-cases"),
])
def test_backbone_cam_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    bc = _tool("backbone_cam")
    with pytest.raises(SystemExit, match=msg):
        bc.main(["--data-name", "synthetic", "--data-path", "-"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("argv,msg", [
    (["--checkpoint", "/nonexistent/best_finetune.pth"], "does not exist"),
    (["-a", "resnet18"], "not supported"),
    (["--mlc-proj", "v9"], "mlc-proj"),
    (["--mlc-proj", "v0", "--mlc-proj-dim", "512"], "v0"),
    (["--max-cases", "0"], "max-cases"),
])
def test_mlc_cam_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    mc = _tool("mlc_cam")
    with pytest.raises(SystemExit, match=msg):
        mc.main(["--data-name", "synthetic", "--data-path", "-"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool,flag", [("backbone_cam", "linear-path"), ("mlc_cam", "checkpoint")])
def test_real_data_needs_weights(tool, flag, no_gpu, tmp_path):
    root = tmp_path / "7PC"
    os.makedirs(root / "images")
    for f in ("meta.csv", "train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        (root / f).write_text("")
    with pytest.raises(SystemExit, match=flag):
        _tool(tool).main(["--data-name", "SevenPCBaseDataset", "--data-path", str(root), "--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool", ["backbone_cam", "mlc_cam"])
def test_unknown_data_and_layer_are_refused(tool, no_gpu, tmp_path, capsys):
    mod = _tool(tool)
    with pytest.raises(SystemExit, match="not available"):
        mod.main(["--data-name", "ImageNet", "--data-path", "-", "--log-path", str(tmp_path)])
    with pytest.raises(SystemExit) as e:
        mod.main(["--data-name", "synthetic", "--data-path", "-", "--cam-layer", "conv1"])
    assert e.value.code == 2 and "--cam-layer" in capsys.readouterr().err
