"""CPU: the BasicBlock encoders (resnet18 / resnet34) -- modules, state_dict layout against the reference's (golden key and
shape lists from tests/golden/gen_resnet18_golden.py), the engine's BasicBlock plan, and the tools' -a handling."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def _lines(name):
    return open(os.path.join(GOLDEN, name)).read().split()


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"_tool_{name}", os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resnet18_and_resnet34_construct_with_the_torchvision_layout():
    from src.models import resnet
    for ctor, counts, nparams in ((resnet.resnet18, [2, 2, 2, 2], 11_689_512), (resnet.resnet34, [3, 4, 6, 3], 21_797_672)):
        m = ctor()
        assert m.block_counts == counts and m.block_type == "basic"
        assert isinstance(m.layer1[0], resnet.BasicBlock) and m.layer1[0].downsample is None
        assert m.layer2[0].downsample is not None and m.layer2[1].downsample is None
        assert m.fc.in_features == 512
        assert sum(p.numel() for p in m.parameters()) == nparams  # torchvision's resnet18 / resnet34 counts
    m = resnet.resnet18(zero_init_residual=True)
    assert all(float(b.bn2.weight.detach().abs().sum()) == 0 for layer in (m.layer1, m.layer4) for b in layer)
    assert float(m.layer1[0].bn1.weight.detach().sum()) == 64
    cache = os.path.join(torch.hub.get_dir(), "checkpoints", "resnet18-f37072fd.pth")  # torchvision's file name
    if not os.path.isfile(cache):  # never downloaded: served from the hub cache or refused
        with pytest.raises(RuntimeError, match="resnet18-f37072fd.pth"):
            resnet.resnet18(weights="IMAGENET1K_V1")


def test_simclr_skin_v32_resnet18_state_dict_equals_the_reference():
    from src.models.simclr import SimCLRSkinV32
    m = SimCLRSkinV32("resnet18", None, 128, 0.1)
    sd = m.state_dict()
    assert list(sd.keys()) == _lines("r18_state_dict_keys.txt")
    shapes = json.load(open(os.path.join(GOLDEN, "r18_state_dict_shapes.json")))
    assert [[k, list(v.shape)] for k, v in sd.items()] == shapes
    assert len(sd) == 304 and sum(v.numel() for v in sd.values()) == 24_748_980
    assert m.derm_feat_dim == m.clinic_feat_dim == m.derm_backbone.encoder_out_dim == 512
    assert m.cross_proj[0][0].in_features == 512 and m.derm_backbone.projector[6].out_features == 128


def test_baseline_resnet18_state_dict_equals_the_reference():
    from src.models.baseline import Baseline
    m = Baseline("resnet18", None)
    assert list(m.state_dict().keys()) == _lines("r18_baseline_state_dict_keys.txt")
    assert len(m.classifier) == 8 and all(c.in_features == 2 * 512 for c in m.classifier)
    assert Baseline("resnet34", None).classifier[0].in_features == 1024
    assert Baseline().classifier[0].in_features == 4096  # the default stays resnet50


def test_baseline_basicblock_default_weights_follow_the_reference():
    """The reference's Baseline defaults to ImageNet weights (baseline.py:61); for the BasicBlock archs the mirror keeps
    that default, served from the torch-hub cache only.  Without the cached file it is refused, never replaced by random
    weights; weights=None is the explicit random initialisation backbone_eval passes by default."""
    from src.models import resnet
    from src.models.baseline import Baseline
    for arch, hub in (("resnet18", "resnet18-f37072fd.pth"), ("resnet34", "resnet34-b627a593.pth")):
        if not os.path.isfile(os.path.join(torch.hub.get_dir(), "checkpoints", hub)):
            with pytest.raises(NotImplementedError, match=hub):
                Baseline(arch)
            with pytest.raises(RuntimeError, match=hub):  # NotImplementedError is a RuntimeError: existing handlers hold
                getattr(resnet, arch)(weights="IMAGENET1K_V1")
        m = Baseline(arch, None)
        m.freeze_backbone()
        assert sum(p.requires_grad for p in m.parameters()) == 16
    assert Baseline("resnet50").classifier[0].in_features == 4096  # Bottleneck default unchanged: random weights


def test_other_models_accept_the_basicblock_archs():
    from src.models.simclr import SimCLR, SimCLRSkinV3, SimCLRSkinV32
    assert SimCLR("resnet18").encoder_out_dim == 512
    assert SimCLRSkinV3("resnet34", None, 64).cross_proj[0].in_features == 512
    assert SimCLRSkinV32("resnet18", None, 128, 0.1, metadata_dim=20).meta_proj[6].out_features == 128


def test_basicblock_encoder_plan():
    from sm3hip.engine import EncoderPlan, SM3Engine
    from src.models.simclr import SimCLRSkinV3, SimCLRSkinV32
    plan = EncoderPlan("enc.", (2, 2, 2, 2), "basic")
    assert plan.basic and plan.out_dim == 512 and len(plan.blocks) == 8
    names = [[blk[k].name for k in ("c1", "c2", "cd") if k in blk] for blk in plan.blocks]
    assert names[0] == ["enc.layer1.0.conv1", "enc.layer1.0.conv2"]
    assert names[2] == ["enc.layer2.0.conv1", "enc.layer2.0.conv2", "enc.layer2.0.downsample.0"]
    assert [("cd" in b) for b in plan.blocks] == [False, False, True, False, True, False, True, False]
    assert all("c3" not in b and "b3" not in b for b in plan.blocks)
    for bi, (ci, co, s) in enumerate([(64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1),
                                      (256, 512, 2), (512, 512, 1)]):
        c1, c2 = plan.blocks[bi]["c1"], plan.blocks[bi]["c2"]
        assert (c1.Ci, c1.Co, c1.k, c1.stride, c1.pad) == (ci, co, 3, s, 1)
        assert (c2.Ci, c2.Co, c2.k, c2.stride, c2.pad) == (co, co, 3, 1, 1)
        if "cd" in plan.blocks[bi]:
            cd = plan.blocks[bi]["cd"]
            assert (cd.Ci, cd.Co, cd.k, cd.stride, cd.pad) == (ci, co, 1, 2, 0)
            assert plan.blocks[bi]["bd"].name == f"enc.layer{bi // 2 + 1}.0.downsample.1"
    assert len(EncoderPlan("", (3, 4, 6, 3), "basic").blocks) == 16
    # the Bottleneck plan is unchanged: a downsample in every stage's first block, 2048 features
    r50 = EncoderPlan("", (3, 4, 6, 3))
    assert not r50.basic and r50.out_dim == 2048 and [("cd" in b) for b in r50.blocks].count(True) == 4
    assert "cd" in r50.blocks[0] and r50.blocks[0]["cd"].stride == 1
    # the engine sizes every projector from the encoder
    eng = SM3Engine(SimCLRSkinV32("resnet18", None, 128, 0.1), torch.float32, "v32")
    assert all(eng.branches[k][0].basic and eng.branches[k][1].l0.Ci == 512 for k in ("derm", "clinic"))
    assert eng.cross[0].l0.Ci == eng.cross[1].l0.Ci == 512
    assert SM3Engine(SimCLRSkinV3("resnet34", None, 128), torch.float32, "v3").cross[0].l0.Ci == 512
    assert SM3Engine(SimCLRSkinV32("resnet50", None, 128, 0.1), torch.float32, "v32").cross[0].l0.Ci == 2048


def test_backbone_tools_parse_the_basicblock_archs():
    for name in ("backbone_train", "backbone_eval"):
        parser = _tool(name).get_parser()
        for arch in ("resnet18", "resnet34"):
            assert parser.parse_args(["-a", arch, "--data-name", "synthetic", "--data-path", "-"]).arch == arch
        assert parser.parse_args(["--data-name", "synthetic", "--data-path", "-"]).arch == "resnet50"  # default kept


def test_multilabel_tools_reject_the_basicblock_archs_cleanly():
    mlc_eval = _tool("mlc_eval")
    with pytest.raises(SystemExit, match="2048-wide"):
        mlc_eval.main(["-a", "resnet18", "--data-name", "synthetic", "--data-path", "-"])
    mlc_train = _tool("mlc_train")
    args = mlc_train.get_parser().parse_args(["-a", "resnet34", "--data-name", "synthetic", "--data-path", "-"])
    args.world_size = 1
    with pytest.raises(SystemExit, match="2048-wide"):
        mlc_train.main(0, args)
    import inference
    with pytest.raises(NotImplementedError, match="2048-wide"):
        inference.build_model("resnet18")
