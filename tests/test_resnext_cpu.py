"""ResNeXt encoders (CPU): model mirrors, state_dict layout against the reference's, the engine's plan, the tools' arch
handling, and the host-side argument checks of the grouped-convolution entry points (nothing is launched)."""
import ctypes as C
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
RESNEXTS = {  # arch: (block counts, groups, width per group)
    "resnext50_32x4d": ([3, 4, 6, 3], 32, 4),
    "resnext101_32x8d": ([3, 4, 23, 3], 32, 8),
    "resnext101_64x4d": ([3, 4, 23, 3], 64, 4),
}


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_rxcpu_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("arch", list(RESNEXTS))
def test_resnext_constructors_layer_layout(arch):
    from src.models import resnet
    counts, groups, wpg = RESNEXTS[arch]
    m = resnet.__dict__[arch]()
    assert m.block_type == "bottleneck" and m.block_counts == counts and (m.groups, m.base_width) == (groups, wpg)
    assert m.fc.in_features == 2048
    for li, planes in enumerate((64, 128, 256, 512), start=1):
        layer = getattr(m, f"layer{li}")
        assert len(layer) == counts[li - 1]
        width = int(planes * wpg / 64) * groups
        for bi, blk in enumerate(layer):
            assert blk.conv1.out_channels == width
            assert blk.conv2.groups == groups and tuple(blk.conv2.weight.shape) == (width, width // groups, 3, 3)
            assert blk.conv2.stride == ((2, 2) if bi == 0 and li > 1 else (1, 1))
            assert tuple(blk.conv3.weight.shape) == (planes * 4, width, 1, 1)
            assert (blk.downsample is not None) == (bi == 0)


def test_resnext50_state_dict_matches_the_reference_lists():
    from src.models.simclr import SimCLRSkinV32
    sd = SimCLRSkinV32("resnext50_32x4d", None, 128, 0.1).state_dict()
    keys = open(os.path.join(GOLDEN, "rx50_state_dict_keys.txt")).read().split()
    assert list(sd.keys()) == keys
    shapes = json.load(open(os.path.join(GOLDEN, "rx50_state_dict_shapes.json")))
    assert [[k, list(v.shape)] for k, v in sd.items()] == shapes


def test_basicblock_refuses_groups_and_wide_resnets_are_refused():
    from src.models import resnet
    with pytest.raises(ValueError, match="groups=1 and base_width=64"):
        resnet.BasicBlock(64, 64, groups=2)
    with pytest.raises(ValueError, match="groups=1 and base_width=64"):
        resnet.BasicBlock(64, 64, base_width=128)
    for arch in ("wide_resnet50_2", "wide_resnet101_2"):
        with pytest.raises(NotImplementedError, match="wide ResNets"):
            resnet.__dict__[arch]()
    with pytest.raises(NotImplementedError, match="wide ResNets"):
        resnet.ResNet(resnet.Bottleneck, [3, 4, 6, 3], width_per_group=128)


def test_uncached_resnext_weights_raise_not_implemented(tmp_path, monkeypatch):
    from src.models import resnet
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))
    for arch, hub in (("resnext50_32x4d", "resnext50_32x4d-7cdf4587.pth"), ("resnext101_32x8d", "resnext101_32x8d-8ba56ff5.pth"),
                      ("resnext101_64x4d", "resnext101_64x4d-173b62eb.pth")):
        with pytest.raises(NotImplementedError, match=hub):
            resnet.__dict__[arch](weights="IMAGENET1K_V1")


@pytest.mark.parametrize("arch", list(RESNEXTS))
def test_resnext_encoder_plan(arch):
    from sm3hip.engine import SM3Engine
    from src.models.simclr import SimCLRSkinV32
    counts, groups, wpg = RESNEXTS[arch]
    eng = SM3Engine(SimCLRSkinV32(arch, None, 128, 0.1), torch.float32, "v32")
    plan = eng.branches["derm"][0]
    assert not plan.basic and plan.out_dim == 2048 and len(plan.blocks) == sum(counts)
    assert eng.branches["derm"][1].l0.Ci == eng.cross[0].l0.Ci == 2048
    bi = 0
    inpl = 64
    for li, planes in enumerate((64, 128, 256, 512), start=1):
        width = int(planes * wpg / 64) * groups
        for b in range(counts[li - 1]):
            blk = plan.blocks[bi]
            s = 2 if (b == 0 and li > 1) else 1
            c1, c2, c3 = blk["c1"], blk["c2"], blk["c3"]
            assert (c1.Ci, c1.Co, c1.k, c1.groups) == (inpl if b == 0 else planes * 4, width, 1, 1)
            assert (c2.Ci, c2.Co, c2.k, c2.stride, c2.pad, c2.groups) == (width, width, 3, s, 1, groups)
            assert (c3.Ci, c3.Co, c3.groups) == (width, planes * 4, 1)
            assert blk["b2"].C == width and c2.name == f"derm_backbone.encoder.layer{li}.{b}.conv2"
            assert ("cd" in blk) == (b == 0)
            bi += 1
        inpl = planes * 4
    # the plain ResNet-50 plan is unchanged: no grouped unit
    r50 = SM3Engine(SimCLRSkinV32("resnet50", None, 128, 0.1), torch.float32, "v32").branches["derm"][0]
    assert all(cu.groups == 1 for cu in r50.conv_units())


def test_tools_accept_resnext_and_backbone_eval_refuses_it():
    for name in ("backbone_train", "backbone_eval", "mlc_train"):
        parser = _tool(name).get_parser()
        assert parser.parse_args(["-a", "resnext50_32x4d", "--data-name", "synthetic", "--data-path", "-"]).arch == \
            "resnext50_32x4d"
    from src.utils.misc import MLC_ARCHS, require_mlc_arch
    for arch in RESNEXTS:
        assert arch in MLC_ARCHS
        require_mlc_arch(arch, "mlc_train")  # no SystemExit
    import inference
    assert inference.build_model("resnext50_32x4d").extractor.derm_feat_dim == 2048
    be = _tool("backbone_eval")
    import sys
    argv = sys.argv
    sys.argv = ["backbone_eval.py", "-a", "resnext50_32x4d", "--data-name", "synthetic", "--data-path", "-"]
    try:
        with pytest.raises(SystemExit, match="plain ResNets"):
            be.main()
    finally:
        sys.argv = argv


def test_grouped_conv_entry_points_reject_bad_arguments():
    """Host-side validation returns SM3_EINVAL / SM3_EALIGN / SM3_EDTYPE before anything is launched."""
    from sm3hip import _lib
    lib = _lib.load()
    buf = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    null = None
    # null pointers
    assert lib.sm3_gconv_fwd(1, null, buf, buf, null, 2, 8, 8, 128, 32, 1, null) == -1
    assert lib.sm3_gconv_dgrad(1, buf, null, buf, 2, 8, 8, 128, 32, 1, null) == -1
    assert lib.sm3_gconv_wgrad_det(1, buf, buf, null, buf, 8, 2, 8, 8, 128, 32, 1, null) == -1
    assert lib.sm3_gconv_weight_prep(1, null, buf, buf, 128, 32, null, null) == -1
    # group sizes outside {4, 8, 16, 32, 64}, widths not divisible, bad stride, empty maps, no slab room
    assert lib.sm3_gconv_fwd(1, buf, buf, buf, null, 2, 8, 8, 128, 64, 1, null) == -1     # cg = 2
    assert lib.sm3_gconv_fwd(1, buf, buf, buf, null, 2, 8, 8, 4096, 32, 1, null) == -1    # cg = 128
    assert lib.sm3_gconv_fwd(1, buf, buf, buf, null, 2, 8, 8, 130, 32, 1, null) == -1     # C % groups
    assert lib.sm3_gconv_fwd(1, buf, buf, buf, null, 2, 8, 8, 128, 32, 3, null) == -1     # stride 3
    assert lib.sm3_gconv_dgrad(1, buf, buf, buf, 0, 8, 8, 128, 32, 2, null) == -1         # N = 0
    assert lib.sm3_gconv_wgrad_det(1, buf, buf, buf, buf, 0, 2, 8, 8, 128, 32, 1, null) == -1  # capacity 0
    assert lib.sm3_gconv_wgrad_slabs(2, 8, 8, 3, 8) == -1
    # dtype and alignment
    assert lib.sm3_gconv_fwd(7, buf, buf, buf, null, 2, 8, 8, 128, 32, 1, null) == -3
    assert lib.sm3_gconv_fwd(1, buf, buf, buf, null, 2, 8, 8, 96, 24, 1, null) == -2      # C % 64
    assert lib.sm3_gconv_fwd(1, C.c_void_p(18), buf, buf, null, 2, 8, 8, 128, 32, 1, null) == -2
    # the slab partition is a function of the geometry and the capacity
    assert lib.sm3_gconv_wgrad_slabs(2, 56, 56, 1, 512) == lib.sm3_gconv_wgrad_slabs(2, 56, 56, 1, 512) == 98
    assert lib.sm3_gconv_wgrad_slabs(2, 8, 8, 2, 512) == 1
