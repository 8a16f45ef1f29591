"""--mlc-proj v0..v4 without a GPU: the label-projector classes carry the reference's state_dict keys and shapes
(tests/golden/mlc_proj_state_dict_shapes.json, written from the reference's own src/models/projector.py), the tools' parsers
take every kind, and unknown kinds and a v0 whose width is not the feature width are rejected before any kernel runs."""
import importlib.util
import json
import os

import pytest

from src.models import projector as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "skin-sm3_amd", "tools")


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_cpu_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind", ["v1", "v2", "v3", "v4"])
@pytest.mark.parametrize("dims", [(64, 32), (4096, 512)])
def test_projector_keys_and_shapes_equal_the_reference(kind, dims):
    want = json.load(open(os.path.join(GOLDEN, "mlc_proj_state_dict_shapes.json")))[f"{kind}_{dims[0]}_{dims[1]}"]
    got = [[k, list(v.shape)] for k, v in P.build_mlc_projectors(kind, dims[0], dims[1], 8).state_dict().items()]
    assert got == want


def test_v1_buffer_keys_as_in_reference_checkpoints():
    sd = P.MultiLabelProjector(64, 32, 8).state_dict()
    assert "projectors.3.1.running_var" in sd and "projectors.3.7.num_batches_tracked" in sd
    assert "projectors.3.7.weight" not in sd          # the last BatchNorm1d is affine=False


def test_v0_is_identity_and_checks_its_width():
    import torch.nn as nn
    assert isinstance(P.build_mlc_projectors("v0", 4096, 4096, 8), nn.Identity)
    with pytest.raises(ValueError, match="feature width"):
        P.build_mlc_projectors("v0", 4096, 512, 8)
    with pytest.raises(ValueError, match="v5"):
        P.build_mlc_projectors("v5", 4096, 512, 8)


@pytest.mark.parametrize("tool", ["mlc_train", "mlc_eval"])
@pytest.mark.parametrize("kind", ["v0", "v1", "v2", "v3", "v4"])
def test_parsers_accept_every_kind(tool, kind):
    from src.utils.misc import require_mlc_proj
    mod = _tool(tool)
    args = mod.get_parser().parse_args(["--data-name", "synthetic", "--data-path", "-", "--mlc-proj", kind, "--mlc-proj-dim",
                                        "4096" if kind == "v0" else "512"])
    assert args.mlc_proj == kind
    require_mlc_proj(args, tool)  # no exit
    assert mod.get_parser().parse_args(["--data-name", "synthetic", "--data-path", "-"]).mlc_proj == "v4"


@pytest.mark.parametrize("tool", ["mlc_train", "mlc_eval"])
@pytest.mark.parametrize("argv,msg", [(["--mlc-proj", "v7"], "not one of"),
                                      (["--mlc-proj", "v0", "--mlc-proj-dim", "512"], "must be 4096"),
                                      (["--num-labels", "7"], "8 labels")])
def test_tools_reject_bad_projector_choices_up_front(tool, argv, msg, monkeypatch):
    import torch
    mod = _tool(tool)
    # nothing may reach a device: any attempt fails the test rather than running a kernel
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("device touched before the check"))
    base = ["--data-name", "synthetic", "--data-path", "-"] + argv
    with pytest.raises(SystemExit, match=msg):
        if tool == "mlc_train":
            args = mod.get_parser().parse_args(base)
            args.world_size = 1
            mod.main(0, args)
        else:
            mod.main(base)
