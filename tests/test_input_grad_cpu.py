"""CPU: the image-gradient entry point (sm3_stem_dgrad_bn) in the header, the binding and the library, its host-side
refusals, and tools/backbone_saliency.py's parser and refusals -- each before anything touches the GPU."""
import ctypes as C
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def _lib():
    from sm3hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_point_is_declared_bound_and_exported():
    from sm3hip import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sm3_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sm3_stem_dgrad_bn\s*\(", text)
    assert "sm3_stem_dgrad_bn" in L.SIGNATURES
    lib = _lib()
    assert hasattr(lib, "sm3_stem_dgrad_bn")
    assert lib.sm3_abi_version() == 9


def _call(lib, dtype=1, dz=0x1000, xo=0x2000, mean=0x3000, invstd=0x4000, gamma=0x5000, gsums=0x6000, count=8.0,
          w=0x7000, dx=0x8000, N=2, H=8, W=8, views=1):
    p = lambda v: C.c_void_p(v) if v else C.c_void_p(0)
    return lib.sm3_stem_dgrad_bn(dtype, p(dz), p(xo), p(mean), p(invstd), p(gamma), p(gsums), float(count), p(w), p(dx),
                                 N, H, W, views, C.c_void_p(0))


@pytest.mark.parametrize("kw,code", [
    (dict(dz=0), -1), (dict(xo=0), -1), (dict(mean=0), -1), (dict(invstd=0), -1), (dict(gsums=0), -1), (dict(w=0), -1),
    (dict(dx=0), -1), (dict(count=0.0), -1), (dict(count=float("nan")), -1), (dict(views=0), -1), (dict(N=3, views=2), -1),
    (dict(N=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(N=2 ** 20, H=2048, W=2048), -1),
    (dict(dtype=7), -3), (dict(dz=0x1008), -2), (dict(xo=0x2004), -2)])
def test_abi_rejects_bad_arguments_before_any_launch(kw, code):
    assert _call(_lib(), **kw) == code, kw


def _tool():
    spec = importlib.util.spec_from_file_location("sm3_saliency_cpu", os.path.join(TOOLS, "backbone_saliency.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parser_takes_backbone_eval_line_and_the_saliency_flags():
    bs = _tool()
    a = bs.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.target, a.split, a.max_cases, a.linear_path, a.arch) == ("pred", "test", 64, None, "resnet50")
    a = bs.get_parser().parse_args(["--data-path", "x", "--data-name", "SevenPCBaseDataset", "--target", "cls",
                                    "--split", "valid", "--max-cases", "5", "--linear-path", "p.pth", "-a", "resnet18", "--img-sz", "64", "96", "--amp",
                                    "--amp-dtype", "bf16"])
    assert (a.target, a.split, a.max_cases, a.linear_path, a.arch, a.img_sz) == ("cls", "valid", 5, "p.pth", "resnet18",
                                                                                   [64, 96])


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that reaches for the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("touched the GPU before refusing")
    monkeypatch.setattr(torch, "Generator", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    monkeypatch.setattr(torch.nn.Module, "to", boom)


@pytest.mark.parametrize("argv,msg", [
    (["--data-name", "synthetic", "--data-path", "-", "--linear-path", "/nonexistent/best_linear.pth"], "does not exist"),
    (["--data-name", "synthetic", "--data-path", "-", "-a", "resnext50_32x4d"], "not supported"),
    (["--data-name", "synthetic", "--data-path", "-", "--max-cases", "0"], "max-cases"),
    (["--data-name", "ImageNet", "--data-path", "-"], "not available"),
])
def test_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    bs = _tool()
    with pytest.raises(SystemExit, match=msg):
        bs.main(argv + ["--log-path", str(tmp_path)])


def test_real_data_needs_a_linear_probe(no_gpu, tmp_path):
    root = tmp_path / "7PC"
    os.makedirs(root / "images")
    for f in ("meta.csv", "train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        (root / f).write_text("")
    bs = _tool()
    with pytest.raises(SystemExit, match="linear-path"):
        bs.main(["--data-name", "SevenPCBaseDataset", "--data-path", str(root), "--log-path", str(tmp_path)])


def test_unknown_target_is_an_argument_error(no_gpu, capsys):
    bs = _tool()
    with pytest.raises(SystemExit) as e:
        bs.main(["--data-name", "synthetic", "--data-path", "-", "--target", "saliency"])
    assert e.value.code == 2 and "--target" in capsys.readouterr().err
