"""CPU: what tools/eval_cli.py gives the evaluation tools that needs no device -- the optional-report registry on every tool's
parser, its refusals, the order and prefix of the optional lines, and encode's concatenation.  No GPU use."""
import argparse
import importlib.util
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_eval_cli_cpu_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _eval_cli():
    _tool("backbone_eval")  # puts the tools' directory on sys.path, as every tool does
    import eval_cli
    return eval_cli


def _flags(module):
    """The option strings module.add_flags gives a parser."""
    p = argparse.ArgumentParser(add_help=False)
    module.add_flags(p)
    return {s for a in p._actions for s in a.option_strings}


def test_registry_order_and_entries():
    ec = _eval_cli()
    assert [flag for flag, _, _ in ec.REPORTS] == ["calibration", "operating", "checklist"]
    for flag, module, validation in ec.REPORTS:
        assert "--" + flag in _flags(module) and callable(getattr(module, validation)) and callable(module.stats_line)


@pytest.mark.parametrize("name", ["backbone_eval", "mlc_eval", "backbone_logreg", "eval_report", "backbone_knn"])
def test_every_tool_parser_has_the_registry_flags(name):
    ec = _eval_cli()
    have = {s for a in _tool(name).get_parser()._actions for s in a.option_strings}
    for flag, module, _ in ec.REPORTS:
        if name == "backbone_knn" and flag == "calibration":  # its votes are not logits
            assert not _flags(module) & have
        else:
            assert _flags(module) <= have, (name, flag)


@pytest.mark.parametrize("bad, text", [(["--calib-bins", "0"], "--calib-bins"), (["--operating-rule", "best"], "--operating-rule"),
                                       (["--checklist-thresholds", "0"], "--checklist-thresholds")])
def test_check_report_flags_refuses_without_the_device(monkeypatch, bad, text):
    ec = _eval_cli()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))
    parser = ec.add_report_flags(argparse.ArgumentParser())
    ec.check_report_flags(parser.parse_args([]))
    with pytest.raises(ValueError, match=text):  # the modules' own refusal, which the tools let through as it is
        ec.check_report_flags(parser.parse_args(bad))
    if "--calib-bins" in bad:  # backbone_knn's case: calibration's flags are neither added nor checked
        ec.check_report_flags(argparse.Namespace(**{k: v for k, v in vars(parser.parse_args([])).items()
                                                    if not k.startswith("calib")}), calibration=False)


@pytest.mark.parametrize("on", [(), ("checklist",), ("operating", "checklist"), ("calibration", "operating", "checklist"),
                                ("checklist", "calibration")])
def test_optional_reports_runs_the_set_flags_in_registry_order(monkeypatch, capsys, on):
    ec = _eval_cli()
    calls = []
    for flag, module, validation in ec.REPORTS:
        monkeypatch.setattr(module, validation, lambda *a, _flag=flag: calls.append((_flag,) + a))
    args = argparse.Namespace(**{flag: True for flag in on})  # a flag the parser lacks (backbone_knn) counts as not set
    preds, targets = [object()], object()
    got = ec.optional_reports("tool x: ", preds, targets, args, "somewhere")
    want = [flag for flag, _, _ in ec.REPORTS if flag in on]
    assert calls == [(flag, preds, targets, args, "somewhere") for flag in want]
    assert got == {flag: None for flag in want} and list(got) == want
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["tool x: " + module.stats_line(None) for flag, module, _ in ec.REPORTS if flag in on]


def test_encode_concatenates_the_two_backbones_as_float32():
    ec = _eval_cli()
    evaluator = types.SimpleNamespace(derm_backbone=lambda x: (x.flatten(1) * 2).half(),
                                      clinic_backbone=lambda x: (x.flatten(1)[:, :3] - 1).half())
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(n, 2, 2, generator=g), torch.randn(n, 2, 2, generator=g), torch.randint(0, 3, (n, 8), generator=g))
               for n in (3, 1, 2)]
    feats, labels = ec.encode(evaluator, iter(batches))
    want = torch.cat([torch.cat([evaluator.derm_backbone(d), evaluator.clinic_backbone(c)], dim=1) for d, c, _ in batches])
    assert feats.dtype == torch.float32 and feats.shape == (6, 7) and feats.is_contiguous()
    assert torch.equal(feats, want.float()) and torch.equal(labels, torch.cat([lab for _, _, lab in batches]))
