"""GPU: the calibration report (csrc/calib.hip, sm3hip/calibration.py, the evaluation tools and tools/eval_report.py).

  * sm3_calib_counts equal (==) to the integer restatement of tests/test_calib_cpu.py, bins and sums: the point table and
    replicate tables, N from a lone case over one wave +- 1 and the scan tiles +- 1 to MAX_CASES, M in {1, 2, 15, 64} and M = N
    (M > N leaves empty bins), both binnings, heavily tied and all-equal scores (ties by case index), q = 0 and q = 2^32, seeds
    that use both key words, replicate offsets up to 2^20, a replicate range cut into launches in several ways; the output
    pre-filled with a sentinel and every element overwritten;
  * replicate r resamples the cases of replicate r of sm3_report_counts: sum_b E_b of a class-wise series == P of its column,
    and sum_b n_b == N for every series;
  * the library: equal bits across calls and chunks, a prefix of a longer bootstrap, temperature of all ones == None, the
    replicates are the restatement's values, intervals by report.interval;
  * argument errors return SM3_EINVAL and leave the sentinel output untouched (nothing here provokes a device fault);
  * the tools: --calibration of backbone_eval / mlc_eval writes val_calibration.json / .csv equal to calibration_report of the
    predictions, eval_report.py --calibration / --fit-on."""
import csv
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
DEV = "cuda:0"
SENTINEL = -0x0123456789ABCDEF
SEEDS = ((7, 0, 1), (2 ** 32 + 5, 1000, 3), (2 ** 63 + 11, 2 ** 20 - 3, 20))     # (seed, r0, c)


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REF = _load("sm3_calib_ref", os.path.join(ROOT, "tests", "test_calib_cpu.py"))  # bin_tables, plain_sums, multiplicities, make_case


def _tool(name):
    return _load("sm3_calib_gpu_" + name, os.path.join(TOOLS, name + ".py"))


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
def _case(N, kind, seed):
    """Logits with the edge scores in: rows certain of one class (q = 2^32 and q = 0 in the class-wise series)."""
    preds, targets = REF.make_case(N, kind, seed)
    if kind != "equal":
        for t, p in enumerate(preds):
            p[::7, t % p.shape[1]] = 2000.0
    return preds, targets


def _device_inputs(preds, targets, temperature=None):
    from sm3hip import calibration
    q, ev, xq = calibration.fixed_point([p.to(DEV) for p in preds], targets.to(DEV), temperature)
    order = torch.sort(q, dim=1, stable=True).indices.int().contiguous()
    slabel = torch.tensor(calibration.SERIES_LABEL, dtype=torch.int32, device=DEV)
    return q, ev, order, slabel, xq


def _device_counts(inp, M, binning, seed, r0, c, point=False):
    from sm3hip import ops
    bins = torch.full((c, 32, M, 3), SENTINEL, dtype=torch.int64, device=DEV)
    sums = torch.full((c, 16), SENTINEL, dtype=torch.int64, device=DEV)
    ops.calib_counts(*inp, bins, sums, 8, binning, seed, r0, point=point)
    torch.cuda.synchronize()
    bins, sums = bins.cpu().numpy(), sums.cpu().numpy()
    assert not (bins == SENTINEL).any() and not (sums == SENTINEL).any()              # every element is overwritten
    return bins, sums


def _host(inp):
    q, ev, order, _, xq = (a.cpu().numpy().astype(np.int64) for a in inp)
    return q, ev, order, xq


def _want(host, m, M, binning):
    q, ev, order, xq = host
    return REF.bin_tables(q, ev, order, m, M, binning), REF.plain_sums(xq, m)


def _max_cases():
    from sm3hip import report
    return report.MAX_CASES


@pytest.mark.parametrize("N", [1, 2, 5, 63, 64, 65, 255, 257, 395, 1023, 1025, "MAX_CASES"])
def test_counts_equal_the_integer_restatement(N):
    big = N == "MAX_CASES"
    N = _max_cases() if big else N
    assert N == 8192 or not big
    for kind, (seed, r0, c) in zip(("ties", "equal", "random"), SEEDS):
        inp = _device_inputs(*_case(N, kind, 7 * N + len(kind)))
        host = _host(inp)
        if kind != "equal":
            assert (host[0] == 0).any() and (host[0] == 1 << 32).any()
        c = min(c, 2) if big else c                                                   # the host restatement is the slow side
        for binning in ("width", "mass"):
            for M in sorted({1, 2, 15, 64} | ({N} if N <= 64 else set())):
                bins, sums = _device_counts(inp, M, binning, seed, 0, 1, point=True)
                wb, ws = _want(host, np.ones(N, dtype=np.int64), M, binning)
                assert np.array_equal(bins[0], wb) and np.array_equal(sums[0], ws), (kind, binning, M, "point")
                bins, sums = _device_counts(inp, M, binning, seed, r0, c)
                for j in (range(c) if c <= 3 else (0, 1, 11, c - 1)):
                    wb, ws = _want(host, REF.multiplicities(seed, r0 + j, N), M, binning)
                    assert np.array_equal(bins[j], wb) and np.array_equal(sums[j], ws), (kind, binning, M, seed, r0 + j)
                assert (bins[..., 0].sum(axis=2) == N).all()
                if M > N:
                    assert (bins[..., 0] == 0).any()                                  # empty bins
                if not big and M == 15:                                               # any cut of [r0, r0 + c) is the one call
                    for step in (1, 7):
                        parts = [_device_counts(inp, M, binning, seed, r0 + k, min(step, c - k)) for k in range(0, c, step)]
                        assert np.array_equal(np.concatenate([p[0] for p in parts]), bins)
                        assert np.array_equal(np.concatenate([p[1] for p in parts]), sums)
        if not big:                                                                   # every seed, offset and count on this input
            for s2, r2, c2 in SEEDS:
                bins, sums = _device_counts(inp, 15, "mass", s2, r2, c2)
                wb, ws = _want(host, REF.multiplicities(s2, r2 + c2 - 1, N), 15, "mass")
                assert np.array_equal(bins[c2 - 1], wb) and np.array_equal(sums[c2 - 1], ws), (kind, s2, r2)


def test_replicates_resample_the_cases_of_the_evaluation_report():
    from sm3hip import ops, report
    for N, seed, r0 in ((395, 2 ** 63 + 11, 5), (65, 7, 2 ** 20)):
        preds, targets = _case(N, "ties", N)
        dp, dt = [p.to(DEV) for p in preds], targets.to(DEV)
        order, gs, ge, yhat = report.ranking(dp, dt)
        colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV)
        counts = torch.empty((4, 24, 6), dtype=torch.int64, device=DEV)
        ops.report_counts(order, gs, ge, dt.int().contiguous(), yhat, colmap, counts, seed, r0)
        P = counts[:, :, 1].cpu().numpy()
        for binning in ("width", "mass"):
            bins, _ = _device_counts(_device_inputs(preds, targets), 15, binning, seed, r0, 4)
            assert np.array_equal(bins[:, 8:, :, 1].sum(axis=2), P), binning          # positives of column k: the same cases
            assert (bins[:, :, :, 0].sum(axis=2) == N).all()
        assert len({tuple(P[r]) for r in range(4)}) > 1                               # and the replicates differ


def test_argument_errors_leave_the_output_untouched():
    from sm3hip import _lib, ops
    inp = _device_inputs(*_case(5, "ties", 1))
    bins = torch.full((2, 32, 64, 3), SENTINEL, dtype=torch.int64, device=DEV)
    sums = torch.full((2, 16), SENTINEL, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    ptr = [ops._ptr(a) for a in inp[:5]] + [ops._ptr(bins), ops._ptr(sums)]

    def call(N=5, M=15, c=1, binning=0, r0=0, point=0):
        return lib.sm3_calib_counts(*ptr, N, 32, 16, 8, M, binning, 0, r0, c, point, ops._stream())
    for kw in ({"N": 0}, {"N": _max_cases() + 1}, {"M": 0}, {"M": 65}, {"c": 0}, {"binning": 2}, {"r0": -1}, {"point": 1, "c": 2}):
        assert call(**kw) == -1, kw                                                   # SM3_EINVAL
    torch.cuda.synchronize()
    assert bool((bins == SENTINEL).all()) and bool((sums == SENTINEL).all())
    for bad in (dict(bins=bins[:1, :, :15].contiguous(), point=True, seed=2 ** 64), dict(bins=bins[:, :, :15].contiguous(), point=True),
                dict(bins=bins[:1, :31, :15].contiguous()), dict(bins=bins[:1, :, :15].contiguous().cpu()),
                dict(bins=bins[:1, :, :15].contiguous(), binning="quantile")):
        kw = dict(bins=None, sums=sums[:bad["bins"].shape[0]], labels=8, binning="width", seed=0, r0=0, point=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.calib_counts(*inp, **kw)
    with pytest.raises(ValueError):
        ops.calib_counts(inp[0].int(), *inp[1:], bins[:1, :, :15].contiguous(), sums[:1], 8, "width", 0, 0)


# ---- 2. the library ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    preds, targets = REF.make_case(395, "random", 42)
    return [(1.5 * p).to(DEV) for p in preds], targets.to(DEV)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


VALUE_KEYS = ("label_values", "class_values", "diagram")
BOOT_KEYS = tuple(f"{t}_{e}" for t in ("label", "class", "diagram") for e in ("replicates", "lo", "hi"))


@pytest.mark.parametrize("binning", ["width", "mass"])
def test_bits_do_not_depend_on_call_chunk_or_bootstrap_size(case, binning):
    from sm3hip import calibration, report
    preds, targets = case
    before = [p.clone() for p in preds], targets.clone()
    B, kw = 23, dict(binning=binning, seed=2 ** 63 + 11)
    first = calibration.calibration_report(preds, targets, bootstrap=B, **kw)
    assert first["bins"].shape == (32, 15, 3) and first["sums"].shape == (16,) and first["label_values"].shape == (4, 9)
    assert first["class_values"].shape == (1, 29) and first["diagram"].shape == (32, 15, 3)
    assert first["label_replicates"].shape == (B, 4, 9) and first["diagram_replicates"].shape == (B, 32, 15, 3)
    assert first["class_columns"] == report.COLUMNS and first["label_columns"][-1] == "AVG" and len(first["series"]) == 32
    for chunk in (None, 1, 7, B):
        again = calibration.calibration_report(preds, targets, bootstrap=B, chunk=chunk, **kw)
        for key in VALUE_KEYS + BOOT_KEYS:
            assert _same(first[key], again[key]), (chunk, key)
        assert torch.equal(first["bins"], again["bins"]) and torch.equal(first["sums"], again["sums"])
        assert torch.equal(first["diagram_undefined"], again["diagram_undefined"])
    seven = calibration.calibration_report(preds, targets, bootstrap=7, **kw)
    five = calibration.calibration_report(preds, targets, bootstrap=5, **kw)
    for t in ("label", "class", "diagram"):
        assert _same(seven[f"{t}_replicates"][:5].contiguous(), five[f"{t}_replicates"])
        assert _same(first[f"{t}_replicates"][:7].contiguous(), seven[f"{t}_replicates"])
    ones = calibration.calibration_report(preds, targets, temperature=[1.0] * 8, bootstrap=5, **kw)
    for key in VALUE_KEYS + BOOT_KEYS:
        assert _same(ones[key], five[key]), key
    assert torch.equal(ones["bins"], five["bins"]) and ones["temperature"] == [1.0] * 8
    other = calibration.calibration_report(preds, targets, bootstrap=5, binning=binning, seed=2 ** 63 + 12)
    assert not _same(other["label_replicates"], five["label_replicates"]) and _same(other["label_values"], five["label_values"])
    none = calibration.calibration_report(preds, targets, binning=binning)
    assert "label_replicates" not in none and _same(none["label_values"], first["label_values"])
    cpu = calibration.calibration_report([p.cpu() for p in preds], targets.cpu(), binning=binning)   # CPU tensors are moved
    assert torch.equal(cpu["bins"], first["bins"]) and _same(cpu["class_values"], first["class_values"])
    for t in ("label", "class", "diagram"):
        lo, hi = report.interval(first[f"{t}_replicates"].numpy(), 0.95)
        assert np.array_equal(first[f"{t}_lo"].numpy(), lo) and np.array_equal(first[f"{t}_hi"].numpy(), hi)
    assert not first["label_undefined"].any() and not first["class_undefined"].any()
    for p, q in zip(preds + [targets], before[0] + [before[1]]):                      # inputs are not modified
        assert torch.equal(p, q)


def test_replicates_are_the_restatement_through_the_library(case):
    from sm3hip import calibration
    preds, targets = case
    N = targets.shape[0]
    temp = [0.5, 1.0, 2.0, 1.25, 1.0, 3.0, 0.75, 1.0]
    for binning, M in (("width", 15), ("mass", 64)):
        rep = calibration.calibration_report(preds, targets, temperature=temp, bins=M, binning=binning, bootstrap=3, seed=7)
        host = _host(_device_inputs(preds, targets, temp))
        wb, ws = _want(host, np.ones(N, dtype=np.int64), M, binning)
        assert np.array_equal(rep["bins"].numpy(), wb) and np.array_equal(rep["sums"].numpy(), ws)
        label, cw, diagram = REF.values(wb.tolist(), ws.tolist(), N)
        assert rep["label_values"].tolist() == label and rep["class_values"][0, :24].tolist() == cw
        assert rep["diagram"].tolist() == diagram
        for r in range(3):
            wb, ws = _want(host, REF.multiplicities(7, r, N), M, binning)
            label, cw, diagram = REF.values(wb.tolist(), ws.tolist(), N)
            assert rep["label_replicates"][r].tolist() == label and rep["class_replicates"][r, 0, :24].tolist() == cw
            assert rep["diagram_replicates"][r].tolist() == diagram
        empty = sum(int((REF.bin_tables(host[0], host[1], host[2], REF.multiplicities(7, r, N), M, binning)[..., 0] == 0).sum())
                    for r in range(3))
        assert int(rep["diagram_undefined"][..., 1].sum()) == int(rep["diagram_undefined"][..., 2].sum()) == empty
        assert not rep["diagram_undefined"][..., 0].any()
    # a temperature changes the probabilities and neither argmax nor the events
    plain = calibration.calibration_report(preds, targets)
    hot = calibration.calibration_report(preds, targets, temperature=[4.0] * 8)
    assert torch.equal(plain["bins"][:8, :, 1].sum(1), hot["bins"][:8, :, 1].sum(1)) and not torch.equal(plain["sums"], hot["sums"])
    c = calibration.compare(hot, plain)
    assert c["label_delta"].any() and "label_lo" not in c
    with pytest.raises(ValueError, match="binning"):
        calibration.compare(plain, calibration.calibration_report(preds, targets, binning="mass"))


# ---- 3. the tools --------------------------------------------------------------------------------------------------------
def _check_files(log_path, stem, preds, targets, **kw):
    from sm3hip import calibration
    rep = calibration.calibration_report([p.to(DEV) for p in preds], targets.to(DEV), **kw)
    saved = json.load(open(os.path.join(log_path, stem + ".json")))
    for key in VALUE_KEYS:
        assert saved[key] == rep[key].tolist(), key
    assert saved["bins"] == rep["bins"].tolist() and saved["n_bins"] == rep["n_bins"] and saved["binning"] == rep["binning"]
    rows = list(csv.reader(open(os.path.join(log_path, stem + ".csv"))))
    by = {(r[0], r[1], r[2]): r for r in rows[1:]}
    for i, m in enumerate(rep["label_metrics"]):
        for k, c in enumerate(rep["label_columns"]):
            assert float(by[("label", m, c)][3]) == float(rep["label_values"][i, k])
            if kw.get("bootstrap"):
                assert float(by[("label", m, c)][4]) == float(rep["label_lo"][i, k])
    if kw.get("bootstrap"):
        assert saved["label_lo"] == rep["label_lo"].tolist() and saved["bootstrap"] == kw["bootstrap"] and saved["seed"] == kw["seed"]
    return rep


def test_backbone_eval_and_mlc_eval_write_the_calibration_of_the_last_validation_pass(tmp_path, capsys):
    be, me = _tool("backbone_eval"), _tool("mlc_eval")
    hist = be.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "-b", "8", "--img-sz", "64", "64",
                    "--epochs", "2", "--steps-per-epoch", "1", "--val-steps", "3", "--finetune", "fc", "--bootstrap", "16",
                    "--bootstrap-seed", "5", "--confidence", "0.9", "--calibration", "--calib-bins", "10", "--calib-binning", "mass",
                    "--log-path", str(tmp_path / "be")])
    out = capsys.readouterr().out
    assert out.count("ECE_AVG") == 1 and "NLL_AVG" in out and out.count("Recall_AVG") == 2       # the last epoch only
    va = hist[-1][1]
    _check_files(str(tmp_path / "be"), "val_calibration", va["preds"], va["targets"], bins=10, binning="mass", bootstrap=16, seed=5,
                 confidence=0.9)
    assert os.path.isfile(tmp_path / "be" / "val_report.json")
    me.main(["--data-name", "synthetic", "--data-path", "-", "-b", "8", "--img-sz", "64", "64", "--epochs", "1", "--steps-per-epoch", "1",
             "--val-steps", "2", "--mlc-proj-dim", "128", "--sa-dim-ff", "64", "--calibration", "--log-path", str(tmp_path / "me")])
    assert "ECE_AVG" in capsys.readouterr().out
    saved = json.load(open(tmp_path / "me" / "val_calibration.json"))
    assert saved["n"] == 16 and saved["n_bins"] == 15 and saved["binning"] == "width" and "label_lo" not in saved
    assert np.array(saved["diagram"]).shape == (32, 15, 3) and os.path.isfile(tmp_path / "me" / "val_calibration.csv")


def test_eval_report_calibration_and_fit_on(tmp_path, capsys):
    from sm3hip import calibration
    er = _tool("eval_report")
    CPU = _load("sm3_calib_cpu_helpers", os.path.join(ROOT, "tests", "test_calib_cpu.py"))
    val_p, val_t = CPU._sampled_case(300, 1, scale=3.0)               # over-confident logits: the fit is near T = 3
    test_p, test_t = CPU._sampled_case(200, 2, scale=3.0)
    torch.save({"preds": [p.float() for p in val_p], "targets": val_t}, tmp_path / "val_predictions.pt")
    torch.save({"preds": [p.float() for p in test_p], "targets": test_t}, tmp_path / "test_predictions.pt")
    plain = er.main([str(tmp_path / "test_predictions.pt"), "--out", str(tmp_path / "plain")])
    assert sorted(plain) == ["report"] and sorted(os.listdir(tmp_path / "plain")) == ["test_predictions_report.csv",
                                                                                      "test_predictions_report.json"]
    capsys.readouterr()
    res = er.main([str(tmp_path / "test_predictions.pt"), "--fit-on", str(tmp_path / "val_predictions.pt"), "--bootstrap", "20",
                   "--bootstrap-seed", "9", "--calib-bins", "10", "--out", str(tmp_path / "er")])
    out = capsys.readouterr().out
    assert "temperatures fitted on" in out and "fitted - unscaled" in out and "ECE difference" in out and "cwECE" in out
    preds, targets = [p.float() for p in test_p], test_t
    fit = calibration.fit_temperature([p.float() for p in val_p], val_t)
    assert res["fit"] == fit and all(2.0 < v < 4.5 for v in fit["temperature"]) and not any(fit["clipped"])
    kw = dict(bins=10, binning="width", bootstrap=20, seed=9)
    a = _check_files(str(tmp_path / "er"), "test_predictions_calibration", preds, targets, **kw)
    b = _check_files(str(tmp_path / "er"), "test_predictions_calibration_fitted", preds, targets, temperature=fit["temperature"], **kw)
    want = calibration.compare(b, a)
    assert torch.equal(res["calibration_compare"]["label_delta"], want["label_delta"])
    assert torch.equal(res["calibration_compare"]["class_lo"], want["class_lo"])
    saved = json.load(open(tmp_path / "er" / "test_predictions_calibration_compare.json"))
    assert saved["label_delta"] == want["label_delta"].tolist() and saved["fit"]["temperature"] == fit["temperature"]
    # the fitted temperature lowers the NLL of held-out data drawn the same way, and leaves the report's AUC alone
    assert float(want["label_delta"][0, 8]) < 0.0 and float(want["label_hi"][0, 8]) < 0.0
    assert torch.equal(res["report"]["values"], plain["report"]["values"])
