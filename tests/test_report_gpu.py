"""GPU: the evaluation report (csrc/report.hip, sm3hip/report.py, the evaluation tools and tools/eval_report.py).

  * sm3_report_counts equal (==) to the integer restatement of tests/test_report_cpu.py: the point table and replicate tables,
    N from a lone case over one wave +- 1 and the scan tiles +- 1 to MAX_CASES, seeds that use both key words, replicate
    offsets up to 2^20, inputs with heavy ties, an absent class and a label predicted as one class throughout; every output
    element overwritten;
  * values and replicates bit-equal across repeated calls and chunks, and a prefix of a longer bootstrap;
  * point values == metrics.auc_avg on the same predictions; compare(a, a) all zeros; inputs not modified;
  * the tools on synthetic data and on a derm7pt-shaped tree: the new keys equal evaluation_report of the saved predictions,
    AUC_AVG and val_predictions.pt as before, val_report.csv parses back to the values, eval_report.py --against."""
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


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REF = _load("sm3_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))  # multiplicities, counts, make_case
KNN = _load("sm3_report_knn_helpers", os.path.join(ROOT, "tests", "test_knn_gpu.py"))  # _write_tree


def _tool(name):
    return _load("sm3_report_gpu_" + name, os.path.join(TOOLS, name + ".py"))


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
def _device_inputs(preds, targets):
    from sm3hip import report
    dp, dt = [p.to(DEV) for p in preds], targets.to(DEV)
    order, gs, ge, yhat = report.ranking(dp, dt)
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV)
    return order, gs, ge, dt.int().contiguous(), yhat, colmap


def _device_counts(inp, seed, r0, c, point=False):
    from sm3hip import ops
    out = torch.full((c, 24, 6), SENTINEL, dtype=torch.int64, device=DEV)
    ops.report_counts(*inp, out, seed, r0, point=point)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got == SENTINEL).any()                                                # every element is overwritten
    return got


def _host(inp):
    order, gs, ge, y, yhat, _ = (a.cpu().numpy().astype(np.int64) for a in inp)
    return order, gs, ge, y, yhat


def _max_cases():
    from sm3hip import report
    return report.MAX_CASES


@pytest.mark.parametrize("N", [1, 2, 5, 63, 64, 65, 255, 257, 1000, "MAX_CASES"])
def test_counts_equal_the_integer_restatement(N):
    big = N == "MAX_CASES"
    N = _max_cases() if big else N
    runs = ((7, 0, 1), (2 ** 32 + 5, 1000, 3), (2 ** 63 + 11, 2 ** 20 - 3, 70))
    for kind, run in zip(("ties", "absent", "constant"), runs):
        seed, r0, c = run
        c = 3 if big else c                                                           # the host restatement is the slow side
        inp = _device_inputs(*REF.make_case(N, kind, 7 * N + len(kind)))
        host = _host(inp)
        point = _device_counts(inp, seed, 0, 1, point=True)
        assert np.array_equal(point[0], REF.counts(*host, np.ones(N, dtype=np.int64))), (kind, "point")
        got = _device_counts(inp, seed, r0, c)
        for j in (range(c) if c <= 3 else (0, 1, 33, 69)):
            want = REF.counts(*host, REF.multiplicities(seed, r0 + j, N))
            assert np.array_equal(got[j], want), (kind, seed, r0 + j)
        if not big:                                                                   # any cut of [r0, r0 + c) is the one call
            parts = [_device_counts(inp, seed, r0 + k, min(8, c - k)) for k in range(0, c, 8)]
            assert np.array_equal(np.concatenate(parts), got)
            for s2, r2, c2 in runs:                                                   # every seed, offset and count on this input
                g2 = _device_counts(inp, s2, r2, c2)
                assert np.array_equal(g2[c2 - 1], REF.counts(*host, REF.multiplicities(s2, r2 + c2 - 1, N))), (kind, s2, r2)


def test_wrapper_refuses_what_the_kernel_does_not_take():
    from sm3hip import ops
    inp = list(_device_inputs(*REF.make_case(5, "ties", 1)))
    out = torch.zeros(2, 24, 6, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ops.report_counts(*inp, out, 0, 0, point=True)                                # the point estimate is one table
    with pytest.raises(ValueError):
        ops.report_counts(*inp, out, 2 ** 64, 0)
    with pytest.raises(ValueError):
        ops.report_counts(inp[0].long(), *inp[1:], out, 0, 0)
    with pytest.raises(ValueError):
        ops.report_counts(*inp, out[:, :23], 0, 0)
    with pytest.raises(ValueError):
        ops.report_counts(*(a.cpu() for a in inp), out, 0, 0)


# ---- 2. equal bits -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    preds, targets = REF.make_case(395, "ties", 42)
    preds = [p + 0.25 * torch.randn(p.shape, generator=torch.Generator().manual_seed(t)).round() for t, p in enumerate(preds)]
    return [p.to(DEV) for p in preds], targets.to(DEV)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


def test_values_and_replicates_do_not_depend_on_call_chunk_or_bootstrap_size(case):
    from sm3hip import report
    preds, targets = case
    before = [p.clone() for p in preds], targets.clone()
    B = 23
    first = report.evaluation_report(preds, targets, bootstrap=B, seed=2 ** 63 + 11)
    assert first["replicates"].shape == (B, 4, 29) and first["values"].shape == (4, 29) and first["counts"].shape == (24, 6)
    assert first["columns"][0] == "DIAG-1" and first["columns"][23] == "RS-2" and first["columns"][24:] == list(report.AVERAGES)
    for chunk in (None, 1, 7, B):
        again = report.evaluation_report(preds, targets, bootstrap=B, seed=2 ** 63 + 11, chunk=chunk)
        for key in ("values", "replicates", "lo", "hi"):
            assert _same(first[key], again[key]), (chunk, key)
        assert torch.equal(first["undefined"], again["undefined"]) and torch.equal(first["counts"], again["counts"])
    seven = report.evaluation_report(preds, targets, bootstrap=7, seed=2 ** 63 + 11)
    five = report.evaluation_report(preds, targets, bootstrap=5, seed=2 ** 63 + 11)
    assert _same(seven["replicates"][:5].contiguous(), five["replicates"]) and _same(first["replicates"][:7].contiguous(),
                                                                                   seven["replicates"])
    other = report.evaluation_report(preds, targets, bootstrap=5, seed=2 ** 63 + 12)
    assert not _same(other["replicates"], five["replicates"]) and _same(other["values"], five["values"])
    none = report.evaluation_report(preds, targets)
    assert "replicates" not in none and _same(none["values"], first["values"])
    # the interval is the order statistic of the replicates, undefined counts the zero denominators
    lo, hi = report.interval(first["replicates"].numpy(), 0.95)
    assert np.array_equal(first["lo"].numpy(), lo) and np.array_equal(first["hi"].numpy(), hi)
    assert bool((first["lo"] <= first["hi"]).all())
    for p, q in zip(preds + [targets], before[0] + [before[1]]):                      # inputs are not modified
        assert torch.equal(p, q)


def test_replicates_are_the_restatement_through_the_library(case):
    from sm3hip import report
    preds, targets = case
    rep = report.evaluation_report(preds, targets, bootstrap=4, seed=7)
    host = _host(_device_inputs(preds, targets))
    for r in range(4):
        values, _ = report.values_from_counts(REF.counts(*host, REF.multiplicities(7, r, targets.shape[0])))
        assert np.array_equal(rep["replicates"][r].numpy().view(np.uint64), values.view(np.uint64))


def test_undefined_counts_the_replicates_without_a_positive():
    from sm3hip import report
    preds, targets = REF.make_case(12, "random", 5)
    targets[:, 0] = 0
    targets[3, 0] = 4                                                                 # DIAG-5 has ONE positive: out of 1/e of the resamples
    rep = report.evaluation_report([p.to(DEV) for p in preds], targets.to(DEV), bootstrap=200, seed=1)
    k = report.COLUMNS.index("DIAG-5")
    want = sum(int(REF.multiplicities(1, r, 12)[3] == 0) for r in range(200))
    assert 40 < want < 110 and int(rep["undefined"][0, k]) == int(rep["undefined"][1, k]) == want
    assert int(rep["undefined"][0, report.COLUMNS.index("DIAG avg")]) >= want          # an average is undefined with any column
    assert int(rep["undefined"][2, k]) == 0                                           # Spec: the negatives never run out


# ---- 3. against metrics.auc_avg --------------------------------------------------------------------------------------------
def test_point_values_equal_auc_avg_and_compare_with_itself_is_zero(case):
    from sm3hip import metrics, report
    preds, targets = case
    rep = report.evaluation_report(preds, targets, bootstrap=9, seed=3)
    per, avg = metrics.auc_avg(preds, targets)
    got = [float(rep["values"][0, k]) for k in report.SELECTED]
    assert got == [float(v) for v in per]
    # Every class, not only the selected.  The report's value is fl(A2 / (2 P Q)), one IEEE division, and so is binary_auroc's
    # on the CPU (tests/test_report_cpu.py).  On the GPU torch divides a device tensor by a host scalar through the reciprocal,
    # so binary_auroc there returns fl((A2 / 2) * fl(1 / (P Q))): the quotient of the same two integers rounded twice, one ulp
    # off the IEEE quotient for some of them (PN-2 of this fixture; none of its 8 selected columns).  Either way it is a
    # function of the report's integers, and that is asserted with ==.
    A2, P, Q = (rep["counts"][:, e].numpy() for e in range(3))
    d = (P * Q).astype(np.float64)
    once = rep["values"][0, :24].numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        twice = np.where(d > 0, (A2 / 2.0) * (1.0 / d), 0.0)
    assert np.array_equal(once, np.where(d > 0, A2 / np.where(d > 0, 2.0 * d, 1.0), 0.0))
    apart = 0
    for t, n in enumerate(report.NUM_CLASSES):
        want = metrics.multiclass_auroc(preds[t], targets[:, t], n).cpu().numpy()
        for c in range(n):
            k = report.COLUMN_PAIRS.index((t, c))
            assert want[c] == once[k] or want[c] == twice[k], (report.COLUMNS[k], want[c], once[k], twice[k])
            apart += want[c] != once[k]
            assert abs(want[c] - once[k]) <= 2.0 ** -53                                 # one ulp of a value in [0.25, 1) at the most
    print(f"columns where the device's reciprocal division is one ulp off the IEEE quotient: {apart} of 24")
    seq = 0.0
    for v in per:
        seq = seq + float(v)
    k8 = report.COLUMNS.index("8 avg")
    assert float(rep["values"][0, k8]) == seq / 8.0 == report.selected(rep, "AUC")["AUC_AVG"]
    # auc_avg's mean is a device reduction whose order of the 8 additions is torch's: each of the 7 roundings of either order is
    # at most 2^-53 of a partial sum below 8, so the two means differ by at most 14 * 8 * 2^-53 / 8 = 14 * 2^-53
    print(f"8 avg {float(rep['values'][0, k8])!r} auc_avg mean {float(avg)!r}")
    assert abs(float(rep["values"][0, k8]) - float(avg)) <= 14 * 2.0 ** -53
    z = report.compare(rep, rep)
    for key in ("delta", "lo", "hi"):
        assert not z[key].any(), key
    assert float(z["frac_le_zero"].min()) == 1.0
    b = report.evaluation_report([p.flip(0) for p in preds], targets, bootstrap=9, seed=3)
    c = report.compare(rep, b)
    assert c["delta"].any() and bool((c["lo"] <= c["hi"]).all())
    with pytest.raises(ValueError, match="seed"):
        report.compare(rep, report.evaluation_report(preds, targets, bootstrap=9, seed=4))
    with pytest.raises(ValueError, match="bootstrap"):
        report.compare(rep, report.evaluation_report(preds, targets, bootstrap=8, seed=3))
    cpu = report.evaluation_report([p.cpu() for p in preds], targets.cpu())           # CPU tensors are moved, not refused
    assert torch.equal(cpu["counts"], rep["counts"]) and _same(cpu["values"], rep["values"])


# ---- 4. the tools --------------------------------------------------------------------------------------------------------
def _check_report_files(log_path, stat, preds, targets, B, seed=0, confidence=0.95):
    """val_report.json / .csv of a tool against evaluation_report of the predictions it scored."""
    from sm3hip import report
    rep = report.evaluation_report([p.to(DEV) for p in preds], targets.to(DEV), bootstrap=B, seed=seed, confidence=confidence)
    for m in report.METRICS[1:]:
        want = report.selected(rep, m)
        assert len(want) == 9
        for key, v in want.items():
            assert stat[key] == v, key
    saved = json.load(open(os.path.join(log_path, "val_report.json")))
    assert saved["columns"] == report.COLUMNS and saved["values"] == rep["values"].tolist()
    rows = list(csv.reader(open(os.path.join(log_path, "val_report.csv"))))
    assert rows[0] == [""] + report.CSV_COLUMNS
    perm = [report.COLUMNS.index(n) for n in report.CSV_COLUMNS]
    by_name = {r[0]: [float(v) for v in r[1:]] for r in rows[1:]}
    for i, m in enumerate(report.METRICS):
        assert by_name[m] == [100.0 * float(rep["values"][i, k]) for k in perm]
        back = np.array(by_name[m])[np.argsort(perm)] / 100.0                         # parses back to the values
        assert np.allclose(back, rep["values"][i].numpy(), rtol=0, atol=2.0 ** -52)
        if B:
            assert by_name[m + " lo"] == [100.0 * float(rep["lo"][i, k]) for k in perm]
            assert by_name[m + " hi"] == [100.0 * float(rep["hi"][i, k]) for k in perm]
            assert saved["lo"] == rep["lo"].tolist() and saved["bootstrap"] == B and saved["seed"] == seed
    assert by_name["Acc"] == by_name["Recall"]
    return rep


def test_backbone_eval_and_knn_on_synthetic_data(tmp_path, capsys):
    from sm3hip import metrics
    be, bk = _tool("backbone_eval"), _tool("backbone_knn")
    hist = be.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "-b", "8", "--img-sz", "64", "64",
                    "--epochs", "2", "--steps-per-epoch", "1", "--val-steps", "3", "--finetune", "fc", "--bootstrap", "16",
                    "--bootstrap-seed", "5", "--confidence", "0.9", "--log-path", str(tmp_path / "be")])
    out = capsys.readouterr().out
    assert out.count("Recall_AVG") == 2 and "Spec_AVG" in out and "Prec_AVG" in out
    for tr, va in hist:
        assert "Recall_AVG" not in tr and all(f"{m}_{n}" in va for m in ("Recall", "Spec", "Prec") for n in metrics.CLASSES_NAME)
        per, avg = metrics.auc_avg(va["preds"], va["targets"])                        # the existing keys are what they were
        assert va["AUC_AVG"] == float(avg) and [va[f"AUC_{n}"] for n in metrics.CLASSES_NAME] == [float(v) for v in per]
    va = hist[-1][1]
    _check_report_files(str(tmp_path / "be"), va, va["preds"], va["targets"], 16, 5, 0.9)
    stat = bk.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "-b", "4", "--img-sz", "64", "64",
                    "--steps-per-epoch", "3", "--val-steps", "2", "--knn-k", "5", "--knn-t", "0.1", "--log-path",
                    str(tmp_path / "bk")])
    assert "Recall_AVG" in capsys.readouterr().out
    from sm3hip import report
    preds, targets = report.load_predictions(str(tmp_path / "bk" / "knn_predictions.pt"), DEV)
    rep = _check_report_files(str(tmp_path / "bk"), stat, preds, targets, 0)
    assert abs(float(rep["values"][0, report.COLUMNS.index("8 avg")]) - stat["AUC_AVG"]) <= 14 * 2.0 ** -53


def test_mlc_eval_on_synthetic_data(tmp_path, capsys):
    me = _tool("mlc_eval")
    hist = me.main(["--data-name", "synthetic", "--data-path", "-", "-b", "8", "--img-sz", "64", "64", "--epochs", "1", "--steps-per-epoch", "1",
                    "--val-steps", "2", "--mlc-proj-dim", "128", "--sa-dim-ff", "64", "--bootstrap", "8", "--log-path",
                    str(tmp_path)])
    from sm3hip import metrics, report
    assert "Recall_AVG" in capsys.readouterr().out
    va = hist[0][1]
    assert all(isinstance(v, float) for v in va.values())                             # the stat dict stays numbers
    saved = json.load(open(tmp_path / "val_report.json"))                             # synthetic data: no predictions file to re-score
    assert saved["bootstrap"] == 8 and saved["n"] == 16 and np.array(saved["lo"]).shape == (4, 29)
    for i, m in enumerate(report.METRICS):
        for n, k in zip(metrics.CLASSES_NAME, report.SELECTED):
            assert abs(va[f"{m}_{n}"] - saved["values"][i][k]) <= (2.0 ** -53 if m == "AUC" else 0.0), (m, n)
        if m != "AUC":
            assert va[f"{m}_AVG"] == saved["values"][i][report.COLUMNS.index("8 avg")]
    rows = list(csv.reader(open(tmp_path / "val_report.csv")))
    assert [r[0] for r in rows[1:4]] == ["Acc", "Acc lo", "Acc hi"] and len(rows) == 16
    assert not os.path.exists(tmp_path / "val_predictions.pt")                        # real data only, as backbone_eval


def test_the_tools_on_a_derm7pt_tree(tmp_path, capsys):
    from sm3hip import metrics, report
    from src.utils.data.datasets import read_split
    tree = KNN._write_tree(tmp_path / "7PC")
    data = ["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4", "--mean", "0.7833", "0.6712", "0.6026",
            "--std", "0.2139", "0.2472", "0.2571"]
    labels = read_split(str(tree), "test")[2]
    be, me, er = _tool("backbone_eval"), _tool("mlc_eval"), _tool("eval_report")
    hist = be.main(data + ["-a", "resnet18", "-b", "6", "--img-sz", "64", "64", "--epochs", "1", "--finetune", "fc",
                           "--bootstrap", "12", "--log-path", str(tmp_path / "be")])
    va = hist[0][1]
    saved = torch.load(tmp_path / "be" / "val_predictions.pt", map_location="cpu", weights_only=False)
    assert sorted(saved) == ["AUC_AVG", "epoch", "preds", "targets"] and torch.equal(saved["targets"], labels)
    _, avg = metrics.auc_avg([p.to(DEV) for p in saved["preds"]], labels.to(DEV))
    assert va["AUC_AVG"] == saved["AUC_AVG"] == float(avg)                            # unchanged: what the tool gave before
    _check_report_files(str(tmp_path / "be"), va, saved["preds"], saved["targets"], 12)
    hist = me.main(data + ["-b", "6", "--train-sz", "64", "--test-sz", "48", "--epochs", "1", "--mlc-proj-dim", "128",
                           "--sa-dim-ff", "64", "--log-path", str(tmp_path / "me")])
    va = hist[0][1]
    msaved = torch.load(tmp_path / "me" / "val_predictions.pt", map_location="cpu", weights_only=False)
    assert sorted(msaved) == sorted(saved) and torch.equal(msaved["targets"], labels) and msaved["AUC_AVG"] == va["AUC_AVG"]
    _, avg = metrics.auc_avg([p.to(DEV) for p in msaved["preds"]], labels.to(DEV))
    assert float(avg) == va["AUC_AVG"] and all(p.shape == (len(labels), n) for p, n in zip(msaved["preds"], report.NUM_CLASSES))
    _check_report_files(str(tmp_path / "me"), va, msaved["preds"], msaved["targets"], 0)
    capsys.readouterr()
    res = er.main([str(tmp_path / "me" / "val_predictions.pt"), "--against", str(tmp_path / "be" / "val_predictions.pt"),
                   "--bootstrap", "20", "--bootstrap-seed", "9", "--out", str(tmp_path / "er")])
    out = capsys.readouterr().out
    assert "AUC difference" in out and "8 avg" in out and "DIAG-5" in out
    want = report.compare(report.evaluation_report(msaved["preds"], labels, bootstrap=20, seed=9),
                          report.evaluation_report(saved["preds"], labels, bootstrap=20, seed=9))
    assert torch.equal(res["compare"]["delta"], want["delta"]) and torch.equal(res["compare"]["lo"], want["lo"])
    for f in ("val_predictions_report.json", "val_predictions_report.csv", "val_predictions_compare.json"):
        assert os.path.isfile(tmp_path / "er" / f), f
    assert json.load(open(tmp_path / "er" / "val_predictions_compare.json"))["delta"] == want["delta"].tolist()
