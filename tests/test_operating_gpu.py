"""GPU: the operating-point report (csrc/operating.hip, sm3hip/operating.py, the evaluation tools and tools/eval_report.py).

  * sm3_operating_counts equal (==), integer for integer, to the plain-Python restatement of tests/test_operating_cpu.py: the
    point record and three replicates at r0 = 5 with a seed above 2^32, N from a lone case over the thread count +- 1 and the
    scan tile +- 1 to MAX_CASES, scores with heavy ties, without ties, all equal and a class without positives, level lists of
    0, 1, 4, 5 (the kernel takes four levels of each list per pass) and 32 entries; the output pre-filled with a sentinel: every
    entry of every record written, nothing after the last;
  * through operating_report: counts and values equal the report's host half around the restatement, replicates, values and
    intervals bit-equal for every chunk and as a prefix of a longer bootstrap, P and Q of replicate r equal sm3_report_counts'
    (the three reports resample the same cases), the wrapper's refusals;
  * the four tools on synthetic data: the files named in their docstrings, the numbers those of operating_report on the
    predictions they scored."""
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
TAIL = 64


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


OC = _load("sm3_operating_ref", os.path.join(ROOT, "tests", "test_operating_cpu.py"))  # the restatement, host_report
REF = OC.REF                                                                           # multiplicities, make_case


def _tool(name):
    return _load("sm3_operating_gpu_" + name, os.path.join(TOOLS, name + ".py"))


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
def _floors(L):
    return [0.9] if L == 1 else ([0.8, 0.9, 0.95, 0.5, 1.0][:L] if L <= 5 else [float(v) for v in np.linspace(0.0, 1.0, L)])


def _levels(kind, N):
    """(Ls, Lr, Lt) of a case: 32 where the restatement stays quick (few operating points, or a small N)."""
    if kind == "ties":
        return 32, 32, 32
    if kind == "equal":
        return 0, 0, 0
    if kind == "absent":
        return 4, 5, 2
    return (32, 1, 32) if N <= 257 else (5, 4, 3) if N <= 1025 else (1, 1, 1)


@pytest.mark.parametrize("kind", ["ties", "random", "equal", "absent"])
@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, "MAX_CASES"])
def test_counts_equal_the_integer_restatement(N, kind):
    from sm3hip import operating, ops, report
    N = report.MAX_CASES if N == "MAX_CASES" else N
    Ls, Lr, Lt = _levels(kind, N)
    seed, r0, c = 2 ** 32 + 5 + 2 ** 63, 5, 3
    preds, targets = REF.make_case(N, kind, 7 * N + len(kind))
    dp, dt = [p.to(DEV) for p in preds], targets.to(DEV)
    order, gs, ge, _ = report.ranking(dp, dt)
    y = dt.int().contiguous()
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV)
    sig = [operating.q32_floor(s) for s in _floors(Ls)]
    rho = [operating.q32_floor(r) for r in reversed(_floors(Lr))]
    g = torch.Generator().manual_seed(N)
    fix = torch.randint(0, N + 1, (24, Lt), generator=g, dtype=torch.int32)
    if Lt:
        fix[0, 0], fix[1, -1] = N, 0
    R = ops.operating_record(Ls, Lr, Lt)
    assert R == 9 + 3 * Ls + 3 * Lr + 2 * Lt
    host = tuple(a.cpu().numpy().astype(np.int64) for a in (order, gs, ge, targets))
    dsig, drho = (torch.tensor(v, dtype=torch.int64, device=DEV) for v in (sig, rho))
    for point, reps in ((True, 1), (False, c)):
        buf = torch.full((reps * 24 * R + TAIL,), SENTINEL, dtype=torch.int64, device=DEV)
        out = buf[:reps * 24 * R].view(reps, 24, R)
        ops.operating_counts(order, gs, ge, y, colmap, dsig, drho, fix.to(DEV), out, seed, 0 if point else r0, point=point)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert not (got[:-TAIL] == SENTINEL).any() and (got[-TAIL:] == SENTINEL).all()   # every entry written, nothing beyond
        got = got[:-TAIL].reshape(reps, 24, R)
        for j in range(reps):
            m = np.ones(N, dtype=np.int64) if point else REF.multiplicities(seed, r0 + j, N)
            want = OC.records(*host, m, sig, rho, fix.numpy())
            assert np.array_equal(got[j], want), (kind, "point" if point else r0 + j, np.argwhere(got[j] != want)[:4])


def test_wrapper_refuses_what_the_kernel_does_not_take():
    from sm3hip import ops, report
    preds, targets = REF.make_case(5, "ties", 1)
    dt = targets.to(DEV)
    order, gs, ge, _ = report.ranking([p.to(DEV) for p in preds], dt)
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV)
    sig = torch.zeros(1, dtype=torch.int64, device=DEV)
    fix = torch.zeros(24, 2, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 24, ops.operating_record(1, 1, 2), dtype=torch.int64, device=DEV)
    args = [order, gs, ge, dt.int().contiguous(), colmap, sig, sig, fix]
    ops.operating_counts(*args, out, 0, 0)
    with pytest.raises(ValueError):
        ops.operating_counts(*args, out, 0, 0, point=True)                               # the point estimate is one table
    with pytest.raises(ValueError):
        ops.operating_counts(*args, out, 2 ** 64, 0)
    with pytest.raises(ValueError):
        ops.operating_counts(order.long(), *args[1:], out, 0, 0)
    with pytest.raises(ValueError):
        ops.operating_counts(*args, out[:, :, :-1].contiguous(), 0, 0)                   # not the record length of these lists
    with pytest.raises(ValueError):
        ops.operating_counts(*args[:5], torch.zeros(33, dtype=torch.int64, device=DEV), sig, fix, out, 0, 0)
    with pytest.raises(ValueError):
        ops.operating_counts(*args[:5], sig.int(), sig, fix, out, 0, 0)
    with pytest.raises(ValueError):
        ops.operating_counts(*args[:7], fix[:23].contiguous(), out, 0, 0)
    with pytest.raises(ValueError):
        ops.operating_counts(*(a.cpu() for a in args), out, 0, 0)


# ---- 2. through the report ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    preds, targets = REF.make_case(395, "ties", 42)
    preds = [p + 0.25 * torch.randn(p.shape, generator=torch.Generator().manual_seed(t)).round() for t, p in enumerate(preds)]
    return [p.to(DEV) for p in preds], targets.to(DEV)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


def test_report_equals_its_host_half_around_the_restatement(case):
    from sm3hip import operating
    preds, targets = case
    before = [p.clone() for p in preds], targets.clone()
    kw = dict(spec_floors=(0.8, 0.9), sens_floors=(0.95,), decision=(0.1, 0.5), bootstrap=3, seed=2 ** 40 + 9)
    got = operating.operating_report(preds, targets, **kw)
    want = OC.host_report(preds, targets, dev=DEV, **kw)                                  # torch's softmax and sort of this device
    assert got["rows"] == want["rows"] and got["points"] == want["points"] and got["columns"] == want["columns"]
    assert torch.equal(got["counts"], want["counts"]) and torch.equal(got["replicate_counts"], want["replicate_counts"])
    for key in ("values", "replicates", "lo", "hi", "thresholds"):
        assert _same(got[key], want[key]), key
    assert torch.equal(got["undefined"], want["undefined"]) and torch.equal(got["point_undefined"], want["point_undefined"])
    for a, b in zip(got["curves"], want["curves"]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    cpu = operating.operating_report([p.cpu() for p in preds], targets.cpu(), **kw)      # CPU tensors are moved, not refused
    assert torch.equal(cpu["counts"], got["counts"]) and _same(cpu["replicates"], got["replicates"])
    for p, q in zip(preds + [targets], before[0] + [before[1]]):                          # inputs are not modified
        assert torch.equal(p, q)
    thr = operating.fit_thresholds(preds, targets, "spec>=0.9")                           # fit, then apply to the same cases
    applied = operating.operating_report(preds, targets, thresholds=thr)
    assert torch.equal(thr, got["thresholds"][got["points"].index("spec>=0.9")])
    assert torch.equal(applied["counts"][:, -2:], got["counts"][:, 12:14])


def test_replicates_do_not_depend_on_chunk_or_bootstrap_size_and_are_joint_with_the_other_reports(case):
    from sm3hip import operating, ops, report
    preds, targets = case
    seed = 2 ** 63 + 11
    first = operating.operating_report(preds, targets, bootstrap=64, seed=seed)
    assert first["replicates"].shape == (64, len(first["rows"]), 29) and first["counts"].shape == (24, 9 + 9 + 9 + 12)
    for chunk in (1, 7, None):
        again = operating.operating_report(preds, targets, bootstrap=16, seed=seed, chunk=chunk)
        assert _same(again["replicates"], first["replicates"][:16].contiguous()), chunk
        assert torch.equal(again["replicate_counts"], first["replicate_counts"][:16]) and _same(again["values"], first["values"])
        lo, hi = report.interval(first["replicates"][:16].numpy(), 0.95)
        assert np.array_equal(again["lo"].numpy(), lo) and np.array_equal(again["hi"].numpy(), hi), chunk
        assert torch.equal(again["undefined"], operating.operating_report(preds, targets, bootstrap=16, seed=seed)["undefined"])
    whole = operating.operating_report(preds, targets, bootstrap=64, seed=seed, chunk=7)
    for key in ("replicates", "lo", "hi", "values"):
        assert _same(whole[key], first[key]), key
    other = operating.operating_report(preds, targets, bootstrap=16, seed=seed + 1)
    assert not _same(other["replicates"], first["replicates"][:16].contiguous()) and _same(other["values"], first["values"])
    # replicate r resamples the cases of replicate r of evaluation_report: P and Q are sm3_report_counts'
    order, gs, ge, yhat = report.ranking(preds, targets)
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV)
    rc = torch.empty((64, 24, 6), dtype=torch.int64, device=DEV)
    ops.report_counts(order, gs, ge, targets.int().contiguous(), yhat, colmap, rc, seed, 0)
    assert torch.equal(rc[:, :, 1:3].cpu(), first["replicate_counts"][:, :, 0:2])
    rep = report.evaluation_report(preds, targets, bootstrap=64, seed=seed)
    assert torch.equal(rep["counts"][:, 1:3], first["counts"][:, 0:2])
    z = operating.compare(first, first)
    assert not z["delta"].any() and not z["lo"].any() and not z["hi"].any()
    with pytest.raises(ValueError, match="seed"):
        operating.compare(operating.operating_report(preds, targets, bootstrap=16, seed=seed), other)
    with pytest.raises(ValueError, match="bootstrap"):
        operating.compare(first, other)


# ---- 3. the tools -------------------------------------------------------------------------------------------------------------
def _recorded(monkeypatch):
    """Keeps what a tool hands to validation_operating, and lets the call through."""
    from sm3hip import operating
    seen, real = [], operating.validation_operating

    def wrapper(preds, targets, args, log_path):
        seen.append(([p.detach().clone() for p in preds], targets.clone()))
        return real(preds, targets, args, log_path)
    monkeypatch.setattr(operating, "validation_operating", wrapper)
    return seen


def _check_files(log_path, preds, targets, stem="val_operating", **kw):
    from sm3hip import operating
    rep = operating.operating_report(preds, targets, **kw)
    saved = json.load(open(os.path.join(log_path, stem + ".json")))
    assert saved["rows"] == rep["rows"] and saved["values"] == rep["values"].tolist() and saved["counts"] == rep["counts"].tolist()
    assert saved["n"] == targets.shape[0] and len(saved["curves"]) == 24
    if kw.get("bootstrap"):
        assert saved["lo"] == rep["lo"].tolist() and saved["hi"] == rep["hi"].tolist() and saved["seed"] == kw["seed"]
    lines = open(os.path.join(log_path, stem + ".csv")).read().splitlines()
    assert len(lines) == 1 + len(rep["rows"]) * 29
    assert float(lines[1].split(",")[2]) == float(rep["values"][0, 0])
    return rep


def test_backbone_eval_and_knn_write_the_operating_report(tmp_path, capsys, monkeypatch):
    seen = _recorded(monkeypatch)
    be, bk = _tool("backbone_eval"), _tool("backbone_knn")
    base = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--img-sz", "64", "64"]
    hist = be.main(base + ["-b", "8", "--epochs", "2", "--steps-per-epoch", "1", "--val-steps", "3", "--finetune", "fc", "--bootstrap",
                           "16", "--bootstrap-seed", "5", "--confidence", "0.9", "--operating", "--operating-spec", "0.9",
                           "--operating-decision", "0.2", "0.4", "--log-path", str(tmp_path / "be")])
    out = capsys.readouterr().out
    assert out.count("AP_AVG") == 1 and len(seen) == 1                                    # the last validation pass alone
    assert torch.equal(seen[0][1], hist[-1][1]["targets"])
    _check_files(str(tmp_path / "be"), *seen[0], spec_floors=[0.9], decision=[0.2, 0.4], bootstrap=16, seed=5, confidence=0.9)
    bk.main(base + ["-b", "4", "--steps-per-epoch", "3", "--val-steps", "2", "--knn-k", "5", "--knn-t", "0.1", "--operating",
                    "--operating-sens", "--log-path", str(tmp_path / "bk")])
    assert "AP_AVG" in capsys.readouterr().out and len(seen) == 2
    from sm3hip import report
    preds, targets = report.load_predictions(str(tmp_path / "bk" / "knn_predictions.pt"), DEV)
    rep = _check_files(str(tmp_path / "bk"), preds, targets, sens_floors=[])
    assert not any(r.startswith("sens>=") for r in rep["rows"]) and torch.equal(seen[1][1], targets)
    be.main(base + ["-b", "8", "--epochs", "1", "--steps-per-epoch", "1", "--val-steps", "1", "--finetune", "fc", "--log-path",
                    str(tmp_path / "off")])
    assert not os.path.exists(tmp_path / "off" / "val_operating.json") and len(seen) == 2  # default off


def test_mlc_eval_writes_the_operating_report(tmp_path, capsys, monkeypatch):
    seen = _recorded(monkeypatch)
    _tool("mlc_eval").main(["--data-name", "synthetic", "--data-path", "-", "-b", "8", "--img-sz", "64", "64", "--epochs", "1",
                            "--steps-per-epoch", "1", "--val-steps", "2", "--mlc-proj-dim", "128", "--sa-dim-ff", "64", "--bootstrap",
                            "8", "--operating", "--log-path", str(tmp_path)])
    assert "AP_AVG" in capsys.readouterr().out and len(seen) == 1
    _check_files(str(tmp_path), *seen[0], bootstrap=8, seed=0)


def test_eval_report_fits_on_one_file_and_reports_the_other(tmp_path, capsys):
    from sm3hip import operating
    er = _tool("eval_report")
    files = {}
    for name, N, s in (("val", 150, 1), ("test", 210, 2), ("other", 210, 2)):
        preds, targets = REF.make_case(N, "random", s)
        if name == "other":
            preds = [p.flip(1) for p in preds]
        files[name] = (str(tmp_path / f"{name}.pt"), preds, targets)
        torch.save({"preds": preds, "targets": targets}, files[name][0])
    res = er.main([files["test"][0], "--operating", "--fit-on", files["val"][0], "--against", files["other"][0], "--bootstrap", "12",
                   "--bootstrap-seed", "9", "--operating-rule", "sens>=0.9", "--operating-sens", "0.9", "--out", str(tmp_path / "er")])
    out = capsys.readouterr().out
    assert "thresholds fitted on" in out and "thr[0] sens" in out and "difference" in out
    for f in ("test_operating.json", "test_operating.csv", "test_operating_compare.json", "test_operating_fitted.json",
              "test_operating_fitted.csv", "test_calibration.json", "test_calibration_fitted.json", "test_report.json"):
        assert os.path.isfile(tmp_path / "er" / f), f
    kw = dict(sens_floors=[0.9], bootstrap=12, seed=9)
    _, tp, tt = files["test"]
    rep = _check_files(str(tmp_path / "er"), tp, tt, stem="test_operating", **kw)
    assert torch.equal(res["operating"]["replicates"], rep["replicates"])
    thr = operating.fit_thresholds(files["val"][1], files["val"][2], "sens>=0.9")
    assert torch.equal(res["operating_thresholds"], thr)
    fitted = _check_files(str(tmp_path / "er"), tp, tt, stem="test_operating_fitted", thresholds=thr, **kw)
    i = fitted["rows"].index("thr[0] sens")
    assert fitted["replicates"].shape[0] == 12 and bool((fitted["lo"][i] <= fitted["hi"][i]).all())
    saved = json.load(open(tmp_path / "er" / "test_operating_fitted.json"))
    assert saved["rule"] == "sens>=0.9" and saved["thresholds"][-1] == thr.tolist()
    want = operating.compare(rep, operating.operating_report(files["other"][1], files["other"][2], **kw))
    cmp = json.load(open(tmp_path / "er" / "test_operating_compare.json"))
    assert cmp["delta"] == want["delta"].tolist() and cmp["lo"] == want["lo"].tolist() and want["delta"].any()
    # the three reports of one seed are joint: replicate r of each resamples the same cases
    assert res["report"]["bootstrap"] == res["calibration"]["bootstrap"] == res["operating"]["bootstrap"] == 12
    assert res["report"]["seed"] == res["calibration"]["seed"] == res["operating"]["seed"] == 9
