"""GPU: the seven-point checklist report (csrc/checklist.hip, sm3hip/checklist.py, the evaluation tools and tools/eval_report.py).

  * sm3_checklist_counts equal (==), integer for integer, to the plain-Python restatement of tests/test_checklist_cpu.py: the
    point record and three replicates at r0 = 5 with a seed above 2^32; N = a Philox quad that is not full, the wave, the
    workgroup and the scan tile +- 1 and MAX_CASES; continuous scores, heavy ties, one tie group and one table bin, all 242
    bins, no melanoma, only melanoma; the output pre-filled with a sentinel and followed by a sentinel tail: every entry of every
    record written, nothing after the last.  A launch of more than 256 replicates (one workgroup per replicate) writes what
    shorter launches (one workgroup per replicate and part) write.  r0 + c = 2^32 is accepted, one more refused;
  * through checklist_report: replicates, values and intervals bit-equal for every chunk and as a prefix of a longer bootstrap,
    the diag AUC of the point estimate and of every replicate equal to evaluation_report's DIAG-3 AUC (the five reports resample
    the same cases), CPU tensors and GPU tensors give equal bits, compare(a, a) is exactly 0;
  * backbone_eval and eval_report on synthetic data: the files named in their docstrings, the numbers those of checklist_report
    on the predictions they scored, two runs byte-equal; mlc_eval and backbone_knn write the same files."""
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
R = 251


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CC = _load("sm3_checklist_ref", os.path.join(ROOT, "tests", "test_checklist_cpu.py"))  # the restatement, make_case, host_report
REF = CC.REF                                                                           # multiplicities


def _tool(name):
    return _load("sm3_checklist_gpu_" + name, os.path.join(TOOLS, name + ".py"))


def _inputs(N, kind, seed):
    from sm3hip import checklist
    preds, targets = CC.make_case(N, kind, seed)
    return checklist.case_inputs([p.to(DEV) for p in preds], targets.to(DEV), [3, 1])[:4]


def _launch(dev_in, reps, seed, r0, point):
    """The records of one launch as numpy [reps, 251], with the sentinel checks around them."""
    from sm3hip import ops
    buf = torch.full((reps * R + TAIL,), SENTINEL, dtype=torch.int64, device=DEV)
    ops.checklist_counts(*dev_in, buf[:reps * R].view(reps, R), seed, r0, point=point)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert not (got[:-TAIL] == SENTINEL).any() and (got[-TAIL:] == SENTINEL).all()       # every entry written, nothing beyond
    return got[:-TAIL].reshape(reps, R)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CC.KINDS)
@pytest.mark.parametrize("N", [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, "MAX_CASES"])
def test_counts_equal_the_integer_restatement(N, kind):
    from sm3hip import checklist
    N = checklist.MAX_CASES if N == "MAX_CASES" else N
    seed, r0, c = 2 ** 32 + 5 + 2 ** 63, 5, 3
    dev_in = _inputs(N, kind, 7 * N + len(kind))
    host = tuple(a.cpu().numpy().astype(np.int64) for a in dev_in)
    for point, reps in ((True, 1), (False, c)):
        got = _launch(dev_in, reps, seed, 0 if point else r0, point)
        want = CC.records(host, seed, r0, reps, point)
        assert np.array_equal(got, want), (kind, N, "point" if point else r0, np.argwhere(got != want)[:4])
        assert (got[:, :242].sum(axis=1) == N).all()
    bins = int((want[0, :242] > 0).sum())
    if kind == "equal":
        assert bins == 1 and (got[:, 243] == N).all() and not got[:, 242].any()           # one table bin; one tie group, all positive
    if kind == "all_bins" and N >= 242:
        assert int((CC.records(host, seed, 0, 1, True)[0, :242] > 0).sum()) == 242        # every bin of the point table
    if kind in ("absent", "only"):
        assert (got[:, 243] == (0 if kind == "absent" else N)).all() and not got[:, 242].any()


@pytest.mark.parametrize("N", [5, 257, 1025, "MAX_CASES"])
def test_a_long_launch_writes_what_short_launches_write(N):
    """More than 256 replicates: one workgroup per replicate does the four parts of a record in turn."""
    from sm3hip import checklist
    N = checklist.MAX_CASES if N == "MAX_CASES" else N
    seed = 2 ** 40 + 3
    dev_in = _inputs(N, "ties" if N == 257 else "random", N)
    long = _launch(dev_in, 257, seed, 2, False)
    short = np.concatenate([_launch(dev_in, 256, seed, 2, False), _launch(dev_in, 1, seed, 2 + 256, False)])  # the split grid
    assert np.array_equal(long, short)
    host = tuple(a.cpu().numpy().astype(np.int64) for a in dev_in)
    assert np.array_equal(long[255:257], CC.records(host, seed, 2 + 255, 2, False))


def test_replicate_range_and_wrapper_refusals():
    from sm3hip import _lib, ops
    dev_in = _inputs(5, "ties", 1)
    host = tuple(a.cpu().numpy().astype(np.int64) for a in dev_in)
    got = _launch(dev_in, 3, 9, 2 ** 32 - 3, False)                                      # r0 + c = 2^32
    assert np.array_equal(got, CC.records(host, 9, 2 ** 32 - 3, 3, False))
    out = torch.zeros(3, R, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.SM3LibraryError, match="SM3_EINVAL"):
        ops.checklist_counts(*dev_in, out, 9, 2 ** 32 - 2)                               # one more
    with pytest.raises(ValueError, match="one record"):
        ops.checklist_counts(*dev_in, out, 0, 0, point=True)
    with pytest.raises(ValueError, match="seed"):
        ops.checklist_counts(*dev_in, out, 2 ** 64, 0)
    with pytest.raises(ValueError):
        ops.checklist_counts(dev_in[0].long(), *dev_in[1:], out, 0, 0)
    with pytest.raises(ValueError):
        ops.checklist_counts(*dev_in, out[:, :-1].contiguous(), 0, 0)                    # not the record length
    with pytest.raises(ValueError):
        ops.checklist_counts(dev_in[0], dev_in[1][:2].contiguous(), *dev_in[2:], out, 0, 0)
    with pytest.raises(ValueError):
        ops.checklist_counts(*(a.cpu() for a in dev_in), out, 0, 0)


# ---- 2. through the report ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    preds, targets = CC.make_case(395, "ties", 42)
    preds = [p + 0.25 * torch.randn(p.shape, generator=torch.Generator().manual_seed(t)).round() for t, p in enumerate(preds)]
    return [p.to(DEV) for p in preds], targets.to(DEV)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


def test_report_equals_its_host_half_around_the_restatement(case):
    from sm3hip import checklist
    preds, targets = case
    before = [p.clone() for p in preds], targets.clone()
    kw = dict(thresholds=(3, 1, 5), bootstrap=3, seed=2 ** 40 + 9)
    got = checklist.checklist_report(preds, targets, **kw)
    want = CC.host_report(preds, targets, dev=DEV, **kw)
    assert got["rows"] == want["rows"] and got["shown"] == want["shown"] and got["thresholds"] == [3, 1, 5]
    assert torch.equal(got["counts"], want["counts"]) and torch.equal(got["replicate_counts"], want["replicate_counts"])
    for key in ("values", "replicates", "lo", "hi"):
        assert _same(got[key], want[key]), key
    assert torch.equal(got["undefined"], want["undefined"]) and torch.equal(got["point_undefined"], want["point_undefined"])
    assert torch.equal(got["scores"]["predicted"], checklist.predicted_scores([p.cpu() for p in preds]))
    assert torch.equal(got["scores"]["annotated"], checklist.true_scores(targets.cpu())) and got["n"] == 395
    cpu = checklist.checklist_report([p.cpu() for p in preds], targets.cpu(), **kw)      # CPU tensors are moved, not refused
    assert torch.equal(cpu["counts"], got["counts"]) and torch.equal(cpu["replicate_counts"], got["replicate_counts"])
    for key in ("values", "replicates", "lo", "hi"):
        assert _same(cpu[key], got[key]), key
    for p, q in zip(preds + [targets], before[0] + [before[1]]):                          # inputs are not modified
        assert torch.equal(p, q)


def test_replicates_do_not_depend_on_chunk_or_bootstrap_size_and_are_joint_with_the_other_reports(case):
    from sm3hip import checklist, report
    preds, targets = case
    seed = 2 ** 63 + 11
    longer = checklist.checklist_report(preds, targets, bootstrap=50, seed=seed)
    first = checklist.checklist_report(preds, targets, bootstrap=37, seed=seed)
    assert first["replicates"].shape == (37, 93, 1) and first["counts"].shape == (R,)
    assert _same(first["replicates"], longer["replicates"][:37].contiguous()) and _same(first["values"], longer["values"])
    assert torch.equal(first["replicate_counts"], longer["replicate_counts"][:37])
    for chunk in (1, 7, 37, None):
        again = checklist.checklist_report(preds, targets, bootstrap=37, seed=seed, chunk=chunk)
        for key in ("replicates", "values", "lo", "hi"):
            assert _same(again[key], first[key]), (key, chunk)
        assert torch.equal(again["replicate_counts"], first["replicate_counts"]) and torch.equal(again["undefined"], first["undefined"])
    lo, hi = report.interval(longer["replicates"][:37].numpy(), 0.95)
    assert np.array_equal(first["lo"].numpy(), lo) and np.array_equal(first["hi"].numpy(), hi)
    other = checklist.checklist_report(preds, targets, bootstrap=37, seed=seed + 1)
    assert not _same(other["replicates"], first["replicates"]) and _same(other["values"], first["values"])
    # replicate r resamples the cases of replicate r of evaluation_report: the diag AUC is its DIAG-3 AUC, bit for bit
    rep = report.evaluation_report(preds, targets, bootstrap=37, seed=seed)
    i, k = first["rows"].index("AUC diag"), report.COLUMNS.index("DIAG-3")
    assert float(first["values"][i, 0]) == float(rep["values"][0, k]) and 0 < float(first["values"][i, 0]) < 1
    assert _same(first["replicates"][:, i, 0].contiguous(), rep["replicates"][:, 0, k].contiguous())
    assert (float(first["lo"][i, 0]), float(first["hi"][i, 0])) == (float(rep["lo"][0, k]), float(rep["hi"][0, k]))
    z = checklist.compare(first, first)
    assert not z["delta"].any() and not z["lo"].any() and not z["hi"].any()
    with pytest.raises(ValueError, match="seed"):
        checklist.compare(first, other)
    with pytest.raises(ValueError, match="bootstrap"):
        checklist.compare(first, longer)


# ---- 3. the tools -------------------------------------------------------------------------------------------------------------
def _recorded(monkeypatch):
    """Keeps what a tool hands to validation_checklist, and lets the call through."""
    from sm3hip import checklist
    seen, real = [], checklist.validation_checklist

    def wrapper(preds, targets, args, log_path):
        seen.append(([p.detach().clone() for p in preds], targets.clone()))
        return real(preds, targets, args, log_path)
    monkeypatch.setattr(checklist, "validation_checklist", wrapper)
    return seen


def _check_files(log_path, preds, targets, stem="val_checklist", **kw):
    from sm3hip import checklist
    rep = checklist.checklist_report(preds, targets, **kw)
    saved = json.load(open(os.path.join(log_path, stem + ".json")))
    assert saved["rows"] == rep["rows"] and saved["values"] == rep["values"].tolist() and saved["counts"] == rep["counts"].tolist()
    assert saved["n"] == targets.shape[0] and saved["scores"]["annotated"] == rep["scores"]["annotated"].tolist()
    if kw.get("bootstrap"):
        assert saved["lo"] == rep["lo"].tolist() and saved["hi"] == rep["hi"].tolist() and saved["seed"] == kw["seed"]
    lines = open(os.path.join(log_path, stem + ".csv")).read().splitlines()
    assert len(lines) == 1 + len(rep["shown"])
    assert float(lines[1].split(",")[1]) == float(rep["values"][rep["shown"][0], 0])
    return rep


def _bytes(folder, names):
    return [open(os.path.join(folder, n), "rb").read() for n in names]


def test_backbone_eval_writes_the_checklist_report(tmp_path, capsys, monkeypatch):
    seen = _recorded(monkeypatch)
    be = _tool("backbone_eval")
    data = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--img-sz", "64", "64", "-b", "8", "--finetune", "fc"]
    base = data + ["--epochs", "2", "--steps-per-epoch", "1", "--val-steps", "3"]
    flags = ["--bootstrap", "20", "--bootstrap-seed", "5", "--confidence", "0.9", "--checklist", "--checklist-thresholds", "3", "2"]
    hist = be.main(base + flags + ["--log-path", str(tmp_path / "a")])
    out = capsys.readouterr().out
    assert out.count("checklist_AUC_hard") == 1 and len(seen) == 1                        # the last validation pass alone
    assert torch.equal(seen[0][1], hist[-1][1]["targets"])
    rep = _check_files(str(tmp_path / "a"), *seen[0], thresholds=[3, 2], bootstrap=20, seed=5, confidence=0.9)
    assert "AUC tail>=3" in rep["rows"] and rep["replicates"].shape == (20, 93, 1)
    be.main(base + flags + ["--log-path", str(tmp_path / "b")])                           # a second run: byte-equal files
    names = ["val_checklist.json", "val_checklist.csv"]
    assert _bytes(tmp_path / "a", names) == _bytes(tmp_path / "b", names) and len(seen) == 2
    be.main(data + ["--epochs", "1", "--steps-per-epoch", "1", "--val-steps", "1", "--log-path", str(tmp_path / "off")])
    assert not os.path.exists(tmp_path / "off" / "val_checklist.json") and len(seen) == 2  # default off


def test_mlc_eval_and_backbone_knn_write_the_checklist_report(tmp_path, capsys, monkeypatch):
    from sm3hip import report
    seen = _recorded(monkeypatch)
    _tool("mlc_eval").main(["--data-name", "synthetic", "--data-path", "-", "-b", "8", "--img-sz", "64", "64", "--epochs", "1",
                            "--steps-per-epoch", "1", "--val-steps", "2", "--mlc-proj-dim", "128", "--sa-dim-ff", "64", "--bootstrap",
                            "8", "--checklist", "--log-path", str(tmp_path / "mlc")])
    assert "checklist_AUC_hard" in capsys.readouterr().out and len(seen) == 1
    _check_files(str(tmp_path / "mlc"), *seen[0], bootstrap=8, seed=0)
    _tool("backbone_knn").main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--img-sz", "64", "64", "-b", "4",
                                "--steps-per-epoch", "3", "--val-steps", "2", "--knn-k", "5", "--knn-t", "0.1", "--checklist",
                                "--checklist-thresholds", "2", "--log-path", str(tmp_path / "bk")])
    assert "checklist_AUC_hard" in capsys.readouterr().out and len(seen) == 2
    preds, targets = report.load_predictions(str(tmp_path / "bk" / "knn_predictions.pt"), DEV)
    rep = _check_files(str(tmp_path / "bk"), preds, targets, thresholds=[2])
    assert "AUC tail>=2" in rep["rows"] and torch.equal(seen[1][1], targets)


def test_eval_report_writes_the_checklist_report_and_its_paired_comparison(tmp_path, capsys):
    from sm3hip import checklist
    er = _tool("eval_report")
    files = {}
    for name, s in (("test", 2), ("other", 2)):
        preds, targets = CC.make_case(210, "random", s)
        if name == "other":
            preds = [p.flip(1) for p in preds]
        files[name] = (str(tmp_path / f"{name}.pt"), preds, targets)
        torch.save({"preds": preds, "targets": targets}, files[name][0])
    argv = [files["test"][0], "--checklist", "--against", files["other"][0], "--bootstrap", "12", "--bootstrap-seed", "9"]
    res = er.main(argv + ["--out", str(tmp_path / "a")])
    out = capsys.readouterr().out
    assert "seven-point checklist, 210 cases" in out and "difference" in out and "pred>=3 sens" in out
    names = ["test_checklist.json", "test_checklist.csv", "test_checklist_compare.json"]
    for f in names + ["test_report.json"]:
        assert os.path.isfile(tmp_path / "a" / f), f
    kw = dict(bootstrap=12, seed=9)
    _, tp, tt = files["test"]
    rep = _check_files(str(tmp_path / "a"), tp, tt, stem="test_checklist", **kw)
    assert torch.equal(res["checklist"]["replicates"], rep["replicates"])
    want = checklist.compare(rep, checklist.checklist_report(files["other"][1], files["other"][2], **kw))
    cmp = json.load(open(tmp_path / "a" / "test_checklist_compare.json"))
    assert cmp["delta"] == want["delta"].tolist() and cmp["lo"] == want["lo"].tolist() and want["delta"].any()
    # the reports of one seed are joint: replicate r of each resamples the same cases
    assert res["report"]["bootstrap"] == res["checklist"]["bootstrap"] == 12 and res["report"]["seed"] == res["checklist"]["seed"] == 9
    er.main(argv + ["--out", str(tmp_path / "b")])                                        # a second run: byte-equal files
    assert _bytes(tmp_path / "a", names) == _bytes(tmp_path / "b", names)
