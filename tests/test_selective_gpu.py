"""GPU: the selective-prediction report (sm3hip/selective.py, csrc/selective.hip) against its restatement in
tests/selective_inputs.py.

  1. sm3_selective_counts == the restatement, integer for integer: the point record and three replicates at r0 = 5 with the seed
     2^32 + 5 + 2^63 (both key words); N around every tile and wave edge up to MAX_CASES; every kind of input; the levels at their
     limits (G = 16, H = 8, Pc = 8 with the cuts 1, N, 0, N and the risks 0 / 1 and 1 / 1; G = 1, H = 0, Pc = 0); the output
     pre-filled with a sentinel and followed by a sentinel tail; the replicate range up to 2^32; every argument error with its
     code, nothing launched (nothing here provokes a device fault);
  2. selective_report: equal bits across chunks, bootstrap sizes and the device of the inputs; compare(a, a) == 0; the correct
     copies of every replicate are those of calibration_report's top-label series (the reports resample the same cases); msp and
     margin coincide on the two-class labels;
  3. eval_report.py --selective writes files equal to selective_report of the predictions it read, twice the same bytes,
     tta-range as the tensor path fed by hand, and nothing without the flag."""
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
SEED, R0, C = 2 ** 32 + 5 + 2 ** 63, 5, 3
MAX_CASES = 8192
SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, MAX_CASES)
VALUE_KEYS = tuple(f"{x}_values" for x in ("summary", "coverage", "risk", "threshold"))
BOOT_KEYS = tuple(f"{x}_{k}" for x in ("summary", "coverage", "risk", "threshold") for k in ("replicates", "lo", "hi", "undefined"))


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SI = _load("sm3_selective_inputs_gpu", os.path.join(ROOT, "tests", "selective_inputs.py"))


def _same(a, b):
    return torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b


def _device_case(N, kind, seed=3):
    """The kernel's inputs on the device through the library's plumbing, and the restatement's as numpy."""
    from sm3hip import selective
    preds, targets = SI.case(N, kind, seed)
    preds, targets = [p.to(DEV) for p in preds], targets.to(DEV)
    key = selective.keys(preds, "msp")
    order, last, _, _ = selective.ranking(key, key)
    packed = selective.pack_flags(preds, targets, order, last)
    table = torch.from_numpy(selective.harmonic_table(N)).to(DEV)
    return (packed, order, table), (order.cpu().numpy().astype(np.int64), SI.flags(preds, targets), last.cpu().numpy())


def _launch(dev_in, kcuts, risks, pcuts, seed, r0, c, point):
    """out [c, 8, R] from one launch into a sentinel-filled buffer with a sentinel tail; both are checked."""
    from sm3hip import ops
    G, H, Pc = len(kcuts), len(risks), len(pcuts[0])
    R = ops.selective_record(G, H, Pc)
    buf = torch.full((c * 8 * R + TAIL,), SENTINEL, dtype=torch.int64, device=DEV)
    out = buf[:c * 8 * R].view(c, 8, R)
    ops.selective_counts(*dev_in, torch.tensor(kcuts, dtype=torch.int32, device=DEV),
                         torch.tensor(pcuts, dtype=torch.int32, device=DEV).reshape(8, Pc),
                         torch.tensor(risks, dtype=torch.int32, device=DEV).reshape(H, 2), out, seed, r0, point=point)
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()), "an entry was not written"
    assert bool((buf[c * 8 * R:] == SENTINEL).all()), "written beyond the records"
    return out.cpu().numpy()


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SI.KINDS)
@pytest.mark.parametrize("N", SIZES)
def test_kernel_is_the_restatement(N, kind):
    dev_in, (order, flg, last) = _device_case(N, kind)
    full = SI.levels(N, 16, 8, 8, seed=N)
    small = SI.levels(N, 1, 0, 0, seed=N)
    assert full[0][:2] == [1, N] and full[1][:2] == [(0, 1), (1, 1)] and all(p[:2] == [0, N] for p in full[2]) and small[0] == [1]
    want_point = SI.records(order, flg, last, None, *full)
    got = _launch(dev_in, *full, SEED, 0, 1, True)
    assert np.array_equal(got[0], want_point), (N, kind, "point")
    assert np.array_equal(_launch(dev_in, *small, SEED, 0, 1, True)[0], want_point[:, :7])
    got = _launch(dev_in, *full, SEED, R0, C, False)
    got_small = _launch(dev_in, *small, SEED, R0, C, False)
    for j in range(C):
        want = SI.records(order, flg, last, SI.multiplicities(SEED, R0 + j, N), *full)
        assert np.array_equal(got[j], want), (N, kind, R0 + j)
        assert np.array_equal(got_small[j], want[:, :7]), (N, kind, R0 + j)
    if N > 1:
        assert not np.array_equal(got[0], got[1])                                 # the replicates differ
    assert np.array_equal(_launch(dev_in, *full, SEED, R0 + 1, 1, False)[0], got[1])  # a record does not depend on r0, c


def test_cuts_out_of_range_are_clamped():
    N = 65
    dev_in, (order, flg, last) = _device_case(N, "random")
    got = _launch(dev_in, [0, -5, N + 1, 2 ** 30], [(-1, 1), (5, 1), (1, 0)], [[-1, N + 1, -(2 ** 31)]] * 8, SEED, 0, 1, True)
    want = SI.records(order, flg, last, None, [1, 1, N, N], [(0, 1), (1, 1), (1, 1)], [[0, N, 0]] * 8)
    assert np.array_equal(got[0], want)


def test_replicate_range_ends_at_2_to_32():
    from sm3hip import ops
    N = 5
    dev_in, (order, flg, last) = _device_case(N, "random")
    lv = SI.levels(N, 2, 2, 2)
    got = _launch(dev_in, *lv, SEED, 2 ** 32 - 1, 1, False)                      # r0 + c = 2^32: the last replicate there is
    assert np.array_equal(got[0], SI.records(order, flg, last, SI.multiplicities(SEED, 2 ** 32 - 1, N), *lv))
    with pytest.raises(Exception, match="sm3_selective_counts"):
        _launch(dev_in, *lv, SEED, 2 ** 32, 1, False)
    with pytest.raises(Exception, match="sm3_selective_counts"):
        _launch(dev_in, *lv, SEED, 2 ** 32 - 1, 2, False)
    with pytest.raises(ValueError, match="point"):
        ops.selective_counts(*dev_in, torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros((8, 0), dtype=torch.int32, device=DEV),
                             torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros((2, 8, 7), dtype=torch.int64, device=DEV),
                             0, 0, point=True)


def test_bad_arguments_give_their_codes_and_launch_nothing():
    import ctypes as C_
    from sm3hip import _lib, ops
    N, G, H, Pc = 9, 2, 1, 1
    (packed, order, table), _ = _device_case(N, "random")
    kc = torch.tensor([1, N], dtype=torch.int32, device=DEV)
    pc = torch.zeros((8, Pc), dtype=torch.int32, device=DEV)
    rk = torch.tensor([[1, 10]], dtype=torch.int32, device=DEV)
    out = torch.full((2 * 8 * ops.selective_record(G, H, Pc) + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    ptr = {"packed": packed, "order": order, "table": table, "kcuts": kc, "pcuts": pc, "risks": rk, "out": out}

    def call(**kw):
        a = dict(N=N, G=G, H=H, Pc=Pc, seed=1, r0=0, c=2, point=0)
        p = {k: C_.c_void_p(v.data_ptr()) for k, v in ptr.items()}
        for k, v in kw.items():
            (p if k in p else a)[k] = v
        return lib.sm3_selective_counts(p["packed"], p["order"], p["table"], p["kcuts"], p["pcuts"], p["risks"], p["out"], a["N"],
                                        a["G"], a["H"], a["Pc"], a["seed"], a["r0"], a["c"], a["point"], ops._stream())
    for kw in ({"packed": None}, {"order": None}, {"table": None}, {"kcuts": None}, {"pcuts": None}, {"risks": None}, {"out": None},
               {"N": 0}, {"N": MAX_CASES + 1}, {"c": 0}, {"r0": -1}, {"r0": 2 ** 32 - 1}, {"point": 1}, {"G": 0}, {"G": 17}, {"H": -1},
               {"H": 9}, {"Pc": -1}, {"Pc": 9}):
        assert call(**kw) == -1, kw                                                  # SM3_EINVAL
    assert call(out=C_.c_void_p(out.data_ptr() + 4)) == -2                           # SM3_EALIGN
    assert call(pcuts=None, Pc=0) == 0 and call(risks=None, H=0) == 0                # what is empty may be null
    torch.cuda.synchronize()
    out[:] = SENTINEL
    for kw in ({"N": 0}, {"G": 17}, {"out": C_.c_void_p(out.data_ptr() + 4)}):
        assert call(**kw) < 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- 2. the report -------------------------------------------------------------------------------------------------------
def test_report_bits_do_not_depend_on_chunk_bootstrap_or_device():
    from sm3hip import selective
    N = 395
    preds, targets = SI.case(N, "ties", 4)
    thr = torch.tensor([[0.0, 1.0]] * 8)
    kw = dict(seed=SEED, confidence=0.9, thresholds=thr, coverages=("0.5", "0.9", "1"), risks=("0.1", "0.3"))
    a = selective.selective_report(preds, targets, bootstrap=20, chunk=None, **kw)
    for chunk in (1, 7):
        b = selective.selective_report(preds, targets, bootstrap=20, chunk=chunk, **kw)
        for key in VALUE_KEYS + BOOT_KEYS + ("counts", "ties", "position_cuts"):
            assert _same(a[key], b[key]), (chunk, key)
    longer = selective.selective_report(preds, targets, bootstrap=33, **kw)
    for x in ("summary", "coverage", "risk", "threshold"):
        assert torch.equal(longer[x + "_replicates"][:20], a[x + "_replicates"])
    gpu = selective.selective_report([p.to(DEV) for p in preds], targets.to(DEV), bootstrap=20, **kw)
    for key in VALUE_KEYS + BOOT_KEYS + ("counts",):
        assert _same(a[key], gpu[key]), key
    assert all(not gpu[k].is_cuda for k in VALUE_KEYS + ("counts", "targets", "ties"))
    cmp = selective.compare(a, a)
    for x in ("summary", "coverage", "risk"):
        assert not cmp[x + "_delta"].any() and not cmp[x + "_lo"].any() and not cmp[x + "_hi"].any()
        assert bool((cmp[x + "_frac_le_zero"] == 1.0).all())


def test_report_is_the_restatement_through_the_host_side():
    from sm3hip import selective
    N = 130
    preds, targets = SI.case(N, "random", 9)
    rep = selective.selective_report(preds, targets, score="entropy", bootstrap=3, seed=11, coverages=("0.25", "1"), risks=("0", "0.2"),
                                     thresholds=torch.tensor([-0.5] * 8))
    order, last, _, ties = SI.ranked(preds, targets, "entropy")
    flg = SI.flags(preds, targets)
    key = selective.keys(preds, "entropy").numpy()
    pcuts = [[int((key[t] >= -0.5).sum())] for t in range(8)]
    kcuts, risks = [33, N], [(0, 1), (1, 5)]
    assert rep["coverage_cuts"] == kcuts and rep["position_cuts"].tolist() == pcuts and rep["ties"].tolist() == ties.tolist()
    assert np.array_equal(rep["counts"].numpy(), SI.records(order, flg, last, None, kcuts, risks, pcuts))
    reps = np.stack([SI.records(order, flg, last, SI.multiplicities(11, r, N), kcuts, risks, pcuts) for r in range(3)])
    want = selective.values_from_counts(reps, N, kcuts, 2, 1)
    for x in ("summary", "coverage", "risk", "threshold"):
        assert np.array_equal(rep[x + "_replicates"].numpy(), want[x + "_values"]), x
    curve = selective.curve(preds, targets, "entropy")
    assert torch.equal(curve[:, -1], rep["summary_values"][3, :8]) and torch.equal(curve[:, 32], rep["coverage_values"][0, 0, :8])


def test_replicates_resample_the_cases_of_the_calibration_report():
    from sm3hip import calibration, selective
    N, B = 257, 12
    preds, targets = SI.case(N, "random", 6)
    sel = selective.selective_report(preds, targets, bootstrap=B, seed=SEED)
    errors = np.rint(sel["summary_replicates"][:, 3, :8].numpy() * N).astype(np.int64)              # E of (replicate, label)
    assert np.array_equal(errors / float(N), sel["summary_replicates"][:, 3, :8].numpy())
    for bins in (1, 15):
        cal = calibration.calibration_report(preds, targets, bins=bins, bootstrap=B, seed=SEED)
        d = cal["diagram_replicates"][:, :8].numpy()                                                 # the top-label series: n_b, acc_b
        correct = np.rint(d[..., 0] * d[..., 1]).astype(np.int64).sum(axis=-1)                       # sum over the bins of E_b
        assert np.array_equal(N - errors, correct), bins
    assert len({tuple(e) for e in errors.tolist()}) > 1


def test_msp_and_margin_coincide_on_two_class_labels():
    from sm3hip import selective
    preds, targets = SI.case(300, "random", 7)
    a = selective.selective_report(preds, targets, score="msp", bootstrap=5, seed=3)
    b = selective.selective_report(preds, targets, score="margin", bootstrap=5, seed=3)
    for t in (2, 7):
        assert torch.equal(a["counts"][t], b["counts"][t])
        for x in ("summary", "coverage", "risk"):
            assert torch.equal(a[x + "_replicates"][..., t], b[x + "_replicates"][..., t])
    assert not torch.equal(a["counts"][0], b["counts"][0])                                           # five classes: another ranking


def test_fit_thresholds_then_report_on_another_split():
    from sm3hip import selective
    fit_preds, fit_targets = SI.case(97, "ties", 1)
    thr = selective.fit_thresholds(fit_preds, fit_targets, "0.4")
    assert thr.dtype == torch.float64 and tuple(thr.shape) == (8,)
    order, last, ks, _ = SI.ranked(fit_preds, fit_targets)
    rec = SI.records(order, SI.flags(fit_preds, fit_targets), last, None, [97], [(2, 5)], [[]] * 8)
    assert np.array_equal(thr.numpy(), selective.cut_thresholds(ks, rec[:, 7]))
    own = selective.selective_report(fit_preds, fit_targets, thresholds=thr, risks=("0.4",))
    assert torch.equal(own["threshold_values"][0, :2], own["risk_values"][0])                        # at home: the risk cut itself
    none = selective.fit_thresholds(*SI.case(97, "all_errors", 1), "0.5")
    assert bool(torch.isinf(none).all())
    other = selective.selective_report(*SI.case(131, "ties", 2), thresholds=none)
    assert not other["threshold_values"][0, 0].any() and bool(other["position_cuts"].eq(0).all())


# ---- 3. the tool ---------------------------------------------------------------------------------------------------------
def _check_files(path, stem, rep):
    from sm3hip import selective
    saved = json.load(open(os.path.join(path, stem + ".json")))
    for key in VALUE_KEYS + ("counts", "thresholds", "ties", "position_cuts") + (BOOT_KEYS[1:4] if "summary_lo" in rep else ()):
        assert saved[key] == rep[key].tolist(), key
    for key in ("coverages", "risks", "coverage_cuts", "n", "temperature"):
        assert saved[key] == rep[key], key
    assert "targets" not in saved and "summary_replicates" not in saved
    rows = open(os.path.join(path, stem + ".csv")).read().splitlines()
    want = selective.csv_rows(rep)
    assert len(rows) == 1 + len(want)
    for row, w in zip(rows[1:], want):
        cells = row.split(",")
        assert cells[:4] == [str(v) for v in w[:4]] and [float(v) for v in cells[4:]] == [float(v) for v in w[4:]]


def test_eval_report_selective(tmp_path, capsys):
    from sm3hip import selective
    er = _load("sm3_selective_gpu_eval_report", os.path.join(TOOLS, "eval_report.py"))
    N = 97
    files = {}
    g = torch.Generator().manual_seed(5)
    for name, kind in (("test", "random"), ("other", "ties")):
        preds, targets = SI.make_case(N, kind, 2)
        preds = [3.0 * p for p in preds]
        lo = torch.randint(0, 2 ** 31, (N, 24), generator=g)
        files[name] = (preds, targets, {"min_q": lo, "max_q": lo + torch.randint(0, 2 ** 31, (N, 24), generator=g)})
        torch.save({"preds": preds, "targets": targets, "tta": files[name][2]}, tmp_path / f"{name}_predictions.pt")
    assert torch.equal(files["test"][1], files["other"][1])
    path = lambda n: str(tmp_path / f"{n}_predictions.pt")                          # noqa: E731
    plain = er.main([path("test"), "--out", str(tmp_path / "plain")])
    assert "selective" not in plain and not [f for f in os.listdir(tmp_path / "plain") if "selective" in f]
    out = capsys.readouterr().out                                                   # the test's own directory name holds the word
    assert "selective prediction" not in out and "AURC" not in out and "thresholds fitted" not in out
    test, other = files["test"][:2], files["other"][:2]
    kw = dict(bootstrap=20, seed=9, confidence=0.95)
    argv = [path("test"), "--selective", "--bootstrap", "20", "--bootstrap-seed", "9", "--selective-score", "margin",
            "--selective-coverage", "0.5", "0.75", "1", "--selective-risk", "0.1", "0.35", "--selective-rule", "0.35",
            "--fit-on", path("other"), "--against", path("other")]
    res = er.main(argv + ["--out", str(tmp_path / "a")])
    out = capsys.readouterr().out
    assert "selective prediction: margin ranking of 97 cases" in out and "AURC_AVG" in out and "thresholds fitted on" in out
    thr = selective.fit_thresholds(*other, "0.35", "margin")
    want = selective.selective_report(*test, score="margin", coverages=("0.5", "0.75", "1"), risks=("0.1", "0.35"), thresholds=thr, **kw)
    for key in VALUE_KEYS + BOOT_KEYS + ("counts", "thresholds"):
        assert _same(res["selective"][key], want[key]), key
    assert res["selective"]["rule"] == "0.35" and torch.equal(res["selective"]["thresholds"][:, 0], thr)
    _check_files(str(tmp_path / "a"), "test_predictions_selective", want)
    against = selective.selective_report(*other, score="margin", coverages=("0.5", "0.75", "1"), risks=("0.1", "0.35"), **kw)
    cmp = selective.compare(want, against)
    saved = json.load(open(tmp_path / "a" / "test_predictions_selective_compare.json"))
    assert saved["summary_delta"] == cmp["summary_delta"].tolist() and saved["risk_hi"] == cmp["risk_hi"].tolist()
    assert saved["coverage_frac_le_zero"] == cmp["coverage_frac_le_zero"].tolist()
    er.main(argv + ["--out", str(tmp_path / "b")])
    capsys.readouterr()
    for f in ("test_predictions_selective.json", "test_predictions_selective.csv", "test_predictions_selective_compare.json"):
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    res = er.main([path("test"), "--selective", "--selective-score", "tta-range", "--out", str(tmp_path / "c")])
    capsys.readouterr()
    tta = files["test"][2]
    yhat = torch.stack([p.argmax(dim=1) for p in test[0]], dim=1)
    first = [0, 5, 8, 10, 13, 16, 19, 22]
    score = torch.stack([-(tta["max_q"] - tta["min_q"])[torch.arange(N), first[t] + yhat[:, t]].double() for t in range(8)], dim=1)
    by_hand = selective.selective_report(*test, score=score)
    for key in VALUE_KEYS + ("counts", "ties"):
        assert _same(res["selective"][key], by_hand[key]), key
    assert res["selective"]["score"] == "tta-range"
    assert json.load(open(tmp_path / "c" / "test_predictions_selective.json"))["score"] == "tta-range"
    torch.save({"preds": test[0], "targets": test[1]}, tmp_path / "bare_predictions.pt")
    with pytest.raises(ValueError, match="tta"):
        er.main([path("bare"), "--selective", "--selective-score", "tta-range", "--out", str(tmp_path / "d")])
