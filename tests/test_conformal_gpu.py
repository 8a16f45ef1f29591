"""GPU: the conformal report (csrc/conformal.hip, sm3hip/conformal.py, tools/eval_report.py --conformal).

  * sm3_conformal_counts equal (==) to the restatement of tests/conformal_inputs.py, counts and thr: the point call and
    replicates; N_cal and N each over {1, 2, 8, 9, 19, 63, 64, 65, 255, 257, 395, 1023, 1025, 8192} (the scan's tile edges, the
    rank edges, the LDS limit), paired so that every size meets several others on the other side; A in {1, 3, 8}; both methods
    and both conditionings; heavily tied, all-equal and continuous scores, q = 0 and q = 2^32, a class absent from the
    calibration split (INF in class mode), a class that some replicates draw zero times; seeds that use both key words,
    replicate offsets up to 2^20, a replicate range cut into launches of 1 and 7; the outputs pre-filled with a sentinel;
  * the shared streams: fixed thresholds come back in every replicate; n_c == P of sm3_report_counts' column (the test
    replicates are those of every report); the calibration multiplicities, recovered from the thresholds, are the host rule on
    stream word 6 and not word 2's;
  * the library: equal bits across calls, chunks and bootstrap sizes, the restatement's values, refit = False, temperature;
  * argument errors return SM3_EINVAL and leave the sentinel untouched (nothing here provokes a device fault);
  * eval_report.py --conformal --fit-on writes files equal to conformal_report of the predictions it read."""
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
SIZES = (1, 2, 8, 9, 19, 63, 64, 65, 255, 257, 395, 1023, 1025, 8192)
LEVELS = {1: (0.1,), 3: (0.05, 0.1, 0.2), 8: (0.5, 0.333333, 0.2, 0.1, 0.05, 0.02, 0.01, 0.001)}
KINDS = ("ties", "equal", "absent", "random")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CI = _load("sm3_conformal_inputs_gpu", os.path.join(ROOT, "tests", "conformal_inputs.py"))
INF = CI.INF


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
def _dev(split):
    return [p.to(DEV) for p in split[0]], split[1].to(DEV)


def _inputs(cal, test, method, temperature=None):
    from sm3hip import conformal
    return conformal._device_inputs(test[0], test[1], cal[0], cal[1], conformal.calibration.check_temperature(temperature), method, DEV)


def _levels(alphas):
    return [(CI.fraction(a).numerator, CI.fraction(a).denominator) for a in alphas]


def _counts(inp, levels, conditional, seed, r0, c, point=False, fixed=None):
    from sm3hip import ops
    A = len(levels)
    counts = torch.full((c, 8, A, 24), SENTINEL, dtype=torch.int64, device=DEV)
    thr = torch.full((c, 8, A, 5), SENTINEL, dtype=torch.int64, device=DEV)
    ops.conformal_counts(*inp, levels, counts, thr, conditional, seed, r0, point=point,
                         fixed_thr=None if fixed is None else torch.as_tensor(fixed, device=DEV).contiguous())
    torch.cuda.synchronize()
    counts, thr = counts.cpu().numpy(), thr.cpu().numpy()
    assert not (counts == SENTINEL).any() and not (thr == SENTINEL).any()          # every element is overwritten
    return counts, thr


def _pairs():
    """Every size on either side, each with three partners: itself shifted by 0, 5 and 9 places."""
    n = len(SIZES)
    return [(SIZES[i], SIZES[(i + s) % n]) for s in (0, 5, 9) for i in range(n)]


@pytest.mark.parametrize("N_cal,N", _pairs())
def test_counts_and_thresholds_equal_the_restatement(N_cal, N):
    i = SIZES.index(N_cal) + 3 * SIZES.index(N)
    kind, big = KINDS[i % 4], max(N_cal, N) > 1100
    cal, test = _dev(CI.case(N_cal, kind, 7 * N_cal + i)), _dev(CI.case(N, KINDS[(i + 1) % 4], 5 * N + i))
    A = (1, 3, 8)[i % 3] if not big else (3, 1)[i % 2]
    alphas, levels = LEVELS[A], _levels(LEVELS[A])
    seed, r0, c = SEEDS[i % 3]
    c = min(c, 2) if big else c                                                     # the host restatement is the slow side
    for method in (("lac", "aps")[i % 2:][:1] if big else ("lac", "aps")):
        R = CI.Restated(cal, test, method)
        if kind != "equal" and method == "lac" and N_cal >= 8:
            assert (R.cal_s == 0).any() and (R.cal_s == 1 << 32).any()              # q = 2^32 and q = 0
        inp = _inputs(cal, test, method)
        for conditional in ("marginal", "class"):
            counts, thr = _counts(inp, levels, conditional, seed, 0, 1, point=True)
            wc, wt = R(alphas, conditional)
            assert np.array_equal(thr[0], wt) and np.array_equal(counts[0], wc), (method, conditional, "point")
            if kind == "absent" and conditional == "class":
                assert (thr[0][:, :, 1] == INF).all()
            if conditional == "marginal" and N_cal == 8 or N_cal in (1, 2):
                assert (thr[0][0, alphas.index(0.1)] == INF).all()                  # the rank edge: every set is full
            counts, thr = _counts(inp, levels, conditional, seed, r0, c)
            for j in (range(c) if c <= 3 else (0, 1, 11, c - 1)):
                w, m = CI.multiplicities(seed, r0 + j, N_cal, 6), CI.multiplicities(seed, r0 + j, N, 2)
                wc, wt = R(alphas, conditional, w=w, m=m)
                assert np.array_equal(thr[j], wt), (method, conditional, seed, r0 + j)
                assert np.array_equal(counts[j], wc), (method, conditional, seed, r0 + j)
            assert (counts[..., 3:9].sum(axis=-1) == N).all()
            if not big:                                                             # any cut of [r0, r0 + c) is the one call
                for step in (1, 7):
                    parts = [_counts(inp, levels, conditional, seed, r0 + k, min(step, c - k)) for k in range(0, c, step)]
                    assert np.array_equal(np.concatenate([p[0] for p in parts]), counts)
                    assert np.array_equal(np.concatenate([p[1] for p in parts]), thr)
                fixed = thr[0]                                                      # fixed thresholds come back, in every replicate
                fc, ft = _counts(inp, levels, conditional, seed, r0, c, fixed=fixed)
                assert (ft == fixed[None]).all()
                wc, _ = R(alphas, conditional, m=CI.multiplicities(seed, r0 + c - 1, N, 2), fixed=fixed)
                assert np.array_equal(fc[c - 1], wc)


def test_a_class_that_some_replicates_never_draw():
    preds, targets = CI.case(19, "random", 3)
    targets[:, 0] = torch.arange(19) % 4
    targets[5, 0] = 4                                                               # one calibration case of DIAG class 4
    cal, test = _dev((preds, targets)), _dev(CI.case(65, "ties", 4))
    R = CI.Restated(cal, test, "aps")
    alphas = (0.5, 0.2)
    counts, thr = _counts(_inputs(cal, test, "aps"), _levels(alphas), "class", 11, 0, 24)
    drawn = []
    for r in range(24):
        w = CI.multiplicities(11, r, 19, 6)
        wc, wt = R(alphas, "class", w=w, m=CI.multiplicities(11, r, 65, 2))
        assert np.array_equal(thr[r], wt) and np.array_equal(counts[r], wc), r
        drawn.append(int(w[5]))
        assert (thr[r, 0, 0, 4] == INF) == (w[5] == 0)                              # alpha = 0.5: k = 1 of one copy or more
    assert 0 in drawn and max(drawn) > 0


def test_permutations_of_the_cases_change_nothing_at_the_point():
    cal, test = CI.case(257, "ties", 1), CI.case(65, "ties", 2)
    g = torch.Generator().manual_seed(0)
    pc, pt = torch.randperm(257, generator=g), torch.randperm(65, generator=g)
    cal2, test2 = ([p[pc] for p in cal[0]], cal[1][pc]), ([p[pt] for p in test[0]], test[1][pt])
    for method in ("lac", "aps"):
        for conditional in ("marginal", "class"):
            a = _counts(_inputs(_dev(cal), _dev(test), method), _levels(LEVELS[3]), conditional, 0, 0, 1, point=True)
            b = _counts(_inputs(_dev(cal2), _dev(test2), method), _levels(LEVELS[3]), conditional, 0, 0, 1, point=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_test_replicates_are_those_of_the_evaluation_report():
    from sm3hip import ops, report
    for N, seed, r0 in ((395, 2 ** 63 + 11, 5), (65, 7, 2 ** 20)):
        test, cal = _dev(CI.case(N, "ties", N)), _dev(CI.case(40, "random", 1))
        order, gs, ge, yhat = report.ranking(*test)
        colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV)
        out = torch.empty((4, 24, 6), dtype=torch.int64, device=DEV)
        ops.report_counts(order, gs, ge, test[1].int().contiguous(), yhat, colmap, out, seed, r0)
        P = out[:, :, 1].cpu().numpy()
        for conditional in ("marginal", "class"):
            counts, _ = _counts(_inputs(cal, test, "lac"), _levels(LEVELS[3]), conditional, seed, r0, 4)
            for k, (t, c) in enumerate(CI.PAIRS):
                assert (counts[:, t, :, 9 + 3 * c] == P[:, k, None]).all(), (conditional, k)
        assert len({tuple(P[r]) for r in range(4)}) > 1


def test_calibration_replicates_are_stream_six():
    """N_cal = 8 distinct scores and the levels j / 9, j = 1 .. 8: k = 9 - j takes every rank, so the eight thresholds of a
    replicate are its w-fold copies in order, and w is their count per case."""
    split = _dev(CI.make_case(8, "random", 21))                                     # continuous logits: no two scores equal
    inp = _inputs(split, split, "lac")
    cal_a = inp[0].cpu().numpy()
    assert all(len(set(cal_a[t].tolist())) == 8 for t in range(8))
    levels = [(j, 9) for j in range(1, 9)]
    seed, r0, c = 2 ** 63 + 11, 2 ** 20 - 3, 6
    _, thr = _counts(inp, levels, "marginal", seed, r0, c)
    differs = 0
    for j in range(c):
        w6, w2 = CI.multiplicities(seed, r0 + j, 8, 6), CI.multiplicities(seed, r0 + j, 8, 2)
        for t in range(8):
            got = np.array([(thr[j, t, :, 0] == v).sum() for v in cal_a[t]])
            assert np.array_equal(got, w6), (j, t)
        differs += not np.array_equal(w6, w2)
    assert differs > 0


def test_argument_errors_leave_the_outputs_untouched():
    import ctypes as C
    from sm3hip import _lib, ops
    split = _dev(CI.case(5, "ties", 1))
    inp = _inputs(split, split, "lac")
    counts = torch.full((2, 8, 8, 24), SENTINEL, dtype=torch.int64, device=DEV)
    thr = torch.full((2, 8, 8, 5), SENTINEL, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    ptr = [ops._ptr(a) for a in inp]

    def call(N_cal=5, N=5, A=1, conditional=0, r0=0, c=1, point=0, alpha=(1, 10)):
        lv = (C.c_int * 16)(*(list(alpha) * 8))
        return lib.sm3_conformal_counts(*ptr, lv, None, ops._ptr(counts), ops._ptr(thr), N_cal, N, 8, 24, A, conditional, 0, r0, c,
                                        point, ops._stream())
    for kw in ({"N_cal": 0}, {"N": 0}, {"N_cal": 8193}, {"N": 8193}, {"A": 0}, {"A": 9}, {"conditional": 2}, {"c": 0}, {"r0": -1},
               {"point": 1, "c": 2}, {"alpha": (0, 10)}, {"alpha": (10, 10)}, {"alpha": (11, 10)}, {"alpha": (1, 0)}, {"alpha": (1, -3)}):
        assert call(**kw) == -1, kw                                                 # SM3_EINVAL
    torch.cuda.synchronize()
    assert bool((counts == SENTINEL).all()) and bool((thr == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.conformal_counts(*inp, [(1, 10)], counts[:1, :, :1].contiguous().cpu(), thr[:1, :, :1].contiguous(), "marginal", 0, 0)
    with pytest.raises(ValueError):
        ops.conformal_counts(*inp, [(1, 10)], counts[:, :, :1].contiguous(), thr[:, :, :1].contiguous(), "marginal", 0, 0, point=True)


# ---- 2. the library ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def splits():
    return _dev(CI.case(150, "random", 41)), _dev(CI.case(395, "random", 42))       # calibration, test


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


VALUE_KEYS = ("label_values", "class_values", "threshold_values")
BOOT_KEYS = tuple(f"{t}_{e}" for t in ("label", "class", "threshold") for e in ("replicates", "lo", "hi"))


@pytest.mark.parametrize("conditional", ["marginal", "class"])
def test_bits_do_not_depend_on_call_chunk_or_bootstrap_size(splits, conditional):
    from sm3hip import conformal, report
    cal, test = splits
    before = [p.clone() for p in test[0] + cal[0]]
    B, kw = 23, dict(conditional=conditional, method="aps", seed=2 ** 63 + 11)
    first = conformal.conformal_report(*test, *cal, bootstrap=B, **kw)
    assert first["counts"].shape == (8, 3, 24) and first["thresholds"].shape == (8, 3, 5) and first["label_values"].shape == (3, 5, 9)
    assert first["class_values"].shape == (3, 2, 29) and first["threshold_values"].shape == (3, 8, 5)
    assert first["label_replicates"].shape == (B, 3, 5, 9) and first["class_columns"] == report.COLUMNS
    assert first["alphas"] == [0.05, 0.1, 0.2] and first["levels"] == [[1, 20], [1, 10], [1, 5]] and first["n_cal"] == 150
    for chunk in (None, 1, 7, B):
        again = conformal.conformal_report(*test, *cal, bootstrap=B, chunk=chunk, **kw)
        for key in VALUE_KEYS + BOOT_KEYS:
            assert _same(first[key], again[key]), (chunk, key)
        assert torch.equal(first["counts"], again["counts"]) and torch.equal(first["thresholds"], again["thresholds"])
        assert torch.equal(first["class_undefined"], again["class_undefined"])
    seven = conformal.conformal_report(*test, *cal, bootstrap=7, **kw)
    for t in ("label", "class", "threshold"):
        assert _same(first[f"{t}_replicates"][:7].contiguous(), seven[f"{t}_replicates"])
    ones = conformal.conformal_report(*test, *cal, temperature=[1.0] * 8, bootstrap=7, refit=False, **kw)
    fixed = conformal.conformal_report(*test, *cal, bootstrap=7, refit=False, **kw)
    for key in VALUE_KEYS + BOOT_KEYS:
        assert _same(ones[key], fixed[key]), key
    assert _same(fixed["label_values"], first["label_values"]) and not _same(fixed["label_replicates"], seven["label_replicates"])
    assert (fixed["threshold_replicates"] == fixed["threshold_values"][None]).all()
    assert (fixed["threshold_lo"] == fixed["threshold_hi"]).all() and not (seven["threshold_lo"] == seven["threshold_hi"]).all()
    other = conformal.conformal_report(*test, *cal, bootstrap=7, conditional=conditional, method="aps", seed=2 ** 63 + 12)
    assert not _same(other["label_replicates"], seven["label_replicates"]) and _same(other["label_values"], seven["label_values"])
    none = conformal.conformal_report(*test, *cal, **kw)
    assert "label_replicates" not in none and _same(none["label_values"], first["label_values"])
    cpu = conformal.conformal_report([p.cpu() for p in test[0]], test[1].cpu(), [p.cpu() for p in cal[0]], cal[1].cpu(), **kw)
    assert torch.equal(cpu["counts"], first["counts"]) and torch.equal(cpu["thresholds"], first["thresholds"])
    for t in ("label", "class", "threshold"):
        lo, hi = report.interval(first[f"{t}_replicates"].numpy(), 0.95)
        assert np.array_equal(first[f"{t}_lo"].numpy(), lo) and np.array_equal(first[f"{t}_hi"].numpy(), hi)
    thr = conformal.fit_thresholds(*cal, alphas=(0.05, 0.1, 0.2), method="aps", conditional=conditional)
    assert torch.equal(thr, first["thresholds"])
    sets = conformal.prediction_sets(test[0], thr, level=1, method="aps").cpu().numpy()
    for k, (t, c) in enumerate(CI.PAIRS):
        assert int(sets[:, k].sum()) == int(first["counts"][t, 1, 11 + 3 * c])       # in_c of the point record
    for p, q in zip(test[0] + cal[0], before):                                      # inputs are not modified
        assert torch.equal(p, q)


def test_replicates_are_the_restatement_through_the_library(splits):
    from sm3hip import conformal
    cal, test = splits
    temp = [0.5, 1.0, 2.0, 1.25, 1.0, 3.0, 0.75, 1.0]
    alphas = (0.25, 0.1)
    for method, conditional, refit in (("lac", "class", True), ("aps", "marginal", True), ("lac", "marginal", False)):
        rep = conformal.conformal_report(*test, *cal, alphas=alphas, method=method, conditional=conditional, temperature=temp,
                                         refit=refit, bootstrap=3, seed=7)
        R = CI.Restated(cal, test, method, temp)
        wc, wt = R(alphas, conditional)
        assert np.array_equal(rep["counts"].numpy(), wc) and np.array_equal(rep["thresholds"].numpy(), wt)
        label, cls, tv = CI.values(wc.tolist(), wt.tolist(), 395)
        assert rep["label_values"].tolist() == label and rep["class_values"][:, :, :24].tolist() == cls
        assert rep["threshold_values"].tolist() == tv
        for r in range(3):
            rc, rt = R(alphas, conditional, w=CI.multiplicities(7, r, 150, 6), m=CI.multiplicities(7, r, 395, 2),
                       fixed=None if refit else wt)
            label, cls, tv = CI.values(rc.tolist(), rt.tolist(), 395)
            assert rep["label_replicates"][r].tolist() == label and rep["class_replicates"][r, :, :, :24].tolist() == cls
            assert rep["threshold_replicates"][r].tolist() == tv
    plain = conformal.conformal_report(*test, *cal)
    hot = conformal.conformal_report(*test, *cal, temperature=[4.0] * 8)
    assert not torch.equal(plain["thresholds"], hot["thresholds"])
    c = conformal.compare(hot, plain)
    assert "label_lo" not in c and c["label_delta"].shape == (3, 5, 9)
    with pytest.raises(ValueError, match="method"):
        conformal.compare(plain, conformal.conformal_report(*test, *cal, method="aps"))


# ---- 3. the tool ---------------------------------------------------------------------------------------------------------
def _check_files(path, stem, rep):
    saved = json.load(open(os.path.join(path, stem + ".json")))
    for key in VALUE_KEYS + ("counts", "thresholds"):
        assert saved[key] == rep[key].tolist(), key
    for key in ("method", "conditional", "refit", "alphas", "temperature", "n", "n_cal"):
        assert saved[key] == rep[key], key
    if "label_lo" in rep:
        assert saved["label_lo"] == rep["label_lo"].tolist() and saved["class_hi"] == rep["class_hi"].tolist()
        assert saved["bootstrap"] == rep["bootstrap"] and saved["seed"] == rep["seed"]
    rows = list(csv.reader(open(os.path.join(path, stem + ".csv"))))
    by = {(r[0], float(r[1]), r[2], r[3]): r for r in rows[1:]}
    for a, alpha in enumerate(rep["alphas"]):
        for i, m in enumerate(rep["label_metrics"]):
            for k, c in enumerate(rep["label_columns"]):
                assert float(by[("label", alpha, m, c)][4]) == float(rep["label_values"][a, i, k])
                if "label_lo" in rep:
                    assert float(by[("label", alpha, m, c)][5]) == float(rep["label_lo"][a, i, k])


def test_eval_report_conformal(tmp_path, capsys):
    from sm3hip import calibration, conformal
    er = _load("sm3_conformal_gpu_eval_report", os.path.join(TOOLS, "eval_report.py"))
    files = {}
    for name, N, kind, seed in (("val", 120, "random", 1), ("test", 200, "random", 2), ("val_b", 120, "ties", 1), ("test_b", 200, "ties", 2)):
        preds, targets = CI.make_case(N, kind, seed)
        preds = [3.0 * p for p in preds]
        files[name] = (preds, targets)
        torch.save({"preds": preds, "targets": targets}, tmp_path / f"{name}_predictions.pt")
    assert torch.equal(files["val"][1], files["val_b"][1]) and torch.equal(files["test"][1], files["test_b"][1])
    path = lambda n: str(tmp_path / f"{n}_predictions.pt")                          # noqa: E731
    plain = er.main([path("test"), "--fit-on", path("val"), "--out", str(tmp_path / "plain")])
    assert "conformal" not in plain and not [f for f in os.listdir(tmp_path / "plain") if "conformal" in f]
    capsys.readouterr()
    test, cal = files["test"], files["val"]
    kw = dict(bootstrap=20, seed=9, confidence=0.95)
    res = er.main([path("test"), "--conformal", "--fit-on", path("val"), "--bootstrap", "20", "--bootstrap-seed", "9",
                   "--conformal-alpha", "0.1", "0.25", "--conformal-conditional", "class", "--out", str(tmp_path / "a")])
    out = capsys.readouterr().out
    assert "conformal: lac scores, class thresholds from 120 cases" in out and "coverage_AVG@0.1" in out
    want = conformal.conformal_report(*test, *cal, alphas=(0.1, 0.25), conditional="class", **kw)
    for key in VALUE_KEYS + BOOT_KEYS:
        assert _same(res["conformal"][key], want[key]), key
    _check_files(str(tmp_path / "a"), "test_predictions_conformal", want)
    assert os.path.isfile(tmp_path / "a" / "test_predictions_calibration_fitted.json")     # --fit-on still implies --calibration
    res = er.main([path("test"), "--conformal", "--fit-on", path("val"), "--bootstrap", "20", "--bootstrap-seed", "9", "--conformal-fixed",
                   "--conformal-scaled", "--conformal-method", "aps", "--against", path("test_b"), "--against-fit-on", path("val_b"),
                   "--out", str(tmp_path / "b")])
    out = capsys.readouterr().out
    assert "fixed in the replicates" in out and "coverage difference" in out
    fit = calibration.fit_temperature(*cal)
    assert res["fit"] == fit
    want = conformal.conformal_report(*test, *cal, method="aps", refit=False, temperature=fit["temperature"], **kw)
    _check_files(str(tmp_path / "b"), "test_predictions_conformal", want)
    other = conformal.conformal_report(*files["test_b"], *files["val_b"], method="aps", refit=False,
                                       temperature=calibration.fit_temperature(*files["val_b"])["temperature"], **kw)
    cmp = conformal.compare(want, other)
    assert torch.equal(res["conformal_compare"]["label_delta"], cmp["label_delta"])
    assert torch.equal(res["conformal_compare"]["class_lo"], cmp["class_lo"])
    saved = json.load(open(tmp_path / "b" / "test_predictions_conformal_compare.json"))
    assert saved["label_delta"] == cmp["label_delta"].tolist() and saved["label_hi"] == cmp["label_hi"].tolist()
    assert torch.equal(res["report"]["values"], plain["report"]["values"])
