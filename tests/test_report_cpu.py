"""CPU: the evaluation report (sm3hip/report.py, csrc/report.hip) restated in numpy and Python integers, and everything about it
that needs no GPU.  tests/test_report_gpu.py loads this file for the restatement.

  * the restatement (Philox multiplicities, integer counts per column, values by one division) against scikit-learn:
    recall_score / precision_score(average=None, zero_division=0), specificity from confusion_matrix, and
    roc_auc_score(sample_weight=m) on resampled columns with P * Q > 0, within 1e-12 (torchmetrics is not installed where this
    was written: parity with it stays a restatement);
  * the point AUROC of every column bit-equal (==) to metrics.multiclass_auroc: integer-quantised logits with many ties,
    all-equal logits (exactly 0.5), an absent class, N in {1, 2, 5, 64, 65, 257, 1000};
  * the five averaging rules reproduce every row of both reference tables (tests/golden/reference_*_results.csv: recorded
    results) to the printed precision;
  * host-side checks: the interval index rule, compare's refusals, the CSV layout, every new flag in the four tools, the
    new entry point's -1 on bad arguments from the built library."""
import csv
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
PAIRS = [(t, c) for t, n in enumerate(NUM_CLASSES) for c in range(n)]
M32 = np.uint64(0xFFFFFFFF)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC 2011) on uint64 arrays holding 32-bit words -> the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def multiplicities(seed, r, N):
    """m_r [N] int64: draw d hits case (w * N) >> 32, w = word d % 4 of call d // 4 with counter (d // 4, r, 0, 2)."""
    q = np.arange((N + 3) // 4, dtype=np.uint64)
    w = np.stack(philox4x32_10(q, np.uint64(r), np.uint64(0), np.uint64(2), seed & 0xFFFFFFFF, seed >> 32), axis=1).reshape(-1)[:N]
    idx = (w * np.uint64(N)) >> np.uint64(32)
    return np.bincount(idx.astype(np.int64), minlength=N).astype(np.int64)


def counts(order, gs, ge, y, yhat, m):
    """[24, 6] int64 (A2, P, Q, TP, FP, FN) of the columns for the multiplicities m, in Python-exact int64 arithmetic."""
    order, gs, ge = (np.asarray(a, dtype=np.int64) for a in (order, gs, ge))
    y, yhat, m = (np.asarray(a, dtype=np.int64) for a in (y, yhat, m))
    N = y.shape[0]
    out = np.zeros((len(PAIRS), 6), dtype=np.int64)
    for k, (t, c) in enumerate(PAIRS):
        mm = m[order[k]]
        pos = y[order[k], t] == c
        S = np.concatenate([[0], np.cumsum(np.where(pos, 0, mm))])
        A2 = int(np.sum(np.where(pos, mm * (S[gs[k]] + S[ge[k]]), 0)))
        P = int(m[y[:, t] == c].sum())
        TP = int(m[(y[:, t] == c) & (yhat[:, t] == c)].sum())
        FP = int(m[(y[:, t] != c) & (yhat[:, t] == c)].sum())
        FN = int(m[(y[:, t] == c) & (yhat[:, t] != c)].sum())
        out[k] = (A2, P, N - P, TP, FP, FN)
    return out


def make_case(N, kind, seed):
    """preds (8 x [N, n_t] float32) and targets [N, 8] int64.  kind: "ties" integer-quantised logits (many tied scores),
    "equal" all-equal logits, "absent" class 1 of every label missing from the targets, "constant" label 0 predicted as class 3
    throughout, "random" continuous logits."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.stack([torch.randint(0, n, (N,), generator=g) for n in NUM_CLASSES], dim=1)
    if kind == "absent":
        targets[targets == 1] = 0
    preds = []
    for t, n in enumerate(NUM_CLASSES):
        if kind == "equal":
            p = torch.zeros(N, n)
        elif kind == "random":
            p = torch.randn(N, n, generator=g)
        else:
            p = torch.randint(-2, 3, (N, n), generator=g).float()
        if kind == "constant" and t == 0:
            p[:, 3] = 7.0
        preds.append(p)
    return preds, targets


def restated_inputs(preds, targets):
    """(order, gs, ge, y, yhat) as numpy int64, through the library's own ranking (torch plumbing) on the tensors' device."""
    from sm3hip import report
    order, gs, ge, yhat = report.ranking(preds, targets)
    return tuple(a.cpu().numpy().astype(np.int64) for a in (order, gs, ge, targets, yhat))


def test_ranking_groups_are_the_tie_groups_of_a_stable_ascending_sort():
    from sm3hip import report
    preds, targets = make_case(257, "ties", 3)
    order, gs, ge, y, yhat = restated_inputs(preds, targets)
    for k, (t, c) in enumerate(PAIRS):
        s = torch.softmax(preds[t].double(), 1)[:, c].numpy()
        assert np.array_equal(order[k], np.argsort(s, kind="stable"))
        ss = s[order[k]]
        for j in range(257):
            same = np.nonzero(ss == ss[j])[0]
            assert gs[k, j] == same[0] and ge[k, j] == same[-1] + 1
        assert np.array_equal(yhat[:, t], preds[t].numpy().argmax(1))
    assert report.COLUMN_PAIRS == PAIRS


def test_multiplicities_are_n_draws_and_a_function_of_seed_replicate_and_n():
    for N in (1, 2, 5, 63, 64, 65, 1000):
        m = multiplicities(2 ** 63 + 11, 5, N)
        assert m.sum() == N and m.min() >= 0 and m.shape == (N,)
    a, b = multiplicities(7, 3, 1000), multiplicities(7, 4, 1000)
    assert not np.array_equal(a, b) and np.array_equal(a, multiplicities(7, 3, 1000))
    assert not np.array_equal(a, multiplicities(2 ** 32 + 7, 3, 1000))      # the high word of the seed reaches the key
    # the share of cases left out of a resample tends to 1 / e
    assert abs(np.mean([np.mean(multiplicities(1, r, 1000) == 0) for r in range(50)]) - np.exp(-1)) < 0.01


# ---- 1. against scikit-learn ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 5, 64, 257, 1000, 8192])
def test_restatement_against_sklearn(N):
    from sklearn.metrics import confusion_matrix, precision_score, recall_score, roc_auc_score
    from sm3hip import report
    worst = 0.0
    for kind, resample in (("ties", False), ("ties", True), ("random", True), ("constant", True)):
        preds, targets = make_case(N, kind, N)
        order, gs, ge, y, yhat = restated_inputs(preds, targets)
        m = multiplicities(11, 2, N) if resample else np.ones(N, dtype=np.int64)
        cnt = counts(order, gs, ge, y, yhat, m)
        assert np.array_equal(cnt[:, 1] + cnt[:, 2], np.full(24, N))
        values, undefined = report.values_from_counts(cnt)
        keep = m > 0  # sklearn's label handling wants the cases that are there
        for t, n in enumerate(NUM_CLASSES):
            labels = list(range(n))
            cols = [PAIRS.index((t, c)) for c in labels]
            yt, yp, w = y[keep, t], yhat[keep, t], m[keep]
            rec = recall_score(yt, yp, labels=labels, average=None, zero_division=0, sample_weight=w)
            prec = precision_score(yt, yp, labels=labels, average=None, zero_division=0, sample_weight=w)
            cm = confusion_matrix(yt, yp, labels=labels, sample_weight=w)
            for c, k in zip(labels, cols):
                tp, fp = cm[c, c], cm[:, c].sum() - cm[c, c]
                fn = cm[c].sum() - cm[c, c]
                tn = cm.sum() - tp - fp - fn
                spec = tn / (tn + fp) if tn + fp else 0.0
                assert abs(values[1, k] - rec[c]) <= 1e-12 and abs(values[3, k] - prec[c]) <= 1e-12
                assert abs(values[2, k] - spec) <= 1e-12
                assert (cnt[k, 3], cnt[k, 4], cnt[k, 5]) == (tp, fp, fn)
                if cnt[k, 1] * cnt[k, 2] > 0:
                    score = torch.softmax(preds[t].double(), 1)[:, c].numpy()
                    ref = roc_auc_score(y[keep, t] == c, score[keep], sample_weight=w)
                    worst = max(worst, abs(values[0, k] - ref))
                else:
                    assert values[0, k] == 0.0 and undefined[0, k]
    print(f"N = {N}: worst |AUC - sklearn| = {worst:.3g}")
    assert worst <= 1e-12


# ---- 2. against metrics.multiclass_auroc ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 5, 64, 65, 257, 1000])
def test_point_auroc_is_bit_equal_to_multiclass_auroc(N):
    from sm3hip import metrics, report
    for kind in ("ties", "equal", "absent", "random", "constant"):
        preds, targets = make_case(N, kind, 100 + N)
        order, gs, ge, y, yhat = restated_inputs(preds, targets)
        values, _ = report.values_from_counts(counts(order, gs, ge, y, yhat, np.ones(N, dtype=np.int64)))
        for t, n in enumerate(NUM_CLASSES):
            want = metrics.multiclass_auroc(preds[t], targets[:, t], n).numpy()
            got = values[0, [PAIRS.index((t, c)) for c in range(n)]]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (kind, t, got, want)
            if kind == "equal":
                present = [(targets[:, t] == c).any() and (targets[:, t] != c).any() for c in range(n)]
                assert all(g == (0.5 if p else 0.0) for g, p in zip(got, present))
            if kind == "absent" and n > 1:
                assert got[1] == 0.0


# ---- 3. the averaging rules against the reference's tables ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["reference_linear_results.csv", "reference_finetune_results.csv"])
def test_the_five_averages_reproduce_the_reference_tables(name):
    """The tables hold float32 percentages printed with their shortest representation (8 significant digits).  Bound on
    |average - printed|: a printed per-class value carries a relative error of at most 2^-24 (float32) of at most 100, the
    reference's float32 running sum of at most 24 values below 2400 rounds by at most 2^-13 (half an ulp in [2048, 4096)) per
    addition, and the quotient and its printing by 2^-24 * 100 each: (24 * 100 * 2^-24 + 24 * 2^-13) / 5 + 2 * 100 * 2^-24 < 7e-4
    for the shortest average (5 columns); the fp64 arithmetic here adds nothing visible."""
    from sm3hip import report
    rows = list(csv.reader(open(os.path.join(GOLDEN, name))))
    header = rows[0][1:]
    assert header == report.CSV_COLUMNS
    assert [r[0] for r in rows[1:]] == list(report.CSV_ROWS)
    for r in rows[1:]:
        by_name = dict(zip(header, (float(v) for v in r[1:])))
        v24 = np.array([by_name[n] for n in report.CLASS_COLUMNS])
        got = report.averages(v24)
        for a, avg_name in enumerate(report.AVERAGES):
            print(f"{name} {r[0]:<7} {avg_name:<10} {got[a]:.6f} printed {by_name[avg_name]}")
            assert abs(got[a] - by_name[avg_name]) < 7e-4, (r[0], avg_name)
            shown = len(str(by_name[avg_name]).split(".")[1])  # to the printed digits, where float32 shows fewer than 4
            assert round(got[a], min(shown, 3)) == round(by_name[avg_name], min(shown, 3))
    assert rows[1][1:] == rows[3][1:]  # Acc is the per-class recall


# ---- 4. host-side checks --------------------------------------------------------------------------------------------------
def test_interval_index_rule():
    from sm3hip import report
    assert report.interval_index(1, 0.95) == 0
    assert report.interval_index(2000, 0.95) == 49     # floor(1999 * 0.025) = floor(49.975)
    assert report.interval_index(1000, 0.9) == 49      # floor(999 * 0.05) = floor(49.95)
    assert report.interval_index(41, 0.95) == 1        # floor(40 * 0.025): 1 - 0.95 is 0.05000000000000004 in float64
    assert report.interval_index(101, 0.5) == 25
    v = np.arange(41, dtype=np.float64)[::-1].copy()
    lo, hi = report.interval(v[:, None], 0.95)
    assert (lo[0], hi[0]) == (1.0, 39.0)


def _fake_report(report, seed=3, B=5, shift=0.0):
    rng = np.random.default_rng(1)
    rep = {"values": torch.from_numpy(rng.random((4, 29)) + shift), "targets": torch.zeros(6, 8, dtype=torch.int64),
           "columns": list(report.COLUMNS), "metrics": list(report.METRICS), "n": 6}
    if B:
        r = rng.random((B, 4, 29)) + shift
        lo, hi = report.interval(r, 0.95)
        rep.update({"replicates": torch.from_numpy(r), "lo": torch.from_numpy(lo.copy()), "hi": torch.from_numpy(hi.copy()),
                    "undefined": torch.zeros(4, 29, dtype=torch.int64), "bootstrap": B, "seed": seed, "confidence": 0.95})
    return rep


def test_compare_pairs_the_replicates_and_refuses_unpaired_reports():
    from sm3hip import report
    a, b = _fake_report(report, shift=1.0), _fake_report(report)
    c = report.compare(a, b)
    assert torch.equal(c["delta"], a["values"] - b["values"])
    d = (a["replicates"] - b["replicates"]).numpy()
    lo, hi = report.interval(d, 0.95)
    assert np.array_equal(c["lo"].numpy(), lo) and np.array_equal(c["hi"].numpy(), hi)
    assert np.array_equal(c["frac_le_zero"].numpy(), (d <= 0).mean(axis=0)) and float(c["frac_le_zero"].max()) == 0.0
    z = report.compare(a, a)
    assert not z["delta"].any() and not z["lo"].any() and not z["hi"].any() and float(z["frac_le_zero"].min()) == 1.0
    with pytest.raises(ValueError, match="seed"):
        report.compare(a, _fake_report(report, seed=4))
    with pytest.raises(ValueError, match="bootstrap"):
        report.compare(a, _fake_report(report, B=0))
    other = _fake_report(report)
    other["targets"] = other["targets"] + 1
    with pytest.raises(ValueError, match="targets"):
        report.compare(a, other)
    other["targets"] = torch.zeros(7, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="targets"):
        report.compare(a, other)
    assert "lo" not in report.compare(_fake_report(report, B=0), _fake_report(report, B=0))


def test_csv_layout_is_the_reference_tables_and_parses_back(tmp_path):
    from sm3hip import report
    for B in (0, 5):
        rep = _fake_report(report, B=B)
        path = tmp_path / f"r{B}.csv"
        report.to_csv(rep, str(path))
        rows = list(csv.reader(open(path)))
        assert rows[0] == [""] + report.CSV_COLUMNS
        names = [r[0] for r in rows[1:]]
        if B:
            assert names == [f"{n}{e}" for n in report.CSV_ROWS for e in ("", " lo", " hi")]
        else:
            assert names == ["Acc", "AUC", "Recall", "Spec", "Prec"]
        perm = [report.COLUMNS.index(n) for n in report.CSV_COLUMNS]
        for r in rows[1:]:
            parts = r[0].split(" ")
            i = report.METRICS.index("Recall" if parts[0] == "Acc" else parts[0])
            src = rep["values"] if len(parts) == 1 else rep[parts[1]]
            assert [float(v) for v in r[1:]] == [100.0 * float(src[i, k]) for k in perm]
    report.to_json(_fake_report(report), str(tmp_path / "r.json"))
    import json
    back = json.load(open(tmp_path / "r.json"))
    assert back["columns"] == report.COLUMNS and "replicates" not in back and len(back["lo"]) == 4


def test_settings_and_inputs_are_refused_before_any_device_work():
    from sm3hip import report
    preds, targets = make_case(5, "ties", 1)
    for kw in ({"bootstrap": -1}, {"bootstrap": 1.5}, {"bootstrap": True}, {"confidence": 0.0}, {"confidence": 1.0},
               {"seed": -1}, {"seed": 2 ** 64}, {"bootstrap": 4, "chunk": 0}, {"bootstrap": 4, "chunk": 5}):
        with pytest.raises(ValueError):
            report.evaluation_report(preds, targets, **kw)
    with pytest.raises(ValueError, match="NaN"):
        report.evaluation_report([p.clone().fill_(float("nan")) if t == 2 else p for t, p in enumerate(preds)], targets)
    with pytest.raises(ValueError, match="int64"):
        report.evaluation_report(preds, targets.int())
    with pytest.raises(ValueError):
        report.evaluation_report(preds[:7], targets)
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        report.evaluation_report(preds, targets + 5)
    big_p, big_t = make_case(report.MAX_CASES + 1, "equal", 1)
    with pytest.raises(ValueError, match=f"MAX_CASES = {report.MAX_CASES}"):
        report.evaluation_report(big_p, big_t)
    assert report.MAX_CASES >= 8192


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_report_cli_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["backbone_eval", "mlc_eval", "backbone_knn", "eval_report"])
def test_the_new_flags_parse(name):
    base = ["x.pt"] if name == "eval_report" else ["--data-name", "synthetic", "--data-path", "-"]
    parser = _tool(name).get_parser()
    d = parser.parse_args(base)
    assert (d.bootstrap, d.bootstrap_seed, d.confidence) == (0, 0, 0.95)
    a = parser.parse_args(base + ["--bootstrap", "2000", "--bootstrap-seed", str(2 ** 63 + 11), "--confidence", "0.9"])
    assert (a.bootstrap, a.bootstrap_seed, a.confidence) == (2000, 2 ** 63 + 11, 0.9)
    if name == "eval_report":
        assert parser.parse_args(["x.pt", "--against", "y.pt"]).against == "y.pt"


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from sm3hip import _lib, ops, report
    lib = _lib.load()
    assert lib.sm3_report_max_cases() == report.MAX_CASES == ops.REPORT_MAX_CASES
    buf = (C.c_int64 * (64 * 64 * 6))()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced, every call below returns before a launch

    def call(order=p, gs=p, ge=p, y=p, yhat=p, colmap=p, out=p, N=5, T=8, K=24, seed=0, r0=0, c=1, point=0):
        return lib.sm3_report_counts(order, gs, ge, y, yhat, colmap, out, N, T, K, seed, r0, c, point, None)
    for name in ("order", "gs", "ge", "y", "yhat", "colmap", "out"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(N=-3) == -1 and call(N=report.MAX_CASES + 1) == -1
    assert call(c=0) == -1 and call(c=-1) == -1
    assert call(T=0) == -1 and call(K=0) == -1 and call(K=65) == -1
    assert call(r0=-1) == -1 and call(r0=2 ** 32) == -1 and call(r0=2 ** 32 - 1, c=2) == -1
    assert call(point=1, c=2) == -1
