"""CPU: the seven-point checklist report (sm3hip/checklist.py, csrc/checklist.hip) restated in plain Python integers, and
everything about it that needs no GPU.  tests/test_checklist_gpu.py loads this file for the restatement.

  * POINTS and MELANOMA against tests/golden/checklist_points.json, the tables of the reference's own dataset class;
  * the restatement of the record (loops over cases and sorted positions, Python ints; multiplicities by the resampling rule of
    sm3hip/resample.py as tests/test_report_cpu.py states it), and values_from_counts on it against scikit-learn within 1e-12,
    the bound operating_report uses for the same kind of comparison (the integer forms differ from scikit-learn's float sums by
    a few 1e-16): roc_auc_score of the five rankings, sens / spec / PPV / NPV of every cut against confusion_matrix,
    cohen_kappa_score(weights="quadratic"), for the point estimate and for Philox multiplicities passed as sample_weight;
  * score_distribution: rows sum to 1, sum s pi[s] = E and T_1 = 1 - pi[0] within bounds derived from the 7 x 11 operations,
    saturated logits give a delta at shat;
  * no melanoma / only melanoma, perfect agreement, one score value; compare, the writers, the flags, every refusal."""
import csv
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REF = _load("sm3_checklist_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))  # philox, multiplicities, make_case
NUM_CLASSES = REF.NUM_CLASSES
LABEL_POINTS = [0, 2, 2, 2, 1, 1, 1, 1]   # restated here, held to the library's below
SCORING = [2, 2, 1, 2, 2, 2, 2, 1]
NS, BINS, RECORD = 11, 242, 251
KINDS = ("random", "ties", "equal", "all_bins", "absent", "only")
U = 2.0 ** -53


def gamma(n):
    """(1 + u)^n - 1 <= n u / (1 - n u): the relative error of n roundings."""
    return n * U / (1.0 - n * U)


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _classes_of(score):
    """Classes of the seven criteria whose points add up to `score` (0 .. 10): the labels in order, each taken if it still fits."""
    cls, rest = [0] * 8, score
    for t in range(1, 8):
        if rest >= LABEL_POINTS[t]:
            cls[t], rest = SCORING[t], rest - LABEL_POINTS[t]
    assert rest == 0
    return cls


def make_case(N, kind, seed):
    """preds (8 x [N, n_t] float32) and targets [N, 8] int64.  "random" continuous logits, "ties" integer-valued logits (many tied
    scores), "equal" one tie group and one table bin, "all_bins" case n in bin n % 242 of J[shat][s*][mel] (every bin from N =
    242), "absent" no melanoma, "only" only melanoma."""
    if kind == "all_bins":
        g = torch.Generator().manual_seed(seed)
        targets = torch.zeros(N, 8, dtype=torch.int64)
        preds = [torch.rand(N, n, generator=g) * 2 - 1 for n in NUM_CLASSES]
        for n in range(N):
            b = (n * 101) % BINS if N >= BINS else n % BINS  # 101 is coprime to 242: the bins in a scattered order
            sh, st, mel = b // 22, (b // 2) % 11, b % 2
            targets[n] = torch.tensor(_classes_of(st))
            targets[n, 0] = 2 if mel else (0, 1, 3, 4)[n % 4]
            for t, c in enumerate(_classes_of(sh)):
                if t:
                    preds[t][n, c] += 8.0
        return preds, targets
    preds, targets = REF.make_case(N, "random" if kind in ("absent", "only") else kind, seed)
    if kind == "equal":
        targets[:] = torch.tensor(SCORING)
    if kind == "absent":
        targets[targets[:, 0] == 2, 0] = 1
    if kind == "only":
        targets[:, 0] = 2
    return preds, targets


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def record(packed, order, gs, ge, m):
    """One record [J (242), 3 x (A2, P, Q)] of Python ints.  packed [N]; order, gs, ge [3][N]; m [N]."""
    N = len(packed)
    J = [0] * BINS
    for n in range(N):
        w = int(packed[n])
        J[((w & 15) * NS + ((w >> 4) & 15)) * 2 + ((w >> 8) & 1)] += int(m[n])
    rec = J
    for k in range(3):
        S, P = [0], 0
        for j in range(N):
            n = int(order[k][j])
            mel = (int(packed[n]) >> 8) & 1
            S.append(S[-1] + (0 if mel else int(m[n])))
            P += int(m[n]) if mel else 0
        A2 = 0
        for j in range(N):
            n = int(order[k][j])
            if (int(packed[n]) >> 8) & 1:
                A2 += int(m[n]) * (S[int(gs[k][j])] + S[int(ge[k][j])])
        rec = rec + [A2, P, N - P]
    return rec


def restated_inputs(preds, targets, thresholds=(1, 3)):
    """(packed, order, gs, ge) as numpy int64, through the library's own per-case plumbing (torch) on the tensors' device."""
    from sm3hip import checklist
    return tuple(a.cpu().numpy().astype(np.int64) for a in checklist.case_inputs(preds, targets, list(thresholds))[:4])


def records(host, seed, r0, c, point):
    """[c, 251] int64 of replicates r0 .. r0 + c - 1, or of the point estimate."""
    N = len(host[0])
    return np.array([record(*host, np.ones(N, dtype=np.int64) if point else REF.multiplicities(seed, r0 + j, N))
                     for j in range(c)], dtype=np.int64)


def restatement_counts_fn(packed, order, gs, ge, out, seed, r0, point=False):
    """Stands in for ops.checklist_counts, on the tensors of any device."""
    host = [a.cpu().numpy() for a in (packed, order, gs, ge)]
    out.copy_(torch.from_numpy(records(host, seed, r0, out.shape[0], point)))


def host_report(preds, targets, thresholds=(1, 3), bootstrap=0, confidence=0.95, seed=0, chunk=None, dev="cpu"):
    """checklist_report's host half around the restatement: what the library does with the kernel's integers."""
    from sm3hip import checklist
    return checklist._report(preds, targets, checklist.check_thresholds(thresholds), bootstrap, confidence, seed, chunk,
                             torch.device(dev), restatement_counts_fn)


# ---- 1. the points ------------------------------------------------------------------------------------------------------------
def test_points_are_the_reference_tables():
    from sm3hip import checklist
    from sm3hip.metrics import CLASSES_NAME, CLS_WEIGHTS
    gold = json.load(open(os.path.join(GOLDEN, "checklist_points.json")))
    assert gold["label_order"] == CLASSES_NAME
    for t, name in enumerate(CLASSES_NAME):
        lab = gold["labels"][name]
        assert lab["nums"] == list(range(NUM_CLASSES[t])) and lab["seven_pt"] == (1 if t else 0)
        if t:
            assert list(checklist.POINTS[t]) == lab["scores"], name
            assert [i for i, v in enumerate(lab["scores"]) if v] == [CLS_WEIGHTS[t]], name  # the scoring class is CLS_WEIGHTS[t]
        else:
            assert lab["scores"] is None and not any(checklist.POINTS[0])
    label, cls = checklist.MELANOMA
    assert gold["labels"][CLASSES_NAME[label]]["abbrevs"][cls] == "MEL"
    assert sum(max(lab["scores"]) for lab in gold["labels"].values() if lab["scores"]) == checklist.MAX_SCORE == 10
    assert checklist.LABEL_POINTS == LABEL_POINTS and CLS_WEIGHTS == SCORING
    assert checklist.RECORD == RECORD and len(checklist.row_names()) == 5 + 3 + 80 + 5


def test_scores_are_the_sums_of_the_points():
    from sm3hip import checklist
    for kind in ("random", "ties", "all_bins"):
        preds, targets = make_case(300, kind, 3)
        shat, sstar = checklist.predicted_scores(preds), checklist.true_scores(targets)
        for n in range(300):
            assert int(sstar[n]) == sum(checklist.POINTS[t][int(targets[n, t])] for t in range(1, 8))
            yhat = [max(range(NUM_CLASSES[t]), key=lambda c: (float(preds[t][n, c]), -c)) for t in range(8)]  # lowest index wins
            assert int(shat[n]) == sum(checklist.POINTS[t][yhat[t]] for t in range(1, 8))
        assert 0 <= int(shat.min()) and int(shat.max()) <= 10
    packed = restated_inputs(*make_case(300, "all_bins", 3))[0]
    assert len(set(packed.tolist())) == BINS                                              # every bin of the table is hit


# ---- 2. against scikit-learn --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,kind,resample", [(5, "random", False), (64, "ties", True), (600, "ties", False), (600, "random", True),
                                             (600, "all_bins", True), (8192, "random", False)])
def test_values_against_sklearn(N, kind, resample):
    from sklearn.metrics import cohen_kappa_score, confusion_matrix, roc_auc_score
    from sm3hip import checklist
    preds, targets = make_case(N, kind, N + 3)
    if N == 5:
        targets[0, 0], targets[1, 0] = 2, 1
    th = [3, 1]
    host = restated_inputs(preds, targets, th)
    m = REF.multiplicities(2 ** 40 + 11, 2, N) if resample else np.ones(N, dtype=np.int64)
    values, undefined = checklist.values_from_counts(np.array(record(*host, m), dtype=np.int64))
    rows = checklist.row_names(th)
    row = dict(zip(rows, values))
    keep = m > 0
    w = m[keep]
    mel = (targets[:, 0].numpy() == 2)[keep]
    assert mel.any() and not mel.all() and not undefined[:8].any() and not undefined[-5:].any()   # a cut may have no case
    pi = checklist.score_distribution(preds)
    rank = {"hard": checklist.predicted_scores(preds), "annotated": checklist.true_scores(targets),
            "expected": checklist.expected_score(preds), "tail>=3": checklist.tail_probability(pi, 3),
            "diag": torch.softmax(preds[0].double(), 1)[:, 2]}
    worst = {"AUC": 0.0, "rule": 0.0, "kappa": 0.0}
    auc = {}
    for name, score in rank.items():
        auc[name] = roc_auc_score(mel, score.numpy()[keep], sample_weight=w)
        worst["AUC"] = max(worst["AUC"], abs(row[f"AUC {name}"] - auc[name]))
    for a, b in checklist.GAPS:
        worst["AUC"] = max(worst["AUC"], abs(row[f"AUC {a}-{b}"] - (auc[a] - auc[b])))
    for src, name in (("pred", "hard"), ("true", "annotated")):
        s = rank[name].numpy()[keep]
        for k in range(1, 11):
            tn, fp, fn, tp = confusion_matrix(mel, s >= k, labels=[False, True], sample_weight=w).ravel()
            for metric, num, den in (("sens", tp, tp + fn), ("spec", tn, tn + fp), ("PPV", tp, tp + fp), ("NPV", tn, tn + fn)):
                i = rows.index(f"{src}>={k} {metric}")
                if den == 0:
                    assert undefined[i] and values[i] == 0.0
                else:
                    worst["rule"] = max(worst["rule"], abs(values[i] - num / den))
    sh, st = rank["hard"].numpy()[keep], rank["annotated"].numpy()[keep]
    worst["kappa"] = abs(row["agree kappa"] - cohen_kappa_score(sh, st, labels=list(range(11)), weights="quadratic", sample_weight=w))
    tot = float(w.sum())
    assert row["agree exact"] == float((w * (sh == st)).sum()) / tot and row["agree MAE"] == float((w * np.abs(sh - st)).sum()) / tot
    assert row["agree within1"] == float((w * (np.abs(sh - st) <= 1)).sum()) / tot
    assert row["agree bias"] == float((w * (sh - st)).sum()) / tot
    print(f"N = {N} {kind} resample = {resample}: worst differences {worst}")
    for name, v in worst.items():
        assert v <= 1e-12, name


# ---- 3. the distribution of the score -------------------------------------------------------------------------------------------
def test_score_distribution_bounds():
    """Per step and entry: 1 - q, two products, one sum -- with non-negative terms at most 3 roundings deep per step, 21 after the
    seven steps; a sum of 11 stored entries adds 10 more, the product s * pi[s] one: gamma(32) covers each row sum, gamma(32) *
    mean + gamma(14) * E the mean (E is seven products and seven sums), and T_1 against 1 - pi[0] is the row sum's bound again
    (T_1 adds pi[1 .. 10], the subtraction rounds once)."""
    from sm3hip import checklist
    for kind, N in (("random", 2000), ("ties", 500), ("all_bins", 484)):
        preds, targets = make_case(N, kind, 11)
        preds = [p * 3 for p in preds]
        pi = checklist.score_distribution(preds)
        e = checklist.expected_score(preds).numpy()
        assert pi.shape == (N, 11) and pi.dtype == torch.float64 and bool((pi >= 0).all())
        p = pi.numpy()
        total = np.zeros(N)
        mean = np.zeros(N)
        for s in range(11):
            total = total + p[:, s]
            mean = mean + s * p[:, s]
        print(f"{kind}: |sum - 1| <= {np.abs(total - 1).max():.3g}, |mean - E| <= {np.abs(mean - e).max():.3g}")
        assert np.abs(total - 1.0).max() <= gamma(32)
        assert (np.abs(mean - e) <= gamma(32) * mean + gamma(14) * e).all()
        t1 = checklist.tail_probability(pi, 1).numpy()
        assert np.abs(t1 - (1.0 - p[:, 0])).max() <= gamma(32)
        assert torch.equal(checklist.tail_probability(pi, 10), pi[:, 10])
        q = checklist.criterion_probabilities(preds)
        assert torch.equal(q[:, 3], torch.softmax(preds[3].double(), 1)[:, 2]) and q.shape == (N, 8)


def test_saturated_logits_give_a_delta_at_the_hard_score():
    from sm3hip import checklist
    preds, targets = make_case(242, "all_bins", 5)
    sat = [torch.nn.functional.one_hot(p.argmax(1), p.shape[1]).float() * 2000 - 1000 for p in preds]
    shat = checklist.predicted_scores(sat)
    assert torch.equal(shat, checklist.predicted_scores(preds)) and len(set(shat.tolist())) == 11
    pi = checklist.score_distribution(sat)
    assert torch.equal(pi, torch.nn.functional.one_hot(shat, 11).double())
    assert torch.equal(checklist.expected_score(sat), shat.double())


# ---- 4. degenerate tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["absent", "only"])
def test_one_diagnosis_class_leaves_every_auc_undefined_and_raises_nothing(kind):
    from sm3hip import checklist
    preds, targets = make_case(40, kind, 2)
    rep = host_report(preds, targets, bootstrap=4, seed=7)
    rows = rep["rows"]
    for i, r in enumerate(rows):
        if r.startswith("AUC "):
            assert float(rep["values"][i, 0]) == 0.0 and bool(rep["point_undefined"][i, 0]) and int(rep["undefined"][i, 0]) == 4
    v = rep["values"].numpy()
    assert np.isfinite(v).all() and not v[rep["point_undefined"].numpy()].any() and np.isfinite(rep["replicates"].numpy()).all()
    gone, stays = ("sens", "spec") if kind == "absent" else ("spec", "sens")
    assert bool(rep["point_undefined"][rows.index(f"pred>=1 {gone}"), 0]) and not bool(rep["point_undefined"][rows.index(f"pred>=1 {stays}"), 0])
    assert "undefined" in checklist.format_table(rep) and "checklist_AUC_hard 0.0000" in checklist.stats_line(rep)


def test_perfect_agreement_is_kappa_one_and_one_score_value_is_undefined():
    from sm3hip import checklist
    rows = checklist.row_names()
    J = np.zeros((11, 11, 2), dtype=np.int64)
    J[0, 0, 0], J[3, 3, 1], J[10, 10, 1] = 5, 2, 1
    cnt = np.concatenate([J.reshape(-1), np.zeros(9, dtype=np.int64)])
    v, u = checklist.values_from_counts(cnt)
    assert v[rows.index("agree kappa")] == 1.0 and not u[rows.index("agree kappa")]
    assert v[rows.index("agree exact")] == 1.0 and v[rows.index("agree MAE")] == 0.0 and v[rows.index("agree bias")] == 0.0
    assert v[rows.index("AUC hard")] == 1.0 and v[rows.index("AUC annotated")] == 1.0 and v[rows.index("AUC annotated-hard")] == 0.0
    assert u[rows.index("AUC expected")] and u[rows.index("AUC diag-expected")] and v[rows.index("AUC diag-expected")] == 0.0
    assert (v[rows.index("pred>=3 sens")], v[rows.index("pred>=3 spec")], v[rows.index("pred>=4 sens")]) == (1.0, 1.0, 1 / 3)
    J[:] = 0
    J[4, 4, 0], J[4, 4, 1] = 3, 4
    v, u = checklist.values_from_counts(np.concatenate([J.reshape(-1), np.zeros(9, dtype=np.int64)]))
    assert u[rows.index("agree kappa")] and v[rows.index("agree kappa")] == 0.0 and v[rows.index("agree exact")] == 1.0
    assert v[rows.index("AUC hard")] == 0.5 and not u[rows.index("AUC hard")]              # one tie group: every pair tied
    # a hand table: shat = s* + 1 for two negatives, s* - 2 for one positive
    J[:] = 0
    J[1, 0, 0], J[2, 1, 0], J[5, 7, 1] = 1, 1, 1
    v, u = checklist.values_from_counts(np.concatenate([J.reshape(-1), np.zeros(9, dtype=np.int64)]))
    assert v[rows.index("agree MAE")] == 4 / 3 and v[rows.index("agree bias")] == 0.0 and v[rows.index("agree within1")] == 2 / 3
    equal = host_report(*make_case(9, "equal", 1))
    assert int(equal["counts"][(0 * 11 + 10) * 2 + 1]) == 9 and int(equal["counts"][:242].sum()) == 9


# ---- 5. host-side checks ------------------------------------------------------------------------------------------------------
def test_bootstrap_through_the_host_half_does_not_depend_on_the_chunk():
    preds, targets = make_case(40, "ties", 2)
    a = host_report(preds, targets, bootstrap=6, seed=2 ** 63 + 1)
    b = host_report(preds, targets, bootstrap=6, seed=2 ** 63 + 1, chunk=4)
    assert torch.equal(a["replicate_counts"], b["replicate_counts"]) and torch.equal(a["replicates"], b["replicates"])
    assert a["replicates"].shape == (6, 93, 1) and a["values"].shape == (93, 1) and bool((a["lo"] <= a["hi"]).all())
    assert torch.equal(a["replicate_counts"][:, :242].sum(dim=1), torch.full((6,), 40))
    assert a["n"] == 40 and a["columns"] == ["value"] and a["thresholds"] == [1, 3]


def test_compare_pairs_the_replicates_and_refuses_unpaired_reports():
    from sm3hip import checklist, report
    preds, targets = make_case(30, "random", 6)
    other = [p.flip(0) for p in preds]
    a, b = host_report(preds, targets, bootstrap=5, seed=3), host_report(other, targets, bootstrap=5, seed=3)
    c = checklist.compare(a, b)
    assert torch.equal(c["delta"], a["values"] - b["values"]) and c["rows"] == a["rows"] and c["delta"].any()
    lo, hi = report.interval((a["replicates"] - b["replicates"]).numpy(), 0.95)
    assert np.array_equal(c["lo"].numpy(), lo) and np.array_equal(c["hi"].numpy(), hi)
    z = checklist.compare(a, a)
    assert not z["delta"].any() and not z["lo"].any() and not z["hi"].any() and float(z["frac_le_zero"].min()) == 1.0
    assert "difference" in checklist.format_compare(c)
    with pytest.raises(ValueError, match="seed"):
        checklist.compare(a, host_report(other, targets, bootstrap=5, seed=4))
    with pytest.raises(ValueError, match="bootstrap"):
        checklist.compare(a, host_report(other, targets, bootstrap=4, seed=3))
    with pytest.raises(ValueError, match="thresholds"):
        checklist.compare(a, host_report(other, targets, bootstrap=5, seed=3, thresholds=(2,)))
    with pytest.raises(ValueError, match="targets"):
        checklist.compare(a, host_report(other, (targets + 1) % 2, bootstrap=5, seed=3))
    with pytest.raises(ValueError, match="checklist_report"):
        checklist.compare(a, {"values": a["values"]})
    assert "lo" not in checklist.compare(host_report(preds, targets), host_report(other, targets))


def test_csv_and_json_parse_back_to_the_values(tmp_path):
    from sm3hip import checklist
    preds, targets = make_case(25, "ties", 12)
    for B in (0, 4):
        rep = host_report(preds, targets, thresholds=(3, 7), bootstrap=B)
        checklist.save(rep, str(tmp_path), f"r{B}")
        lines = list(csv.reader(open(tmp_path / f"r{B}.csv")))
        assert lines[0] == ["row", "value"] + (["lo", "hi", "undefined"] if B else [])
        shown = [rep["rows"][i] for i in rep["shown"]]
        assert [ln[0] for ln in lines[1:]] == shown and len(shown) == 5 + 3 + 2 * 2 * 4 + 5
        assert "AUC tail>=3" in shown and "pred>=7 NPV" in shown and "true>=3 sens" in shown and "pred>=1 sens" not in shown
        for ln, i in zip(lines[1:], rep["shown"]):
            assert float(ln[1]) == float(rep["values"][i, 0])
            if B:
                assert (float(ln[2]), float(ln[3]), int(ln[4])) == (float(rep["lo"][i, 0]), float(rep["hi"][i, 0]),
                                                                      int(rep["undefined"][i, 0]))
        back = json.load(open(tmp_path / f"r{B}.json"))
        assert back["values"] == rep["values"].tolist() and back["rows"] == rep["rows"] and back["counts"] == rep["counts"].tolist()
        assert "replicates" not in back and "targets" not in back and "pred>=1 sens" in back["rows"]      # all ten cuts
        assert back["scores"]["predicted"] == rep["scores"]["predicted"].tolist() and back["thresholds"] == [3, 7]
    text = checklist.format_table(rep)
    assert "pred>=7 PPV" in text and "pred>=1 sens" not in text and "checklist_agree_kappa" in checklist.stats_line(rep)
    assert "MAX_CASES" in checklist.stats_line(None)


def test_settings_and_inputs_are_refused_before_any_device_work():
    from sm3hip import checklist
    preds, targets = make_case(5, "ties", 1)
    for kw, msg in (({"bootstrap": -1}, "bootstrap must be"), ({"confidence": 1.0}, "confidence must be"),
                    ({"seed": 2 ** 64}, "seed must be"), ({"bootstrap": 4, "chunk": 5}, "chunk must be"),
                    ({"thresholds": [0]}, r"integer in \[1, 10\]"), ({"thresholds": [11]}, r"integer in \[1, 10\]"),
                    ({"thresholds": [1.0]}, r"integer in \[1, 10\]"), ({"thresholds": [True]}, r"integer in \[1, 10\]"),
                    ({"thresholds": ["3"]}, r"integer in \[1, 10\]"), ({"thresholds": [3, 1, 3]}, "duplicates"),
                    ({"thresholds": []}, "empty"), ({"thresholds": None}, "must be a list"), ({"thresholds": 2.5}, "must be a list")):
        with pytest.raises(ValueError, match="checklist_report: .*" + msg):
            checklist.checklist_report(preds, targets, **kw)
    with pytest.raises(ValueError, match="checklist_report: .*NaN"):
        checklist.checklist_report([p.clone().fill_(float("nan")) if t == 2 else p for t, p in enumerate(preds)], targets)
    with pytest.raises(ValueError, match="checklist_report: preds must be a list of 8"):
        checklist.checklist_report(preds[:7], targets)
    with pytest.raises(ValueError, match=r"targets\[:, \d\] must lie in"):
        checklist.checklist_report(preds, targets + 3)
    big_p, big_t = REF.make_case(checklist.MAX_CASES + 1, "equal", 1)
    with pytest.raises(ValueError, match="MAX_CASES"):
        checklist.checklist_report(big_p, big_t)
    assert checklist.check_thresholds(4) == [4] and checklist.check_thresholds((10, 1)) == [10, 1]
    assert checklist.validation_checklist(big_p, big_t, None, None) is None


def _tool(name):
    return _load("sm3_checklist_cli_" + name, os.path.join(TOOLS, name + ".py"))


@pytest.mark.parametrize("name", ["backbone_eval", "mlc_eval", "backbone_knn", "eval_report"])
def test_the_new_flags_parse(name):
    from sm3hip import checklist
    base = ["x.pt"] if name == "eval_report" else ["--data-name", "synthetic", "--data-path", "-"]
    parser = _tool(name).get_parser()
    d = parser.parse_args(base)
    assert d.checklist is False and d.checklist_thresholds == [1, 3] and d.operating is False
    checklist.check_flags(d)
    a = parser.parse_args(base + ["--checklist", "--checklist-thresholds", "3", "5", "1"])
    assert a.checklist and checklist.flag_settings(a) == {"thresholds": [3, 5, 1]}
    checklist.check_flags(a)
    for bad, msg in ((["0"], r"integer in \[1, 10\]"), (["11"], r"integer in \[1, 10\]"), (["2", "2"], "duplicates")):
        with pytest.raises(ValueError, match="--checklist-thresholds: .*" + msg):
            checklist.check_flags(parser.parse_args(base + ["--checklist-thresholds"] + bad))
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--checklist-thresholds", "1.5"])


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from sm3hip import _lib, checklist, ops
    lib = _lib.load()
    assert lib.sm3_checklist_record() == checklist.RECORD == ops.CHECKLIST_RECORD == RECORD
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced, every call below returns before a launch
    odd = C.c_void_p(p.value + 4)

    def call(packed=p, order=p, gs=p, ge=p, out=p, N=5, seed=0, r0=0, c=1, point=0):
        return lib.sm3_checklist_counts(packed, order, gs, ge, out, N, seed, r0, c, point, None)
    for name in ("packed", "order", "gs", "ge", "out"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(N=-3) == -1 and call(N=checklist.MAX_CASES + 1) == -1
    assert call(c=0) == -1 and call(c=-1) == -1
    assert call(r0=-1) == -1 and call(r0=2 ** 32) == -1 and call(r0=2 ** 32 - 1, c=2) == -1
    assert call(point=1, c=2) == -1
    assert call(out=odd) == -2
