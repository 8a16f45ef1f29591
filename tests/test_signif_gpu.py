"""GPU: the significance tests of a paired comparison (csrc/signif.hip, sm3hip/significance.py, tools/eval_report.py
--significance).  tests/signif_inputs.py holds the cases and the by-definition restatements.

  * sm3_signif_counts equal (==) to the recount of swapped predictions that are formed one replicate at a time: N over the
    swap-word (32), Philox-call (128) and scan-tile (1024 joint positions = 512 cases) boundaries +- 1 up to MAX_CASES, tied
    integer logits, b == a, permuted columns, empty and one-case classes; every output element overwritten;
  * sm3_signif_placements == the psi-matrix definition, their sums == the report's A2;
  * the point record == evaluation_report's counts of a and of b;
  * exchange: permutation_test(b, a) gives the same p and the negated statistics to the bit; a against a gives p = 1 everywhere
    and DeLong undefined;
  * equal bits across chunks and calls, and replicate r of B = 16 is replicate r of B = 64;
  * replicate AUCs within 1e-12 of sklearn's roc_auc_score on the swapped fp64 scores;
  * power: a clearly better model against a noisy copy of it on DIAG-3;
  * the tool writes <name>_significance.json / .csv with the values of significance_report, and neither without the flag."""
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


SI = _load("sm3_signif_inputs_gpu", os.path.join(ROOT, "tests", "signif_inputs.py"))


def _bits(t):
    return t.numpy().view(np.uint64)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _to(preds):
    return [p.to(DEV) for p in preds]


def _scores(preds):
    """SI.scores with the softmax taken on the device: the scores are DEFINED as the device's fp64 softmax columns, and two rows
    whose softmax is equal in exact arithmetic may differ in the last bit there and not on the CPU (or the reverse), which
    moves a tie."""
    return torch.cat([torch.softmax(p.to(DEV).double(), dim=1).t() for p in preds], dim=0).cpu().numpy()


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------------
def _device_inputs(a, b, targets):
    from sm3hip import report, significance
    order, gs, ge, yhat_a, yhat_b = significance.joint_ranking(_to(a), _to(b))
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV)
    return order, gs, ge, targets.to(DEV).int().contiguous(), yhat_a, yhat_b, colmap


def _device_counts(inp, seed, r0, c, point=False):
    from sm3hip import ops
    out = torch.full((c, 24, 2, 3), SENTINEL, dtype=torch.int64, device=DEV)
    ops.signif_counts(*inp, out, seed, r0, point=point)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got == SENTINEL).any()                                                # every element is overwritten
    return got


@pytest.mark.parametrize("N", [1, 2, 3, 31, 32, 33, 127, 128, 129, 511, 512, 513, 8191, 8192])
def test_counts_equal_the_recount_of_swapped_predictions(N):
    big = N > 1024
    c = 8 if big else 64
    kinds = ("other",) if big else ("other", "sparse") if N > 129 else ("other", "permuted", "same", "sparse")
    for i, kind in enumerate(kinds):
        seed, r0 = ((2 ** 63 + 11, 2 ** 20 - 3), (7, 0), (2 ** 32 + 5, 1000), (1, 2 ** 32 - c))[i]
        a, b, targets = SI.make_pair(N, kind, 13 * N + i)
        inp = _device_inputs(a, b, targets)
        sa, sb, ha, hb, y = _scores(a), _scores(b), SI.argmax(a), SI.argmax(b), targets.numpy()
        assert np.array_equal(inp[4].cpu().numpy(), ha) and np.array_equal(inp[5].cpu().numpy(), hb)
        point = _device_counts(inp, seed, 0, 1, point=True)
        assert np.array_equal(point[0], SI.recount(sa, sb, ha, hb, y, np.zeros(N, dtype=bool))), (kind, "point")
        got = _device_counts(inp, seed, r0, c)
        check = range(c) if i == 0 or big else (0, 1, c - 1)                         # the restatement is the slow side
        for j in check:
            want = SI.recount(sa, sb, ha, hb, y, SI.swap_bits(seed, r0 + j, N))
            assert np.array_equal(got[j], want), (kind, seed, r0 + j)
        parts = [_device_counts(inp, seed, r0 + k, min(5, c - k)) for k in range(0, c, 5)]  # any cut of [r0, r0 + c) is the one call
        assert np.array_equal(np.concatenate(parts), got)


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from sm3hip import ops
    a, b, targets = SI.make_pair(5, "other", 1)
    inp = list(_device_inputs(a, b, targets))
    out = torch.zeros(2, 24, 2, 3, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ops.signif_counts(*inp, out, 0, 0, point=True)                                # the point record is one record
    with pytest.raises(ValueError):
        ops.signif_counts(*inp, out, 2 ** 64, 0)
    with pytest.raises(ValueError):
        ops.signif_counts(inp[0].long(), *inp[1:], out, 0, 0)
    with pytest.raises(ValueError):
        ops.signif_counts(inp[0][:, :5].contiguous(), *inp[1:], out, 0, 0)            # a ranking of N, not 2N, positions
    with pytest.raises(ValueError):
        ops.signif_counts(*inp, out[:, :23], 0, 0)
    with pytest.raises(ValueError):
        ops.signif_counts(*inp, out.view(2, 24, 6), 0, 0)
    with pytest.raises(ValueError):
        ops.signif_counts(*(x.cpu() for x in inp), out, 0, 0)
    order, gs, ge, y, colmap = inp[0][:, :5].contiguous(), inp[1][:, :5].contiguous(), inp[2][:, :5].contiguous(), inp[3], inp[6]
    place = torch.zeros(24, 5, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.signif_placements(order, gs, ge, y, colmap, place.long())
    with pytest.raises(ValueError):
        ops.signif_placements(order, gs, ge, y, colmap, place[:, :4].contiguous())
    with pytest.raises(ValueError):
        ops.signif_placements(order.cpu(), gs, ge, y, colmap, place)


@pytest.mark.parametrize("N", [1, 2, 33, 129, 513, 1025, 8192])
def test_placements_equal_the_definition_and_sum_to_the_reports_a2(N):
    from sm3hip import report, significance
    for kind in ("other", "sparse"):
        a, _, targets = SI.make_pair(N, kind, 17 * N)
        got = significance.placements(a, targets, DEV)
        full = torch.full_like(got, -7)
        # every entry is written: a second buffer pre-filled with a value no placement takes
        from sm3hip import ops
        order, gs, ge, _ = report.ranking(_to(a), targets.to(DEV))
        ops.signif_placements(order, gs, ge, targets.to(DEV).int().contiguous(),
                              torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=DEV), full)
        assert torch.equal(full, got) and int(got.min()) >= 0
        got = got.cpu().numpy().astype(np.int64)
        s, y = _scores(a), targets.numpy()
        counts = report.evaluation_report(_to(a), targets.to(DEV))["counts"].numpy()
        for k, (t, c) in enumerate(SI.PAIRS):
            pos = y[:, t] == c
            want = SI.placements_by_psi(s[k], pos) if N <= SI.PSI_LIMIT else SI.placements_by_sort(s[k], pos)
            assert np.array_equal(got[k], want), (kind, k)
            assert int(got[k][pos].sum()) == int(counts[k, 0])                        # the report's A2
            assert int(got[k][~pos].sum()) == int(counts[k, 0])                       # the same psi matrix, summed the other way


# ---- 2. the library ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    a, b, targets = SI.make_pair(395, "other", 42)
    return _to(a), _to(b), targets.to(DEV)


def test_point_record_equals_the_two_evaluation_reports(pair):
    from sm3hip import report, significance
    for kind in ("other", "sparse", "permuted"):
        a, b, targets = SI.make_pair(257, kind, 8)
        res = significance.permutation_test(_to(a), _to(b), targets.to(DEV), permutations=3, seed=1)
        ra, rb = report.evaluation_report(_to(a), targets.to(DEV)), report.evaluation_report(_to(b), targets.to(DEV))
        assert torch.equal(res["counts"][0], ra["counts"]) and torch.equal(res["counts"][1], rb["counts"]), kind
        assert _same(res["values_a"], ra["values"]) and _same(res["values_b"], rb["values"])
        assert _same(res["statistic"], ra["values"] - rb["values"])
        d = significance.delong(_to(a), _to(b), targets.to(DEV))
        assert _same(d["theta_a"], ra["values"][0, :24].contiguous()) and _same(d["theta_b"], rb["values"][0, :24].contiguous())


def test_exchange_and_a_against_itself(pair):
    from sm3hip import significance
    a, b, targets = pair
    before = [p.clone() for p in a + b] + [targets.clone()]
    ab = significance.permutation_test(a, b, targets, permutations=64, seed=2 ** 63 + 11)
    ba = significance.permutation_test(b, a, targets, permutations=64, seed=2 ** 63 + 11)
    assert ab["replicates"].shape == (64, 4, 29) and ab["p"].shape == (4, 29) and ab["columns"][24:] == list(significance.report.AVERAGES)
    assert _same(ab["p"], ba["p"]) and torch.equal(ab["exceed"], ba["exceed"]) and torch.equal(ab["undefined"], ba["undefined"])
    assert _same(ab["statistic"] + 0.0, -ba["statistic"] + 0.0) and _same(ab["replicates"] + 0.0, -ba["replicates"] + 0.0)
    assert torch.equal(ab["counts"], ba["counts"].flip(0)) and ab["statistic"].any()
    assert float(ab["p"].min()) >= 1 / 65 and float(ab["p"].max()) <= 1.0
    dab, dba = significance.delong(a, b, targets), significance.delong(b, a, targets)
    assert _same(dab["p"], dba["p"]) and _same(dab["z"] + 0.0, -dba["z"] + 0.0) and _same(dab["var"], dba["var"])
    assert _same(dab["lo"] + 0.0, -dba["hi"] + 0.0) and not dab["undefined"].any()
    aa = significance.significance_report(a, a, targets, permutations=64, seed=3)
    assert bool((aa["permutation"]["p"] == 1.0).all()) and not aa["permutation"]["replicates"].any()
    assert bool(aa["delong"]["undefined"].all()) and bool((aa["delong"]["p"] == 1.0).all()) and not aa["delong"]["z"].any()
    assert aa["mcnemar"]["p"].tolist() == [1.0] * 8
    assert bool((aa["permutation"]["p_holm_classes"] == 1.0).all())
    for p, q in zip(a + b + [targets], before):                                       # inputs are not modified
        assert torch.equal(p, q)
    cpu = significance.permutation_test([p.cpu() for p in a], [p.cpu() for p in b], targets.cpu(), permutations=64, seed=2 ** 63 + 11)
    assert _same(cpu["p"], ab["p"]) and _same(cpu["replicates"], ab["replicates"])   # CPU tensors are moved, not refused


def test_chunks_calls_and_the_number_of_replicates_do_not_show(pair):
    from sm3hip import significance
    a, b, targets = pair
    first = significance.permutation_test(a, b, targets, permutations=64, seed=9)
    for chunk in (None, 1, 7, 64):
        again = significance.permutation_test(a, b, targets, permutations=64, seed=9, chunk=chunk)
        for key in ("statistic", "p", "replicates", "values_a", "values_b", "p_holm_classes", "p_holm_selected"):
            assert _same(first[key], again[key]), (chunk, key)
        assert torch.equal(first["undefined"], again["undefined"]) and torch.equal(first["counts"], again["counts"])
    short = significance.permutation_test(a, b, targets, permutations=16, seed=9)
    assert _same(short["replicates"], first["replicates"][:16].contiguous()) and _same(short["statistic"], first["statistic"])
    other = significance.permutation_test(a, b, targets, permutations=16, seed=10)
    assert not _same(other["replicates"], short["replicates"]) and _same(other["statistic"], short["statistic"])
    # p is the definition on the returned statistics; Holm is the definition on p
    assert np.array_equal(first["p"].numpy(), SI.permutation_p(first["statistic"].numpy(), first["replicates"].numpy()))
    for i in range(4):
        assert np.array_equal(first["p_holm_classes"][i].numpy(), SI.holm_by_definition(first["p"][i, :24].numpy()))
        assert np.array_equal(first["p_holm_selected"][i].numpy(),
                              SI.holm_by_definition(first["p"][i].numpy()[significance.SELECTED]))


def test_replicates_are_the_restatement_through_the_library():
    from sm3hip import report, significance
    a, b, targets = SI.make_pair(129, "sparse", 6)
    res = significance.permutation_test(_to(a), _to(b), targets.to(DEV), permutations=6, seed=2 ** 32 + 5)
    sa, sb, ha, hb, y = _scores(a), _scores(b), SI.argmax(a), SI.argmax(b), targets.numpy()
    undefined = np.zeros((4, 29), dtype=np.int64)
    for r in range(6):
        full = SI.full_counts(SI.recount(sa, sb, ha, hb, y, SI.swap_bits(2 ** 32 + 5, r, 129)), y)
        values, und = report.values_from_counts(full)
        assert np.array_equal(_bits(res["replicates"][r]), (values[0] - values[1]).view(np.uint64)), r
        undefined += und.any(axis=0)
    assert np.array_equal(res["undefined"].numpy(), undefined) and undefined[0].max() == 6   # the empty classes: every replicate


def test_replicate_aucs_against_sklearn():
    from sklearn.metrics import roc_auc_score
    a, b, targets = SI.make_pair(395, "other", 21)
    g = torch.Generator().manual_seed(2)
    a = [p + 0.5 * torch.randn(p.shape, generator=g) for p in a]                      # continuous beside the tied: both occur
    inp = _device_inputs(a, b, targets)
    got = _device_counts(inp, 4, 0, 8)
    sa, sb, y = _scores(a), _scores(b), targets.numpy()
    worst = 0.0
    for r in range(8):
        swap = SI.swap_bits(4, r, 395)
        sides = (np.where(swap[None], sb, sa), np.where(swap[None], sa, sb))
        for k, (t, c) in enumerate(SI.PAIRS):
            pos = y[:, t] == c
            P, Q = int(pos.sum()), int((~pos).sum())
            for w in range(2):
                worst = max(worst, abs(int(got[r, k, w, 0]) / float(2 * P * Q) - roc_auc_score(pos, sides[w][k])))
    print(f"largest |replicate AUC - roc_auc_score|: {worst:.3g}")
    assert worst <= 1e-12


def test_a_clearly_better_model_is_found_on_diag_3():
    """signif_inputs.power_case: b is a noisy copy of a.  Restated on the CPU (its softmax) for DIAG-3 (AUC) with 999 replicates
    at seed 0: T = 0.22597402597402594, permutation p = 0.001 (no replicate reaches |T|), DeLong z = 5.051511265715187, p =
    4.3832807851332113e-07.  The device's softmax may move a tie by its last bit, so those figures are held to 1 % here and the
    library is held to the restatement on the device's scores, with ==."""
    from sm3hip import significance
    a, b, targets = SI.power_case()
    k = significance.COLUMNS.index("DIAG-3")
    t, p, z, pz = SI.restated_auc_test(a, b, targets, k, 999, 0, score=_scores)
    print(f"restated on the device's scores: T {t!r} p {p!r} z {z!r} p {pz!r}")
    assert abs(t - 0.22597402597402594) <= 0.01 * 0.226 and p == 0.001 and abs(z - 5.051511265715187) <= 0.0506 and pz < 1e-5
    res = significance.significance_report(_to(a), _to(b), targets.to(DEV), permutations=999, seed=0)
    perm, dl = res["permutation"], res["delong"]
    assert float(perm["statistic"][0, k]) == t and float(perm["p"][0, k]) == p == 1 / 1000
    assert float(dl["z"][k]) == z and float(dl["p"][k]) == pz and float(dl["lo"][k]) > 0
    assert float(perm["p_holm_classes"][0, k]) <= 24 / 1000 and float(dl["p_holm_classes"][k]) < 1e-4
    assert float(res["mcnemar"]["p"][0]) < 0.01 and int(res["mcnemar"]["n10"][0]) > int(res["mcnemar"]["n01"][0])
    text = significance.format_table(res)
    assert "DIAG-3" in text and "DeLong" in text and "McNemar" in text and "8 avg" in text


# ---- 3. the tool -------------------------------------------------------------------------------------------------------------
def test_the_tool_writes_the_two_files_only_with_the_flag(tmp_path, capsys):
    from sm3hip import significance
    er = _load("sm3_signif_gpu_eval_report", os.path.join(TOOLS, "eval_report.py"))
    a, b, targets = SI.make_pair(129, "other", 12)
    torch.save({"preds": a, "targets": targets}, tmp_path / "a.pt")
    torch.save({"preds": b, "targets": targets}, tmp_path / "b.pt")
    plain = er.main([str(tmp_path / "a.pt"), "--against", str(tmp_path / "b.pt"), "--out", str(tmp_path / "plain")])
    assert "significance" not in plain and sorted(os.listdir(tmp_path / "plain")) == ["a_compare.json", "a_report.csv", "a_report.json"]
    capsys.readouterr()
    res = er.main([str(tmp_path / "a.pt"), "--against", str(tmp_path / "b.pt"), "--significance", "--permutations", "50",
                   "--permutation-seed", "7", "--confidence", "0.9", "--out", str(tmp_path / "sig")])
    out = capsys.readouterr().out
    assert "permutation p" in out and "McNemar" in out and "50 swap replicates, seed 7" in out
    assert sorted(os.listdir(tmp_path / "sig")) == ["a_compare.json", "a_report.csv", "a_report.json", "a_significance.csv",
                                                   "a_significance.json"]
    want = significance.significance_report(_to(a), _to(b), targets.to(DEV), permutations=50, seed=7, confidence=0.9)
    got = res["significance"]
    assert _same(got["permutation"]["p"], want["permutation"]["p"]) and _same(got["delong"]["lo"], want["delong"]["lo"])
    saved = json.load(open(tmp_path / "sig" / "a_significance.json"))
    assert saved["permutation"]["p"] == want["permutation"]["p"].tolist() and "replicates" not in saved["permutation"]
    assert saved["permutation"]["statistic"] == want["permutation"]["statistic"].tolist()
    assert saved["delong"]["z"] == want["delong"]["z"].tolist() and saved["delong"]["p"] == want["delong"]["p"].tolist()
    assert saved["mcnemar"]["p"] == want["mcnemar"]["p"].tolist() and saved["mcnemar"]["n10"] == want["mcnemar"]["n10"].tolist()
    assert (saved["permutations"], saved["seed"], saved["confidence"], saved["n"]) == (50, 7, 0.9, 129)
    rows = list(csv.reader(open(tmp_path / "sig" / "a_significance.csv")))
    assert rows[0] == ["test", "metric", "column", "statistic", "p", "p_holm_classes", "p_holm_selected", "undefined"]
    assert len(rows) == 1 + 4 * 29 + 24 + 8
    by = {(r[0], r[1], r[2]): r for r in rows[1:]}
    for i, m in enumerate(significance.METRICS):
        for k, name in enumerate(significance.COLUMNS):
            r = by[("permutation", m, name)]
            assert float(r[3]) == float(want["permutation"]["statistic"][i, k]) and float(r[4]) == float(want["permutation"]["p"][i, k])
            assert (r[5] == "") == (k >= 24) and (r[6] == "") == (k not in significance.SELECTED)
    for k, name in enumerate(significance.CLASS_COLUMNS):
        assert float(by[("delong", "AUC", name)][4]) == float(want["delong"]["p"][k])
    with pytest.raises(ValueError, match="same cases"):                               # another file's cases are refused
        torch.save({"preds": b, "targets": (targets + 1) % 2}, tmp_path / "c.pt")
        er.main([str(tmp_path / "a.pt"), "--against", str(tmp_path / "c.pt"), "--significance", "--out", str(tmp_path / "no")])
