"""CPU: the selective-prediction report (sm3hip/selective.py, csrc/selective.hip) through its restatement in
tests/selective_inputs.py, and everything about it that needs no GPU.

  * the harmonic-tail table against fractions.Fraction, and its size at MAX_CASES;
  * point-estimate records of the restatement through values_from_counts: AURC within 2^-32 of the exact Fraction value for
    N <= 1025; above that within 2^-31 of math.fsum of the fp64 quotients -- fewer than N error terms, each off by less than
    2^-32, divided by N, plus N * 2^-53 of summation error, which is below 2^-32 at N = 8192; the edge kinds;
  * the keys against their torch expressions, the ranking against a literal sort, the tie count;
  * fit_thresholds' host part against a plain >= count; every refusal; the tool's flags."""
import argparse
import fractions
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SI = _load("sm3_selective_inputs_cpu", os.path.join(ROOT, "tests", "selective_inputs.py"))
MAX_CASES = 8192
RISKS = [(0, 1), (1, 20), (1, 10), (1, 5), (999999, 1000000), (1, 1)]


def _point(N, kind, seed=3, score="msp", coverages=("0.5", "1.0"), risks=RISKS, pcuts=None):
    """(records [8, R], kcuts, order, flags) of the point estimate, restated."""
    from sm3hip import selective
    preds, targets = SI.case(N, kind, seed)
    order, last, _, _ = SI.ranked(preds, targets, score)
    flg = SI.flags(preds, targets)
    kcuts = selective.coverage_cuts(N, selective.check_coverages(coverages)[1])
    pcuts = [[] for _ in range(8)] if pcuts is None else pcuts
    return SI.records(order, flg, last, None, kcuts, risks, pcuts), kcuts, order, flg


# ---- the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 300])
def test_table_is_within_2_to_minus_32_of_the_harmonic_tails(N):
    from sm3hip import selective
    ph = selective.harmonic_table(N)
    tail, ph_ref = SI.tails(N)
    assert ph.dtype == np.int64 and ph.tolist() == ph_ref and ph[0] == 0
    exact = fractions.Fraction(0)
    for r in range(N, 0, -1):
        exact += fractions.Fraction(1, r)
        assert abs(fractions.Fraction(int(ph[r] - ph[r - 1]), SI.ONE) - exact) <= fractions.Fraction(1, SI.ONE), r


def test_table_fits_at_max_cases():
    from sm3hip import report, selective
    assert report.MAX_CASES == MAX_CASES
    ph = selective.harmonic_table(MAX_CASES)
    assert ph.shape == (MAX_CASES + 1,) and int(ph[-1]) < 2 ** 46 and (np.diff(ph) > 0).all()
    assert abs(int(ph[-1]) - MAX_CASES * SI.ONE) <= MAX_CASES  # sum_r sum_{k >= r} 1 / k = N, every entry off by under 1


# ---- point-estimate records through values_from_counts -------------------------------------------------------------------
@pytest.mark.parametrize("kind", SI.KINDS)
@pytest.mark.parametrize("N", [1, 2, 5, 65, 300, 1025])
def test_aurc_is_within_2_to_minus_32_of_the_exact_value(N, kind):
    from sm3hip import selective
    rec, kcuts, order, flg = _point(N, kind)
    v = selective.values_from_counts(rec, N, kcuts, len(RISKS), 0)
    for t in range(8):
        exact = SI.exact_aurc(order[t], flg[0][t])
        got = fractions.Fraction(float(v["summary_values"][0, t]))
        print(N, kind, t, float(abs(got - exact)) * 2.0 ** 32)
        assert abs(got - exact) <= fractions.Fraction(1, SI.ONE)
        assert float(v["summary_values"][3, t]) == int(flg[0][t].sum()) / N
    assert not v["summary_undefined"].any()


def test_aurc_at_max_cases_is_within_2_to_minus_31_of_the_float_sum():
    from sm3hip import selective
    N = MAX_CASES
    rec, kcuts, order, flg = _point(N, "random")
    v = selective.values_from_counts(rec, N, kcuts, len(RISKS), 0)
    for t in range(8):
        e = np.cumsum(flg[0][t][order[t]].astype(np.int64))
        want = math.fsum(float(e[k]) / float(k + 1) for k in range(N)) / N
        print(t, abs(float(v["summary_values"][0, t]) - want) * 2.0 ** 31)
        assert abs(float(v["summary_values"][0, t]) - want) <= 2.0 ** -31


@pytest.mark.parametrize("N", [5, 65, 300])
def test_a_perfect_ranking_has_excess_aurc_zero(N):
    from sm3hip import selective
    rec, kcuts, _, flg = _point(N, "errors_last")
    v = selective.values_from_counts(rec, N, kcuts, len(RISKS), 0)
    assert flg[0].sum() == 8 * (N // 4)
    assert (v["summary_values"][2] == 0.0).all() and (v["summary_values"][0] == v["summary_values"][1]).all()
    first, _, _, _ = _point(N, "errors_first")
    vf = selective.values_from_counts(first, N, kcuts, len(RISKS), 0)
    assert (vf["summary_values"][2] > 0.0).all() and (vf["summary_values"][1] == v["summary_values"][1]).all()


def test_no_errors_keeps_everything_at_risk_zero():
    from sm3hip import selective
    N = 65
    rec, kcuts, _, _ = _point(N, "no_errors")
    v = selective.values_from_counts(rec, N, kcuts, len(RISKS), 0)
    assert (v["summary_values"][[0, 1, 2, 3]] == 0.0).all()
    assert (v["risk_values"][0, 0] == 1.0).all() and (v["risk_values"][:, 1] == 0.0).all()   # coverage 1 at risk 0
    assert (v["coverage_values"][:, 0] == 0.0).all() and not v["risk_undefined"].any()


def test_all_errors_keeps_nothing_below_risk_one_and_counts_the_undefined():
    from sm3hip import selective
    N = 65
    rec, kcuts, _, _ = _point(N, "all_errors", pcuts=[[0, N]] * 8)
    v = selective.values_from_counts(rec, N, kcuts, len(RISKS), 2)
    assert (v["risk_values"][:-1, 0] == 0.0).all() and (v["risk_values"][-1, 0] == 1.0).all()
    assert v["risk_undefined"][:-1, 1].all() and (v["risk_values"][:-1, 1] == 0.0).all()      # E* / k* = 0 / 0: noticed
    assert not v["risk_undefined"][:, 0].any() and not v["risk_undefined"][-1].any()
    assert (v["summary_values"][3] == 1.0).all() and (v["coverage_values"][:, 0] == 1.0).all()
    assert v["threshold_undefined"][0, 1:].all() and not v["threshold_undefined"][0, 0].any()  # the cut at 0 keeps nothing
    assert (v["threshold_values"][1, 0] == 1.0).all() and (v["threshold_values"][1, 1] == 1.0).all()
    # all wrong: no true positive, so sensitivity is 0 / FN or 0 / 0 and PPV 0 / FP or 0 / 0 -- a value or a counted undefined
    assert np.isfinite(v["coverage_values"]).all() and (v["coverage_values"][~v["coverage_undefined"]] >= 0).all()


def test_values_are_single_divisions_of_the_record():
    from sm3hip import selective
    N = 257
    pcuts = SI.levels(N, 3, 4, 3)[2]
    rec, kcuts, _, _ = _point(N, "ties", coverages=("0.25", "0.5", "1"), risks=RISKS[:4], pcuts=pcuts)
    v = selective.values_from_counts(rec, N, kcuts, 4, 3)
    _, ph = SI.tails(N)
    for t in range(8):
        r = [int(x) for x in rec[t]]
        A, E, P = r[:3]
        opt = ph[N] - ph[N - E]
        assert v["summary_values"][:, t].tolist() == [A / (N * SI.ONE), opt / (N * SI.ONE), (A - opt) / (N * SI.ONE), E / N]
        for g, k in enumerate(kcuts):
            err, TP, FP, FN = r[3 + 4 * g:7 + 4 * g]
            TN = k - TP - FP - FN
            want = [(err, k), (TP, TP + FN), (TN, TN + FP), (TP, TP + FP), (TN, TN + FN), (P - TP - FN, P)]
            assert v["coverage_values"][g, :, t].tolist() == [a / b if b else 0.0 for a, b in want]
            assert v["coverage_undefined"][g, :, t].tolist() == [b == 0 for _, b in want]
        for h in range(4):
            k, e = r[3 + 12 + 2 * h:5 + 12 + 2 * h]
            assert v["risk_values"][h, :, t].tolist() == [k / N, e / k if k else 0.0]
        for i in range(3):
            C, e, TP, FP, FN = r[3 + 12 + 8 + 5 * i:8 + 12 + 8 + 5 * i]
            TN = C - TP - FP - FN
            want = [(C, N), (e, C), (TP, TP + FN), (TN, TN + FP), (TP, TP + FP), (TN, TN + FN)]
            assert v["threshold_values"][i, :, t].tolist() == [a / b if b else 0.0 for a, b in want]
    for x in ("summary", "coverage", "risk", "threshold"):
        vals = v[x + "_values"]
        acc = np.zeros(vals.shape[:-1])
        for t in range(8):
            acc = acc + vals[..., t]
        assert np.array_equal(vals[..., 8], acc / 8.0)
        assert np.array_equal(v[x + "_undefined"][..., 8], v[x + "_undefined"][..., :8].any(axis=-1))


def test_records_obey_their_identities_under_multiplicities():
    N = 300
    preds, targets = SI.case(N, "ties", 5)
    order, last, _, _ = SI.ranked(preds, targets)
    flg = SI.flags(preds, targets)
    m = SI.multiplicities(7, 2, N)
    kcuts, risks, pcuts = SI.levels(N, 4, 4, 3)
    rec = SI.records(order, flg, last, m, kcuts, risks, pcuts)
    for t in range(8):
        r = rec[t].tolist()
        assert r[1] == int((m * flg[0][t]).sum()) and r[2] == int((m * flg[1][t]).sum())
        assert r[3 + 4:3 + 8] == [r[1], int((m * (flg[1][t] & flg[2][t])).sum()), int((m * (~flg[1][t] & flg[2][t])).sum()),
                                  int((m * (flg[1][t] & ~flg[2][t])).sum())]                      # k = N: the totals
        assert r[3 + 16:3 + 18] == [0, 0] or r[3 + 17] == 0                                      # risk 0: no error kept
        assert r[3 + 18] == N                                                                     # risk 1: everything
        assert r[3 + 24:3 + 29] == [0] * 5 and r[3 + 29] == N                                     # the cuts at 0 and N


# ---- keys and ranking ----------------------------------------------------------------------------------------------------
def test_msp_orders_as_the_top_probability_and_does_not_saturate():
    from sm3hip import selective
    preds, _ = SI.case(257, "random", 1)
    key = selective.keys(preds, "msp")
    assert key.dtype == torch.float64 and tuple(key.shape) == (8, 257)
    for t, p in enumerate(preds):
        top = torch.softmax(p.double(), dim=1).max(dim=1).values
        a, b = top[:, None], top[None, :]
        ka, kb = key[t][:, None], key[t][None, :]
        assert bool(((ka > kb) | ~(a > b)).all())                     # a larger top probability has the larger key
    sat = [torch.zeros(2, n) for n in SI.NUM_CLASSES]
    for p in sat:
        p[0, 0], p[1, 0] = 50.0, 60.0
    assert all(float(torch.softmax(p.double(), 1)[0, 0]) == 1.0 == float(torch.softmax(p.double(), 1)[1, 0]) for p in sat)
    k = selective.keys(sat, "msp")
    assert bool((k[:, 1] > k[:, 0]).all())


def test_margin_and_entropy_are_their_torch_expressions_and_temperature_divides():
    from sm3hip import selective
    preds, _ = SI.case(65, "random", 2)
    temp = [0.5, 1.0, 2.0, 1.5, 3.0, 0.25, 1.0, 4.0]
    for temperature in (None, temp):
        mg, en, ms = (selective.keys(preds, s, temperature) for s in ("margin", "entropy", "msp"))
        for t, p in enumerate(preds):
            z = p.double() / (1.0 if temperature is None else temperature[t])
            top2 = torch.topk(z, 2, dim=1).values
            assert torch.equal(mg[t], top2[:, 0] - top2[:, 1])
            assert torch.equal(en[t], (torch.softmax(z, 1) * torch.log_softmax(z, 1)).sum(dim=1))
            yhat = p.argmax(dim=1)
            for n in range(0, 65, 9):
                others = torch.stack([z[n, c] for c in range(z.shape[1]) if c != int(yhat[n])])
                lse = float(torch.logsumexp(others, 0))     # the same terms in another order: a few ulp of the operands
                top = float(z[n, yhat[n]])
                assert abs(float(ms[t, n]) - (top - lse)) <= 8 * 2.0 ** -52 * max(1.0, abs(top), abs(lse))
    two = selective.keys(preds, "msp")[[2, 7]], selective.keys(preds, "margin")[[2, 7]]
    assert torch.equal(*two)                                           # two classes: msp is the margin
    given = torch.randn(65, 8, generator=torch.Generator().manual_seed(0))
    assert torch.equal(selective.keys(preds, given), given.double().t())


def test_ties_take_the_lowest_class_and_the_ranking_breaks_them_by_msp_then_index():
    from sm3hip import selective
    preds = [torch.zeros(6, n) for n in SI.NUM_CLASSES]
    preds[0][:, 1] = preds[0][:, 3] = 2.0                               # classes 1 and 3 tie: yhat = 1
    assert selective.predicted(preds)[:, 0].tolist() == [1] * 6 and selective.predicted(preds)[:, 1].tolist() == [0] * 6
    primary = torch.tensor([[1.0, 2.0, 2.0, 1.0, 2.0, 0.0]] * 8, dtype=torch.float64)
    msp = torch.tensor([[0.0, 1.0, 3.0, 0.0, 1.0, 9.0]] * 8, dtype=torch.float64)
    order, last, ties, ks = selective.ranking(primary, msp)
    assert order.dtype == torch.int32 and order[0].tolist() == [2, 1, 4, 0, 3, 5]
    assert last[0].tolist() == [False, False, True, False, True, True] and ks[0].tolist() == [2.0, 2.0, 2.0, 1.0, 1.0, 0.0]
    assert ties.tolist() == [4] * 8                                     # (2, 1) twice and (1, 0) twice


@pytest.mark.parametrize("kind", ["ties", "equal", "random"])
def test_ranking_is_the_literal_sort(kind):
    from sm3hip import selective
    N = 130
    preds, targets = SI.case(N, kind, 4)
    for score in ("margin", "entropy"):
        key, msp = selective.keys(preds, score), selective.keys(preds, "msp")
        order, last, ties, ks = selective.ranking(key, msp)
        for t in range(8):
            k, m = key[t].tolist(), msp[t].tolist()
            want = sorted(range(N), key=lambda n: (-k[n], -m[n], n))
            assert order[t].tolist() == want
            assert last[t].tolist() == [j == N - 1 or k[want[j]] != k[want[j + 1]] for j in range(N)]
            pairs = [(k[n], m[n]) for n in range(N)]
            assert int(ties[t]) == sum(pairs.count(p) > 1 for p in pairs)
            assert ks[t].tolist() == [k[n] for n in want]
    if kind == "equal":
        assert int(ties[0]) == N and last[0].tolist() == [False] * (N - 1) + [True]


def test_pack_flags_puts_last_on_the_case():
    from sm3hip import selective
    preds, targets = SI.case(65, "ties", 6)
    order, last, _, _ = SI.ranked(preds, targets)
    err, pos, call = SI.flags(preds, targets)
    packed = selective.pack_flags(preds, targets, torch.from_numpy(order).int(), torch.from_numpy(last)).numpy()
    assert packed.dtype == np.int32 and packed.shape == (8, 65)
    for t in range(8):
        at_case = np.zeros(65, dtype=bool)
        at_case[order[t]] = last[t]
        assert np.array_equal(packed[t], err[t] * 1 + pos[t] * 2 + call[t] * 4 + at_case * 8)


def test_curve_is_the_running_error_rate():
    from sm3hip import selective
    preds, targets = SI.case(65, "random", 8)
    order, _, _, _ = SI.ranked(preds, targets, "margin")
    err = SI.flags(preds, targets)[0]
    got = selective.curve(preds, targets, "margin")
    assert tuple(got.shape) == (8, 65) and got.dtype == torch.float64
    for t in range(8):
        e = np.cumsum(err[t][order[t]])
        assert got[t].tolist() == [int(e[k]) / (k + 1) for k in range(65)]


# ---- thresholds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "ties", "all_errors"])
def test_fitted_thresholds_cut_where_a_plain_count_cuts(kind):
    from sm3hip import selective
    N, M = 97, 131
    fit_preds, fit_targets = SI.case(N, kind, 11)
    order, last, ks, _ = SI.ranked(fit_preds, fit_targets)
    rec = SI.records(order, SI.flags(fit_preds, fit_targets), last, None, [N], [(1, 10)], [[] for _ in range(8)])
    cuts = rec[:, 3 + 4]
    thr = selective.cut_thresholds(ks, cuts)
    key = selective.keys(fit_preds, "msp").numpy()
    for t in range(8):
        if cuts[t] == 0:
            assert thr[t] == np.inf
        else:
            assert int((key[t] >= thr[t]).sum()) == cuts[t]            # on the fitted split: exactly the cut
    if kind == "all_errors":
        assert (cuts == 0).all()
    other_preds, other_targets = SI.case(M, "random" if kind == "all_errors" else kind, 12)
    okey = selective.keys(other_preds, "msp")
    p = selective.position_cuts(okey, selective.check_thresholds(thr))
    assert p.dtype == torch.int32 and tuple(p.shape) == (8, 1)
    want = [sum(1 for v in okey[t].tolist() if v >= thr[t]) for t in range(8)]
    assert p[:, 0].tolist() == want
    oorder, olast, _, _ = SI.ranked(other_preds, other_targets)
    orec = SI.records(oorder, SI.flags(other_preds, other_targets), olast, None, [M], [], [[w] for w in want])
    oerr = SI.flags(other_preds, other_targets)[0]
    for t in range(8):
        kept = okey[t].numpy() >= thr[t]
        assert orec[t, 7] == kept.sum() and orec[t, 8] == (oerr[t] & kept).sum()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))


def test_refusals_come_before_the_device(monkeypatch):
    from sm3hip import selective
    _no_device(monkeypatch)
    preds, targets = SI.case(9, "random", 0)
    nan = [p.clone() for p in preds]
    nan[3][2, 1] = float("nan")
    bad_score = torch.zeros(9, 8)
    bad_score[4, 4] = float("inf")
    big = [torch.zeros(MAX_CASES + 1, n) for n in SI.NUM_CLASSES]
    cases = [
        (dict(preds=nan), "NaN"),
        (dict(score=bad_score), "score"),
        (dict(score=torch.zeros(8, 8)), "score"),
        (dict(score=torch.zeros(9, 8, dtype=torch.int64)), "score"),
        (dict(score="confidence"), "score"),
        (dict(preds=preds[:7]), "preds"),
        (dict(preds=[p[:, :1] for p in preds]), "preds"),
        (dict(targets=targets[:, :7]), "targets"),
        (dict(preds=big, targets=torch.zeros(MAX_CASES + 1, 8, dtype=torch.int64)), "MAX_CASES"),
        (dict(coverages=(0.0,)), "coverages"),
        (dict(coverages=(1.5,)), "coverages"),
        (dict(coverages=()), "coverages"),
        (dict(coverages=("0.1234567",)), "coverages"),
        (dict(coverages=[0.5] * 17), "coverages"),
        (dict(risks=(-0.1,)), "risks"),
        (dict(risks=(1.01,)), "risks"),
        (dict(risks=("0.0000001",)), "risks"),
        (dict(risks=[0.1] * 9), "risks"),
        (dict(risks=("a tenth",)), "risks"),
        (dict(thresholds=torch.zeros(7)), "thresholds"),
        (dict(thresholds=torch.zeros(8, 9)), "thresholds"),
        (dict(thresholds=torch.full((8,), float("nan"))), "thresholds"),
        (dict(temperature=[1.0] * 7), "temperature"),
        (dict(bootstrap=-1), "bootstrap"),
    ]
    for kw, text in cases:
        kw = dict(dict(preds=preds, targets=targets), **kw)
        with pytest.raises(ValueError, match=text):
            selective.selective_report(kw.pop("preds"), kw.pop("targets"), **kw)
    with pytest.raises(ValueError, match="risk"):
        selective.fit_thresholds(preds, targets, risk="1.5")
    with pytest.raises(ValueError, match="score"):
        selective.fit_thresholds(preds, targets, score="best")
    with pytest.raises(ValueError, match="score"):
        selective.curve(preds, targets, "best")
    with pytest.raises(AssertionError, match="the device was touched"):   # and a good call goes on to the device
        selective.selective_report(preds, targets)


def test_levels_are_the_rationals_of_their_strings():
    from sm3hip import selective
    names, pairs = selective.check_coverages((0.1, "0.30", 1, 1.0, "0.000001"))
    assert names == ["0.1", "0.30", "1", "1.0", "0.000001"] and pairs == [(1, 10), (3, 10), (1, 1), (1, 1), (1, 1000000)]
    assert selective.check_risks(()) == ([], []) and selective.check_risks((0, 1))[1] == [(0, 1), (1, 1)]
    for N in (1, 7, 10, 395, MAX_CASES):
        for num, den in pairs + [(7, 10), (999999, 1000000)]:
            (k,) = selective.coverage_cuts(N, [(num, den)])
            assert k == math.ceil(fractions.Fraction(num, den) * N) and 1 <= k <= N
    assert selective.coverage_cuts(100, [(7, 100)]) == [7] and math.ceil(0.07 * 100) == 8   # what a float product would do


def test_check_flags_refuses_without_the_device(monkeypatch):
    from sm3hip import selective
    _no_device(monkeypatch)
    parser = selective.add_flags(argparse.ArgumentParser())
    selective.check_flags(parser.parse_args([]))
    for bad, text in ((["--selective-coverage", "0"], "--selective-coverage"), (["--selective-risk", "2"], "--selective-risk"),
                      (["--selective-rule", "0.12345678"], "--selective-rule"), (["--selective-coverage", "x"], "--selective-coverage")):
        with pytest.raises(ValueError, match=text):
            selective.check_flags(parser.parse_args(bad))
    with pytest.raises(SystemExit):
        parser.parse_args(["--selective-score", "best"])
    args = parser.parse_args(["--selective", "--selective-score", "margin", "--selective-coverage", "0.5", "1", "--selective-risk"])
    assert selective.flag_settings(args) == dict(score="margin", coverages=["0.5", "1"], risks=[])
    assert "score" not in selective.flag_settings(parser.parse_args(["--selective-score", "tta-range"]))


def test_compare_refuses_what_is_not_paired():
    from sm3hip import selective
    N = 33
    preds, targets = SI.case(N, "random", 1)

    def rep(score, coverages=("0.5", "1"), seed=0):
        order, last, _, ties = SI.ranked(preds, targets, score)
        names, pairs = selective.check_coverages(coverages)
        kcuts = selective.coverage_cuts(N, pairs)
        flg = SI.flags(preds, targets)
        point = SI.records(order, flg, last, None, kcuts, [(1, 10)], [[]] * 8)
        reps = np.stack([SI.records(order, flg, last, SI.multiplicities(seed, r, N), kcuts, [(1, 10)], [[]] * 8) for r in range(4)])
        return selective.assemble(point, reps, targets, names, kcuts, ["0.1"], torch.zeros(8, 0), torch.zeros(8, 0), ties, score,
                                  [1.0] * 8, 4, seed, 0.9)
    a, b = rep("msp"), rep("margin")
    cmp = selective.compare(a, b)
    assert torch.equal(cmp["summary_delta"], a["summary_values"] - b["summary_values"]) and cmp["scores"] == ["msp", "margin"]
    assert tuple(cmp["coverage_lo"].shape) == (2, 6, 9) and tuple(cmp["risk_frac_le_zero"].shape) == (1, 2, 9)
    same = selective.compare(a, a)
    for x in ("summary", "coverage", "risk"):
        assert not same[x + "_delta"].any() and not same[x + "_lo"].any() and not same[x + "_hi"].any()
    with pytest.raises(ValueError, match="coverages"):
        selective.compare(a, rep("msp", ("0.5",)))
    with pytest.raises(ValueError, match="seed"):
        selective.compare(a, rep("msp", seed=1))
    with pytest.raises(ValueError, match="selective_report"):
        selective.compare(a, {})
    assert "AURC" in selective.format_table(a) and "difference" in selective.format_compare(cmp)
    assert selective.stats_line(a).startswith("AURC_AVG") and "MAX_CASES" in selective.stats_line(None)


def test_files_round_trip(tmp_path):
    import csv
    import json
    from sm3hip import selective
    N = 33
    preds, targets = SI.case(N, "ties", 2)
    order, last, _, ties = SI.ranked(preds, targets)
    kcuts = [17, N]
    rec = SI.records(order, SI.flags(preds, targets), last, None, kcuts, [(1, 10)], [[5]] * 8)
    rep = selective.assemble(rec, None, targets, ["0.5", "1"], kcuts, ["0.1"], torch.full((8, 1), float("inf")),
                             torch.full((8, 1), 5), ties, "msp", [1.0] * 8)
    selective.save(rep, str(tmp_path), "x_selective")
    with open(tmp_path / "x_selective.json") as f:
        d = json.load(f)
    assert "targets" not in d and d["summary_values"] == rep["summary_values"].tolist() and d["coverages"] == ["0.5", "1"]
    assert d["thresholds"] == [[float("inf")]] * 8 and d["ties"] == rep["ties"].tolist()
    with open(tmp_path / "x_selective.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["table", "level", "row", "column", "value"] and len(rows) == 1 + 9 * (4 + 2 * 6 + 2 + 6)
    for row, want in zip(rows[1:], selective.csv_rows(rep)):
        assert row[:4] == [str(v) for v in want[:4]] and float(row[4]) == want[4]


# ---- the tool and the ABI ------------------------------------------------------------------------------------------------
def test_the_tool_carries_the_flags_and_the_registry_is_unchanged():
    tool = _load("sm3_selective_cpu_eval_report", os.path.join(TOOLS, "eval_report.py"))
    import eval_cli
    have = {s for a in tool.get_parser()._actions for s in a.option_strings}
    assert {"--selective", "--selective-score", "--selective-coverage", "--selective-risk", "--selective-rule"} <= have
    assert [flag for flag, _, _ in eval_cli.REPORTS] == ["calibration", "operating", "checklist"]
    args = tool.get_parser().parse_args(["x.pt"])
    assert args.selective is False and args.selective_score == "msp" and args.selective_rule == "0.1"


def test_header_binding_and_record_size_agree():
    from sm3hip import _lib, ops
    assert len(_lib.SIGNATURES["sm3_selective_counts"]) == 16 and len(_lib.SIGNATURES["sm3_selective_record"]) == 3
    lib = _lib.load()
    for G, H, Pc in ((1, 0, 0), (16, 8, 8), (6, 3, 1)):
        assert lib.sm3_selective_record(G, H, Pc) == ops.selective_record(G, H, Pc) == 3 + 4 * G + 2 * H + 5 * Pc
    assert lib.sm3_selective_counts(None, None, None, None, None, None, None, 1, 1, 0, 0, 0, 0, 1, 1, None) == -1
