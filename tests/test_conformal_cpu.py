"""CPU: the conformal report (sm3hip/conformal.py, csrc/conformal.hip) through its restatement in tests/conformal_inputs.py, and
everything about it that needs no GPU.

  * hand cases of the scores; the rank edges (N_cal = 8 / 9 at alpha = 0.1, 18 / 19 at 0.05); the integer rank formula against
    fractions.Fraction for every n' in 0 .. 8192, with at least one n' at which ceil((n' + 1)(1 - alpha)) in floats is wrong;
  * the point threshold against np.sort(a)[k - 1];
  * validity of the procedure (on the restatement): R = 200 independent splits, N_cal = 100, N_test = 200, 5 classes, logits
    2 N(0, 1), labels from their own softmax, alpha = 0.1, seed 0.  Mean marginal coverage in [0.9 - 0.013, 0.9 + 1/101 + 0.013]:
    coverage given the threshold is Binomial(N_test, p) / N_test with p ~ Beta(k, N_cal + 1 - k), so its variance is at most
    alpha (1 - alpha)(1 / N_test + 1 / (N_cal + 2)), sd <= 0.0365, and 5 * 0.0365 / sqrt(200) = 0.013.  In class mode every
    class's mean coverage is at least 0.9 - 0.013 * sqrt(5) (class counts are a fifth of N_test);
  * identities on every record, monotonicity in alpha, == under a joint permutation of the cases, temperature of ones == None;
  * the library's host side: scores and prediction_sets against the restatement, values_from_counts against Python numbers,
    argument refusals, compare's refusals, the JSON / CSV round trip, the tool's flags, the header <-> ctypes entry."""
import csv
import importlib.util
import json
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


CI = _load("sm3_conformal_inputs_cpu", os.path.join(ROOT, "tests", "conformal_inputs.py"))
ONE, INF = CI.ONE, CI.INF
ALPHAS = (0.05, 0.1, 0.2)


# ---- scores --------------------------------------------------------------------------------------------------------------
def test_hand_cases_of_the_scores():
    from sm3hip import conformal
    assert conformal.INF == INF and conformal.ONE == ONE
    preds = [torch.zeros(2, n) for n in CI.NUM_CLASSES]
    preds[0][0, 3] = 1e4                                                 # a certain prediction
    preds[3] = torch.tensor([[1.0, 3.0, 2.0], [0.0, 0.0, 0.0]])
    lac, aps = conformal.scores(preds, None, "lac").numpy(), conformal.scores(preds, None, "aps").numpy()
    q = CI.q32(preds)
    assert lac[:5, 0].tolist() == [ONE, ONE, ONE, 0, ONE]
    k = CI.FIRST[3]
    assert aps[k + 1, 0] == q[k + 1, 0]                                  # the top class: its own q
    assert aps[k, 0] == q[k:k + 3, 0].sum()                              # the last class: all of them
    assert aps[k + 2, 0] == q[k + 1, 0] + q[k + 2, 0]
    third = q[k, 1]
    assert q[k:k + 3, 1].tolist() == [third] * 3 and aps[k:k + 3, 1].tolist() == [third, 2 * third, 3 * third]   # ties by class index
    for method, got in (("lac", lac), ("aps", aps)):
        assert np.array_equal(got, CI.scores(q, method)), method


@pytest.mark.parametrize("kind", ["ties", "equal", "random"])
def test_scores_and_sets_equal_the_restatement(kind):
    from sm3hip import conformal
    preds, targets = CI.case(67, kind, 3)
    temp = [0.5, 1.0, 2.0, 1.25, 1.0, 3.0, 0.75, 1.0]
    for method in ("lac", "aps"):
        for temperature in (None, temp):
            s = conformal.scores(preds, temperature, method)
            want = CI.scores(CI.q32(preds, temperature), method)
            assert s.dtype == torch.int64 and np.array_equal(s.numpy(), want)
            a = conformal.true_class_scores(s, targets).numpy()
            assert np.array_equal(a, CI.true_scores(want, targets.numpy()))
        _, thr = CI.restate((preds, targets), (preds, targets), ALPHAS, method, "class")
        sets = conformal.prediction_sets(preds, torch.from_numpy(thr), level=1, method=method).numpy()
        want = np.stack([CI.scores(CI.q32(preds), method)[k] <= thr[t, 1, c] for k, (t, c) in enumerate(CI.PAIRS)], axis=1)
        assert sets.shape == (67, 24) and sets.dtype == bool and np.array_equal(sets, want)
    with pytest.raises(ValueError):
        conformal.prediction_sets(preds, torch.from_numpy(thr), level=3)
    with pytest.raises(ValueError):
        conformal.prediction_sets(preds, torch.from_numpy(thr[:, :, :4]))


# ---- ranks ---------------------------------------------------------------------------------------------------------------
def test_rank_edges():
    from sm3hip import conformal
    assert CI.rank(8, 0.1) == 9 and CI.rank(9, 0.1) == 9 and CI.rank(18, 0.05) == 19 and CI.rank(19, 0.05) == 19
    for n, alpha, inf in ((8, 0.1, True), (9, 0.1, False), (18, 0.05, True), (19, 0.05, False)):
        preds, targets = CI.case(n, "random", n)
        for method in ("lac", "aps"):
            R = CI.Restated((preds, targets), (preds, targets), method)
            counts, thr = R([alpha], "marginal")
            for t, nt in enumerate(CI.NUM_CLASSES):
                if inf:
                    assert (thr[t, 0, :nt] == INF).all() and counts[t, 0, 3 + nt] == n and counts[t, 0, 0] == n   # every set is full
                else:
                    assert (thr[t, 0, :nt] == R.cal_a[t].max()).all()                                            # k = n: the largest
                assert (thr[t, 0, nt:] == 0).all()
    _, levels = conformal.check_alphas([0.1, 0.05])
    assert levels == [(1, 10), (1, 20)]
    assert conformal.rank(8, 1, 10) == 9 and conformal.rank(9, 1, 10) == 9 and conformal.rank(0, 1, 10) == 1


def test_integer_rank_equals_the_rational_rank_where_floats_do_not():
    """The integer formula == the rational one for every n' in 0 .. 8192 at the six levels 0.01, 0.05, 0.1, 0.2, 0.5, 0.333333.
    Where floats go wrong, counted here: the literal ceil((n' + 1) * (1 - alpha)) in fp64 happens to agree at all of those six
    levels (0 differences), so the n' at which a float form differs come from (a) the usual way the rank reaches a quantile
    routine, as the level (n' + 1)(1 - alpha) / n' multiplied back by n' (wrong at n' = 29 for alpha = 0.5, 304 for 0.2, 4299
    for 0.1, 2119 for 0.05), and (b) two further levels, 0.7 and 0.45, at which the literal form itself is wrong (n' = 9:
    10 * (1 - 0.7) = 3.0000000000000004, rank 4 instead of 3)."""
    from sm3hip import conformal
    literal, by_level = {}, {}
    for alpha in (0.01, 0.05, 0.1, 0.2, 0.5, 0.333333, 0.7, 0.45):
        (num, den), = conformal.check_alphas([alpha])[1]
        assert num / den == alpha
        literal[alpha] = by_level[alpha] = 0
        for n in range(8193):
            k = CI.rank(n, alpha)
            assert conformal.rank(n, num, den) == k and 1 <= k <= n + 1
            literal[alpha] += math.ceil((n + 1) * (1 - alpha)) != k
            by_level[alpha] += n > 0 and math.ceil(((n + 1) * (1 - alpha) / n) * n) != k
    print("float ranks that differ, literal form:", literal, "through the quantile level:", by_level)
    assert literal[0.7] > 0 and literal[0.45] > 0 and math.ceil(10 * (1 - 0.7)) == 4 and CI.rank(9, 0.7) == 3
    assert by_level[0.5] > 0 and by_level[0.2] > 0 and by_level[0.1] > 0 and by_level[0.05] > 0
    assert math.ceil((30 * (1 - 0.5) / 29) * 29) == 16 and CI.rank(29, 0.5) == 15


@pytest.mark.parametrize("conditional", ["marginal", "class"])
def test_point_threshold_is_the_order_statistic_of_numpy(conditional):
    preds, targets = CI.case(257, "ties", 11)
    for method in ("lac", "aps"):
        R = CI.Restated((preds, targets), (preds, targets), method)
        _, thr = R(ALPHAS, conditional)
        for t, nt in enumerate(CI.NUM_CLASSES):
            for a, alpha in enumerate(ALPHAS):
                for c in range(nt):
                    sel = R.cal_a[t] if conditional == "marginal" else R.cal_a[t][R.cal_y[:, t] == c]
                    k = CI.rank(len(sel), alpha)
                    assert thr[t, a, c] == (INF if k > len(sel) else np.sort(sel)[k - 1])
        # a weighted split: the w-fold copies
        w = CI.multiplicities(5, 3, 257, 6)
        _, thr = R(ALPHAS, conditional, w=w)
        rep = np.repeat(np.arange(257), w)
        for t, nt in enumerate(CI.NUM_CLASSES):
            for c in range(nt):
                sel = R.cal_a[t][rep] if conditional == "marginal" else R.cal_a[t][rep][R.cal_y[rep, t] == c]
                k = CI.rank(len(sel), 0.1)
                assert thr[t, 1, c] == (INF if k > len(sel) else np.sort(sel)[k - 1])


# ---- validity ------------------------------------------------------------------------------------------------------------
def _q_rows(z):
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return np.rint(p * float(ONE)).astype(np.int64)


@pytest.mark.parametrize("method", ["lac", "aps"])
def test_validity_of_the_procedure(method):
    R, n_cal, n_test, alpha, band = 200, 100, 200, 0.1, 0.013
    assert 5 * math.sqrt(alpha * (1 - alpha) * (1 / n_test + 1 / (n_cal + 2))) / math.sqrt(R) <= band
    g = np.random.default_rng(0)
    marginal, classwise = [], [[] for _ in range(5)]
    for _ in range(R):
        z, y = CI.sampled_split(n_cal + n_test, g)
        s = np.array([CI.scores_of_row([int(v) for v in row], method) for row in _q_rows(z)], dtype=np.int64)   # [n, 5]
        a = s[np.arange(len(y)), y]
        ones = np.ones(n_cal, dtype=np.int64)
        qhat = CI.kth(a[:n_cal], ones, alpha)
        marginal.append(float((a[n_cal:] <= qhat).mean()))
        for c in range(5):
            cal = a[:n_cal][y[:n_cal] == c]
            qc = CI.kth(cal, np.ones(len(cal), dtype=np.int64), alpha)
            test = a[n_cal:][y[n_cal:] == c]
            if len(test):
                classwise[c].append(float((test <= qc).mean()))
    mean = float(np.mean(marginal))
    print(f"{method}: mean marginal coverage {mean:.4f}, sd {np.std(marginal):.4f}; class means "
          + " ".join(f"{np.mean(v):.4f}" for v in classwise))
    assert 0.9 - band <= mean <= 0.9 + 1 / 101 + band
    for c in range(5):
        assert np.mean(classwise[c]) >= 0.9 - band * math.sqrt(5), c


# ---- records -------------------------------------------------------------------------------------------------------------
def _identities(counts, N):
    counts = np.asarray(counts)
    hist = counts[..., 3:9]
    assert (hist.sum(axis=-1) == N).all()
    assert ((hist * np.arange(6)).sum(axis=-1) == counts[..., 1]).all()
    assert (counts[..., 9::3].sum(axis=-1) == N).all()
    assert (counts[..., 10::3].sum(axis=-1) == counts[..., 0]).all()
    assert (counts[..., 11::3].sum(axis=-1) == counts[..., 1]).all()
    assert (counts[..., 2] <= np.minimum(counts[..., 0], counts[..., 4])).all()


@pytest.mark.parametrize("kind", ["ties", "equal", "absent", "random"])
def test_identities_monotonicity_and_the_two_counters(kind):
    cal, test = CI.case(131, kind, 5), CI.case(90, kind, 6)
    alphas = (0.5, 0.2, 0.1, 0.05, 0.01)                                  # decreasing
    for method in ("lac", "aps"):
        R = CI.Restated(cal, test, method)
        for conditional in ("marginal", "class"):
            for w, m in ((None, None), (CI.multiplicities(9, 4, 131, 6), CI.multiplicities(9, 4, 90, 2))):
                counts, thr = R(alphas, conditional, w=w, m=m)
                _identities(counts, 90)
                assert (np.diff(thr, axis=1) >= 0).all()
                assert (np.diff(counts[:, :, 0], axis=1) >= 0).all() and (np.diff(counts[:, :, 1], axis=1) >= 0).all()
                mm = np.ones(90, dtype=np.int64) if m is None else m
                assert np.array_equal(counts, CI.records_np(R.s, R.y, mm, thr))
                assert np.array_equal(counts, CI.records(R.s, R.y, mm, thr))
                if kind == "absent" and conditional == "class":
                    assert (thr[:, :, 1] == INF).all()                     # no calibration case of class 1 anywhere
    assert not np.array_equal(CI.multiplicities(9, 4, 90, 6), CI.multiplicities(9, 4, 90, 2))
    assert np.array_equal(CI.multiplicities(9, 4, 90, 2), CI.REP.multiplicities(9, 4, 90))


def test_joint_permutations_change_nothing():
    cal, test = CI.case(77, "ties", 1), CI.case(65, "ties", 2)
    g = torch.Generator().manual_seed(0)
    pc, pt = torch.randperm(77, generator=g), torch.randperm(65, generator=g)
    cal2 = ([p[pc] for p in cal[0]], cal[1][pc])
    test2 = ([p[pt] for p in test[0]], test[1][pt])
    w, m = CI.multiplicities(3, 1, 77, 6), CI.multiplicities(3, 1, 65, 2)
    for method in ("lac", "aps"):
        for conditional in ("marginal", "class"):
            base = CI.restate(cal, test, ALPHAS, method, conditional)
            both = CI.restate(cal2, test2, ALPHAS, method, conditional)
            assert np.array_equal(base[0], both[0]) and np.array_equal(base[1], both[1])
            base = CI.restate(cal, test, ALPHAS, method, conditional, w=w, m=m)
            both = CI.restate(cal2, test, ALPHAS, method, conditional, w=w[pc.numpy()], m=m)   # the copies move with their case
            assert np.array_equal(base[0], both[0]) and np.array_equal(base[1], both[1])
            ones = CI.restate(cal, test, ALPHAS, method, conditional, temperature=[1.0] * 8, fixed=base[1])
            none = CI.restate(cal, test, ALPHAS, method, conditional, fixed=base[1])
            assert np.array_equal(ones[0], none[0]) and np.array_equal(ones[1], base[1])


# ---- the library's host side -----------------------------------------------------------------------------------------------
def _report(seed=0, method="lac", conditional="marginal", refit=True, bootstrap=6, cal=None, test=None, alphas=ALPHAS):
    from sm3hip import conformal
    cal, test = cal or CI.case(60, "random", 1), test or CI.case(45, "random", 2)
    R = CI.Restated(cal, test, method)
    alphas, levels = conformal.check_alphas(alphas)
    pc, pt = R(alphas, conditional)
    reps = [R(alphas, conditional, w=CI.multiplicities(seed, r, 60, 6), m=CI.multiplicities(seed, r, 45, 2),
              fixed=None if refit else pt) for r in range(bootstrap)]
    rc, rt = (np.stack([r[e] for r in reps]) for e in (0, 1)) if bootstrap else (None, None)
    return conformal.assemble(pc, pt, rc, rt, test[1], cal[1], alphas, levels, method, conditional, [1.0] * 8, refit, bootstrap,
                              seed, 0.9), (pc, pt, rc, rt)


def test_values_are_one_division_each():
    from sm3hip import conformal, report
    rep, (pc, pt, rc, rt) = _report(conditional="class", alphas=(0.4, 0.1))
    label, cls, tv = CI.values(pc.tolist(), pt.tolist(), 45)
    assert rep["label_values"].tolist() == label and rep["class_values"][:, :, :24].tolist() == cls
    assert rep["threshold_values"].tolist() == tv
    assert np.array_equal(rep["class_values"][:, :, 24:].numpy(), report.averages(rep["class_values"][:, :, :24].numpy()))
    assert rep["label_values"].shape == (2, 5, 9) and rep["class_values"].shape == (2, 2, 29) and rep["threshold_values"].shape == (2, 8, 5)
    assert torch.equal(rep["threshold_inf"], torch.from_numpy(np.moveaxis(pt, 0, 1) >= INF))
    for r in range(6):
        label, cls, tv = CI.values(rc[r].tolist(), rt[r].tolist(), 45)
        assert rep["label_replicates"][r].tolist() == label and rep["class_replicates"][r, :, :, :24].tolist() == cls
        assert rep["threshold_replicates"][r].tolist() == tv
    for x in conformal.TABLES:
        lo, hi = report.interval(rep[f"{x}_replicates"].numpy(), 0.9)
        assert np.array_equal(rep[f"{x}_lo"].numpy(), lo) and np.array_equal(rep[f"{x}_hi"].numpy(), hi)
    n_c = np.moveaxis(rc[:, :, :, 9::3], 1, 2)                            # [B, A, 8, 5]
    want = sum(int((n_c[:, :, t, c] == 0).sum()) for t, c in CI.PAIRS)
    assert int(rep["class_undefined"][:, 0, :24].sum()) == want and not rep["class_undefined"][:, 1, :24].any()
    assert torch.equal(rep["threshold_undefined"], torch.from_numpy((np.moveaxis(rt, 1, 2) >= INF).sum(axis=0)))
    # undefined: a zero denominator gives 0 and is flagged
    counts = np.zeros((8, 1, 24), dtype=np.int64)
    counts[:, 0, 3] = 7
    v = conformal.values_from_counts(counts, np.zeros((8, 1, 5), dtype=np.int64), 7)
    assert v["label_undefined"][0, 4].all() and (v["label_values"][0, 4] == 0).all() and (v["label_values"][0, 2] == 1).all()
    assert v["class_undefined"][0, 0].all() and not v["class_undefined"][0, 1].any() and not v["label_undefined"][0, :4].any()


def test_argument_refusals():
    from sm3hip import conformal
    cal, test = CI.case(9, "random", 1), CI.case(5, "random", 2)
    ok = dict(alphas=(0.1,), method="lac", conditional="marginal")
    for bad in (dict(alphas=()), dict(alphas=[0.1] * 9), dict(alphas=(0.0,)), dict(alphas=(1.0,)), dict(alphas=(True,)),
                dict(alphas=("0.1",)), dict(alphas=(0.1234567,)), dict(alphas=(1e-7,)), dict(method="raps"),
                dict(conditional="label"), dict(refit=1), dict(temperature=[1.0] * 7), dict(temperature=[0.0] * 8),
                dict(bootstrap=-1), dict(confidence=1.0), dict(seed=2 ** 64), dict(bootstrap=4, chunk=5)):
        with pytest.raises(ValueError):
            conformal.conformal_report(*test, *cal, **dict(ok, **bad))
    for args in ((test[0][:7], test[1], *cal), (*test, cal[0], cal[1][:8]), (*test, cal[0], cal[1].int()),
                 ([p[:0] for p in test[0]], test[1][:0], *cal), (*test, [p[:0] for p in cal[0]], cal[1][:0]),
                 (*test, *CI.make_case(8193, "equal", 0))):
        with pytest.raises(ValueError):
            conformal.conformal_report(*args, **ok)
    for bad in (dict(alphas=(0.1234567,)), dict(method="x"), dict(conditional="x"), dict(temperature=[-1.0] * 8)):
        with pytest.raises(ValueError):
            conformal.fit_thresholds(*cal, **bad)
    assert conformal.check_alphas(0.25) == ([0.25], [(1, 4)]) and conformal.check_alphas([0.333333])[1] == [(333333, 1000000)]


def test_ops_wrapper_checks_shapes_and_levels():
    from sm3hip import ops
    import fakelib
    T, K, A, Nc, N = 8, 24, 2, 6, 4
    with fakelib.installed() as fake:
        def tensors():
            return dict(cal_a=torch.zeros(T, Nc, dtype=torch.int64), cal_order=torch.zeros(T, Nc, dtype=torch.int32),
                        cal_y=torch.zeros(Nc, T, dtype=torch.int32), s=torch.zeros(K, N, dtype=torch.int64),
                        y=torch.zeros(N, T, dtype=torch.int32), colmap=torch.zeros(K, 2, dtype=torch.int32),
                        alphas=[(1, 10), (1, 5)], counts=torch.zeros(3, T, A, 24, dtype=torch.int64),
                        thr=torch.zeros(3, T, A, 5, dtype=torch.int64), conditional="class", seed=1, r0=0)
        ops.conformal_counts(**tensors())
        ops.conformal_counts(**dict(tensors(), fixed_thr=torch.zeros(T, A, 5, dtype=torch.int64)))
        assert fake.calls == ["sm3_conformal_counts"] * 2
        for bad in (dict(alphas=[(1, 10)]), dict(alphas=[(0, 10), (1, 5)]), dict(alphas=[(10, 10), (1, 5)]),
                    dict(alphas=[(0.1, 1), (1, 5)]), dict(conditional="x"), dict(seed=2 ** 64), dict(point=True),
                    dict(cal_order=torch.zeros(T, Nc, dtype=torch.int64)), dict(cal_y=torch.zeros(Nc + 1, T, dtype=torch.int32)),
                    dict(thr=torch.zeros(3, T, A, 4, dtype=torch.int64)), dict(counts=torch.zeros(3, T, A, 23, dtype=torch.int64)),
                    dict(fixed_thr=torch.zeros(T, 1, 5, dtype=torch.int64)), dict(s=torch.zeros(K, 0, dtype=torch.int64)),
                    dict(counts=torch.zeros(3, T, 9, 24, dtype=torch.int64), thr=torch.zeros(3, T, 9, 5, dtype=torch.int64))):
            with pytest.raises(ValueError):
                ops.conformal_counts(**dict(tensors(), **bad))
        assert len(fake.calls) == 2


def test_compare_refuses_what_is_not_paired():
    from sm3hip import conformal
    a, _ = _report()
    b, _ = _report(test=CI.case(45, "ties", 2))
    b["targets"] = a["targets"].clone()
    cmp = conformal.compare(a, b)
    assert torch.equal(cmp["label_delta"], a["label_values"] - b["label_values"]) and cmp["class_lo"].shape == (3, 2, 29)
    d = (a["label_replicates"] - b["label_replicates"]).numpy()
    assert np.array_equal(cmp["label_frac_le_zero"].numpy(), (d <= 0).mean(axis=0))
    for other in (_report(method="aps")[0], _report(conditional="class")[0], _report(refit=False)[0], _report(alphas=(0.05, 0.1))[0],
                  _report(seed=1)[0], _report(bootstrap=5)[0], _report(test=CI.case(45, "random", 3))[0],
                  _report(cal=CI.case(60, "random", 4))[0], {"label_values": a["label_values"]}, None):
        with pytest.raises(ValueError):
            conformal.compare(a, other)
    assert "label_lo" not in conformal.compare(_report(bootstrap=0)[0], _report(bootstrap=0)[0])


def test_json_and_csv_round_trip(tmp_path):
    from sm3hip import conformal
    rep, _ = _report(conditional="class", alphas=(0.4, 0.1))
    rep["threshold_values"][0, 0, 0] = float("inf")
    conformal.save(rep, str(tmp_path), "x_conformal")
    saved = json.load(open(tmp_path / "x_conformal.json"))
    for key in ("label_values", "class_values", "threshold_values", "label_lo", "class_hi", "threshold_undefined", "counts",
                "thresholds", "threshold_inf"):
        assert saved[key] == rep[key].tolist(), key
    assert saved["alphas"] == [0.4, 0.1] and saved["levels"] == [[2, 5], [1, 10]] and saved["method"] == "lac"
    assert saved["conditional"] == "class" and saved["refit"] is True and saved["n"] == 45 and saved["n_cal"] == 60
    assert saved["bootstrap"] == 6 and "label_replicates" not in saved and "targets" not in saved and "cal_targets" not in saved
    rows = list(csv.reader(open(tmp_path / "x_conformal.csv")))
    assert rows[0] == ["table", "alpha", "row", "column", "value", "lo", "hi", "undefined"]
    by = {(r[0], float(r[1]), r[2], r[3]): r for r in rows[1:]}
    assert len(by) == len(rows) - 1 == 2 * (5 * 9 + 2 * 29 + 24)
    for a, alpha in enumerate(rep["alphas"]):
        for i, m in enumerate(rep["label_metrics"]):
            for k, c in enumerate(rep["label_columns"]):
                r = by[("label", alpha, m, c)]
                assert (float(r[4]), float(r[5]), float(r[6]), int(r[7])) == (
                    float(rep["label_values"][a, i, k]), float(rep["label_lo"][a, i, k]), float(rep["label_hi"][a, i, k]),
                    int(rep["label_undefined"][a, i, k]))
        for i, m in enumerate(rep["class_metrics"]):
            for k, c in enumerate(rep["class_columns"]):
                assert float(by[("class", alpha, m, c)][4]) == float(rep["class_values"][a, i, k])
        for t, c in CI.PAIRS:
            assert float(by[("threshold", alpha, rep["label_columns"][t], str(c + 1))][4]) == float(rep["threshold_values"][a, t, c])
    assert float(by[("threshold", 0.4, rep["label_columns"][0], "1")][4]) == float("inf")
    text = conformal.format_table(rep)
    assert "alpha 0.4" in text and "singleton accuracy" in text and "class coverage" in text and "[" in text
    assert "coverage_AVG@0.1" in conformal.stats_line(rep) and "no conformal report" in conformal.stats_line(None)
    point, _ = _report(bootstrap=0)
    conformal.save(point, str(tmp_path), "p")
    assert list(csv.reader(open(tmp_path / "p.csv")))[0] == ["table", "alpha", "row", "column", "value"]
    assert "bootstrap" not in json.load(open(tmp_path / "p.json"))


def test_tool_flags(capsys):
    er = _load("sm3_conformal_cpu_eval_report", os.path.join(TOOLS, "eval_report.py"))
    with pytest.raises(SystemExit):
        er.main(["x.pt", "--conformal"])
    assert "--fit-on" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        er.main(["x.pt", "--conformal", "--fit-on", "v.pt", "--conformal-alpha", "1.5"])
    assert "alpha" in capsys.readouterr().err
    args = er.get_parser().parse_args(["x.pt"])
    assert not args.conformal and args.conformal_alpha == [0.05, 0.1, 0.2] and args.conformal_method == "lac"
    assert args.conformal_conditional == "marginal" and not args.conformal_fixed and not args.conformal_scaled
    assert args.against_fit_on is None and not args.calibration
    args = er.get_parser().parse_args(["x.pt", "--conformal", "--fit-on", "v.pt", "--conformal-alpha", "0.1", "--conformal-method", "aps",
                                       "--conformal-conditional", "class", "--conformal-fixed", "--conformal-scaled"])
    from sm3hip import conformal
    assert conformal.flag_settings(args) == dict(alphas=[0.1], method="aps", conditional="class", refit=False)
    # the training / evaluation tools hold one split and take none of the flags
    import eval_cli
    import argparse
    p = eval_cli.add_report_flags(argparse.ArgumentParser())
    assert not any("conformal" in s for a in p._actions for s in a.option_strings)


def test_header_and_binding_hold_the_symbol():
    from sm3hip import _lib
    text = open(os.path.join(ROOT, "include", "sm3_hip.h")).read()
    decl = text[text.index("int sm3_conformal_counts("):]
    decl = decl[:decl.index(";")]
    assert len(decl.split(",")) == len(_lib.SIGNATURES["sm3_conformal_counts"]) == 21
    lib = _lib.load()
    assert lib.sm3_abi_version() == 9
    # argument errors are refused on the host, before any launch: checkable without a GPU
    import ctypes as C
    lv = (C.c_int * 2)(1, 10)
    one = C.c_void_p(8)

    def call(N_cal=5, N=5, A=1, conditional=0, r0=0, c=1, point=0, alpha=lv):
        return lib.sm3_conformal_counts(one, one, one, one, one, one, alpha, None, one, one, N_cal, N, 8, 24, A, conditional, 0, r0,
                                        c, point, None)
    for kw in ({"N_cal": 0}, {"N": 0}, {"N_cal": 8193}, {"N": 8193}, {"A": 0}, {"A": 9}, {"conditional": 2}, {"conditional": -1},
               {"c": 0}, {"r0": -1}, {"r0": 2 ** 32}, {"point": 1, "c": 2}, {"alpha": (C.c_int * 2)(0, 10)},
               {"alpha": (C.c_int * 2)(10, 10)}, {"alpha": (C.c_int * 2)(1, 0)}, {"alpha": (C.c_int * 2)(-1, -10)}, {"alpha": None}):
        assert call(**kw) == -1, kw
