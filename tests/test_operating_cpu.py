"""CPU: the operating-point report (sm3hip/operating.py, csrc/operating.hip) restated in plain Python integers, and everything
about it that needs no GPU.  tests/test_operating_gpu.py loads this file for the restatement.

  * the restatement (loops, Python ints, tuple keys for the lexicographic orders and functools.cmp_to_key for F1's) against scikit-learn, for the point
    estimate and for Philox multiplicities passed as sample_weight: average_precision_score within 2^-32 (every precQ_g is within
    2^-33 of the exact precision and the weights dTP_g / P sum to 1; the float sums of scikit-learn add rounding far below
    that), max tpr - fpr, max tpr subject to 1 - fpr >= s0 and max 1 - fpr subject to tpr >= r0 from
    roc_curve(drop_intermediate=False), max F1 from precision_recall_curve, each within 1e-12, on tied and untied scores;
  * the rules: the floor at an exactly attained boundary, each tie-break order, columns without positives or negatives and N = 1,
    the empty point's F1, the hand formula of net benefit;
  * host-side: fit-then-apply reproduces the fitted point's counts (the report's host half around the restatement), compare's
    refusals, the CSV / JSON round trip, the new flags in the four tools, the entry point's refusals from the built library."""
import csv
import ctypes as C
import functools
import importlib.util
import itertools
import json
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


REF = _load("sm3_operating_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))  # philox, multiplicities, make_case
PAIRS = REF.PAIRS
ONE = 1 << 32


# ---- the restatement --------------------------------------------------------------------------------------------------------
def _sign(a, b):
    return (a > b) - (a < b)


def column_record(order, gs, ge, positive, m, sigmas, rhos, fixpos):
    """One record [P, Q, APN, youden (3), f1 (3), sens at spec (3 each), spec at sens (3 each), fixed (2 each)] of Python ints.
    order, gs, ge: the column's ranking; positive[n], m[n]: per case."""
    N = len(order)
    pm = [int(m[n]) if positive[n] else 0 for n in (int(v) for v in order)]
    nm = [0 if positive[n] else int(m[n]) for n in (int(v) for v in order)]
    Ppre, S = [0] + list(itertools.accumulate(pm)), [0] + list(itertools.accumulate(nm))
    P, Q = Ppre[N], S[N]
    starts = [j for j in range(N) if int(gs[j]) == j]
    points = [(P - Ppre[a], Q - S[a], a) for a in starts] + [(0, 0, N)]
    apn = 0
    for a in starts:
        dtp = Ppre[int(ge[a])] - Ppre[a]
        if dtp:
            tp, fp = P - Ppre[a], Q - S[a]
            den = tp + fp
            apn += dtp * ((tp * ONE + den // 2) // den)

    def by_f1(u, v):  # 2 TP / (TP + FP + P) by cross-multiplication, then pos
        l, r = u[0] * (v[0] + v[1] + P), v[0] * (u[0] + u[1] + P)
        return _sign(l, r) or _sign(u[2], v[2])

    # the other three orders are lexicographic: a tuple key is that total order
    rec = [P, Q, apn, *max(points, key=lambda p: (p[0] * Q - p[1] * P, p[2])), *max(points, key=functools.cmp_to_key(by_f1))]
    for sigma in sigmas:
        rec += max((p for p in points if (Q - p[1]) * ONE >= int(sigma) * Q), key=lambda p: (p[0], -p[1], p[2]))
    for rho in rhos:
        rec += max((p for p in points if p[0] * ONE >= int(rho) * P), key=lambda p: (-p[1], p[0], p[2]))
    for f in fixpos:
        rec += [P - Ppre[int(f)], Q - S[int(f)]]
    return rec


def records(order, gs, ge, y, m, sigmas, rhos, fixpos):
    """[24, R] int64 of the columns for the multiplicities m.  order, gs, ge [24, N], y [N, 8], fixpos [24, Lt]."""
    return np.array([column_record(order[k], gs[k], ge[k], y[:, t] == c, m, sigmas, rhos, fixpos[k])
                     for k, (t, c) in enumerate(PAIRS)], dtype=np.int64).reshape(len(PAIRS), -1)


def restated_inputs(preds, targets):
    order, gs, ge, y, _ = REF.restated_inputs(preds, targets)
    return order, gs, ge, y


def restatement_counts_fn(order, gs, ge, y, colmap, sigma, rho, fixpos, out, seed, r0, point=False):
    """Stands in for ops.operating_counts, on the tensors of any device."""
    N = y.shape[0]
    host = [a.cpu().numpy() for a in (order, gs, ge, y)]
    for j in range(out.shape[0]):
        m = np.ones(N, dtype=np.int64) if point else REF.multiplicities(seed, r0 + j, N)
        out[j] = torch.from_numpy(records(*host, m, sigma.tolist(), rho.tolist(), fixpos.cpu().numpy())).to(out.device)


def host_report(preds, targets, spec_floors=(0.8, 0.9, 0.95), sens_floors=(0.8, 0.9, 0.95), decision=(0.05, 0.1, 0.2, 0.3, 0.4, 0.5),
                thresholds=None, bootstrap=0, confidence=0.95, seed=0, chunk=None, dev="cpu"):
    """operating_report's host half around the restatement: what the library does with the kernel's integers (the ranking and
    the threshold search are torch's on `dev`)."""
    from sm3hip import operating
    s, r, d = operating.check_levels(spec_floors, sens_floors, decision)
    return operating._report(preds, targets, s, r, d, operating.check_thresholds(thresholds), bootstrap, confidence, seed, chunk,
                             torch.device(dev), restatement_counts_fn)


# ---- 1. against scikit-learn ------------------------------------------------------------------------------------------------
FLOORS = (0.8, 0.9, 0.95)


@pytest.mark.parametrize("N,kind,resample", [(600, "ties", False), (600, "ties", True), (600, "random", False),
                                             (600, "random", True), (257, "constant", True), (64, "absent", True)])
def test_restatement_against_sklearn(N, kind, resample):
    from sklearn.metrics import average_precision_score, precision_recall_curve, roc_curve
    from sm3hip import operating
    preds, targets = REF.make_case(N, kind, N + 3)
    order, gs, ge, y = restated_inputs(preds, targets)
    m = REF.multiplicities(2 ** 40 + 11, 2, N) if resample else np.ones(N, dtype=np.int64)
    sig = [operating.q32_floor(s) for s in FLOORS]
    cnt = records(order, gs, ge, y, m, sig, sig, np.zeros((24, 0), dtype=np.int64))
    values, undefined = operating.values_from_counts(cnt, 3, 3, 0, [], N)
    rows = operating.row_names(operating.point_names(FLOORS, FLOORS, []), [])
    row = {name: values[i, :24] for i, name in enumerate(rows)}
    keep = m > 0
    worst = {"AP": 0.0, "J": 0.0, "F1": 0.0, "sens@spec": 0.0, "spec@sens": 0.0}
    seen = 0
    for k, (t, c) in enumerate(PAIRS):
        P, Q = int(cnt[k, 0]), int(cnt[k, 1])
        assert P + Q == N
        if P == 0 or Q == 0:
            assert undefined[rows.index("youden J"), k] and row["youden J"][k] == 0.0
            continue
        seen += 1
        yb = (y[keep, t] == c).astype(int)
        score = torch.softmax(preds[t].double(), 1)[:, c].numpy()[keep]
        w = m[keep]
        worst["AP"] = max(worst["AP"], abs(row["AP"][k] - average_precision_score(yb, score, sample_weight=w)))
        fpr, tpr, _ = roc_curve(yb, score, sample_weight=w, drop_intermediate=False)
        worst["J"] = max(worst["J"], abs(row["youden J"][k] - np.max(tpr - fpr)))
        for s0 in FLOORS:
            worst["sens@spec"] = max(worst["sens@spec"], abs(row[f"spec>={s0!r} sens"][k] - tpr[1 - fpr >= s0].max()))
            worst["spec@sens"] = max(worst["spec@sens"], abs(row[f"sens>={s0!r} spec"][k] - (1 - fpr)[tpr >= s0].max()))
        prec, rec, _ = precision_recall_curve(yb, score, sample_weight=w)
        with np.errstate(divide="ignore", invalid="ignore"):
            f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        worst["F1"] = max(worst["F1"], abs(row["f1 F1"][k] - f1.max()))
    print(f"N = {N} {kind} resample = {resample}: {seen} columns, worst differences {worst}")
    assert seen >= 12
    assert worst["AP"] <= 2.0 ** -32
    for name in ("J", "F1", "sens@spec", "spec@sens"):
        assert worst[name] <= 1e-12, name


# ---- 2. the rules -----------------------------------------------------------------------------------------------------------
def _untied(n):
    return list(range(n)), list(range(n)), list(range(1, n + 1))


def test_floor_rule_accepts_an_exactly_attained_boundary():
    from sm3hip import operating
    sigma = operating.q32_floor(0.8)
    assert sigma * 100 <= 80 * ONE < round(0.8 * ONE) * 100                              # floor accepts 80 / 100, rint would not
    # ascending: 80 negatives, 5 positives, 20 negatives, 5 positives.  Position 80 has FP = 20 of Q = 100 and TP = 10
    positive = [False] * 80 + [True] * 5 + [False] * 20 + [True] * 5
    order, gs, ge = _untied(110)
    rec = column_record(order, gs, ge, positive, [1] * 110, [sigma], [], [])
    assert rec[:2] == [10, 100] and rec[9:12] == [10, 20, 80]
    assert column_record(order, gs, ge, positive, [1] * 110, [sigma + 1], [], [])[9:12] == [5, 0, 105]
    for s0, q in ((0.9, 10), (0.95, 20), (0.8, 5), (0.7, 10), (0.3, 10), (0.1, 10), (1.0, 3), (0.0, 7)):
        assert operating.q32_floor(s0) * q <= round(s0 * q) * ONE, s0                    # every attained decimal floor is accepted


def test_tie_break_orders():
    order, gs, ge = _untied(3)
    # cases in ascending score: a negative, a positive nobody drew, a positive: positions 1 and 2 have equal counts
    rec = column_record(order, gs, ge, [False, True, True], [1, 0, 1], [ONE], [ONE], [])
    assert rec[:3] == [1, 1, ONE]
    assert rec[3:6] == [1, 0, 2] and rec[6:9] == [1, 0, 2]                               # Youden, F1: equal value -> the larger pos
    assert rec[9:12] == [1, 0, 2] and rec[12:15] == [1, 0, 2]                            # both floors: equal (TP, FP) -> the larger pos
    # two negatives, then a positive: TP = 1 at positions 0, 1, 2 with FP = 2, 1, 0
    rec = column_record(order, gs, ge, [False, False, True], [1, 1, 1], [0], [0], [])
    assert rec[9:12] == [1, 0, 2]                                                        # (TP, -FP, pos): equal TP -> the smaller FP
    assert rec[12:15] == [1, 0, 2]                                                       # (-FP, TP, pos): FP = 0 at pos 2 and 3 -> the larger TP
    # a positive below a negative: the sens floor 1 leaves pos 0 alone, the spec floor 1 the positions 2 (empty point: N = 2)
    rec = column_record(*_untied(2), [True, False], [1, 1], [ONE], [ONE], [0, 1, 2])
    assert rec[9:12] == [0, 0, 2] and rec[12:15] == [1, 1, 0]
    assert rec[3:6] == [0, 0, 2]                                                         # J = 0 at pos 0 and 2, -1 at pos 1: the larger pos
    assert rec[6:9] == [1, 1, 0]                                                         # F1 = 2 / 3 at pos 0, 0 elsewhere
    assert rec[15:] == [1, 1, 0, 1, 0, 0]
    # a tie group is one point: both cases tied -> points 0 and N only
    rec = column_record([0, 1], [0, 0], [2, 2], [True, False], [1, 1], [], [], [])
    assert rec[:3] == [1, 1, ONE // 2] and rec[3:6] == [0, 0, 2]


def test_empty_point_wins_f1_without_a_drawn_positive_and_undefined_values_are_zero():
    from sm3hip import operating
    order, gs, ge = _untied(3)
    rec = column_record(order, gs, ge, [False, True, False], [2, 0, 1], [ONE // 2], [ONE // 2], [1])
    assert rec[:3] == [0, 3, 0] and rec[6:9] == [0, 0, 3]                                # P = 0: every F1 compares equal, pos = N wins
    for kind, N in (("absent", 9), ("ties", 1), ("equal", 2), ("random", 1)):
        preds, targets = REF.make_case(N, kind, 5)
        rep = host_report(preds, targets, bootstrap=3, seed=9)
        v, u = rep["values"].numpy(), rep["point_undefined"].numpy()
        assert np.isfinite(v).all() and not v[:, :24][u[:, :24]].any()                   # an undefined class value is 0
        cnt = rep["counts"].numpy()
        rows = rep["rows"]
        for k in range(24):
            P, Q = cnt[k, 0], cnt[k, 1]
            assert u[rows.index("AP"), k] == (P == 0) and u[rows.index("youden sens"), k] == (P == 0)
            assert u[rows.index("youden spec"), k] == (Q == 0) and u[rows.index("youden J"), k] == (P * Q == 0)
            assert not u[rows.index("NB pt=0.05"), k]
        if kind == "absent":
            assert u[rows.index("AP"), 24:].all()                                        # an average is undefined with any column
        assert rep["undefined"].shape == rep["values"].shape and np.isfinite(rep["replicates"].numpy()).all()


def test_net_benefit_is_the_hand_formula():
    preds, targets = REF.make_case(50, "random", 8)
    rep = host_report(preds, targets, decision=(0.05, 0.3, 0.5))
    cnt, rows, N = rep["counts"].numpy(), rep["rows"], 50
    for i, pt in enumerate((0.05, 0.3, 0.5)):
        for k, (t, c) in enumerate(PAIRS):
            score = torch.softmax(preds[t].double(), 1)[:, c].numpy()
            yb = targets[:, t].numpy() == c
            tp, fp = int((yb & (score >= pt)).sum()), int((~yb & (score >= pt)).sum())
            off = 9 + 9 + 9 + 2 * i
            assert (cnt[k, off], cnt[k, off + 1]) == (tp, fp)
            w = pt / (1 - pt)
            assert float(rep["values"][rows.index(f"NB pt={pt!r}"), k]) == (tp - fp * w) / N
            assert float(rep["values"][rows.index(f"NB_all pt={pt!r}"), k]) == (int(yb.sum()) - int((~yb).sum()) * w) / N
            assert float(rep["values"][rows.index(f"pt={pt!r} sens"), k]) == (tp / int(yb.sum()) if yb.any() else 0.0)
    assert float(rep["thresholds"][rep["points"].index("pt=0.3"), 7]) == 0.3


def test_curves_are_the_operating_points():
    from sklearn.metrics import roc_curve
    preds, targets = REF.make_case(120, "ties", 4)
    rep = host_report(preds, targets)
    for k, (t, c) in enumerate(PAIRS):
        cur = rep["curves"][k]
        score = torch.softmax(preds[t].double(), 1)[:, c].numpy()
        assert cur["thresholds"][-1] == float("inf") and np.array_equal(cur["thresholds"][:-1].numpy(), np.unique(score))
        assert int(cur["pos"][-1]) == 120 and cur["tpr"][-1] == 0 and cur["fpr"][-1] == 0 and cur["tpr"][0] == 1
        fpr, tpr, thr = roc_curve(targets[:, t].numpy() == c, score, drop_intermediate=False)
        assert np.allclose(cur["fpr"].numpy()[::-1], fpr, rtol=0, atol=1e-15)
        assert np.allclose(cur["tpr"].numpy()[::-1], tpr, rtol=0, atol=1e-15) and np.array_equal(cur["thresholds"].numpy()[::-1], thr)
        assert torch.equal(cur["recall"], cur["tpr"])


# ---- 3. host-side checks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["youden", "f1", "spec>=0.9", "sens>=0.85"])
def test_fitted_thresholds_reproduce_the_fitted_point(rule):
    from sm3hip import operating
    for kind in ("ties", "random", "absent"):
        preds, targets = REF.make_case(90, kind, 17)
        spec, sens, name = operating.rule_settings(rule)
        fit = host_report(preds, targets, spec_floors=spec, sens_floors=sens, decision=())
        i = fit["points"].index(name)
        thr = fit["thresholds"][i]
        off = operating.point_offsets(len(spec), len(sens), 0)[i]
        applied = host_report(preds, targets, thresholds=thr)
        assert applied["points"][-1] == "thr[0]" and not any(r.startswith("NB") for r in applied["rows"])
        assert torch.equal(applied["counts"][:, -2:], fit["counts"][:, off:off + 2])
        assert torch.equal(applied["thresholds"][-1], thr)
        empty = fit["counts"][:, off + 2] == 90
        assert bool((thr[empty] == float("inf")).all()) and bool((thr[~empty] <= 1).all())
        for m in operating.POINT_METRICS:                                                # and so the values
            assert torch.equal(applied["values"][applied["rows"].index(f"thr[0] {m}")], fit["values"][fit["rows"].index(f"{name} {m}")])


def test_bootstrap_through_the_host_half_does_not_depend_on_the_chunk():
    preds, targets = REF.make_case(40, "ties", 2)
    a = host_report(preds, targets, bootstrap=6, seed=2 ** 63 + 1)
    b = host_report(preds, targets, bootstrap=6, seed=2 ** 63 + 1, chunk=4)
    assert torch.equal(a["replicate_counts"], b["replicate_counts"]) and torch.equal(a["replicates"], b["replicates"])
    assert a["replicates"].shape == (6, len(a["rows"]), 29) and bool((a["lo"] <= a["hi"]).all())
    assert torch.equal(a["replicate_counts"][:, :, 0] + a["replicate_counts"][:, :, 1], torch.full((6, 24), 40))


def test_compare_pairs_the_replicates_and_refuses_unpaired_reports():
    from sm3hip import operating, report
    preds, targets = REF.make_case(30, "random", 6)
    other = [p.flip(0) for p in preds]
    a, b = host_report(preds, targets, bootstrap=5, seed=3), host_report(other, targets, bootstrap=5, seed=3)
    c = operating.compare(a, b)
    assert torch.equal(c["delta"], a["values"] - b["values"]) and c["rows"] == a["rows"]
    lo, hi = report.interval((a["replicates"] - b["replicates"]).numpy(), 0.95)
    assert np.array_equal(c["lo"].numpy(), lo) and np.array_equal(c["hi"].numpy(), hi)
    z = operating.compare(a, a)
    assert not z["delta"].any() and not z["lo"].any() and float(z["frac_le_zero"].min()) == 1.0
    with pytest.raises(ValueError, match="seed"):
        operating.compare(a, host_report(other, targets, bootstrap=5, seed=4))
    with pytest.raises(ValueError, match="bootstrap"):
        operating.compare(a, host_report(other, targets, bootstrap=4, seed=3))
    with pytest.raises(ValueError, match="rows"):
        operating.compare(a, host_report(other, targets, bootstrap=5, seed=3, spec_floors=(0.5,)))
    with pytest.raises(ValueError, match="targets"):
        operating.compare(a, host_report(other, (targets + 1) % 2, bootstrap=5, seed=3))
    assert "lo" not in operating.compare(host_report(preds, targets), host_report(other, targets))


def test_csv_and_json_parse_back_to_the_values(tmp_path):
    from sm3hip import operating
    preds, targets = REF.make_case(25, "ties", 12)
    for B in (0, 4):
        rep = host_report(preds, targets, bootstrap=B)
        operating.save(rep, str(tmp_path), f"r{B}")
        rows = list(csv.reader(open(tmp_path / f"r{B}.csv")))
        assert rows[0] == ["row", "column", "value"] + (["lo", "hi", "undefined"] if B else [])
        assert len(rows) == 1 + len(rep["rows"]) * 29
        for line, (i, k) in zip(rows[1:], itertools.product(range(len(rep["rows"])), range(29))):
            assert line[:2] == [rep["rows"][i], rep["columns"][k]] and float(line[2]) == float(rep["values"][i, k])
            if B:
                assert (float(line[3]), float(line[4]), int(line[5])) == (float(rep["lo"][i, k]), float(rep["hi"][i, k]),
                                                                           int(rep["undefined"][i, k]))
        back = json.load(open(tmp_path / f"r{B}.json"))
        assert back["values"] == rep["values"].tolist() and back["rows"] == rep["rows"] and back["counts"] == rep["counts"].tolist()
        assert "replicates" not in back and "targets" not in back and back["thresholds"] == rep["thresholds"].tolist()
        assert back["curves"][3]["thresholds"][-1] == float("inf") and back["curves"][3]["tpr"] == rep["curves"][3]["tpr"].tolist()
    assert "8 avg" in operating.format_table(rep) and "AP_AVG" in operating.stats_line(rep)
    assert "MAX_CASES" in operating.stats_line(None)


def test_settings_and_inputs_are_refused_before_any_device_work():
    from sm3hip import operating
    preds, targets = REF.make_case(5, "ties", 1)
    for kw in ({"bootstrap": -1}, {"confidence": 1.0}, {"seed": 2 ** 64}, {"bootstrap": 4, "chunk": 5}, {"spec_floors": [1.5]},
               {"spec_floors": [-0.1]}, {"sens_floors": [float("nan")]}, {"sens_floors": [True]}, {"decision": [0.0]},
               {"decision": [1.0]}, {"spec_floors": [0.5] * 33}, {"sens_floors": [0.5] * 33}, {"decision": [0.5] * 33},
               {"thresholds": np.zeros(23)}, {"thresholds": np.zeros((24, 33))}, {"thresholds": np.full(24, np.nan)}):
        with pytest.raises(ValueError):
            operating.operating_report(preds, targets, **kw)
    with pytest.raises(ValueError, match="NaN"):
        operating.operating_report([p.clone().fill_(float("nan")) if t == 2 else p for t, p in enumerate(preds)], targets)
    big_p, big_t = REF.make_case(operating.report.MAX_CASES + 1, "equal", 1)
    with pytest.raises(ValueError, match="MAX_CASES"):
        operating.operating_report(big_p, big_t)
    for rule in ("best", "spec>=", "spec>=2", "sens>=x", "spec>0.9", None):
        with pytest.raises(ValueError, match="rule"):
            operating.fit_thresholds(preds, targets, rule)
    assert operating.parse_rule("sens>=0.9") == ("sens", 0.9) and operating.parse_rule("f1") == ("f1", None)
    assert operating.MAX_LEVELS == 32


def _tool(name):
    return _load("sm3_operating_cli_" + name, os.path.join(TOOLS, name + ".py"))


@pytest.mark.parametrize("name", ["backbone_eval", "mlc_eval", "backbone_knn", "eval_report"])
def test_the_new_flags_parse(name):
    from sm3hip import operating
    base = ["x.pt"] if name == "eval_report" else ["--data-name", "synthetic", "--data-path", "-"]
    parser = _tool(name).get_parser()
    d = parser.parse_args(base)
    assert d.operating is False and d.operating_rule == "youden"
    assert (d.operating_spec, d.operating_sens) == ([0.8, 0.9, 0.95], [0.8, 0.9, 0.95])
    assert d.operating_decision == [0.05, 0.1, 0.2, 0.3, 0.4, 0.5]
    operating.check_flags(d)
    a = parser.parse_args(base + ["--operating", "--operating-spec", "0.5", "0.99", "--operating-sens", "--operating-decision", "0.25",
                                  "--operating-rule", "spec>=0.9"])
    assert a.operating and (a.operating_spec, a.operating_sens, a.operating_decision) == ([0.5, 0.99], [], [0.25])
    operating.check_flags(a)
    assert operating.flag_settings(a) == {"spec_floors": [0.5, 0.99], "sens_floors": [], "decision": [0.25]}
    for bad in (["--operating-spec", "1.5"], ["--operating-decision", "1"], ["--operating-rule", "auc"]):
        with pytest.raises(ValueError):
            operating.check_flags(parser.parse_args(base + bad))


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from sm3hip import _lib, operating, ops
    lib = _lib.load()
    assert lib.sm3_operating_max_levels() == operating.MAX_LEVELS == ops.OPERATING_MAX_LEVELS
    assert ops.operating_record(3, 2, 5) == 9 + 9 + 6 + 10
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced, every call below returns before a launch
    odd = C.c_void_p(p.value + 4)

    def call(order=p, gs=p, ge=p, y=p, colmap=p, sigma=p, rho=p, fixpos=p, out=p, N=5, T=8, K=24, Ls=1, Lr=1, Lt=1, seed=0, r0=0,
             c=1, point=0):
        return lib.sm3_operating_counts(order, gs, ge, y, colmap, sigma, rho, fixpos, out, N, T, K, Ls, Lr, Lt, seed, r0, c, point,
                                        None)
    for name in ("order", "gs", "ge", "y", "colmap", "sigma", "rho", "fixpos", "out"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(N=-3) == -1 and call(N=operating.report.MAX_CASES + 1) == -1
    assert call(c=0) == -1 and call(T=0) == -1 and call(T=65) == -1 and call(K=0) == -1 and call(K=65) == -1
    for name in ("Ls", "Lr", "Lt"):
        assert call(**{name: -1}) == -1 and call(**{name: 33}) == -1, name
    assert call(r0=-1) == -1 and call(r0=2 ** 32) == -1 and call(r0=2 ** 32 - 1, c=2) == -1
    assert call(point=1, c=2) == -1
    assert call(out=odd) == -2 and call(sigma=odd) == -2 and call(rho=odd) == -2
