"""CPU: the calibration report (sm3hip/calibration.py, csrc/calib.hip) restated in numpy and Python integers, and everything
about it that needs no GPU.  tests/test_calib_gpu.py loads this file for the restatement.

  * the restatement: bin tables of both binnings for integer multiplicities (the multiplicities are those of
    tests/test_report_cpu.py: one stream for both reports), plain sums, values by one division in Python numbers;
  * the fixed-point series of hand-computed cases;
  * values from counts against scikit-learn: log_loss, the multiclass Brier score as the sum of brier_score_loss over the
    classes (both also with sample_weight = resampled multiplicities) and calibration_curve(strategy="uniform") against the
    class-wise acc_b / conf_b.  Bound 2^-32 absolute, derived: every q is within 2^-33 of its fp64 value (rint of x * 2^32), so
    any weighted mean of them is too; the other half covers the fp64 roundings of either side's own arithmetic, a few 2^-53 of
    values below 1024;
  * the mass binning against a brute force that repeats each case m times, sorts the list and cuts it at u * M // N;
  * fit_temperature against scipy.optimize.minimize_scalar on the same fp64 NLL (relative 1e-6 on T, derived: 60 halvings of a
    width-12 interval in log2 beta leave 12 * 2^-60, and Brent's minimiser resolves a minimum to about sqrt(2^-52) = 1.5e-8
    relative), scaling of the logits, the clipped flag on separable data, permuted case order;
  * compare's refusals, the CSV / JSON round trip, the flags of the three tools, the header <-> ctypes entry of the symbol."""
import csv
import ctypes as C
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
PAIRS = [(t, c) for t, n in enumerate(NUM_CLASSES) for c in range(n)]
ONE = 1 << 32
BOUND = 2.0 ** -32


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REP = _load("sm3_calib_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))  # multiplicities, make_case
multiplicities, make_case = REP.multiplicities, REP.make_case


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _accumulate(b, evc, qc, M):
    """[M, 3] int64 (n_b, E_b, Q_b) of copies with bins b, events evc and scores qc: integer sums of the copies sorted by bin."""
    by_bin = np.argsort(b, kind="stable")
    edges = np.searchsorted(b[by_bin], np.arange(M + 1))
    out = np.zeros((M, 3), dtype=np.int64)
    out[:, 0] = np.diff(edges)
    for e, v in ((1, evc), (2, qc)):
        run = np.concatenate([[0], np.cumsum(v[by_bin], dtype=np.int64)])
        out[:, e] = run[edges[1:]] - run[edges[:-1]]
    return out


def bin_tables(q, ev, order, m, M, binning):
    """[S, M, 3] int64 (n_b, E_b, Q_b) of the series q, ev [S, N] with the order [S, N] for the multiplicities m [N]: every case
    becomes m copies; a copy's bin comes from its q (width) or from its rank among the copies in sorted order (mass)."""
    q, ev, order, m = (np.asarray(a, dtype=np.int64) for a in (q, ev, order, m))
    S, N = q.shape
    out = np.zeros((S, M, 3), dtype=np.int64)
    for s in range(S):
        if binning == "width":
            copies = np.repeat(np.arange(N), m)
            b = np.minimum((q[s, copies] * M) >> 32, M - 1)
        else:
            copies = np.repeat(order[s], m[order[s]])        # the cases of the copy ranks 0 .. N - 1, in rank order
            b = (np.arange(N, dtype=np.int64) * M) // N
        assert copies.shape[0] == N
        out[s] = _accumulate(b, ev[s, copies], q[s, copies], M)
    return out


def plain_sums(xq, m):
    return (np.asarray(xq, dtype=np.int64) * np.asarray(m, dtype=np.int64)[None, :]).sum(axis=1)


def brute_mass(q, ev, m, M):
    """One series, literally: every case m times in a list, sorted by (q, case index), cut at u * M // N."""
    copies = sorted((int(q[n]), n) for n in range(len(q)) for _ in range(int(m[n])))
    N = len(copies)
    out = [[0, 0, 0] for _ in range(M)]
    for u, (qv, n) in enumerate(copies):
        b = u * M // N
        out[b][0] += 1
        out[b][1] += int(ev[n])
        out[b][2] += qv
    return out


def values(bins, sums, N):
    """(label [4][9], class-wise ECE [24], diagram [32][M][3]) in Python numbers: each value ONE division of two integers."""
    ece, mce, diagram = [], [], []
    for s in range(len(bins)):
        gaps = [abs(int(Q) - int(E) * ONE) for _, E, Q in bins[s]]
        ece.append(float(sum(gaps)) / float(N * ONE))
        mce.append(max([float(g) / float(int(b[0]) * ONE) for g, b in zip(gaps, bins[s]) if int(b[0])] or [0.0]))
        diagram.append([[float(n), float(int(E)) / float(int(n)) if n else 0.0, float(int(Q)) / float(int(n) * ONE) if n else 0.0]
                        for n, E, Q in bins[s]])
    label = [[float(int(sums[t])) / float(N * ONE) for t in range(8)], [float(int(sums[8 + t])) / float(N * ONE) for t in range(8)],
             ece[:8], mce[:8]]
    for row in label:
        acc = 0.0
        for v in row[:8]:
            acc = acc + v
        row.append(acc / 8.0)
    return label, ece[8:], diagram


def series(preds, targets, temperature=None):
    """(q, ev, order, xq) as numpy int64 through the library's own plumbing on the tensors' device."""
    from sm3hip import calibration
    q, ev, xq = calibration.fixed_point(preds, targets, temperature)
    order = torch.sort(q, dim=1, stable=True).indices
    return tuple(a.cpu().numpy().astype(np.int64) for a in (q, ev, order, xq))


# ---- 1. the fixed-point series ----------------------------------------------------------------------------------------------
def test_fixed_point_series_of_hand_computed_cases():
    from sm3hip import calibration, report
    assert report.COLUMN_PAIRS == PAIRS and calibration.S == 32 and calibration.X == 16 and calibration.ONE == ONE
    assert calibration.SERIES_LABEL == list(range(8)) + [t for t, _ in PAIRS]
    preds, targets = make_case(4, "equal", 1)
    # label 2 (two classes): certain and right, certain and wrong, past the NLL clamp, undecided (argmax: lowest index)
    preds[2] = torch.tensor([[1000.0, 0.0], [1000.0, 0.0], [2000.0, 0.0], [0.0, 0.0]])
    targets[:, 2] = torch.tensor([0, 1, 1, 1])
    targets[:, 1] = torch.tensor([0, 1, 2, 0])                      # label 1 (three classes): all-equal logits, p = 1/3
    q, ev, order, xq = series(preds, targets)
    assert q.shape == (32, 4) and ev.shape == (32, 4) and xq.shape == (16, 4)
    assert q[2].tolist() == [ONE, ONE, ONE, ONE // 2] and ev[2].tolist() == [1, 0, 0, 0]     # top label, yhat = 0 throughout
    k0, k1 = 8 + PAIRS.index((2, 0)), 8 + PAIRS.index((2, 1))
    assert q[k0].tolist() == [ONE, ONE, ONE, ONE // 2] and ev[k0].tolist() == [1, 0, 0, 0]
    assert q[k1].tolist() == [0, 0, 0, ONE // 2] and ev[k1].tolist() == [0, 1, 1, 1]
    assert xq[2].tolist()[:3] == [0, 1000 * ONE, 1024 * ONE]                                 # -lp, clamped at 1024
    assert abs(xq[2][3] - math.log(2.0) * ONE) <= 1.0
    assert xq[8 + 2].tolist() == [0, 2 * ONE, 2 * ONE, ONE // 2]                             # Brier: 0, 1 + 1, 1 + 1, 1/4 + 1/4
    third = 1431655765                                                                       # rint(2^32 / 3) = floor: .33
    assert q[1].tolist() == [third] * 4 and ev[1].tolist() == [1, 0, 0, 1]                   # yhat = 0: right where y = 0
    assert abs(xq[8 + 1][0] - (6.0 / 9.0) * ONE) <= 1.0                                      # (2/3)^2 + 2 (1/3)^2
    # bins: 2^32 lands in bin M - 1, 2^31 in bin M // 2 (upper of an inner edge when M is even), 0 in bin 0
    one = np.ones(4, dtype=np.int64)
    for M in (1, 2, 15, 64):
        tab = bin_tables(q, ev, order, one, M, "width")
        assert tab[2, M - 1].tolist()[:2] == ([4, 1] if M <= 2 else [3, 1]) and tab[2, M // 2, 0] >= 1
        assert tab[k1, 0, 0] == (4 if M == 1 else 3) and tab[:, :, 0].sum(axis=1).tolist() == [4] * 32
        assert tab[1, min((third * M) >> 32, M - 1)].tolist() == [4, 2, 4 * third]
    # temperature: a division of the logits; T = 1000 turns the certain rows into 1 / (1 + 1/e)
    qT = series(preds, targets, [1.0, 1.0, 1000.0] + [1.0] * 5)[0]
    assert abs(qT[2][0] - ONE / (1.0 + math.exp(-1.0))) <= 1.0 and np.array_equal(qT[1], q[1])
    assert np.array_equal(order[2], [3, 0, 1, 2])                                            # ties by ascending case index
    with pytest.raises(ValueError):
        calibration.fixed_point(preds, targets, [1.0] * 7 + [0.0])


# ---- 2. values against scikit-learn ---------------------------------------------------------------------------------------
N_SK, M_SK = 395, 15


@pytest.fixture(scope="module")
def sk_case():
    preds, targets = make_case(N_SK, "random", 12)
    preds = [2.0 * p for p in preds]                                 # sharper than N(0, 1): the upper bins are populated
    return preds, targets, series(preds, targets)


def test_the_fixture_stays_off_the_bin_edges(sk_case):
    """sklearn puts a value on an inner edge into the lower bin, the definition into the upper one: the comparison below
    needs every probability at least 1e-6 away from every k / M, and every case is compared."""
    preds, _, _ = sk_case
    for p in preds:
        s = torch.softmax(p.double(), 1).numpy()
        for k in range(M_SK + 1):
            assert np.abs(s - k / M_SK).min() >= 1e-6


@pytest.mark.parametrize("resample", [False, True])
def test_values_from_counts_against_sklearn(sk_case, resample):
    from sklearn.calibration import calibration_curve
    from sklearn.metrics import brier_score_loss, log_loss
    from sm3hip import calibration
    preds, targets, (q, ev, order, xq) = sk_case
    N = N_SK
    m = multiplicities(11, 2, N) if resample else np.ones(N, dtype=np.int64)
    bins = bin_tables(q, ev, order, m, M_SK, "width")
    v = calibration.values_from_counts(bins, plain_sums(xq, m), N)
    y = targets.numpy()
    worst = {"nll": 0.0, "brier": 0.0, "acc": 0.0, "conf": 0.0}
    for t, n in enumerate(NUM_CLASSES):
        p = torch.softmax(preds[t].double(), 1).numpy()
        worst["nll"] = max(worst["nll"], abs(v["label_values"][0, t] - log_loss(y[:, t], p, labels=list(range(n)), sample_weight=m)))
        brier = 0.0
        for c in range(n):
            brier += brier_score_loss((y[:, t] == c).astype(int), p[:, c], sample_weight=m, pos_label=1)
        worst["brier"] = max(worst["brier"], abs(v["label_values"][1, t] - brier))
        if not resample:                                             # calibration_curve takes no weights
            for c in range(n):
                s = 8 + PAIRS.index((t, c))
                acc, conf = calibration_curve((y[:, t] == c).astype(int), p[:, c], n_bins=M_SK, strategy="uniform", pos_label=1)
                full = bins[s, :, 0] > 0
                assert acc.shape[0] == int(full.sum())
                assert np.array_equal(v["diagram"][s, :, 0], bins[s, :, 0].astype(np.float64))
                worst["acc"] = max(worst["acc"], np.abs(v["diagram"][s, full, 1] - acc).max())
                worst["conf"] = max(worst["conf"], np.abs(v["diagram"][s, full, 2] - conf).max())
                assert not v["diagram"][s, ~full, 1:].any() and v["diagram_undefined"][s, ~full, 1:].all()
                assert not v["diagram_undefined"][s, full].any() and not v["diagram_undefined"][s, :, 0].any()
    print(f"resample {resample}: worst differences {worst}, bound {BOUND:.3g}")
    for name, w in worst.items():
        assert w <= BOUND, name


@pytest.mark.parametrize("binning", ["width", "mass"])
def test_library_values_equal_the_python_restatement(sk_case, binning):
    """values_from_counts == the one-division-per-value restatement, and ECE / MCE are what their definition says of acc / conf."""
    from sm3hip import calibration, report
    _, _, (q, ev, order, xq) = sk_case
    for m in (np.ones(N_SK, dtype=np.int64), multiplicities(2 ** 63 + 11, 7, N_SK)):
        for M in (1, 15, 64):
            bins, sums = bin_tables(q, ev, order, m, M, binning), plain_sums(xq, m)
            assert bins[:, :, 0].sum(axis=1).tolist() == [N_SK] * 32
            v = calibration.values_from_counts(bins, sums, N_SK)
            label, cw, diagram = values(bins.tolist(), sums.tolist(), N_SK)
            assert v["label_values"].tolist() == label and v["class_values"][0, :24].tolist() == cw
            assert v["class_values"][0, 24:].tolist() == report.averages(np.array(cw)).tolist()
            assert v["diagram"].tolist() == diagram
            n, acc, conf = (v["diagram"][..., e] for e in range(3))
            ece = (n / N_SK * np.abs(acc - conf)).sum(axis=1)         # the textbook form, in floating point
            assert np.abs(ece[:8] - v["label_values"][2, :8]).max() <= 1e-12
            assert np.abs(np.abs(acc - conf).max(axis=1)[:8] - v["label_values"][3, :8]).max() <= 1e-12
            if binning == "mass" and M == 15:                        # equal mass: bin sizes differ by one at the most
                assert n.max() - n.min() <= 1.0
    stacked = calibration.values_from_counts(np.stack([bins, bins]), np.stack([sums, sums]), N_SK)   # leading replicate axis
    assert stacked["label_values"].shape == (2, 4, 9) and stacked["label_values"][1].tolist() == label


# ---- 3. the mass binning against brute force ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 5, 64, 65, 257])
def test_mass_binning_against_brute_force(N):
    for kind in ("ties", "equal", "random"):
        preds, targets = make_case(N, kind, 3 * N)
        q, ev, order, _ = series(preds, targets)
        for m in (np.ones(N, dtype=np.int64), multiplicities(5, 1, N), multiplicities(2 ** 40 + 1, 2 ** 20, N)):
            for M in (1, 2, 15, 64):
                tab = bin_tables(q, ev, order, m, M, "mass")
                for s in (0, 3, 8, 20, 31):
                    assert tab[s].tolist() == brute_mass(q[s], ev[s], m, M), (kind, M, s)
                sizes = [-(-(b + 1) * N // M) - -(-b * N // M) for b in range(M)]   # bin b: ranks [ceil(b N / M), ceil((b + 1) N / M))
                assert tab[0, :, 0].tolist() == sizes


# ---- 4. fit_temperature -------------------------------------------------------------------------------------------------
def _sampled_case(N, seed, scale=1.0):
    """Logits z ~ N(0, 1.5^2) and targets drawn from softmax(z): data calibrated at T = 1; the logits are then multiplied."""
    g = torch.Generator().manual_seed(seed)
    preds, cols = [], []
    for n in NUM_CLASSES:
        z = 1.5 * torch.randn(N, n, generator=g, dtype=torch.float64)
        cols.append(torch.multinomial(torch.softmax(z, 1), 1, generator=g)[:, 0])
        preds.append(z * scale)
    return preds, torch.stack(cols, dim=1)


def _nll(z, y, beta):
    a = z * beta
    a = a - a.max(axis=1, keepdims=True)
    return math.fsum((np.log(np.exp(a).sum(axis=1)) - a[np.arange(len(y)), y]).tolist())


def test_fit_temperature_against_scipy_and_under_scaling():
    from scipy.optimize import minimize_scalar
    from sm3hip import calibration
    preds, targets = _sampled_case(2000, 5)
    fit = calibration.fit_temperature(preds, targets)
    assert not any(fit["clipped"]) and len(fit["temperature"]) == 8
    for t in range(8):
        z, y = preds[t].numpy(), targets[:, t].numpy()
        res = minimize_scalar(lambda x: _nll(z, y, 2.0 ** x), bounds=(-6.0, 6.0), method="bounded", options={"xatol": 1e-12})
        want = 2.0 ** -res.x
        print(f"label {t}: T {fit['temperature'][t]!r} scipy {want!r}")
        assert abs(fit["temperature"][t] - want) <= 1e-6 * want
        assert fit["temperature"][t] * fit["beta"][t] == pytest.approx(1.0, abs=1e-15)
        # calibrated at T = 1: the maximum-likelihood beta has standard error 1 / sqrt(Fisher information), and the information
        # at beta = 1 is the sum over the cases of Var_p(z); six standard errors
        p = torch.softmax(preds[t], 1).numpy()
        info = float(((p * z * z).sum(axis=1) - (p * z).sum(axis=1) ** 2).sum())
        assert abs(fit["beta"][t] - 1.0) < 6.0 / math.sqrt(info)
    for factor in (4.0, 0.25):                                       # powers of two: the products z * beta are the same numbers
        scaled = calibration.fit_temperature([p * factor for p in preds], targets)
        for t in range(8):
            assert abs(scaled["temperature"][t] - factor * fit["temperature"][t]) <= 1e-6 * factor * fit["temperature"][t]
    perm = torch.randperm(2000, generator=torch.Generator().manual_seed(1))
    again = calibration.fit_temperature([p[perm] for p in preds], targets[perm])
    assert again == fit                                              # fsum: the case order does not show
    f32 = calibration.fit_temperature([p.float() for p in preds], targets)
    assert all(abs(a - b) <= 1e-4 * b for a, b in zip(f32["temperature"], fit["temperature"]))


def test_fit_temperature_flags_a_clipped_fit():
    from sm3hip import calibration
    preds, targets = make_case(50, "random", 2)
    sep = [p.clone() for p in preds]
    for t in range(8):
        sep[t][torch.arange(50), targets[:, t]] += 10.0               # separable: the NLL falls with beta without end
    fit = calibration.fit_temperature(sep, targets)
    assert fit["clipped"] == [True] * 8 and fit["temperature"] == [2.0 ** -6] * 8 and fit["beta"] == [64.0] * 8
    wrong = [-p for p in sep]                                         # always wrong: the NLL grows with beta throughout
    fit = calibration.fit_temperature(wrong, targets)
    assert fit["clipped"] == [True] * 8 and fit["temperature"] == [64.0] * 8
    with pytest.raises(ValueError, match="NaN"):
        calibration.fit_temperature([p.clone().fill_(float("nan")) for p in preds], targets)


# ---- 5. library and tool surface ------------------------------------------------------------------------------------------
def _fake(calibration, seed=3, B=5, shift=0.0, M=15, binning="width"):
    rng = np.random.default_rng(1)
    shapes = {"label": (4, 9), "class": (1, 29), "diagram": (32, M, 3)}
    rep = {"label_values": torch.from_numpy(rng.random(shapes["label"]) + shift),
           "class_values": torch.from_numpy(rng.random(shapes["class"]) + shift), "diagram": torch.from_numpy(rng.random(shapes["diagram"])),
           "bins": torch.zeros(32, M, 3, dtype=torch.int64), "sums": torch.zeros(16, dtype=torch.int64),
           "label_metrics": list(calibration.LABEL_METRICS), "label_columns": list(calibration.LABEL_COLUMNS),
           "class_metrics": list(calibration.CLASS_METRICS), "class_columns": list(calibration.CLASS_COLUMNS),
           "series": list(calibration.SERIES), "temperature": [1.0] * 8, "n_bins": M, "binning": binning,
           "targets": torch.zeros(6, 8, dtype=torch.int64), "n": 6}
    if B:
        from sm3hip import report
        for name, shape in shapes.items():
            r = rng.random((B,) + shape) + shift
            lo, hi = report.interval(r, 0.95)
            rep.update({f"{name}_replicates": torch.from_numpy(r), f"{name}_lo": torch.from_numpy(lo.copy()),
                        f"{name}_hi": torch.from_numpy(hi.copy()), f"{name}_undefined": torch.zeros(shape, dtype=torch.int64)})
        rep.update({"bootstrap": B, "seed": seed, "confidence": 0.95})
    return rep


def test_compare_pairs_the_replicates_and_refuses_unpaired_reports():
    from sm3hip import calibration, report
    a, b = _fake(calibration, shift=1.0), _fake(calibration)
    c = calibration.compare(a, b)
    for name in ("label", "class"):
        assert torch.equal(c[f"{name}_delta"], a[f"{name}_values"] - b[f"{name}_values"])
        d = (a[f"{name}_replicates"] - b[f"{name}_replicates"]).numpy()
        lo, hi = report.interval(d, 0.95)
        assert np.array_equal(c[f"{name}_lo"].numpy(), lo) and np.array_equal(c[f"{name}_hi"].numpy(), hi)
        assert np.array_equal(c[f"{name}_frac_le_zero"].numpy(), (d <= 0).mean(axis=0))
    z = calibration.compare(a, a)
    assert not z["label_delta"].any() and not z["class_lo"].any() and float(z["label_frac_le_zero"].min()) == 1.0
    for word, other in (("seed", _fake(calibration, seed=4)), ("bootstrap", _fake(calibration, B=0)), ("bins", _fake(calibration, M=10)),
                        ("binning", _fake(calibration, binning="mass"))):
        with pytest.raises(ValueError, match=word):
            calibration.compare(a, other)
    other = _fake(calibration)
    other["confidence"] = 0.9
    with pytest.raises(ValueError, match="confidence"):
        calibration.compare(a, other)
    other = _fake(calibration)
    other["targets"] = other["targets"] + 1
    with pytest.raises(ValueError, match="targets"):
        calibration.compare(a, other)
    with pytest.raises(ValueError):
        calibration.compare(a, {"values": 1})
    assert "label_lo" not in calibration.compare(_fake(calibration, B=0), _fake(calibration, B=0))


def test_csv_and_json_parse_back_to_the_values(tmp_path):
    from sm3hip import calibration
    for B in (0, 5):
        rep = _fake(calibration, B=B, M=4)
        calibration.save(rep, str(tmp_path), f"c{B}")
        rows = list(csv.reader(open(tmp_path / f"c{B}.csv")))
        assert rows[0] == ["table", "row", "column", "value"] + (["lo", "hi", "undefined"] if B else [])
        assert len(rows) == 1 + 4 * 9 + 29 + 3 * 32 * 4
        for r in rows[1:]:
            if r[0] in ("label", "class"):
                i = rep[f"{r[0]}_metrics"].index(r[1])
                k = rep[f"{r[0]}_columns"].index(r[2])
                assert float(r[3]) == float(rep[f"{r[0]}_values"][i, k])             # repr: exactly
                if B:
                    assert float(r[4]) == float(rep[f"{r[0]}_lo"][i, k]) and float(r[5]) == float(rep[f"{r[0]}_hi"][i, k])
            else:
                e = ("n", "acc", "conf").index(r[0].split(" ")[1])
                assert float(r[3]) == float(rep["diagram"][rep["series"].index(r[1]), int(r[2]), e])
        back = json.load(open(tmp_path / f"c{B}.json"))
        assert back["label_values"] == rep["label_values"].tolist() and back["diagram"] == rep["diagram"].tolist()
        assert back["n_bins"] == 4 and back["binning"] == "width" and "targets" not in back
        assert not any(k.endswith("_replicates") for k in back) and ("label_lo" in back) == bool(B)
        text = calibration.format_table(rep)
        assert "NLL" in text and "cwECE" in text and "8 avg" in text and ("[" in text) == bool(B)
    assert "no calibration report" in calibration.stats_line(None) and "ECE_AVG" in calibration.stats_line(rep)


def test_settings_and_inputs_are_refused_before_any_device_work():
    from sm3hip import calibration, report
    preds, targets = make_case(5, "ties", 1)
    for kw in ({"bins": 0}, {"bins": 65}, {"bins": 1.5}, {"bins": True}, {"binning": "quantile"}, {"bootstrap": -1},
               {"confidence": 1.0}, {"seed": 2 ** 64}, {"bootstrap": 4, "chunk": 5}, {"temperature": [1.0] * 7},
               {"temperature": [1.0] * 7 + [0.0]}, {"temperature": [1.0] * 7 + [float("inf")]}, {"temperature": [1.0] * 7 + [-2.0]}):
        with pytest.raises(ValueError):
            calibration.calibration_report(preds, targets, **kw)
    with pytest.raises(ValueError, match="NaN"):
        calibration.calibration_report([p.clone().fill_(float("nan")) if t == 2 else p for t, p in enumerate(preds)], targets)
    big_p, big_t = make_case(report.MAX_CASES + 1, "equal", 1)
    with pytest.raises(ValueError, match=f"MAX_CASES = {report.MAX_CASES}"):
        calibration.calibration_report(big_p, big_t)
    assert calibration.MAX_BINS == 64 and calibration.DEFAULT_BINS == 15 and calibration.BINNINGS == ("width", "mass")


@pytest.mark.parametrize("name", ["backbone_eval", "mlc_eval", "eval_report"])
def test_the_new_flags_parse_and_are_validated(name):
    from sm3hip import calibration
    tool = _load("sm3_calib_cli_" + name, os.path.join(TOOLS, name + ".py"))
    base = ["x.pt"] if name == "eval_report" else ["--data-name", "synthetic", "--data-path", "-"]
    parser = tool.get_parser()
    d = parser.parse_args(base)
    assert (d.calibration, d.calib_bins, d.calib_binning) == (False, 15, "width")
    a = parser.parse_args(base + ["--calibration", "--calib-bins", "64", "--calib-binning", "mass", "--bootstrap", "20"])
    assert (a.calibration, a.calib_bins, a.calib_binning, a.bootstrap) == (True, 64, "mass", 20)
    calibration.check_flags(a)
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--calib-binning", "quantile"])
    for bad in ("0", "65", "-1"):
        with pytest.raises(ValueError, match="bins"):
            calibration.check_flags(parser.parse_args(base + ["--calib-bins", bad]))
        with pytest.raises(ValueError, match="bins"):                # the tool refuses before it loads anything
            tool.main(base + ["--calib-bins", bad])
    if name == "eval_report":
        assert d.fit_on is None and parser.parse_args(["x.pt", "--fit-on", "y.pt"]).fit_on == "y.pt"
    else:
        assert not hasattr(d, "fit_on")
    knn = _load("sm3_calib_cli_knn", os.path.join(TOOLS, "backbone_knn.py")).get_parser()
    assert not hasattr(knn.parse_args(["--data-name", "synthetic", "--data-path", "-"]), "calibration")   # votes are not logits


def test_header_binding_and_entry_point_agree():
    from sm3hip import _lib, ops, report
    text = open(os.path.join(ROOT, "include", "sm3_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+sm3_calib_counts\s*\(([^)]*)\)", text)
    assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES["sm3_calib_counts"]) == 18
    assert "calib.hip" in open(os.path.join(ROOT, "skin-sm3_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    assert lib.sm3_abi_version() == 9 and hasattr(lib, "sm3_calib_counts") and ops.CALIB_MAX_BINS == 64
    buf = (C.c_int64 * (64 * 64 * 3))()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced, every call below returns before a launch

    def call(q=p, ev=p, order=p, slabel=p, xq=p, bins=p, sums=p, N=5, S=32, X=16, T=8, M=15, binning=0, seed=0, r0=0, c=1, point=0):
        return lib.sm3_calib_counts(q, ev, order, slabel, xq, bins, sums, N, S, X, T, M, binning, seed, r0, c, point, None)
    for name in ("q", "ev", "order", "slabel", "xq", "bins", "sums"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(N=-3) == -1 and call(N=report.MAX_CASES + 1) == -1
    assert call(M=0) == -1 and call(M=65) == -1 and call(c=0) == -1 and call(c=-1) == -1
    assert call(S=0) == -1 and call(S=65) == -1 and call(X=0) == -1 and call(X=65) == -1 and call(T=0) == -1 and call(T=65) == -1
    assert call(binning=2) == -1 and call(binning=-1) == -1
    assert call(r0=-1) == -1 and call(r0=2 ** 32) == -1 and call(r0=2 ** 32 - 1, c=2) == -1 and call(point=1, c=2) == -1
