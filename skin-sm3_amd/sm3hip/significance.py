"""Significance tests of a paired comparison: two sets of predictions a, b of the SAME cases (linear probe against fine-tune, two
checkpoints, kNN against logreg).  Beside report.compare's paired bootstrap interval this gives the three tests a reader of a
medical-imaging table asks for: DeLong's test for two correlated AUCs, an exact-arithmetic paired randomisation (permutation) test
for everything without a closed form -- Recall / Spec / Prec and the five averages, and AUC too -- and McNemar's test for the argmax
decisions; Holm-adjusted p-values beside the raw ones.

Inputs: a, b as report.check_inputs accepts them (8 float tensors [N, n_t], NaN refused), targets [N, 8] int64, N <=
report.MAX_CASES.  Columns k = 0 .. 23 are report.COLUMN_PAIRS; the score of a column is the fp64 softmax column, exactly as
report.ranking forms it.

JOINT RANKING (torch plumbing, once per column): the 2N scores of column k, element e = 2 * i + w (w = 0: a's score of case i,
w = 1: b's), sorted ascending and stably; tie groups by ==; gs / ge as report.rank_scores gives them.

SWAP BITS: replicate r swaps case i iff bit i & 31 of word i >> 5 of resample.philox_words(ceil(N / 32), seed, r, 5) is set (on the
device: Philox4x32-10, key = the seed, counter (i >> 7, r, 0, 5), word (i >> 5) & 3; stream 5).  The point record swaps nothing.
A' takes element w == swap_i of every case and B' the other; yhat is swapped the same way.  ONE swap vector serves all 24 columns
and all metrics of a replicate, so the averages' tests are joint.  A replicate is a function of (seed, r, N) alone.

COUNTS per replicate, column and side (A', B'), all int64, from sm3_signif_counts (csrc/signif.hip):
    A2 = sum over the side's positive elements j of (S[gs[j]] + S[ge[j]]),  S[j] = the side's negative elements at joint
    positions < j;  TP, FP of the side's yhat.  P, Q and FN = P - TP do not depend on the swap (host).
The point record's (A2, P, Q, TP, FP, FN) per side equals evaluation_report(a)["counts"] and evaluation_report(b)["counts"]: a
subset's A2 from the joint tie groups is the A2 of its own ranking.

PERMUTATION TEST: values by report.values_from_counts (the same single divisions, the same rule for averages and `undefined`);
T = value(A') - value(B') per metric for all 29 columns; p = (1 + #{r : |T_r| >= |T_point|}) / (B + 1), compared in fp64,
two-sided.  undefined[metric, column] = the replicates in which either side's value was undefined.

DELONG (the 24 class columns only: the five averages mix different positive sets, so they get the permutation test alone).
Placements times two, integers in case order, per model and column, from the model's OWN report.ranking
(sm3_signif_placements): positive i: u_i = 2 * (negatives below) + tied negatives in [0, 2Q]; negative j: v_j = 2 * (positives
above) + tied positives in [0, 2P].  With d = u^a - u^b, e = v^a - v^b:
    theta_x = sum(u^x) / (2 P Q)                     (the report's AUC, same bits)
    Var(theta_a - theta_b) = [P sum(d^2) - (sum d)^2] / (4 Q^2 P^2 (P - 1)) + [Q sum(e^2) - (sum e)^2] / (4 P^2 Q^2 (Q - 1))
    Var(theta_x): the same form with u^x, v^x in place of d, e.
The sums are int64; each variance is ONE exact rational (fractions.Fraction: 4 Q^2 P^2 (P - 1) reaches 4.6e18 at the size limit)
rounded once; z = float(theta_a - theta_b, exact) / sqrt(var); p = erfc(|z| / sqrt(2)); the intervals of each AUC and of the
difference are value -+ statistics.NormalDist().inv_cdf((1 + confidence) / 2) * sqrt(var), not clipped to [0, 1].
P < 2, Q < 2 or var == 0 gives z = 0, p = 1, flagged `undefined`.

MCNEMAR per label (8): n10 = a right and b wrong by argmax (the lowest index of the row maximum), n01 the reverse; n = n10 + n01;
exact two-sided binomial p = min(1, 2 * sum_{k <= min(n10, n01)} C(n, k) / 2^n) in Python integers, rounded once; n = 0: p = 1.

HOLM: per metric over the 24 class columns and over the 8 report.SELECTED columns (McNemar: over its 8 labels): the p-values sorted
ascending, ties by column index; adjusted_(i) = max over j <= i of min(1, (m - j) * p_(j)), j = 0 .. m - 1.  Host arithmetic.

The kernels give integers only, the host rounds once per value, and every chunk gives the same bits.  Outputs on the CPU; the
inputs are not modified."""
import math
import statistics
from fractions import Fraction

import numpy as np
import torch

from . import ops, report, resample
from .metrics import CLASSES_NAME
from .report import CLASS_COLUMNS, COLUMN_PAIRS, COLUMNS, K, MAX_CASES, METRICS, SELECTED  # noqa: F401  (this module's names too)

STREAM = 5                 # the last counter word of the swap words (resample.philox_words lists the streams)
DEFAULT_CHUNK = 4096       # replicates per launch: a choice (4096 x 24 x 2 x 3 int64 = 4.5 MiB of counts)
DEFAULT_PERMUTATIONS = 10000
MAX_PERMUTATIONS = resample.MAX_BOOTSTRAP


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def check_same_cases(targets, targets_b, who):
    """a's and b's targets must be the same cases."""
    if targets_b is not None and (not isinstance(targets, torch.Tensor) or not isinstance(targets_b, torch.Tensor)
                                  or tuple(targets.shape) != tuple(targets_b.shape)
                                  or not bool(torch.equal(targets.cpu(), targets_b.cpu()))):
        raise ValueError(f"{who}: the two sets of predictions must be of the same cases (equal targets)")


def check_permutation_settings(permutations, seed, chunk, who="permutation_test"):
    """The refusals that need neither a tensor nor a device."""
    if not resample.is_int(permutations) or not 1 <= permutations <= MAX_PERMUTATIONS:
        raise ValueError(f"{who}: permutations must be an integer in [1, 2^24], got {permutations!r}")
    if not resample.is_int(seed) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64), got {seed!r}")
    if chunk is not None and (not resample.is_int(chunk) or not 1 <= chunk <= permutations):
        raise ValueError(f"{who}: chunk must be None or an integer in [1, {permutations}], got {chunk!r}")


def check_confidence(confidence, who="delong"):
    if isinstance(confidence, bool) or not isinstance(confidence, (int, float)) or not 0 < confidence < 1:
        raise ValueError(f"{who}: confidence must be a number with 0 < confidence < 1, got {confidence!r}")


def _check_pair(a, b, targets, targets_b, who):
    """Unequal targets, then a's and b's shapes, the size limit and NaN (report.check_inputs); returns N."""
    check_same_cases(targets, targets_b, who)
    N = report.check_inputs(a, targets, who)
    report.check_inputs(b, targets, who)
    return N


# ---- host arithmetic --------------------------------------------------------------------------------------------------------
def swap_bits(seed, r, N):
    """[N] bool: the cases that replicate r swaps."""
    w = resample.philox_words((N + 31) // 32, seed, r, STREAM)
    i = np.arange(N, dtype=np.uint64)
    return ((w[i >> np.uint64(5)] >> (i & np.uint64(31))) & np.uint64(1)).astype(bool)


def holm(p):
    """Holm's step-down adjustment of the p-values p [m] (fp64): sorted ascending, ties by index; adjusted_(i) = the running
    maximum of min(1, (m - i) * p_(i))."""
    p = np.asarray(p, dtype=np.float64)
    m = p.shape[0]
    idx = np.argsort(p, kind="stable")
    out = np.empty(m, dtype=np.float64)
    run = 0.0
    for i, k in enumerate(idx):
        run = max(run, min(1.0, float(m - i) * float(p[k])))
        out[k] = run
    return out


def mcnemar_p(n10, n01):
    """The exact two-sided binomial p of n10 against n01 discordant pairs: ONE rounding of an exact rational."""
    n, lo = n10 + n01, min(n10, n01)
    if n == 0:
        return 1.0
    tail, term = 0, 1  # term = C(n, k)
    for k in range(lo + 1):
        tail += term
        term = term * (n - k) // (k + 1)
    return float(min(Fraction(1), Fraction(2 * tail, 2 ** n)))


def delong_variance(x, y, P, Q):
    """The exact variance (a Fraction, or None when P < 2 or Q < 2) from the doubled placements x [P] of the positives and y [Q]
    of the negatives (of one model, or the differences of two): [P sum x^2 - (sum x)^2] / (4 Q^2 P^2 (P - 1)) + [Q sum y^2 -
    (sum y)^2] / (4 P^2 Q^2 (Q - 1)).  The sums are int64, the rest Python integers."""
    if P < 2 or Q < 2:
        return None
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    sx, sxx, sy, syy = int(x.sum()), int((x * x).sum()), int(y.sum()), int((y * y).sum())
    return Fraction(P * sxx - sx * sx, 4 * Q * Q * P * P * (P - 1)) + Fraction(Q * syy - sy * sy, 4 * P * P * Q * Q * (Q - 1))


def delong_column(ua, ub, va, vb, confidence=0.95):
    """DeLong's test of one column from the doubled placements of its P positives (ua, ub) and Q negatives (va, vb), int64.
    Returns a dict of floats and `undefined`."""
    ua, ub, va, vb = (np.asarray(x, dtype=np.int64) for x in (ua, ub, va, vb))
    P, Q = int(ua.shape[0]), int(va.shape[0])
    sa, sb = int(ua.sum()), int(ub.sum())
    zc = statistics.NormalDist().inv_cdf((1.0 + float(confidence)) / 2.0)
    theta_a, theta_b = (float(resample.safe_div(s, 2 * P * Q)[0]) for s in (sa, sb))
    delta = float(Fraction(sa - sb, 2 * P * Q)) if P * Q else 0.0
    var = delong_variance(ua - ub, va - vb, P, Q)
    var_a, var_b = (delong_variance(u, v, P, Q) for u, v in ((ua, va), (ub, vb)))
    fa, fb, fv = (0.0 if v is None else float(v) for v in (var_a, var_b, var))
    undefined = var is None or var == 0
    z = 0.0 if undefined else delta / math.sqrt(fv)
    p = 1.0 if undefined else math.erfc(abs(z) / math.sqrt(2.0))
    out = {"theta_a": theta_a, "theta_b": theta_b, "delta": delta, "var": fv, "var_a": fa, "var_b": fb, "z": z, "p": p,
           "undefined": bool(undefined)}
    for name, mid, v in (("_a", theta_a, fa), ("_b", theta_b, fb), ("", delta, fv)):
        out["lo" + name], out["hi" + name] = mid - zc * math.sqrt(v), mid + zc * math.sqrt(v)
    return out


def _holm_both(p):
    """p [..., >= 24] -> (Holm over the 24 class columns [..., 24], Holm over the 8 selected columns [..., 8])."""
    p = np.asarray(p, dtype=np.float64)
    rows = p.reshape(-1, p.shape[-1])
    allc = np.stack([holm(r[:K]) for r in rows]).reshape(p.shape[:-1] + (K,))
    sel = np.stack([holm(r[SELECTED]) for r in rows]).reshape(p.shape[:-1] + (len(SELECTED),))
    return torch.from_numpy(allc), torch.from_numpy(sel)


def full_counts(side, targets):
    """side [..., 24, 2, 3] int64 (A2, TP, FP) -> [..., 2, 24, 6] int64 (A2, P, Q, TP, FP, FN) per side, P and Q from targets."""
    side = np.asarray(side, dtype=np.int64)
    y = np.asarray(targets, dtype=np.int64)
    P = np.array([int((y[:, t] == c).sum()) for t, c in COLUMN_PAIRS], dtype=np.int64)
    out = np.empty(side.shape[:-3] + (2, K, 6), dtype=np.int64)
    s = np.moveaxis(side, -2, -3)  # [..., 2, 24, 3]
    out[..., 0], out[..., 3], out[..., 4] = s[..., 0], s[..., 1], s[..., 2]
    out[..., 1] = P
    out[..., 2] = y.shape[0] - P
    out[..., 5] = P - s[..., 1]
    return out


# ---- the three tests --------------------------------------------------------------------------------------------------------
def _scores(preds):
    """[24, N] fp64: the score of every column, the expression of report.ranking."""
    return torch.cat([torch.softmax(p.double(), dim=1).t() for p in preds], dim=0)


def joint_ranking(a, b):
    """(order, gs, ge [24, 2N] int32, yhat_a, yhat_b [N, 8] int32) on the device of a: element 2 * i + w of a column = model w's
    score of case i."""
    sa, sb = _scores(a), _scores(b)
    joint = torch.stack([sa, sb], dim=2).reshape(sa.shape[0], 2 * sa.shape[1])
    yhat = [torch.stack([p.argmax(dim=1) for p in preds], dim=1).int().contiguous() for preds in (a, b)]
    return (*report.rank_scores(joint), *yhat)


def permutation_test(a, b, targets, permutations=DEFAULT_PERMUTATIONS, seed=0, chunk=None, targets_b=None):
    """The paired randomisation test of a against b (the module docstring: swap bits, counts, p).

    permutations: B, the swap replicates.  seed: a replicate is a function of (seed, r, N) alone.  chunk: replicates per launch
    (None: at most DEFAULT_CHUNK); every chunk gives the same bits.  targets_b: b's targets when they come from another file;
    refused unless equal to targets.
    Returns {"statistic" [4, 29] fp64 = value(a) - value(b), "p" [4, 29] fp64, "exceed" [4, 29] int64 = #{r : |T_r| >=
    |T_point|}, "replicates" [B, 4, 29] fp64 = T_r, "undefined" [4, 29] int64, "values_a", "values_b" [4, 29] fp64, "counts"
    [2, 24, 6] int64 (A2, P, Q, TP, FP, FN) of a and b, "p_holm_classes" [4, 24], "p_holm_selected" [4, 8], "columns", "metrics",
    "permutations", "seed", "n"}."""
    who = "permutation_test"
    N = _check_pair(a, b, targets, targets_b, who)
    check_permutation_settings(permutations, seed, chunk, who)
    dev = resample.device_for(a, who)
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        order, gs, ge, yhat_a, yhat_b = joint_ranking([p.detach().to(dev) for p in a], [p.detach().to(dev) for p in b])
        y = targets.to(dev).int().contiguous()
        colmap = torch.tensor(COLUMN_PAIRS, dtype=torch.int32, device=dev)
        (point,), (reps,) = resample.replicate_tables(
            lambda outs, seed, r0, point: ops.signif_counts(order, gs, ge, y, yhat_a, yhat_b, colmap, outs[0], seed, r0,
                                                            point=point),
            [(K, 2, 3)], permutations, seed, chunk, DEFAULT_CHUNK, dev)
    host_y = targets.detach().cpu().numpy()
    counts = full_counts(point, host_y)
    values, _ = report.values_from_counts(counts)
    stat = values[0] - values[1]
    rv, ru = report.values_from_counts(full_counts(reps, host_y))  # [B, 2, 4, 29]
    t_r = rv[:, 0] - rv[:, 1]
    exceed = (np.abs(t_r) >= np.abs(stat)[None]).sum(axis=0).astype(np.int64)
    p = (1.0 + exceed.astype(np.float64)) / float(permutations + 1)
    hc, hs = _holm_both(p)
    return {"statistic": torch.from_numpy(stat), "p": torch.from_numpy(p), "exceed": torch.from_numpy(exceed),
            "replicates": torch.from_numpy(t_r), "undefined": torch.from_numpy(ru.any(axis=1).sum(axis=0).astype(np.int64)),
            "values_a": torch.from_numpy(values[0].copy()), "values_b": torch.from_numpy(values[1].copy()),
            "counts": torch.from_numpy(counts), "p_holm_classes": hc, "p_holm_selected": hs, "columns": list(COLUMNS),
            "metrics": list(METRICS), "permutations": permutations, "seed": seed, "n": N}


def placements(preds, targets, dev):
    """[24, N] int32 on dev: the doubled placements of one model, in case order (sm3_signif_placements on its own ranking)."""
    order, gs, ge, _ = report.ranking([p.detach().to(dev) for p in preds], targets.to(dev))
    out = torch.empty(order.shape, dtype=torch.int32, device=dev)
    ops.signif_placements(order, gs, ge, targets.to(dev).int().contiguous(),
                          torch.tensor(COLUMN_PAIRS, dtype=torch.int32, device=dev), out)
    return out


def delong_from_placements(pa, pb, targets, confidence=0.95):
    """DeLong's test of the 24 class columns from the two models' doubled placements [24, N] (numpy, case order): host only."""
    y = np.asarray(targets, dtype=np.int64)
    keys = ("theta_a", "theta_b", "delta", "var", "var_a", "var_b", "z", "p", "lo_a", "hi_a", "lo_b", "hi_b", "lo", "hi")
    cols = {k: np.zeros(K, dtype=np.float64) for k in keys}
    undefined = np.zeros(K, dtype=bool)
    for k, (t, c) in enumerate(COLUMN_PAIRS):
        pos = y[:, t] == c
        one = delong_column(pa[k][pos], pb[k][pos], pa[k][~pos], pb[k][~pos], confidence)
        for key in keys:
            cols[key][k] = one[key]
        undefined[k] = one["undefined"]
    out = {key: torch.from_numpy(v) for key, v in cols.items()}
    hc, hs = _holm_both(cols["p"])
    out.update({"undefined": torch.from_numpy(undefined), "p_holm_classes": hc, "p_holm_selected": hs,
                "columns": list(CLASS_COLUMNS), "confidence": float(confidence), "n": int(y.shape[0])})
    return out


def delong(a, b, targets, confidence=0.95, targets_b=None):
    """DeLong's test for the two correlated AUCs of every class column (the module docstring).
    Returns per column [24] fp64 "theta_a", "theta_b", "delta", "var", "var_a", "var_b", "z", "p", the intervals "lo_a", "hi_a",
    "lo_b", "hi_b", "lo", "hi" (of the difference), "undefined" [24] bool, "p_holm_classes" [24], "p_holm_selected" [8],
    "columns", "confidence", "n"."""
    who = "delong"
    _check_pair(a, b, targets, targets_b, who)
    check_confidence(confidence, who)
    dev = resample.device_for(a, who)
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        pa, pb = (placements(x, targets, dev).cpu().numpy().astype(np.int64) for x in (a, b))
    return delong_from_placements(pa, pb, targets.detach().cpu().numpy(), confidence)


def mcnemar(a, b, targets, targets_b=None):
    """McNemar's exact test of the argmax decisions, per label.  Needs no GPU.
    Returns {"n10", "n01" [8] int64, "p", "p_holm" [8] fp64, "labels"}."""
    who = "mcnemar"
    _check_pair(a, b, targets, targets_b, who)
    n10, n01, p = [], [], []
    for t in range(len(CLASSES_NAME)):
        y = targets[:, t].cpu()
        ra, rb = a[t].detach().argmax(dim=1).cpu() == y, b[t].detach().argmax(dim=1).cpu() == y
        n10.append(int((ra & ~rb).sum()))
        n01.append(int((~ra & rb).sum()))
        p.append(mcnemar_p(n10[-1], n01[-1]))
    return {"n10": torch.tensor(n10, dtype=torch.int64), "n01": torch.tensor(n01, dtype=torch.int64),
            "p": torch.tensor(p, dtype=torch.float64), "p_holm": torch.from_numpy(holm(p)), "labels": list(CLASSES_NAME)}


def significance_report(a, b, targets, permutations=DEFAULT_PERMUTATIONS, seed=0, confidence=0.95, chunk=None, targets_b=None):
    """The three tests of a against b with their Holm-adjusted p-values: {"permutation": permutation_test(...), "delong":
    delong(...), "mcnemar": mcnemar(...), "n", "permutations", "seed", "confidence"}."""
    who = "significance_report"
    N = _check_pair(a, b, targets, targets_b, who)
    check_permutation_settings(permutations, seed, chunk, who)
    check_confidence(confidence, who)
    return {"permutation": permutation_test(a, b, targets, permutations, seed, chunk),
            "delong": delong(a, b, targets, confidence), "mcnemar": mcnemar(a, b, targets),
            "n": N, "permutations": permutations, "seed": seed, "confidence": float(confidence)}


# ---- writers ----------------------------------------------------------------------------------------------------------------
def to_json(rep, path):
    """Everything but the replicate statistics, as lists."""
    resample.write_json(rep, path, ("replicates",))


def csv_rows(rep):
    """The long format: (test, metric, column, statistic, p, p_holm_classes, p_holm_selected, undefined); a cell that does not
    apply is empty."""
    perm, dl, mc = rep["permutation"], rep["delong"], rep["mcnemar"]
    rows = []
    for i, m in enumerate(perm["metrics"]):
        for k, name in enumerate(perm["columns"]):
            rows.append(("permutation", m, name, float(perm["statistic"][i, k]), float(perm["p"][i, k]),
                         float(perm["p_holm_classes"][i, k]) if k < K else "",
                         float(perm["p_holm_selected"][i, SELECTED.index(k)]) if k in SELECTED else "",
                         int(perm["undefined"][i, k])))
    for k, name in enumerate(dl["columns"]):
        rows.append(("delong", "AUC", name, float(dl["z"][k]), float(dl["p"][k]), float(dl["p_holm_classes"][k]),
                     float(dl["p_holm_selected"][SELECTED.index(k)]) if k in SELECTED else "", int(dl["undefined"][k])))
    for t, name in enumerate(mc["labels"]):
        rows.append(("mcnemar", "argmax", name, int(mc["n10"][t]) - int(mc["n01"][t]), float(mc["p"][t]), "",
                     float(mc["p_holm"][t]), 0))
    return rows


def to_csv(rep, path):
    resample.write_long_csv(path, "test,metric,column,statistic,p,p_holm_classes,p_holm_selected,undefined", csv_rows(rep))


def save(rep, log_path, stem):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(rep, log_path, stem, to_json, to_csv)


def format_table(rep):
    """The tests as text: per metric and column the difference in percent, the permutation p (Holm over the classes in
    brackets) and for AUC DeLong's z and p; then McNemar per label."""
    perm, dl, mc = rep["permutation"], rep["delong"], rep["mcnemar"]
    lines = [f"{rep['n']} cases, {rep['permutations']} swap replicates, seed {rep['seed']}"]
    for i, m in enumerate(perm["metrics"]):
        lines.append(f"{m} difference, permutation p" + (", DeLong z and p" if m == "AUC" else ""))
        for k, name in enumerate(perm["columns"]):
            s = f"  {name:<10} {100.0 * float(perm['statistic'][i, k]):+7.2f}  p {float(perm['p'][i, k]):.4f}"
            if k < K:
                s += f" [{float(perm['p_holm_classes'][i, k]):.4f}]"
                if m == "AUC":
                    s += ("  DeLong undefined" if bool(dl["undefined"][k]) else
                          f"  z {float(dl['z'][k]):+6.2f}  p {float(dl['p'][k]):.4f} [{float(dl['p_holm_classes'][k]):.4f}]")
            if int(perm["undefined"][i, k]):
                s += f"  undefined in {int(perm['undefined'][i, k])} of {rep['permutations']}"
            lines.append(s)
    lines.append("McNemar (argmax): a right and b wrong / b right and a wrong, exact p [Holm]")
    for t, name in enumerate(mc["labels"]):
        lines.append(f"  {name:<10} {int(mc['n10'][t]):5d} / {int(mc['n01'][t]):5d}  p {float(mc['p'][t]):.4f} "
                     f"[{float(mc['p_holm'][t]):.4f}]")
    return "\n".join(lines)
