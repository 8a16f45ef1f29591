"""Operating-point report of the 8 derm7pt labels: what happens when a threshold is picked.  Average precision, the Youden and
F1 optima, sensitivity at a specificity floor, specificity at a sensitivity floor, the counts at given thresholds and
decision-curve net benefit of every (label, class) column and the five averages of report.AVERAGES, the ROC and PR point lists,
and case-resampling bootstrap intervals that share their replicates with report.evaluation_report and
calibration.calibration_report.

Inputs (as evaluation_report): preds, 8 float tensors [N, n_t] (NaN is refused); targets [N, 8] int64; 1 <= N <=
report.MAX_CASES.  Columns k = 0 .. 23 are report.COLUMN_PAIRS; the score of column (t, c) is softmax(preds[t].double(), 1)[:, c];
the ranking is report.ranking, unchanged: ascending, stable, tie groups by == on the fp64 scores, gs[j] / ge[j] = first and
one-past-last sorted position of position j's group.

  * operating points of a column: one per tie group g with sorted positions [a_g, b_g), "positive iff score >= the group's
    value", named by pos = a_g, and the empty point (pos = N, threshold +inf, TP = FP = 0).
  * multiplicities: integers m[n] >= 0, sum m = N; the point estimate has m = 1, replicate r the m_r of resample.py's rule.
    With one seed, replicate r here resamples the same cases as replicate r of evaluation_report and calibration_report: the
    intervals of the three reports are joint, and comparisons are paired.
  * counts, all int64: Ppre[j] / S[j] = the sum of m over the positive / negative cases at positions < j; P = Ppre[N], Q = S[N];
    TP(a) = P - Ppre[a], FP(a) = Q - S[a].  A group whose cases all have m = 0 stays a point: it repeats a neighbour's counts
    and matters for the tie-breaks alone.  Per (replicate, column):
        P, Q;
        APN = sum over groups of dTP_g * precQ_g, dTP_g = Ppre[b_g] - Ppre[a_g], precQ_g = (TP * 2^32 + den // 2) // den with
              den = TP + FP at a_g; a group with dTP_g = 0 contributes 0, and its precision, possibly 0 / 0, is never formed;
        four searches, each the maximum under a TOTAL order (no reduction order can show), each giving (TP, FP, pos):
          Youden              maximise (TP * Q - FP * P, pos);
          F1                  maximise 2 TP / (TP + FP + P), compared by cross-multiplication in int64, then pos;
          sens at spec >= s0  with sigma = floor(s0 * 2^32): among the points with (Q - FP) * 2^32 >= sigma * Q maximise
                              (TP, -FP, pos);
          spec at sens >= r0  with rho = floor(r0 * 2^32): among the points with TP * 2^32 >= rho * P maximise (-FP, TP, pos);
          (floor, not round: rint(0.8 * 2^32) * 100 > 80 * 2^32 would refuse the specificity of exactly 80 / 100 at the floor
          0.8; floor accepts every exactly attained decimal floor.  The empty point meets every spec floor and pos = 0 every
          sens floor, so a search always has a point.)
        fixed thresholds: (TP(f), FP(f)) at f = torch.searchsorted(sorted scores, threshold, right=False), for thresholds
          [24, Lt] fp64: the caller's per-column thresholds, or the decision-curve threshold probabilities `decision`, the same
          for every column.
    Every integer stays below 2^53 (the largest is sigma * Q <= 2^45).
  * values, fp64, on the host, each ONE IEEE division of two exactly represented integers, 0 and `undefined` when the
    denominator is 0:
        AP = APN / (P * 2^32);  and per point, with TN = Q - FP, FN = P - TP:
        sens = TP / P,  spec = TN / Q,  PPV = TP / (TP + FP),  NPV = TN / (TN + FN),
        J = (TP * Q - FP * P) / (P * Q),  F1 = 2 TP / (TP + FP + P).
    The threshold of a searched point is the sorted score at pos (+inf at pos = N).
    Net benefit, for the `decision` thresholds pt (0 < pt < 1) alone, operations in exactly this order:
        w = pt / (1 - pt),  NB = (TP - FP * w) / N,  NB_all = (P - Q * w) / N.
  * rows of the value table: "AP"; "<point> <metric>" for the points "youden", "f1", "spec>=<s0>", "sens>=<r0>" and the fixed
    ones ("pt=<pt>" or "thr[i]") and the six metrics; "NB pt=<pt>" and "NB_all pt=<pt>".  Columns: the 24 classes and the five
    averages of report.averages.  Intervals and undefined counts by resample.interval, unchanged; an average
    is undefined in the replicates in which any contributing column is.
  * curves (point estimate): per column the ROC and PR point lists at every operating point in ascending pos (descending
    threshold last): fpr = FP / Q, tpr = recall = TP / P, precision = TP / (TP + FP), thresholds -- from the integer cumulative
    counts at the group starts, one pass of host cumsums.  The ROC band is what spec_floors given as a grid yields.

The counts come from sm3_operating_counts (csrc/operating.hip): one workgroup per replicate and label, integers only, so equal
inputs give equal bits whatever the chunk.  len(spec_floors), len(sens_floors), Lt <= MAX_LEVELS; floors lie in [0, 1]."""
import math

import numpy as np
import torch

from . import ops, report, resample
from .resample import safe_div as _div

MAX_LEVELS = ops.OPERATING_MAX_LEVELS
ONE = 1 << 32                       # 1.0 in Q32
POINT_METRICS = ("sens", "spec", "PPV", "NPV", "J", "F1")
RULES = ("youden", "f1", "spec>=X", "sens>=X")
DEFAULT_SPEC = (0.8, 0.9, 0.95)
DEFAULT_SENS = (0.8, 0.9, 0.95)
DEFAULT_DECISION = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5)
DEFAULT_CHUNK = 1024  # replicates per launch: a choice (1024 x 24 x 265 int64 = 50 MiB of records at the most)
K = report.K


# ---- settings -----------------------------------------------------------------------------------------------------------------
def _numbers(v, name, who, lo_open, hi_open):
    """A list of at most MAX_LEVELS numbers in [0, 1] (open ends where asked) -> floats."""
    if isinstance(v, torch.Tensor):
        v = v.tolist()
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        v = [v]
    v = list(v)
    if len(v) > MAX_LEVELS:
        raise ValueError(f"{who}: {name} holds {len(v)} entries, at most MAX_LEVELS = {MAX_LEVELS} are supported")
    for x in v:
        ok = isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x)
        if not ok or not (0 < x if lo_open else 0 <= x) or not (x < 1 if hi_open else x <= 1):
            ends = ("(" if lo_open else "[") + "0, 1" + (")" if hi_open else "]")
            raise ValueError(f"{who}: every entry of {name} must be a number in {ends}, got {x!r}")
    return [float(x) for x in v]


def check_levels(spec_floors, sens_floors, decision, who="operating_report"):
    """(spec_floors, sens_floors, decision) as lists of floats; the refusals that need neither a tensor nor a device."""
    return (_numbers(spec_floors, "spec_floors", who, False, False), _numbers(sens_floors, "sens_floors", who, False, False),
            _numbers(decision, "decision", who, True, True))


def q32_floor(x):
    """floor(x * 2^32) of a floor value in [0, 1]: the product is exact in fp64 (a power of two), so this is the integer part."""
    return int(math.floor(float(x) * float(ONE)))


def parse_rule(rule, who="fit_thresholds"):
    """"youden" | "f1" | "spec>=X" | "sens>=X" -> (kind, X or None)."""
    if rule in ("youden", "f1"):
        return rule, None
    if isinstance(rule, str):
        for kind in ("spec", "sens"):
            if rule.startswith(kind + ">="):
                try:
                    x = float(rule[len(kind) + 2:])
                except ValueError:
                    break
                return kind, _numbers([x], "the floor of the rule", who, False, False)[0]
    raise ValueError(f"{who}: rule must be one of {RULES} with X in [0, 1], got {rule!r}")


def check_thresholds(thresholds, who="operating_report"):
    """None, or per-column thresholds [24] / [24, Lt] -> fp64 numpy [24, Lt]."""
    if thresholds is None:
        return None
    th = np.asarray(thresholds.detach().cpu().numpy() if isinstance(thresholds, torch.Tensor) else thresholds, dtype=np.float64)
    if th.ndim == 1:
        th = th[:, None]
    if th.ndim != 2 or th.shape[0] != K or th.shape[1] > MAX_LEVELS:
        raise ValueError(f"{who}: thresholds must be [{K}] or [{K}, Lt] with Lt <= MAX_LEVELS = {MAX_LEVELS}, got {th.shape}")
    if np.isnan(th).any():
        raise ValueError(f"{who}: thresholds hold a NaN")
    return np.ascontiguousarray(th)


# ---- the record of sm3_operating_counts ---------------------------------------------------------------------------------------
def point_names(spec_floors, sens_floors, fixed_names):
    return (["youden", "f1"] + [f"spec>={s!r}" for s in spec_floors] + [f"sens>={r!r}" for r in sens_floors] + list(fixed_names))


def point_offsets(Ls, Lr, Lt):
    """Offset of each point's (TP, FP[, pos]) in a record, in the order of point_names."""
    return ([3, 6] + [9 + 3 * i for i in range(Ls)] + [9 + 3 * Ls + 3 * i for i in range(Lr)]
            + [9 + 3 * (Ls + Lr) + 2 * i for i in range(Lt)])


def row_names(points, decision):
    return (["AP"] + [f"{p} {m}" for p in points for m in POINT_METRICS]
            + [f"{kind} pt={pt!r}" for pt in decision for kind in ("NB", "NB_all")])


def values_from_counts(counts, Ls, Lr, Lt, decision, N):
    """counts [..., 24, 9 + 3 Ls + 3 Lr + 2 Lt] int64 -> (values [..., rows, 29] fp64, undefined [..., rows, 29] bool), rows as
    row_names; decision: the threshold probabilities of the Lt fixed points, or () when those are the caller's thresholds."""
    counts = np.asarray(counts, dtype=np.int64)
    P, Q, APN = counts[..., 0], counts[..., 1], counts[..., 2]
    series = [_div(APN, P * ONE)]
    offs = point_offsets(Ls, Lr, Lt)
    for off in offs:
        TP, FP = counts[..., off], counts[..., off + 1]
        TN, FN = Q - FP, P - TP
        for num, den in ((TP, P), (TN, Q), (TP, TP + FP), (TN, TN + FN), (TP * Q - FP * P, P * Q), (2 * TP, TP + FP + P)):
            series.append(_div(num, den))
    for i, pt in enumerate(decision):
        off = offs[2 + Ls + Lr + i]
        TP, FP = counts[..., off], counts[..., off + 1]
        w = np.float64(pt) / (np.float64(1.0) - np.float64(pt))
        never = np.zeros(P.shape, dtype=bool)
        series.append(((TP.astype(np.float64) - FP.astype(np.float64) * w) / np.float64(N), never))
        series.append(((P.astype(np.float64) - Q.astype(np.float64) * w) / np.float64(N), never))
    lead = counts.shape[:-2]
    values = np.zeros(lead + (len(series), report.NV), dtype=np.float64)
    undefined = np.zeros(values.shape, dtype=bool)
    for i, (v, u) in enumerate(series):
        values[..., i, :K], undefined[..., i, :K] = v, u
        values[..., i, K:] = report.averages(v)
        for a, cols in enumerate(report.AVERAGES.values()):
            undefined[..., i, K + a] = u[..., cols].any(axis=-1)
    return values, undefined


def curves_from_ranking(sorted_scores, order, gs, y_cols):
    """The ROC and PR point lists of the point estimate.  sorted_scores [24, N] fp64, order, gs [24, N], y_cols [24, N] bool (case n
    is a positive of column k), all numpy on the host -> 24 dicts of fp64 tensors, one entry per operating point in ascending
    pos: "fpr", "tpr", "precision", "recall", "thresholds" (the empty point last, threshold +inf) and "pos" int64."""
    N = order.shape[1]
    out = []
    for k in range(order.shape[0]):
        pos_k = y_cols[k][order[k]]
        Ppre = np.concatenate([[0], np.cumsum(pos_k, dtype=np.int64)])
        S = np.concatenate([[0], np.cumsum(~pos_k, dtype=np.int64)])
        a = np.concatenate([np.nonzero(gs[k] == np.arange(N))[0], [N]]).astype(np.int64)
        TP, FP = Ppre[N] - Ppre[a], S[N] - S[a]
        tpr, fpr, prec = _div(TP, np.full_like(TP, Ppre[N]))[0], _div(FP, np.full_like(FP, S[N]))[0], _div(TP, TP + FP)[0]
        thr = np.concatenate([sorted_scores[k][a[:-1]], [np.inf]])
        out.append({"fpr": torch.from_numpy(fpr), "tpr": torch.from_numpy(tpr), "precision": torch.from_numpy(prec),
                    "recall": torch.from_numpy(tpr.copy()), "thresholds": torch.from_numpy(thr), "pos": torch.from_numpy(a)})
    return out


# ---- the report ---------------------------------------------------------------------------------------------------------------
def operating_report(preds, targets, spec_floors=DEFAULT_SPEC, sens_floors=DEFAULT_SENS, decision=DEFAULT_DECISION, thresholds=None,
                     bootstrap=0, confidence=0.95, seed=0, chunk=None):
    """The operating-point report of one set of predictions.

    preds, targets: as report.evaluation_report.  spec_floors / sens_floors: the floors s0 / r0 in [0, 1] of "sens at spec >= s0" /
    "spec at sens >= r0".  decision: threshold probabilities 0 < pt < 1; the fixed points are "score >= pt" in every column and
    carry the net benefit rows.  thresholds: [24] or [24, Lt] fp64 per-column thresholds (those of fit_thresholds, say); when
    given THEY are the fixed points ("thr[i]"), and there are no net benefit rows.  bootstrap, confidence, seed, chunk: as
    evaluation_report (chunk None: at most DEFAULT_CHUNK replicates per launch; every chunk gives the same bits).
    Returns {"counts" [24, R] int64 (the records of sm3_operating_counts), "values" [rows, 29] fp64, "point_undefined" [rows, 29]
    bool, "rows", "columns", "points" (names, in record order), "thresholds" [points, 24] fp64 (of a searched point the sorted
    score at its pos, +inf at pos = N; of a fixed point the threshold given), "curves" (24 dicts: fpr, tpr, precision, recall,
    thresholds, pos), "spec_floors", "sens_floors", "decision", "targets", "n"} and, with bootstrap > 0, "replicates" [B, rows, 29]
    fp64, "replicate_counts" [B, 24, R] int64, "lo", "hi" [rows, 29] fp64, "undefined" [rows, 29] int64, "bootstrap", "seed",
    "confidence".  All tensors on the CPU.
    The inputs are not modified."""
    who = "operating_report"
    report.check_settings(bootstrap, confidence, seed, chunk, who)
    spec_floors, sens_floors, decision = check_levels(spec_floors, sens_floors, decision, who)
    thresholds = check_thresholds(thresholds, who)
    report.check_inputs(preds, targets, who)
    dev = resample.device_for(preds, who)
    with torch.cuda.device(dev), ops.stream_scope():
        return _report(preds, targets, spec_floors, sens_floors, decision, thresholds, bootstrap, confidence, seed, chunk, dev,
                       ops.operating_counts)


def _report(preds, targets, spec_floors, sens_floors, decision, thresholds, bootstrap, confidence, seed, chunk, dev, counts_fn):
    """operating_report after its checks, on the device dev, with the counts from counts_fn (ops.operating_counts)."""
    N, B = targets.shape[0], bootstrap
    Ls, Lr = len(spec_floors), len(sens_floors)
    if thresholds is not None:
        decision = []
    with torch.no_grad():
        dp, dt = [p.detach().to(dev) for p in preds], targets.to(dev)
        order, gs, ge, _ = report.ranking(dp, dt)
        score = torch.cat([torch.softmax(p.double(), dim=1).t() for p in dp], dim=0)  # [24, N], the scores ranking sorted
        sorted_scores = score.gather(1, order.long()).contiguous()
        fixed = torch.from_numpy(thresholds if thresholds is not None
                                 else np.tile(np.asarray(decision, dtype=np.float64), (K, 1)).reshape(K, len(decision))).to(dev)
        Lt = fixed.shape[1]
        fixpos = torch.searchsorted(sorted_scores, fixed.contiguous(), right=False).int().contiguous()
        y = dt.int().contiguous()
        colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=dev)
        sigma = torch.tensor([q32_floor(s) for s in spec_floors], dtype=torch.int64, device=dev)
        rho = torch.tensor([q32_floor(r) for r in sens_floors], dtype=torch.int64, device=dev)
        R = ops.operating_record(Ls, Lr, Lt)
        (point,), (reps,) = resample.replicate_tables(
            lambda outs, seed, r0, point: counts_fn(order, gs, ge, y, colmap, sigma, rho, fixpos, outs[0], seed, r0, point=point),
            [(K, R)], B, seed, chunk, DEFAULT_CHUNK, dev)
        ss, fixed = sorted_scores.cpu().numpy(), fixed.cpu().numpy()
        y_cols = np.stack([dt[:, t].cpu().numpy() == c for t, c in report.COLUMN_PAIRS])
        curves = curves_from_ranking(ss, order.cpu().numpy(), gs.cpu().numpy(), y_cols)
    fixed_names = [f"thr[{i}]" for i in range(Lt)] if thresholds is not None else [f"pt={pt!r}" for pt in decision]
    points = point_names(spec_floors, sens_floors, fixed_names)
    offs = point_offsets(Ls, Lr, Lt)
    thr = np.empty((len(points), K), dtype=np.float64)
    padded = np.concatenate([ss, np.full((K, 1), np.inf)], axis=1)
    for i, off in enumerate(offs[:2 + Ls + Lr]):
        thr[i] = padded[np.arange(K), point[:, off + 2]]
    thr[2 + Ls + Lr:] = fixed.T
    values, undefined = values_from_counts(point, Ls, Lr, Lt, decision, N)
    out = {"counts": torch.from_numpy(point), "values": torch.from_numpy(values), "point_undefined": torch.from_numpy(undefined),
           "rows": row_names(points, decision), "columns": list(report.COLUMNS), "points": points,
           "thresholds": torch.from_numpy(thr), "curves": curves, "spec_floors": spec_floors, "sens_floors": sens_floors,
           "decision": list(decision), "targets": targets.detach().cpu().clone(), "n": N}
    if B:
        rv, ru = values_from_counts(reps, Ls, Lr, Lt, decision, N)
        boot = resample.pack_intervals({}, [("", rv, ru.sum(axis=0))], B, seed, confidence)
        out.update({"replicates": boot.pop("replicates"), "replicate_counts": torch.from_numpy(reps)}, **boot)
    return out


def rule_settings(rule, who="fit_thresholds"):
    """The (spec_floors, sens_floors, point name) that make `rule`'s point part of a report."""
    kind, x = parse_rule(rule, who)
    return ([x] if kind == "spec" else []), ([x] if kind == "sens" else []), (kind if x is None else f"{kind}>={x!r}")


def fit_thresholds(preds, targets, rule):
    """The 24 thresholds (fp64 tensor [24]) that `rule` picks on the point estimate of these predictions: "youden", "f1",
    "spec>=X" (the most sensitive point whose specificity is at least X) or "sens>=X" (the most specific point whose sensitivity
    is at least X).  A threshold is the sorted score at the point's pos, +inf for the empty point: "positive iff score >=
    threshold", so operating_report(thresholds=...) of the same predictions finds the fitted point's counts again."""
    spec_floors, sens_floors, name = rule_settings(rule)
    rep = operating_report(preds, targets, spec_floors=spec_floors, sens_floors=sens_floors, decision=[])
    return rep["thresholds"][rep["points"].index(name)].clone()


# ---- comparison and writers -----------------------------------------------------------------------------------------------------
def compare(a, b):
    """The paired difference of two operating-point reports of the SAME cases with the same settings: equal targets, rows,
    bootstrap, seed and confidence (ValueError otherwise), so replicate r of both resamples the same cases.  Returns {"delta":
    a.values - b.values [rows, 29], "rows", "columns"} and, with a bootstrap, "lo", "hi" by the interval rule on a.replicates -
    b.replicates, "frac_le_zero" = the fraction of replicates with a difference <= 0, "bootstrap", "seed", "confidence"."""
    resample.check_paired(a, b, "operating_report", ("values", "targets", "rows"),
                          (("rows", "the two reports hold different rows (floors, decision thresholds or thresholds differ)"),))
    return resample.paired_intervals({"delta": a["values"] - b["values"], "rows": list(a["rows"]), "columns": list(a["columns"])},
                                     a, b)


def csv_rows(rep):
    """Long format: (row, column, value[, lo, hi, undefined]) of the value table."""
    boot = "lo" in rep
    rows = []
    for i, r in enumerate(rep["rows"]):
        for k, c in enumerate(rep["columns"]):
            row = [r, c, float(rep["values"][i, k])]
            if boot:
                row += [float(rep["lo"][i, k]), float(rep["hi"][i, k]), int(rep["undefined"][i, k])]
            rows.append(row)
    return rows


def to_csv(rep, path):
    """The long format of csv_rows with a header; repr of the fp64 values: they parse back exactly."""
    resample.write_long_csv(path, "row,column,value" + (",lo,hi,undefined" if "lo" in rep else ""), csv_rows(rep))


def to_json(rep, path):
    """Everything but the replicates and the targets, as lists (json writes repr of a float: the values parse back exactly; the
    empty point's threshold is written as Infinity, which json reads back)."""
    resample.write_json(rep, path, ("replicates", "replicate_counts", "targets"))


def _shown():
    return list(report.SELECTED) + [report.COLUMNS.index("8 avg")]


def format_table(rep):
    """The table as text: one line per row with the 8 selected columns (class CLS_WEIGHTS[t] of label t) and "8 avg", four
    decimals, the interval of "8 avg" in brackets; the files hold every column and every interval."""
    cols = _shown()
    lines = ["operating points" + " " * 13 + " ".join(f"{rep['columns'][k]:>8}" for k in cols)]
    for i, r in enumerate(rep["rows"]):
        s = f"  {r:<26} " + " ".join(f"{float(rep['values'][i, k]):8.4f}" for k in cols)
        if "lo" in rep:
            s += f"  [{float(rep['lo'][i, cols[-1]]):.4f}, {float(rep['hi'][i, cols[-1]]):.4f}]"
        lines.append(s)
    return "\n".join(lines)


def format_compare(cmp):
    cols = _shown()
    lines = ["difference" + " " * 20 + " ".join(f"{cmp['columns'][k]:>8}" for k in cols)]
    for i, r in enumerate(cmp["rows"]):
        lines.append(f"  {r:<26} " + " ".join(f"{float(cmp['delta'][i, k]):+8.4f}" for k in cols))
        if "lo" in cmp:
            k = cols[-1]
            lines.append(f"    8 avg [{float(cmp['lo'][i, k]):+.4f}, {float(cmp['hi'][i, k]):+.4f}]  <= 0 in "
                         f"{float(cmp['frac_le_zero'][i, k]):.3f}")
    return "\n".join(lines)


# ---- what the command-line tools share ----------------------------------------------------------------------------------------
def add_flags(parser):
    """--operating / --operating-spec / --operating-sens / --operating-decision / --operating-rule of the evaluation tools."""
    parser.add_argument("--operating", action="store_true",
                        help="operating-point report (AP, Youden and F1 optima, sens at spec floors, spec at sens floors, net "
                             "benefit) of the predictions")
    parser.add_argument("--operating-spec", type=float, nargs="*", default=list(DEFAULT_SPEC),
                        help=f"specificity floors in [0, 1], at most {MAX_LEVELS}")
    parser.add_argument("--operating-sens", type=float, nargs="*", default=list(DEFAULT_SENS),
                        help=f"sensitivity floors in [0, 1], at most {MAX_LEVELS}")
    parser.add_argument("--operating-decision", type=float, nargs="*", default=list(DEFAULT_DECISION),
                        help=f"decision-curve threshold probabilities in (0, 1), at most {MAX_LEVELS}")
    parser.add_argument("--operating-rule", type=str, default="youden",
                        help="the rule that --fit-on fits thresholds by: youden, f1, spec>=X or sens>=X")
    return parser


def check_flags(args):
    """The refusals of the flags that argparse does not make, before any work is done."""
    check_levels(args.operating_spec, args.operating_sens, args.operating_decision, "--operating")
    parse_rule(args.operating_rule, "--operating-rule")


def flag_settings(args):
    return dict(spec_floors=args.operating_spec, sens_floors=args.operating_sens, decision=args.operating_decision)


def save(rep, log_path, stem="val_operating"):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(rep, log_path, stem, to_json, to_csv)


def stats_line(rep):
    """The one printed line: the "8 avg" of AP, of J at the Youden point and of the sensitivity at the first spec floor."""
    if rep is None:
        return f"no operating-point report: more than MAX_CASES = {report.MAX_CASES} cases"
    k = report.COLUMNS.index("8 avg")
    names = ["AP", "youden J"] + [f"{p} sens" for p in rep["points"][2:3] if p.startswith("spec>=")]
    parts = []
    for name in names:
        i = rep["rows"].index(name)
        s = f"{name.replace(' ', '_')}_AVG {float(rep['values'][i, k]):.4f}"
        if "lo" in rep:
            s += f" [{float(rep['lo'][i, k]):.4f}, {float(rep['hi'][i, k]):.4f}]"
        parts.append(s)
    return " ".join(parts)


def validation_operating(preds, targets, args, log_path):
    """What a tool does under --operating after its last validation pass: the report with the tool's --operating-* lists and its
    --bootstrap, --bootstrap-seed and --confidence, written as val_operating.json / .csv under log_path.  Beyond MAX_CASES
    cases: None, which stats_line words."""
    if targets.shape[0] > report.MAX_CASES:
        return None
    rep = operating_report(list(preds), targets, bootstrap=args.bootstrap, confidence=args.confidence, seed=args.bootstrap_seed,
                           **flag_settings(args))
    save(rep, log_path)
    return rep

