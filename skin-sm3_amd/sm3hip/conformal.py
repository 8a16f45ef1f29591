"""Conformal prediction-set report of the 8 derm7pt labels: split conformal thresholds fitted on one split (validation), the
prediction sets of another (test) under them -- coverage, set size, empty and singleton sets, class-conditional coverage -- and
case-resampling bootstrap intervals that resample BOTH splits and refit the thresholds in every replicate.  This docstring is
the normative text; include/sm3_hip.h repeats the integer part.

Inputs.  A test split, preds (8 float tensors [N, n_t]) and targets [N, 8] int64, and a calibration split, cal_preds and
cal_targets with N_cal cases; both as report.check_inputs asks, each with 1 to report.MAX_CASES cases.  Optional temperature,
8 positive numbers as calibration.check_temperature asks, applied to both splits.

  * probabilities: q[n, c] is the Q32 integer of the class-wise series of calibration.fixed_point, rint(softmax(preds[t].double()
    / T_t)[n, c] * 2^32).
  * scores, int64, columns in the order of report.COLUMN_PAIRS (K = 24):
        method = "lac":  s[n, c] = 2^32 - q[n, c];
        method = "aps":  (adaptive prediction sets, the deterministic form) s[n, c] = the sum of q[n, c'] over the classes c' of
                         the label with q[n, c'] > q[n, c], or with q[n, c'] == q[n, c] and c' <= c -- class c itself included.
    The true-class score of a case is a[n] = s[n, y_n].
  * levels: A of them, 1 <= A <= MAX_LEVELS = 8, each 0 < alpha < 1, taken as the exact rational fractions.Fraction(str(alpha))
    = num / den; a denominator above MAX_DENOMINATOR = 10^6 is refused.  The kernel gets (num, den): no float product decides a
    rank.
  * threshold, given integer multiplicities w >= 0 on the calibration cases:
        conditional = "marginal": n' = sum w = N_cal;  k = (n' + 1) - floor((n' + 1) * num / den) in integers;  qhat = the
            true-class score at the first position j of the ascending ranking of a (ties by case index: one stable torch sort
            per label, done once) with R_j + w_j >= k, R_j = the sum of w before j -- the k-th smallest of the w-fold copies.
            k > n': qhat = INF = 2^40, above any score, and every class is in every set.  qhat is the threshold of every class
            of the label.
        conditional = "class" (Mondrian): the same rule per class c of the label over the calibration cases with y = c only;
            n' = sum w [y = c] changes from replicate to replicate; a class without calibration cases gets INF.
  * sets and the record: the set of test case n is {c : s[n, c] <= thr[t, a, c]}.  With multiplicities m on the test cases the
    record of a (label, level) is 24 int64: cov = sum m [true class in set], size = sum m |set|, single_hit = sum m [|set| = 1
    and covered], hist[0 .. 5] = sum m [|set| = k], then for c = 0 .. 4: n_c = sum m [y = c], cov_c = sum m [y = c][covered],
    in_c = sum m [c in set]; the slots of classes the label lacks are 0.  thresholds [8, A, 5] int64 holds the thr the record
    was counted under (0 in those slots).
  * values, fp64, on the host, ONE IEEE division each through resample.safe_div:
        label_values [A, 5, 9]: rows coverage = cov / N, mean size = size / N, empty = hist0 / N, singleton = hist1 / N,
            singleton accuracy = single_hit / hist1; columns the 8 labels and "AVG" (summed in label order, divided once);
        class_values [A, 2, 29]: class coverage cov_c / n_c and inclusion in_c / N of the 24 columns, and report.averages of each;
        threshold_values [A, 8, 5] = thr / 2^32, inf where the threshold is INF (threshold_inf flags those).
    A zero denominator (hist1 = 0, n_c = 0) makes that value undefined for that replicate (value 0, counted), as
    resample.interval handles; an average is undefined where one of its columns is.
  * resampling: the test multiplicities of replicate r are resample.py's m_r (stream word 2, N): the same test cases as
    replicate r of every other report, so the intervals are joint.  The calibration multiplicities follow the same rule on N_cal
    with stream word 6, from the same seed.  refit = True: every replicate refits its thresholds from its own calibration
    multiplicities -- the interval of the whole procedure.  refit = False: the point thresholds are used in every replicate --
    the interval conditional on the calibration split that was drawn.  The point estimate has all multiplicities 1.

Records and thresholds come from sm3_conformal_counts (csrc/conformal.hip): one workgroup per replicate and label, integers
only, so equal inputs give equal bits."""
import fractions

import numpy as np
import torch

from . import calibration, ops, report, resample
from .metrics import CLASSES_NAME, NUM_CLASSES

MAX_LEVELS = ops.CONFORMAL_MAX_LEVELS
MAX_CLASSES = ops.CONFORMAL_MAX_CLASSES
RECORD = ops.CONFORMAL_RECORD
METHODS = ("lac", "aps")
CONDITIONALS = ops.CONFORMAL_CONDITIONALS
MAX_DENOMINATOR = 10 ** 6
ONE = 1 << 32                       # 1.0 in Q32
INF = 1 << 40                       # the threshold that admits every class
DEFAULT_ALPHAS = (0.05, 0.1, 0.2)
LABEL_METRICS = ("coverage", "mean size", "empty", "singleton", "singleton accuracy")
CLASS_METRICS = ("class coverage", "inclusion")
LABEL_COLUMNS = list(CLASSES_NAME) + ["AVG"]
CLASS_COLUMNS = list(report.COLUMNS)  # the 24 classes, then the five averages
T, K = len(NUM_CLASSES), report.K
DEFAULT_CHUNK = 4096  # replicates per launch: a choice (4096 x 8 x 8 x 29 int64 = 58 MiB at the most)
TABLES = ("label", "class", "threshold")


# ---- settings --------------------------------------------------------------------------------------------------------------
def check_alphas(alphas, who="conformal_report"):
    """1 to MAX_LEVELS numbers in (0, 1) -> (the levels as floats, [(num, den), ...] of Fraction(str(alpha)))."""
    if isinstance(alphas, (int, float)) and not isinstance(alphas, bool):
        alphas = (alphas,)
    try:
        alphas = list(alphas)
    except TypeError:
        raise ValueError(f"{who}: alphas must be 1 to {MAX_LEVELS} numbers in (0, 1), got {alphas!r}") from None
    if not 1 <= len(alphas) <= MAX_LEVELS:
        raise ValueError(f"{who}: alphas must be 1 to {MAX_LEVELS} numbers in (0, 1), got {alphas!r}")
    levels = []
    for a in alphas:
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0 < a < 1:
            raise ValueError(f"{who}: every alpha must be a number with 0 < alpha < 1, got {a!r}")
        f = fractions.Fraction(str(a))
        if f.denominator > MAX_DENOMINATOR:
            raise ValueError(f"{who}: alpha {a!r} = {f} has a denominator above {MAX_DENOMINATOR}")
        levels.append((f.numerator, f.denominator))
    return [float(a) for a in alphas], levels


def check_method(method, conditional, who="conformal_report"):
    if method not in METHODS:
        raise ValueError(f"{who}: method must be one of {METHODS}, got {method!r}")
    if conditional not in CONDITIONALS:
        raise ValueError(f"{who}: conditional must be one of {CONDITIONALS}, got {conditional!r}")


def rank(n, num, den):
    """k of the threshold rule for n' = n calibration copies at the level num / den, in integers."""
    return (n + 1) - ((n + 1) * num) // den


# ---- scores and sets: torch on the device of the tensors, plumbing -------------------------------------------------------
def scores(preds, temperature=None, method="lac"):
    """s [24, N] int64 on the device of preds: the scores of the 24 columns."""
    check_method(method, CONDITIONALS[0], "scores")
    N = preds[0].shape[0]
    q = calibration.fixed_point(preds, torch.zeros((N, T), dtype=torch.int64, device=preds[0].device), temperature)[0][T:]
    if method == "lac":
        return (ONE - q).contiguous()
    out, k0 = [], 0
    for n in NUM_CLASSES:
        ql = q[k0:k0 + n]                                          # [n, N]
        other, own = ql[:, None, :], ql[None, :, :]                # [c', c, N]
        idx = torch.arange(n, device=q.device)
        first = (other > own) | ((other == own) & (idx[:, None] <= idx[None, :])[:, :, None])
        out.append((other * first).sum(dim=0))
        k0 += n
    return torch.cat(out, dim=0).contiguous()


def true_class_scores(s, targets):
    """a [8, N] int64: a[t, n] = s[column (t, y_n), n]."""
    first = torch.tensor([report.COLUMN_PAIRS.index((t, 0)) for t in range(T)], device=s.device)
    return s.gather(0, (targets + first[None, :]).t().contiguous())


def prediction_sets(preds, thresholds, level=0, temperature=None, method="lac"):
    """The sets themselves: [N, 24] bool, column k = (t, c) true where class c is in the set of label t at the level `level` of
    thresholds [8, A, 5] int64 (conformal_report's "thresholds", fit_thresholds)."""
    thresholds = torch.as_tensor(thresholds)
    if thresholds.dtype != torch.int64 or thresholds.dim() != 3 or thresholds.shape[0] != T or thresholds.shape[2] != MAX_CLASSES:
        raise ValueError(f"prediction_sets: thresholds must be an int64 tensor [{T}, A, {MAX_CLASSES}]")
    if not resample.is_int(level) or not 0 <= level < thresholds.shape[1]:
        raise ValueError(f"prediction_sets: level must be an integer in [0, {thresholds.shape[1]}), got {level!r}")
    s = scores(preds, temperature, method)
    thr = torch.stack([thresholds[t, level, c] for t, c in report.COLUMN_PAIRS]).to(s.device)
    return (s <= thr[:, None]).t().contiguous()


# ---- values --------------------------------------------------------------------------------------------------------------
def values_from_counts(counts, thr, N):
    """counts [..., 8, A, 24], thr [..., 8, A, 5] int64 -> {"label_values" [..., A, 5, 9], "class_values" [..., A, 2, 29],
    "threshold_values" [..., A, 8, 5] fp64 and "<table>_undefined" bool of the same shapes (threshold: where it is INF)}."""
    counts, thr = np.asarray(counts, dtype=np.int64), np.asarray(thr, dtype=np.int64)
    counts, thr = np.moveaxis(counts, -3, -2), np.moveaxis(thr, -3, -2)      # [..., A, 8, *]
    lead = counts.shape[:-2]
    n = np.int64(N)
    cov, size, hit, h0, h1 = (counts[..., e] for e in (0, 1, 2, 3, 4))
    label = np.zeros(lead + (len(LABEL_METRICS), T + 1), dtype=np.float64)
    lundef = np.zeros(label.shape, dtype=bool)
    for i, (num, den) in enumerate(((cov, n), (size, n), (h0, n), (h1, n), (hit, h1))):
        label[..., i, :T], lundef[..., i, :T] = resample.safe_div(num, den)
    acc = np.zeros(lead + (len(LABEL_METRICS),), dtype=np.float64)
    for t in range(T):
        acc = acc + label[..., t]
    label[..., T] = acc / float(T)
    lundef[..., T] = lundef[..., :T].any(axis=-1)
    cls = np.zeros(lead + (len(CLASS_METRICS), report.NV), dtype=np.float64)
    cundef = np.zeros(cls.shape, dtype=bool)
    for k, (t, c) in enumerate(report.COLUMN_PAIRS):
        cls[..., 0, k], cundef[..., 0, k] = resample.safe_div(counts[..., t, 10 + 3 * c], counts[..., t, 9 + 3 * c])
        cls[..., 1, k], cundef[..., 1, k] = resample.safe_div(counts[..., t, 11 + 3 * c], n)
    for i in range(len(CLASS_METRICS)):
        cls[..., i, K:] = report.averages(cls[..., i, :K])
        for a, cols in enumerate(report.AVERAGES.values()):
            cundef[..., i, K + a] = cundef[..., i, cols].any(axis=-1)
    inf = thr >= INF
    tv = np.where(inf, np.inf, resample.safe_div(np.where(inf, 0, thr), np.int64(ONE))[0])
    return {"label_values": label, "label_undefined": lundef, "class_values": cls, "class_undefined": cundef,
            "threshold_values": tv, "threshold_undefined": inf}


# ---- the report ----------------------------------------------------------------------------------------------------------
def _device_inputs(preds, targets, cal_preds, cal_targets, temperature, method, dev):
    s = scores([p.detach().to(dev) for p in preds], temperature, method)
    cal_s = scores([p.detach().to(dev) for p in cal_preds], temperature, method)
    cal_a = true_class_scores(cal_s, cal_targets.to(dev)).contiguous()
    cal_order = torch.sort(cal_a, dim=1, stable=True).indices.int().contiguous()
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=dev)
    return cal_a, cal_order, cal_targets.to(dev).int().contiguous(), s, targets.to(dev).int().contiguous(), colmap


def _check_splits(preds, targets, cal_preds, cal_targets, who):
    N = report.check_inputs(preds, targets, who)
    N_cal = report.check_inputs(cal_preds, cal_targets, who + " (calibration split)")
    return N, N_cal


def fit_thresholds(cal_preds, cal_targets, alphas=(0.1,), method="lac", conditional="marginal", temperature=None):
    """The point thresholds [8, A, 5] int64 (CPU) of the calibration split, every case once, through the kernel's point call."""
    who = "fit_thresholds"
    _, levels = check_alphas(alphas, who)
    check_method(method, conditional, who)
    temperature = calibration.check_temperature(temperature, who)
    report.check_inputs(cal_preds, cal_targets, who)
    dev = resample.device_for(cal_preds, who)
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        inp = _device_inputs(cal_preds, cal_targets, cal_preds, cal_targets, temperature, method, dev)
        counts = torch.empty((1, T, len(levels), RECORD), dtype=torch.int64, device=dev)
        thr = torch.empty((1, T, len(levels), MAX_CLASSES), dtype=torch.int64, device=dev)
        ops.conformal_counts(*inp, levels, counts, thr, conditional, 0, 0, point=True)
    return thr[0].cpu()


def conformal_report(preds, targets, cal_preds, cal_targets, alphas=DEFAULT_ALPHAS, method="lac", conditional="marginal",
                     temperature=None, refit=True, bootstrap=0, confidence=0.95, seed=0, chunk=None):
    """The conformal report of a test split under thresholds fitted on a calibration split.

    preds, targets: the test split, as report.evaluation_report; cal_preds, cal_targets: the calibration split.  alphas: the
    levels; method: "lac" or "aps"; conditional: "marginal" or "class"; temperature: None or 8 positive numbers, for both splits;
    refit: whether a replicate refits its thresholds; bootstrap, confidence, seed, chunk: as evaluation_report (chunk None: at
    most DEFAULT_CHUNK replicates per launch; every chunk gives the same bits).
    Returns {"counts" [8, A, 24] int64, "thresholds" [8, A, 5] int64, "label_values" [A, 5, 9], "class_values" [A, 2, 29],
    "threshold_values" [A, 8, 5] fp64, "threshold_inf" [A, 8, 5] bool, "label_metrics", "label_columns", "class_metrics",
    "class_columns", "alphas", "levels", "method", "conditional", "refit", "temperature", "targets", "cal_targets", "n",
    "n_cal"} and, with bootstrap > 0, for each table x of "label", "class", "threshold": x_replicates [B, ...] fp64, x_lo, x_hi
    fp64 and x_undefined int64 of the table's shape (threshold: the replicates with INF), and "bootstrap", "seed",
    "confidence".  All tensors on the CPU.  The inputs are not modified."""
    who = "conformal_report"
    report.check_settings(bootstrap, confidence, seed, chunk, who)
    alphas, levels = check_alphas(alphas, who)
    check_method(method, conditional, who)
    if not isinstance(refit, bool):
        raise ValueError(f"{who}: refit must be True or False, got {refit!r}")
    temperature = calibration.check_temperature(temperature, who)
    N, N_cal = _check_splits(preds, targets, cal_preds, cal_targets, who)
    dev = resample.device_for(preds, who)
    A = len(levels)
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        inp = _device_inputs(preds, targets, cal_preds, cal_targets, temperature, method, dev)
        fixed = []

        def launch(outs, seed, r0, point):
            ops.conformal_counts(*inp, levels, outs[0], outs[1], conditional, seed, r0, point=point,
                                 fixed_thr=None if point or refit else fixed[0])
            if point:
                fixed.append(outs[1][0].clone())  # the point thresholds: what refit = False counts every replicate under
        (pc, pt), (rc, rt) = resample.replicate_tables(launch, [(T, A, RECORD), (T, A, MAX_CLASSES)], bootstrap, seed, chunk,
                                                       DEFAULT_CHUNK, dev)
    return assemble(pc, pt, rc, rt, targets, cal_targets, alphas, levels, method, conditional, temperature, refit, bootstrap, seed,
                    confidence)


def assemble(counts, thr, rep_counts, rep_thr, targets, cal_targets, alphas, levels, method, conditional, temperature, refit,
             bootstrap=0, seed=0, confidence=0.95):
    """The report dict of conformal_report from the point tables counts [8, A, 24], thr [8, A, 5] and (with a bootstrap) the
    replicate tables [B, 8, A, 24], [B, 8, A, 5]: host arithmetic only."""
    N, N_cal = targets.shape[0], cal_targets.shape[0]
    counts, thr = np.asarray(counts, dtype=np.int64), np.asarray(thr, dtype=np.int64)
    v = values_from_counts(counts, thr, N)
    out = {"counts": torch.from_numpy(counts), "thresholds": torch.from_numpy(thr)}
    out.update({f"{x}_values": torch.from_numpy(v[f"{x}_values"]) for x in TABLES})
    out.update({"threshold_inf": torch.from_numpy(v["threshold_undefined"]),
                "label_metrics": list(LABEL_METRICS), "label_columns": list(LABEL_COLUMNS), "class_metrics": list(CLASS_METRICS),
                "class_columns": list(CLASS_COLUMNS), "alphas": list(alphas), "levels": [list(l) for l in levels], "method": method,
                "conditional": conditional, "refit": refit, "temperature": list(temperature),
                "targets": targets.detach().cpu().clone(), "cal_targets": cal_targets.detach().cpu().clone(), "n": N, "n_cal": N_cal})
    if bootstrap:
        rv = values_from_counts(rep_counts, rep_thr, N)
        resample.pack_intervals(out, [(f"{x}_", rv[f"{x}_values"], rv[f"{x}_undefined"].sum(axis=0)) for x in TABLES],
                                bootstrap, seed, confidence)
    return out


# ---- comparison and writers ----------------------------------------------------------------------------------------------
def compare(a, b):
    """The paired difference of two conformal reports of the SAME test cases and the SAME calibration cases (equal targets and
    cal_targets) with the same method, conditional, alphas, refit, bootstrap, seed and confidence (ValueError otherwise), so
    replicate r of both resamples the same cases of both splits.  Returns {"label_delta" [A, 5, 9], "class_delta" [A, 2, 29] = a
    - b, the names} and, with a bootstrap, x_lo, x_hi by the interval rule on the replicates' differences and x_frac_le_zero,
    for x in "label", "class", and "bootstrap", "seed", "confidence"."""
    resample.check_paired(a, b, "conformal_report", ("label_values", "targets", "cal_targets"),
                          (("method", "method differs ({} and {})"), ("conditional", "conditional differs ({} and {})"),
                           ("alphas", "alphas differ ({} and {})"), ("refit", "refit differs ({} and {})")))
    if tuple(a["cal_targets"].shape) != tuple(b["cal_targets"].shape) or not bool(torch.equal(a["cal_targets"], b["cal_targets"])):
        raise ValueError("compare: the two reports must be fitted on the same calibration cases (equal cal_targets)")
    out = {"label_delta": a["label_values"] - b["label_values"], "class_delta": a["class_values"] - b["class_values"],
           "label_metrics": list(LABEL_METRICS), "label_columns": list(LABEL_COLUMNS), "class_metrics": list(CLASS_METRICS),
           "class_columns": list(CLASS_COLUMNS), "alphas": list(a["alphas"]), "method": a["method"],
           "conditional": a["conditional"], "refit": a["refit"]}
    return resample.paired_intervals(out, a, b, ("label_", "class_"))


def _tables(rep):
    """(table name, row names, column names) of the two value tables."""
    return (("label", rep["label_metrics"], rep["label_columns"]), ("class", rep["class_metrics"], rep["class_columns"]))


def csv_rows(rep):
    """Long format: (table, alpha, row, column, value[, lo, hi, undefined]) of the two value tables, then of the thresholds
    (table "threshold", row = the label, column = the class)."""
    boot = "label_lo" in rep
    rows = []

    def add(name, a, r, c, idx):
        row = [name, rep["alphas"][a], r, c, float(rep[f"{name}_values"][idx])]
        if boot:
            row += [float(rep[f"{name}_lo"][idx]), float(rep[f"{name}_hi"][idx]), int(rep[f"{name}_undefined"][idx])]
        rows.append(row)
    for a in range(len(rep["alphas"])):
        for name, rnames, cnames in _tables(rep):
            for i, r in enumerate(rnames):
                for k, c in enumerate(cnames):
                    add(name, a, r, c, (a, i, k))
        for t, n in enumerate(NUM_CLASSES):
            for c in range(n):
                add("threshold", a, CLASSES_NAME[t], str(c + 1), (a, t, c))
    return rows


def to_csv(rep, path):
    """The long format of csv_rows with a header; repr of the fp64 values: they parse back exactly (inf as inf)."""
    resample.write_long_csv(path, "table,alpha,row,column,value" + (",lo,hi,undefined" if "label_lo" in rep else ""), csv_rows(rep))


def to_json(rep, path):
    """Everything but the replicates and the targets of both splits, as lists."""
    resample.write_json(rep, path, tuple(f"{x}_replicates" for x in TABLES) + ("targets", "cal_targets"))


def format_table(rep):
    """The two tables as text per level: one line per metric and column, six decimals, the interval in brackets."""
    lines = [f"conformal: {rep['method']} scores, {rep['conditional']} thresholds from {rep['n_cal']} cases"
             + ("" if rep["refit"] else ", fixed in the replicates") + ", temperature "
             + " ".join(f"{v:.4f}" for v in rep["temperature"])]
    for a, alpha in enumerate(rep["alphas"]):
        lines.append(f"alpha {alpha!r}")
        for name, rnames, cnames in _tables(rep):
            for i, r in enumerate(rnames):
                lines.append(f" {r}")
                for k, c in enumerate(cnames):
                    s = f"  {c:<10} {float(rep[name + '_values'][a, i, k]):9.6f}"
                    if f"{name}_lo" in rep:
                        s += f"  [{float(rep[name + '_lo'][a, i, k]):9.6f}, {float(rep[name + '_hi'][a, i, k]):9.6f}]"
                    lines.append(s)
    return "\n".join(lines)


def format_compare(cmp):
    lines = []
    for a, alpha in enumerate(cmp["alphas"]):
        lines.append(f"alpha {alpha!r}")
        for name in ("label", "class"):
            for i, r in enumerate(cmp[f"{name}_metrics"]):
                lines.append(f" {r} difference")
                for k, c in enumerate(cmp[f"{name}_columns"]):
                    s = f"  {c:<10} {float(cmp[name + '_delta'][a, i, k]):+9.6f}"
                    if f"{name}_lo" in cmp:
                        s += (f"  [{float(cmp[name + '_lo'][a, i, k]):+9.6f}, {float(cmp[name + '_hi'][a, i, k]):+9.6f}]"
                              f"  <= 0 in {float(cmp[name + '_frac_le_zero'][a, i, k]):.3f}")
                    lines.append(s)
    return "\n".join(lines)


# ---- what the command-line tool needs ------------------------------------------------------------------------------------
def add_flags(parser):
    """--conformal and its settings, for a tool that has a second split at hand (tools/eval_report.py: --fit-on)."""
    parser.add_argument("--conformal", action="store_true",
                        help="conformal prediction-set report: thresholds from --fit-on, coverage and set size of the predictions")
    parser.add_argument("--conformal-alpha", type=float, nargs="+", default=list(DEFAULT_ALPHAS), metavar="ALPHA",
                        help=f"miscoverage levels, 1 to {MAX_LEVELS} numbers in (0, 1)")
    parser.add_argument("--conformal-method", choices=METHODS, default="lac", help="score: 1 - p (lac) or adaptive sets (aps)")
    parser.add_argument("--conformal-conditional", choices=CONDITIONALS, default="marginal",
                        help="one threshold per label, or one per class (Mondrian)")
    parser.add_argument("--conformal-fixed", action="store_true",
                        help="keep the point thresholds in every bootstrap replicate instead of refitting them")
    parser.add_argument("--conformal-scaled", action="store_true",
                        help="divide the logits of both splits by the temperatures fitted on --fit-on")
    return parser


def check_flags(args):
    """The refusals of the flags that argparse does not make, before any work is done."""
    check_alphas(args.conformal_alpha, "--conformal-alpha")


def flag_settings(args):
    """The keyword arguments of conformal_report that the flags set (the temperature comes from the tool's own fit)."""
    return dict(alphas=args.conformal_alpha, method=args.conformal_method, conditional=args.conformal_conditional,
                refit=not args.conformal_fixed)


def save(rep, log_path, stem="val_conformal"):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(rep, log_path, stem, to_json, to_csv)


def stats_line(rep):
    """The one printed line: average coverage and mean set size per level (with the interval when the report has one)."""
    if rep is None:
        return f"no conformal report: more than MAX_CASES = {report.MAX_CASES} cases in a split"
    parts = []
    for a, alpha in enumerate(rep["alphas"]):
        for i, m in ((0, "coverage"), (1, "size")):
            s = f"{m}_AVG@{alpha!r} {float(rep['label_values'][a, i, T]):.4f}"
            if "label_lo" in rep:
                s += f" [{float(rep['label_lo'][a, i, T]):.4f}, {float(rep['label_hi'][a, i, T]):.4f}]"
            parts.append(s)
    return " ".join(parts)
