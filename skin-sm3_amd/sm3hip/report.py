"""Evaluation report of the 8 derm7pt labels: AUROC, Recall, Spec and Prec of every (label, class) column and the five averages of
the reference's result tables (linear_results.csv, finetune_results.csv; METRICS_NAME = ["AUC", "Recall", "Spec", "Prec"],
tools/backbone_eval.py:59,333-336, aggregated in src/utils/misc.py:299-327), with case-resampling bootstrap intervals.

Inputs: preds, 8 float tensors [N, n_t] (NaN is refused); targets [N, 8] int64.  Columns k = 0 .. 23 are the (label t, class c)
pairs, label-major in CLASSES_NAME order with NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2].

  * predicted class: yhat[n, t] = the lowest index of the row maximum (argmax; the reference calls torchmetrics with top_k = 1).
  * score of column (t, c): softmax(preds[t].double(), 1)[:, c], exactly as metrics.multiclass_auroc forms it, sorted ascending
    and stably ONCE per column; tie groups by == on the fp64 values; gs[j], ge[j] = first and one-past-last sorted position of
    position j's group.  The sort and the bounds are torch (plumbing).
  * counts per column, all int64, with integer case multiplicities m[n] >= 0, sum m = N (point estimate: m = 1):
        P = sum m[y == c],  Q = N - P,  S[j] = sum of m over the negative cases at sorted positions < j,
        A2 = sum over positive j of m_j * (S[gs[j]] + S[ge[j]])     (twice the negatives strictly below, plus the tied negatives),
        TP = sum m[y == c & yhat == c],  FP = sum m[y != c & yhat == c],  FN = sum m[y == c & yhat != c],  TN = N - TP - FP - FN.
  * values, fp64, each ONE IEEE division of two exactly represented integers and 0 when the denominator is 0 (torchmetrics' safe
    divide; what metrics.binary_auroc returns today):
        AUC = A2 / (2 P Q),  Recall = TP / (TP + FN),  Spec = TN / (TN + FP),  Prec = TP / (TP + FP).
    The tables' "Acc" row is the per-class recall.
  * averages, five per metric, each summed one column at a time in ascending column index, then one division:
        "8 all avg" all 24 columns; "8 avg" the 8 columns (t, CLS_WEIGHTS[t]) -- the reference's AUC_AVG, Recall_AVG, ...
        (misc.py:312-316); "7 all avg" the 19 non-DIAG columns; "7 avg" the 7 selected non-DIAG columns; "DIAG avg" DIAG's 5.
  * resampling and interval: the rule of resample.py.  ONE m_r is shared by all 24 columns and all four metrics, so the
    averages' intervals are joint.  undefined[metric, column] = the replicates whose denominator was 0 (their value is 0); for
    an average, the replicates in which any contributing column was undefined.

The counts come from sm3_report_counts (csrc/report.hip): one workgroup per replicate and label, integers only, so equal inputs give equal
bits; values, averages and order statistics are small and done on the host, adding one at a time (as faith.auc does).
N <= MAX_CASES (the multiplicities and the prefix sums of a replicate live in LDS)."""
import numpy as np
import torch

from . import ops, resample
from .metrics import CLASSES_NAME, CLS_WEIGHTS, NUM_CLASSES
from .resample import MAX_BOOTSTRAP, check_settings, interval, interval_index  # noqa: F401  (this module's names too)

MAX_CASES = ops.REPORT_MAX_CASES
METRICS = ("AUC", "Recall", "Spec", "Prec")
COLUMN_PAIRS = [(t, c) for t, n in enumerate(NUM_CLASSES) for c in range(n)]  # column k -> (label, class)
CLASS_COLUMNS = [f"{CLASSES_NAME[t]}-{c + 1}" for t, c in COLUMN_PAIRS]
SELECTED = [COLUMN_PAIRS.index((t, CLS_WEIGHTS[t])) for t in range(len(NUM_CLASSES))]  # the column (t, CLS_WEIGHTS[t]) of label t
_DIAG = [k for k, (t, _) in enumerate(COLUMN_PAIRS) if t == 0]
AVERAGES = {
    "8 all avg": list(range(len(COLUMN_PAIRS))),
    "8 avg": SELECTED,
    "7 all avg": [k for k in range(len(COLUMN_PAIRS)) if k not in _DIAG],
    "7 avg": [k for k in SELECTED if k not in _DIAG],
    "DIAG avg": _DIAG,
}
COLUMNS = CLASS_COLUMNS + list(AVERAGES)
K, NV = len(COLUMN_PAIRS), len(COLUMNS)  # 24, 29
# the column order of the reference's CSVs: the seven point labels by name, DIAG, the averages
CSV_COLUMNS = [n for lab in ("BWV", "DaG", "PIG", "PN", "RS", "STR", "VS", "DIAG") for n in CLASS_COLUMNS
               if n.split("-")[0] == lab] + list(AVERAGES)
CSV_ROWS = ("Acc",) + METRICS  # Acc = Recall
DEFAULT_CHUNK = 4096  # replicates per launch: a choice (4096 x 24 x 6 int64 = 4.5 MiB of counts)


def check_inputs(preds, targets, who="evaluation_report"):
    """Shapes, types and the size limit; returns N."""
    T = len(NUM_CLASSES)
    if not isinstance(preds, (list, tuple)) or len(preds) != T or not all(isinstance(p, torch.Tensor) for p in preds):
        raise ValueError(f"{who}: preds must be a list of {T} tensors [N, n_t]")
    if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int64 or targets.dim() != 2 or targets.shape[1] != T:
        raise ValueError(f"{who}: targets must be an int64 tensor [N, {T}]")
    N = targets.shape[0]
    if N < 1:
        raise ValueError(f"{who}: no cases")
    if N > MAX_CASES:
        raise ValueError(f"{who}: {N} cases, at most MAX_CASES = {MAX_CASES} are supported")
    for t, p in enumerate(preds):
        if not p.is_floating_point() or tuple(p.shape) != (N, NUM_CLASSES[t]):
            raise ValueError(f"{who}: preds[{t}] must be a float tensor [{N}, {NUM_CLASSES[t]}], got {tuple(p.shape)} {p.dtype}")
        if bool(torch.isnan(p).any()):
            raise ValueError(f"{who}: preds[{t}] holds a NaN (a NaN has no rank)")
    for t, n in enumerate(NUM_CLASSES):
        col = targets[:, t]
        if int(col.min()) < 0 or int(col.max()) >= n:
            raise ValueError(f"{who}: targets[:, {t}] must lie in [0, {n})")
    return N


def rank_scores(score):
    """score [K, N] fp64 -> (order, gs, ge [K, N] int32): each row sorted ascending and stably once, tie groups by ==, gs[j] / ge[j] =
    first and one-past-last sorted position of position j's group."""
    K, N = score.shape
    dev = score.device
    s, order = torch.sort(score, dim=1, stable=True)
    idx = torch.arange(N, device=dev).expand(K, N)
    new = s[:, 1:] != s[:, :-1]
    edge = torch.ones(K, 1, dtype=torch.bool, device=dev)
    first = torch.cat([edge, new], dim=1)  # position j opens a tie group
    last = torch.cat([new, edge], dim=1)   # position j closes one
    gs = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), dim=1).values
    ge = torch.cummin(torch.where(last, idx + 1, torch.full_like(idx, N)).flip(1), dim=1).values.flip(1)
    return order.int().contiguous(), gs.int().contiguous(), ge.int().contiguous()


def ranking(preds, targets):
    """The plumbing around the kernel, on the device of preds: (order, gs, ge [24, N] int32, yhat [N, 8] int32)."""
    score = torch.cat([torch.softmax(p.double(), dim=1).t() for p in preds], dim=0)  # [24, N]
    yhat = torch.stack([p.argmax(dim=1) for p in preds], dim=1)
    return (*rank_scores(score), yhat.int().contiguous())


def averages(v):
    """v [..., 24] fp64 -> the five averages [..., 5]: each summed one column at a time in ascending column index, then ONE
    division by the number of columns."""
    v = np.asarray(v, dtype=np.float64)
    out = np.empty(v.shape[:-1] + (len(AVERAGES),), dtype=np.float64)
    for a, cols in enumerate(AVERAGES.values()):
        acc = np.zeros(v.shape[:-1], dtype=np.float64)
        for k in cols:
            acc = acc + v[..., k]
        out[..., a] = acc / float(len(cols))
    return out


def values_from_counts(counts):
    """counts [..., 24, 6] int64 (A2, P, Q, TP, FP, FN) -> (values [..., 4, 29] fp64, undefined [..., 4, 29] bool)."""
    counts = np.asarray(counts, dtype=np.int64)
    A2, P, Q, TP, FP, FN = (counts[..., e] for e in range(6))
    TN = P + Q - TP - FP - FN
    nums = (A2, TP, TN, TP)
    dens = (2 * P * Q, TP + FN, TN + FP, TP + FP)
    values = np.zeros(counts.shape[:-2] + (len(METRICS), NV), dtype=np.float64)
    undefined = np.zeros(values.shape, dtype=bool)
    for i, (num, den) in enumerate(zip(nums, dens)):
        values[..., i, :K], undefined[..., i, :K] = resample.safe_div(num, den)
        values[..., i, K:] = averages(values[..., i, :K])
        for a, cols in enumerate(AVERAGES.values()):
            undefined[..., i, K + a] = undefined[..., i, cols].any(axis=-1)
    return values, undefined


def evaluation_report(preds, targets, bootstrap=0, confidence=0.95, seed=0, chunk=None):
    """The report of one set of predictions.

    preds: 8 float tensors [N, n_t] (logits; any float type, CPU or GPU); targets [N, 8] int64; N <= MAX_CASES.  bootstrap: B,
    the number of case-resampling replicates (0: point estimate only).  confidence: of the interval.  seed: the replicates are a
    function of (seed, r, N) alone.  chunk: replicates per launch (None: at most DEFAULT_CHUNK); every chunk gives the same bits.
    Returns {"counts": [24, 6] int64 (A2, P, Q, TP, FP, FN), "values": [4, 29] fp64 (rows AUC, Recall, Spec, Prec; columns the
    24 classes, then the five averages), "columns": the 29 names, "metrics", "targets": [N, 8] int64, "n": N} and, with
    bootstrap > 0, "replicates" [B, 4, 29] fp64, "lo", "hi" [4, 29] fp64, "undefined" [4, 29] int64, "bootstrap", "seed",
    "confidence".  All tensors on the CPU.  The inputs are not modified."""
    who = "evaluation_report"
    check_settings(bootstrap, confidence, seed, chunk, who)
    N = check_inputs(preds, targets, who)
    dev = resample.device_for(preds, who)
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        order, gs, ge, yhat = ranking([p.detach().to(dev) for p in preds], targets.to(dev))
        y = targets.to(dev).int().contiguous()
        colmap = torch.tensor(COLUMN_PAIRS, dtype=torch.int32, device=dev)
        (point,), (reps,) = resample.replicate_tables(
            lambda outs, seed, r0, point: ops.report_counts(order, gs, ge, y, yhat, colmap, outs[0], seed, r0, point=point),
            [(K, 6)], bootstrap, seed, chunk, DEFAULT_CHUNK, dev)
    values, _ = values_from_counts(point)
    out = {"counts": torch.from_numpy(point), "values": torch.from_numpy(values), "columns": list(COLUMNS),
           "metrics": list(METRICS), "targets": targets.detach().cpu().clone(), "n": N}
    if bootstrap:
        rv, ru = values_from_counts(reps)
        resample.pack_intervals(out, [("", rv, ru.sum(axis=0))], bootstrap, seed, confidence)
    return out


def compare(a, b):
    """The paired difference of two reports of the SAME cases: equal targets, bootstrap and seed (ValueError otherwise), so
    replicate r of both resamples the same cases.  Returns {"delta": a.values - b.values [4, 29], "columns", "metrics"} and,
    with a bootstrap, "lo", "hi" by the interval rule on a.replicates - b.replicates, "frac_le_zero" [4, 29] = the fraction of
    replicates with a difference <= 0, "bootstrap", "seed", "confidence"."""
    resample.check_paired(a, b, "evaluation_report", ("values", "targets"))
    return resample.paired_intervals({"delta": a["values"] - b["values"], "columns": list(COLUMNS), "metrics": list(METRICS)}, a, b)


def selected(report, metric):
    """The reference's per-label stat of `metric` ("AUC", "Recall", "Spec", "Prec"): {"<metric>_<label>": value of the column (t,
    CLS_WEIGHTS[t])} for the 8 labels and "<metric>_AVG" = "8 avg"."""
    row = report["values"][METRICS.index(metric)]
    stat = {f"{metric}_{n}": float(row[k]) for n, k in zip(CLASSES_NAME, SELECTED)}
    stat[f"{metric}_AVG"] = float(row[COLUMNS.index("8 avg")])
    return stat


def csv_rows(report):
    """The rows of the reference's table layout: [(name, [29 values in CSV_COLUMNS order, percent])], Acc = Recall first; with a
    bootstrap each metric row is followed by its "<name> lo" and "<name> hi" rows."""
    perm = [COLUMNS.index(n) for n in CSV_COLUMNS]
    rows = []
    for name in CSV_ROWS:
        i = METRICS.index("Recall" if name == "Acc" else name)
        rows.append((name, [100.0 * float(report["values"][i, k]) for k in perm]))
        if "lo" in report:
            for end in ("lo", "hi"):
                rows.append((f"{name} {end}", [100.0 * float(report[end][i, k]) for k in perm]))
    return rows


def to_csv(report, path):
    """Write the reference's layout (linear_results.csv): a header of CSV_COLUMNS, rows Acc, AUC, Recall, Spec, Prec in percent
    (repr of the fp64 values: they parse back exactly), the lo / hi rows after each when the report has a bootstrap."""
    with open(path, "w") as f:
        f.write("," + ",".join(CSV_COLUMNS) + "\n")
        for name, vals in csv_rows(report):
            f.write(name + "," + ",".join(repr(v) for v in vals) + "\n")


def to_json(report, path):
    """Everything but the replicates and the targets, as lists."""
    resample.write_json(report, path, ("replicates", "targets"))


def format_table(report):
    """The table as text: one line per metric and column group, percent with two decimals, the interval in brackets."""
    lines = []
    for i, m in enumerate(METRICS):
        lines.append(m)
        for k, name in enumerate(COLUMNS):
            s = f"  {name:<10} {100.0 * float(report['values'][i, k]):7.2f}"
            if "lo" in report:
                s += f"  [{100.0 * float(report['lo'][i, k]):6.2f}, {100.0 * float(report['hi'][i, k]):6.2f}]"
                if int(report["undefined"][i, k]):
                    s += f"  undefined in {int(report['undefined'][i, k])} of {report['bootstrap']}"
            lines.append(s)
    return "\n".join(lines)


def format_compare(cmp):
    lines = []
    for i, m in enumerate(cmp["metrics"]):
        lines.append(f"{m} difference")
        for k, name in enumerate(cmp["columns"]):
            s = f"  {name:<10} {100.0 * float(cmp['delta'][i, k]):+7.2f}"
            if "lo" in cmp:
                s += (f"  [{100.0 * float(cmp['lo'][i, k]):+6.2f}, {100.0 * float(cmp['hi'][i, k]):+6.2f}]"
                      f"  <= 0 in {float(cmp['frac_le_zero'][i, k]):.3f}")
            lines.append(s)
    return "\n".join(lines)


# ---- what the command-line tools share ----------------------------------------------------------------------------------
def add_flags(parser):
    """--bootstrap / --bootstrap-seed / --confidence of the evaluation tools."""
    return resample.add_bootstrap_flags(parser, " of the last validation pass's report")


def save(report, log_path, stem="val_report"):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(report, log_path, stem, to_json, to_csv)


def validation_stats(preds, targets, args, final, log_path=None):
    """What a tool adds to the stat dict of a validation pass: Recall_*, Spec_*, Prec_* of the 8 labels (class CLS_WEIGHTS[t])
    and their _AVG.  final: the last pass -- with --bootstrap its intervals, and val_report.json / .csv under log_path.  Beyond
    MAX_CASES cases: ({}, None), which stats_line words."""
    if targets.shape[0] > MAX_CASES:  # the tools ran at such sizes before the report existed: they keep running, and say so
        return {}, None
    rep = evaluation_report(list(preds), targets, bootstrap=args.bootstrap if final else 0, confidence=args.confidence,
                            seed=args.bootstrap_seed)
    stat = {}
    for m in METRICS[1:]:
        stat.update(selected(rep, m))
    if final and log_path is not None:
        save(rep, log_path)
    return stat, rep


def stats_line(stat, rep=None):
    """The one printed line of the three new averages (with the interval when the report has one)."""
    if rep is None:
        return f"no Recall / Spec / Prec report: more than MAX_CASES = {MAX_CASES} cases"
    parts = []
    for i, m in enumerate(METRICS):
        if m == "AUC":
            continue
        s = f"{m}_AVG {stat[m + '_AVG']:.4f}"
        if rep is not None and "lo" in rep:
            k = COLUMNS.index("8 avg")
            s += f" [{float(rep['lo'][i, k]):.4f}, {float(rep['hi'][i, k]):.4f}]"
        parts.append(s)
    return " ".join(parts)


def load_predictions(path, device="cpu"):
    """(preds, targets) of a val_predictions.pt (backbone_eval, mlc_eval: "preds" logits) or a knn_predictions.pt (backbone_knn:
    "votes", scored as log(votes / sum votes), whose softmax is the vote fraction), on `device` (the logarithm is taken there:
    on the GPU it is the one backbone_knn took)."""
    d = torch.load(path, map_location=device, weights_only=False)
    if "preds" in d:
        preds = [p for p in d["preds"]]
    elif "votes" in d:
        preds = [(v.double() / v.double().sum(dim=1, keepdim=True)).log() for v in d["votes"]]
    else:
        raise ValueError(f"{path}: neither 'preds' (val_predictions.pt) nor 'votes' (knn_predictions.pt)")
    return preds, d["targets"].long()
