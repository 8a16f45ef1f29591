"""Seven-point checklist report of the 8 derm7pt labels: the seven criteria heads added up to the checklist score, and how well
that score finds melanoma -- beside the DIAG head, and beside the score of the annotated criteria -- with case-resampling
bootstrap intervals that share their replicates with the other four reports (resample.py: the rule).

The points (POINTS) are the `scores` of the reference's label tables (src/utils/data/datasets.py:65-113, and :454-474 for the
grouped VS, PIG and RS that its dataset uses); tests/golden/checklist_points.json holds them as the reference states them.  Per
criterion exactly ONE grouped class scores, and it is class CLS_WEIGHTS[t] -- the class whose column the reference's "8 avg"
selects; asserted below.  p_t = the points of label t (2, 2, 2, 1, 1, 1, 1 for PN, BWV, VS, PIG, STR, DaG, RS; MAX_SCORE = 10).

Inputs (as evaluation_report): preds, 8 float tensors [N, n_t] (NaN is refused); targets [N, 8] int64; 1 <= N <= MAX_CASES.

  * per case, on the host, in a fixed order:
        s*[n]  = sum over t = 1 .. 7 of POINTS[t][y[n, t]]                       (true_scores; 0 .. 10)
        shat[n] = the same sum over yhat[n, t], the lowest index of the row maximum (predicted_scores; report.ranking's yhat)
        q_t[n] = softmax(preds[t].double(), 1)[:, CLS_WEIGHTS[t]]                 (criterion_probabilities)
        pi[n]  = the distribution of the score IF THE SEVEN CRITERIA WERE INDEPENDENT given the image (score_distribution): from
                 pi = delta_0, for t = 1 .. 7 in label order pi[s] <- pi[s] * (1 - q_t) + pi[s - p_t] * q_t
        E[n]   = sum over t of p_t * q_t in label order (expected_score);  T_k[n] = sum of pi[s] over s = k .. 10 in ascending s
                 (tail_probability)
  * five rankings of the cases for "is it melanoma" (MELANOMA: y[:, 0] == 2): RANKINGS = "hard" shat, "annotated" s* (the ceiling:
    what the rule gives with perfect criteria), "expected" E, "tail" T_k for the first entry of `thresholds`, "diag" the DIAG
    head's softmax column 2 -- bit for bit the score of evaluation_report's column DIAG-3.  The three continuous ones are sorted
    once, ascending and stably, with == tie groups (report.rank_scores); the two integer ones need no sort.
  * counts, all int64, with integer case multiplicities m[n] >= 0, sum m = N (point estimate m = 1, replicate r the m_r of the
    rule): the joint table J[shat][s*][mel] and (A2, P, Q) of the three continuous rankings as report.py defines them, positive
    = melanoma -- one record of 242 + 9 entries from sm3_checklist_counts (csrc/checklist.hip).
  * values (values_from_counts), fp64, each ONE IEEE division of two exactly represented integers (resample.safe_div), 0 and
    `undefined` when the denominator is 0:
        AUC of the five rankings, A2 / (2 P Q); for an integer ranking from J's marginals pos[v], neg[v] of its score value v:
            A2 = sum over v of pos[v] * (2 * neg_below[v] + neg[v]);
        the paired gaps "diag-expected", "diag-hard", "annotated-hard": differences of two AUCs of the same replicate, undefined
            when either is;
        the rule "score >= k => melanoma", k = 1 .. 10, for shat ("pred>=k") and s* ("true>=k"): sens = TP / P, spec = TN / Q,
            PPV = TP / (TP + FP), NPV = TN / (TN + FN);
        the agreement of shat with s*, O = J summed over mel, r / c its row / column sums: "exact" sum O_ii / N, "within1" sum
            over |i - j| <= 1 of O_ij / N, "MAE" sum |i - j| O_ij / N, "bias" sum (i - j) O_ij / N, and the quadratic weighted
            "kappa" 1 - N sum w_ij O_ij / sum w_ij r_i c_j, w = (i - j)^2: int64 throughout, then one division and one
            subtraction; undefined when the denominator is 0 (one score value only).
    `thresholds` (default (1, 3): the revised and the classical cut) picks the rule rows shown in the table and the CSV; the JSON
    holds all ten.

The counts are integers, so equal inputs give equal bits whatever the chunk."""
import numpy as np
import torch

from . import ops, report, resample
from .metrics import CLASSES_NAME, CLS_WEIGHTS, NUM_CLASSES
from .resample import safe_div as _div

# points of grouped class c of label t; label 0 (DIAG) is no criterion
POINTS = ([0, 0, 0, 0, 0], [0, 0, 2], [0, 2], [0, 0, 2], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1])
MAX_SCORE = 10
MELANOMA = (0, 2)  # (label, class): DIAG's class MEL
CRITERIA = tuple(range(1, len(NUM_CLASSES)))
LABEL_POINTS = [POINTS[t][CLS_WEIGHTS[t]] for t in range(len(NUM_CLASSES))]  # p_t
assert [len(p) for p in POINTS] == NUM_CLASSES and not any(POINTS[0])
assert all(p > 0 and sum(v != 0 for v in POINTS[t]) == 1 for t, p in enumerate(LABEL_POINTS) if t), \
    "the scoring class of every criterion is CLS_WEIGHTS[t]"
assert sum(LABEL_POINTS) == MAX_SCORE and MELANOMA[1] == CLS_WEIGHTS[MELANOMA[0]]

NS = MAX_SCORE + 1                  # score values 0 .. 10
BINS = NS * NS * 2                  # J[shat][s*][mel]
RECORD = ops.CHECKLIST_RECORD       # 242 + 3 * 3
RANKINGS = ("hard", "annotated", "expected", "tail", "diag")
CONTINUOUS = ("expected", "tail", "diag")   # record order of the three (A2, P, Q)
GAPS = (("diag", "expected"), ("diag", "hard"), ("annotated", "hard"))
RULE_METRICS = ("sens", "spec", "PPV", "NPV")
AGREEMENT = ("exact", "within1", "MAE", "bias", "kappa")
DEFAULT_THRESHOLDS = (1, 3)
DEFAULT_CHUNK = 4096  # replicates per launch: a choice (4096 x 251 int64 = 7.8 MiB of records)
COLUMNS = ["value"]
MAX_CASES = report.MAX_CASES
assert RECORD == BINS + 3 * len(CONTINUOUS)


# ---- settings -----------------------------------------------------------------------------------------------------------------
def check_thresholds(thresholds, who="checklist_report"):
    """A non-empty list of distinct integers in 1 .. MAX_SCORE -> list of ints; needs neither a tensor nor a device."""
    if resample.is_int(thresholds):
        thresholds = [thresholds]
    try:
        th = list(thresholds)
    except TypeError:
        raise ValueError(f"{who}: thresholds must be a list of integers in [1, {MAX_SCORE}], got {thresholds!r}") from None
    if not th:
        raise ValueError(f"{who}: thresholds is empty (its first entry is the tail ranking's cut)")
    for k in th:
        if not resample.is_int(k) or not 1 <= k <= MAX_SCORE:
            raise ValueError(f"{who}: every threshold must be an integer in [1, {MAX_SCORE}], got {k!r}")
    if len(set(th)) != len(th):
        raise ValueError(f"{who}: thresholds holds duplicates: {th}")
    return th


# ---- per case -----------------------------------------------------------------------------------------------------------------
def _points_of(classes):
    """classes [N, 8] integer -> the checklist score [N] int64: label 1 first, one label added at a time."""
    score = torch.zeros(classes.shape[0], dtype=torch.int64, device=classes.device)
    for t in CRITERIA:
        score = score + torch.tensor(POINTS[t], dtype=torch.int64, device=classes.device)[classes[:, t].long()]
    return score


def true_scores(targets):
    """s* [N] int64: the checklist score of the annotated criteria."""
    return _points_of(targets)


def predicted_scores(preds):
    """shat [N] int64: the checklist score of the predicted classes (the lowest index of the row maximum)."""
    return _points_of(torch.stack([p.argmax(dim=1) for p in preds], dim=1))


def criterion_probabilities(preds):
    """q [N, 8] fp64: q[:, t] = softmax(preds[t].double(), 1)[:, CLS_WEIGHTS[t]] (column 0, DIAG's, is the melanoma score)."""
    return torch.stack([torch.softmax(p.double(), dim=1)[:, CLS_WEIGHTS[t]] for t, p in enumerate(preds)], dim=1)


def score_distribution(preds):
    """pi [N, 11] fp64: the distribution of the checklist score under the ASSUMPTION THAT THE SEVEN CRITERIA ARE INDEPENDENT given
    the image -- the heads are trained jointly and the criteria correlate, so this is a model, not a fact; the report ranks by
    it and never reads it as a calibrated probability.  From pi = delta_0, for t = 1 .. 7 in label order: pi[s] <- pi[s] * (1 -
    q_t) + pi[s - p_t] * q_t, every product and sum rounded on its own."""
    q = criterion_probabilities(preds)
    pi = torch.zeros(q.shape[0], NS, dtype=torch.float64, device=q.device)
    pi[:, 0] = 1.0
    for t in CRITERIA:
        p, qt = LABEL_POINTS[t], q[:, t:t + 1]
        stay = pi * (1.0 - qt)
        move = torch.zeros_like(pi)
        move[:, p:] = pi[:, :NS - p] * qt
        pi = stay + move
    return pi


def expected_score(preds):
    """E [N] fp64 = sum over t = 1 .. 7 of p_t * q_t, one label added at a time in label order."""
    q = criterion_probabilities(preds)
    e = torch.zeros(q.shape[0], dtype=torch.float64, device=q.device)
    for t in CRITERIA:
        e = e + float(LABEL_POINTS[t]) * q[:, t]
    return e


def tail_probability(pi, k):
    """T_k [N] fp64 = sum of pi[:, s] over s = k .. 10, one at a time in ascending s."""
    tail = torch.zeros(pi.shape[0], dtype=torch.float64, device=pi.device)
    for s in range(k, NS):
        tail = tail + pi[:, s]
    return tail


def pack_cases(shat, sstar, mel):
    """shat | sstar << 4 | mel << 8 as int32 [N]: the case word of sm3_checklist_counts."""
    return (shat | (sstar << 4) | (mel.long() << 8)).int().contiguous()


# ---- the record of sm3_checklist_counts -----------------------------------------------------------------------------------------
def row_names(thresholds=DEFAULT_THRESHOLDS):
    """The rows of the value table; only the tail ranking's name depends on the thresholds."""
    auc = [f"AUC {r}" if r != "tail" else f"AUC tail>={thresholds[0]}" for r in RANKINGS]
    return (auc + [f"AUC {a}-{b}" for a, b in GAPS]
            + [f"{src}>={k} {m}" for src in ("pred", "true") for k in range(1, NS) for m in RULE_METRICS]
            + [f"agree {a}" for a in AGREEMENT])


def shown_rows(rows, thresholds):
    """Indices of the rows that the table and the CSV show: everything but the rule rows of a k outside `thresholds`."""
    keep = {f"{src}>={k}" for src in ("pred", "true") for k in thresholds}
    return [i for i, r in enumerate(rows) if ">=" not in r or r.startswith("AUC ") or r.split(" ")[0] in keep]


def values_from_counts(counts):
    """counts [..., 251] int64 -> (values [..., 93] fp64, undefined [..., 93] bool), rows as row_names."""
    counts = np.asarray(counts, dtype=np.int64)
    lead = counts.shape[:-1]
    J = counts[..., :BINS].reshape(lead + (NS, NS, 2))
    marg = {"hard": J.sum(axis=-2), "annotated": J.sum(axis=-3)}  # [..., 11 score values, mel]
    auc = {}
    for name, mv in marg.items():
        neg, pos = mv[..., 0], mv[..., 1]
        below = np.cumsum(neg, axis=-1) - neg
        auc[name] = _div((pos * (2 * below + neg)).sum(axis=-1), 2 * pos.sum(axis=-1) * neg.sum(axis=-1))
    for i, name in enumerate(CONTINUOUS):
        A2, P, Q = (counts[..., BINS + 3 * i + e] for e in range(3))
        auc[name] = _div(A2, 2 * P * Q)
    series = [auc[r] for r in RANKINGS]
    series += [(auc[a][0] - auc[b][0], auc[a][1] | auc[b][1]) for a, b in GAPS]
    for name in ("hard", "annotated"):
        neg, pos = marg[name][..., 0], marg[name][..., 1]
        P, Q = pos.sum(axis=-1), neg.sum(axis=-1)
        for k in range(1, NS):
            TP, FP = pos[..., k:].sum(axis=-1), neg[..., k:].sum(axis=-1)
            TN, FN = Q - FP, P - TP
            series += [_div(TP, P), _div(TN, Q), _div(TP, TP + FP), _div(TN, TN + FN)]
    O = J.sum(axis=-1)
    N = O.sum(axis=(-1, -2))
    d = np.arange(NS)[:, None] - np.arange(NS)[None, :]  # i - j: predicted minus annotated
    r, c = O.sum(axis=-1), O.sum(axis=-2)
    for w in ((d == 0), (np.abs(d) <= 1), np.abs(d), d):
        series.append(_div((O * w.astype(np.int64)).sum(axis=(-1, -2)), N))
    w = d * d
    ratio, undefined = _div(N * (O * w).sum(axis=(-1, -2)), (w * (r[..., :, None] * c[..., None, :])).sum(axis=(-1, -2)))
    series.append((np.where(undefined, 0.0, 1.0 - ratio), undefined))
    values = np.stack([np.where(u, 0.0, v) for v, u in series], axis=-1)
    return values, np.stack([np.broadcast_to(u, v.shape) for v, u in series], axis=-1)


# ---- the report ---------------------------------------------------------------------------------------------------------------
def checklist_report(preds, targets, thresholds=DEFAULT_THRESHOLDS, bootstrap=0, confidence=0.95, seed=0, chunk=None):
    """The seven-point checklist report of one set of predictions.

    preds, targets: as report.evaluation_report.  thresholds: distinct integers k in 1 .. 10, the cuts "score >= k => melanoma"
    shown in the table and the CSV; the first is the tail ranking's k.  bootstrap, confidence, seed, chunk: as evaluation_report
    (chunk None: at most DEFAULT_CHUNK replicates per launch; every chunk gives the same bits).
    Returns {"counts" [251] int64 (the record of sm3_checklist_counts), "values" [rows, 1] fp64, "point_undefined" [rows, 1] bool,
    "rows", "columns" (["value"]), "shown" (indices of the rows of the table and the CSV), "thresholds", "scores" {"predicted":
    shat, "annotated": s*} int64 [N], "targets", "n"} and, with bootstrap > 0, "replicates" [B, rows, 1] fp64,
    "replicate_counts" [B, 251] int64, "lo", "hi" [rows, 1] fp64, "undefined" [rows, 1] int64, "bootstrap", "seed", "confidence".
    All tensors on the CPU.  The inputs are not modified."""
    who = "checklist_report"
    report.check_settings(bootstrap, confidence, seed, chunk, who)
    thresholds = check_thresholds(thresholds, who)
    report.check_inputs(preds, targets, who)
    dev = resample.device_for(preds, who)
    with torch.cuda.device(dev), ops.stream_scope():
        return _report(preds, targets, thresholds, bootstrap, confidence, seed, chunk, dev, ops.checklist_counts)


def case_inputs(preds, targets, thresholds):
    """What the kernel reads, on the device of preds: (packed [N] int32, order, gs, ge [3, N] int32, shat, s* [N] int64); the
    rankings in CONTINUOUS order."""
    shat, sstar = predicted_scores(preds), true_scores(targets)
    mel = targets[:, MELANOMA[0]] == MELANOMA[1]
    pi, e = score_distribution(preds), expected_score(preds)
    diag = torch.softmax(preds[MELANOMA[0]].double(), dim=1)[:, MELANOMA[1]]
    order, gs, ge = report.rank_scores(torch.stack([e, tail_probability(pi, thresholds[0]), diag], dim=0))
    return pack_cases(shat, sstar, mel), order, gs, ge, shat, sstar


def _report(preds, targets, thresholds, bootstrap, confidence, seed, chunk, dev, counts_fn):
    """checklist_report after its checks, on the device dev, with the counts from counts_fn (ops.checklist_counts)."""
    N = targets.shape[0]
    with torch.no_grad():
        packed, order, gs, ge, shat, sstar = case_inputs([p.detach().to(dev) for p in preds], targets.to(dev), thresholds)
        (point,), (reps,) = resample.replicate_tables(
            lambda outs, seed, r0, point: counts_fn(packed, order, gs, ge, outs[0], seed, r0, point=point),
            [(RECORD,)], bootstrap, seed, chunk, DEFAULT_CHUNK, dev)
    values, undefined = values_from_counts(point)
    rows = row_names(thresholds)
    out = {"counts": torch.from_numpy(point), "values": torch.from_numpy(values[:, None].copy()),
           "point_undefined": torch.from_numpy(undefined[:, None].copy()), "rows": rows, "columns": list(COLUMNS),
           "shown": shown_rows(rows, thresholds), "thresholds": list(thresholds),
           "scores": {"predicted": shat.cpu(), "annotated": sstar.cpu()},
           "targets": targets.detach().cpu().clone(), "n": N}
    if bootstrap:
        rv, ru = values_from_counts(reps)
        boot = resample.pack_intervals({}, [("", rv[:, :, None].copy(), ru.sum(axis=0)[:, None])], bootstrap, seed, confidence)
        out.update({"replicates": boot.pop("replicates"), "replicate_counts": torch.from_numpy(reps)}, **boot)
    return out


# ---- comparison and writers -----------------------------------------------------------------------------------------------------
def compare(a, b):
    """The paired difference of two checklist reports of the SAME cases with the same thresholds: equal targets, rows, bootstrap,
    seed and confidence (ValueError otherwise), so replicate r of both resamples the same cases.  Returns {"delta": a.values -
    b.values [rows, 1], "rows", "columns", "shown"} and, with a bootstrap, "lo", "hi" by the interval rule on a.replicates -
    b.replicates, "frac_le_zero", "bootstrap", "seed", "confidence"."""
    resample.check_paired(a, b, "checklist_report", ("values", "targets", "rows", "thresholds"),
                          (("thresholds", "the two reports use different thresholds ({} and {})"),))
    return resample.paired_intervals({"delta": a["values"] - b["values"], "rows": list(a["rows"]), "columns": list(a["columns"]),
                                      "shown": list(a["shown"])}, a, b)


def csv_rows(rep):
    """Long format: (row, value[, lo, hi, undefined]) of the shown rows."""
    rows = []
    for i in rep["shown"]:
        row = [rep["rows"][i], float(rep["values"][i, 0])]
        if "lo" in rep:
            row += [float(rep["lo"][i, 0]), float(rep["hi"][i, 0]), int(rep["undefined"][i, 0])]
        rows.append(row)
    return rows


def to_csv(rep, path):
    """The long format of csv_rows with a header; repr of the fp64 values: they parse back exactly."""
    resample.write_long_csv(path, "row,value" + (",lo,hi,undefined" if "lo" in rep else ""), csv_rows(rep))


def to_json(rep, path):
    """Everything but the replicates and the targets, as lists: every row, the rules of all ten cuts among them."""
    resample.write_json(rep, path, ("replicates", "replicate_counts", "targets"))


def format_table(rep):
    """The shown rows as text, four decimals, the interval in brackets and the undefined replicates where there are any."""
    lines = [f"seven-point checklist, {rep['n']} cases"]
    for i in rep["shown"]:
        s = f"  {rep['rows'][i]:<22} {float(rep['values'][i, 0]):8.4f}"
        if "lo" in rep:
            s += f"  [{float(rep['lo'][i, 0]):.4f}, {float(rep['hi'][i, 0]):.4f}]"
            if int(rep["undefined"][i, 0]):
                s += f"  undefined in {int(rep['undefined'][i, 0])} of {rep['bootstrap']}"
        elif bool(rep["point_undefined"][i, 0]):
            s += "  undefined"
        lines.append(s)
    return "\n".join(lines)


def format_compare(cmp):
    lines = ["difference"]
    for i in cmp["shown"]:
        s = f"  {cmp['rows'][i]:<22} {float(cmp['delta'][i, 0]):+8.4f}"
        if "lo" in cmp:
            s += (f"  [{float(cmp['lo'][i, 0]):+.4f}, {float(cmp['hi'][i, 0]):+.4f}]"
                  f"  <= 0 in {float(cmp['frac_le_zero'][i, 0]):.3f}")
        lines.append(s)
    return "\n".join(lines)


# ---- what the command-line tools share ----------------------------------------------------------------------------------------
def add_flags(parser):
    """--checklist / --checklist-thresholds of the evaluation tools."""
    parser.add_argument("--checklist", action="store_true",
                        help="seven-point checklist report (melanoma by the score of the predicted criteria, beside the DIAG "
                             "head and the annotated score) of the predictions")
    parser.add_argument("--checklist-thresholds", type=int, nargs="+", default=list(DEFAULT_THRESHOLDS),
                        help=f"the cuts 'score >= k' shown, distinct integers in [1, {MAX_SCORE}]; the first is the tail ranking's")
    return parser


def check_flags(args):
    """The refusals of the flags that argparse does not make, before any work is done."""
    check_thresholds(args.checklist_thresholds, "--checklist-thresholds")


def flag_settings(args):
    return dict(thresholds=args.checklist_thresholds)


def save(rep, log_path, stem="val_checklist"):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(rep, log_path, stem, to_json, to_csv)


def stats_line(rep):
    """The one printed line: the melanoma AUC by the hard score, by the DIAG head and by the annotated score, and kappa."""
    if rep is None:
        return f"no checklist report: more than MAX_CASES = {MAX_CASES} cases"
    parts = []
    for name in ("AUC hard", "AUC diag", "AUC annotated", "agree kappa"):
        i = rep["rows"].index(name)
        s = f"checklist_{name.replace(' ', '_')} {float(rep['values'][i, 0]):.4f}"
        if "lo" in rep:
            s += f" [{float(rep['lo'][i, 0]):.4f}, {float(rep['hi'][i, 0]):.4f}]"
        parts.append(s)
    return " ".join(parts)


def validation_checklist(preds, targets, args, log_path):
    """What a tool does under --checklist after its last validation pass: the report with the tool's --checklist-thresholds and its
    --bootstrap, --bootstrap-seed and --confidence, written as val_checklist.json / .csv under log_path.  Beyond MAX_CASES
    cases: None, which stats_line words."""
    if targets.shape[0] > MAX_CASES:
        return None
    rep = checklist_report(list(preds), targets, bootstrap=args.bootstrap, confidence=args.confidence, seed=args.bootstrap_seed,
                           **flag_settings(args))
    save(rep, log_path)
    return rep
