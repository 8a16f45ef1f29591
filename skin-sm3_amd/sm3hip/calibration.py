"""Calibration report of the 8 derm7pt labels: negative log-likelihood, Brier score, expected and maximum calibration error of
the top label, class-wise ECE of every (label, class) column and the five averages of report.AVERAGES, the reliability diagram,
temperature scaling, and case-resampling bootstrap intervals that share their replicates with report.evaluation_report.

Inputs (as evaluation_report): preds, 8 float tensors [N, n_t] (NaN is refused); targets [N, 8] int64; optional temperature, 8
positive floats (default all 1); 1 <= N <= report.MAX_CASES.

  * per case and label t (torch, on the device of the tensors: plumbing, as the ranking of report.py):
        z = preds[t].double() / T_t (a division),  p = softmax(z, 1),  lp = log_softmax(z, 1),
        yhat = the lowest index of the row maximum of preds[t], as in the report.
    Every value below becomes an int64 in Q32, rint(x * 2^32) (round half to even):
        q_top[n, t] = p[n, yhat], event e_top = (yhat == y);
        q_cls[n, k] = p[n, c] for every column k = (t, c) of report.COLUMN_PAIRS, event e_cls = (y == c);
        q_nll[n, t] = min(-lp[n, y], 1024)         (the clamp keeps every later sum below 2^56);
        q_br[n, t]  = sum over c of (p[n, c] - [y == c])^2, added one class at a time in ascending class index.
  * a series is a pair (q [N] int64, e [N] 0/1).  S = 32 series: s = 0 .. 7 the top-label series of the labels, s = 8 + k the
    class-wise series of column k.  X = 16 plain sums: x = t is q_nll, x = 8 + t is q_br of label t.
  * multiplicities: integers m[n] >= 0, sum m = N; the point estimate has m = 1, replicate r the m_r of resample.py's rule.
    With one seed, replicate r here resamples the same cases as replicate r of evaluation_report: the intervals of
    discrimination and calibration are joint, and comparisons are paired.
  * bins: M of them, 1 <= M <= MAX_BINS = 64, default 15.
        binning = "width": a case's bin is min((q * M) >> 32, M - 1) in 64-bit integers (q = 2^32, a probability of exactly 1,
                           lands in bin M - 1; a value on an inner edge in the upper bin);
        binning = "mass":  equal-mass, rank-based.  The series' cases sorted ascending by q, ties by ascending case index (one
                           stable torch sort per series, done once: order [S, N] int32).  The case at sorted position j owns the
                           copy ranks [R_j, R_j + m_j), R_j = the sum of m over the positions < j; the copy at rank u goes to bin
                           (u * M) / N (integer division).  A case whose ranks straddle a boundary is split between the bins
                           copy by copy; M > N leaves empty bins.
    Per series and bin three int64: n_b = the copies in the bin, E_b = the sum of their events, Q_b = the sum of their q.
    Per plain sum: sum over n of m[n] * q[n].  Everything is an integer, so no summation order shows.
  * values, fp64, on the host, each ONE IEEE division of two integers and 0 when the denominator is 0:
        gap_b = Q_b - E_b * 2^32,   ECE = (sum_b |gap_b|) / (N * 2^32),   MCE = max over the non-empty b of |gap_b| / (n_b * 2^32),
        NLL = sum / (N * 2^32),   Brier = sum / (N * 2^32),   acc_b = E_b / n_b,   conf_b = Q_b / (n_b * 2^32).
    Every integer here is below 2^53 and so exact in fp64, but the NLL sum where the mean NLL exceeds 2^53 / (N * 2^32) (256
    at N = 8192): int64 -> fp64 then rounds it once, to nearest, which is still a function of the integer alone.
  * tables: label_values [4, 9], rows NLL, Brier, ECE, MCE of the top-label series, columns the 8 labels and "AVG" (summed in
    ascending label order, then ONE division by 8); class_values [1, 29], the class-wise ECE of the 24 columns and the five
    averages of report.AVERAGES (report.averages); diagram [32, M, 3] = (n_b, acc_b, conf_b).
  * intervals and undefined: resample.interval, unchanged.  No table value has a zero denominator (N >=
    1); a bin with n_b = 0 in a replicate makes that replicate undefined for that bin's acc_b / conf_b only (their value is 0).

The bin tables and sums come from sm3_calib_counts (csrc/calib.hip): one workgroup per replicate and label, integers only, so
equal inputs give equal bits.  fit_temperature is a function of its inputs alone and runs on the host."""
import math

import numpy as np
import torch

from . import ops, report, resample
from .metrics import CLASSES_NAME, NUM_CLASSES

MAX_BINS = ops.CALIB_MAX_BINS
BINNINGS = ops.CALIB_BINNINGS
DEFAULT_BINS = 15
ONE = 1 << 32                       # 1.0 in Q32
NLL_CLAMP = 1024.0
LABEL_METRICS = ("NLL", "Brier", "ECE", "MCE")
CLASS_METRICS = ("cwECE",)
LABEL_COLUMNS = list(CLASSES_NAME) + ["AVG"]
CLASS_COLUMNS = list(report.COLUMNS)  # the 24 classes, then the five averages
T, K = len(NUM_CLASSES), report.K
S, X = T + K, 2 * T                   # 32 series, 16 plain sums
SERIES = [f"{n} top" for n in CLASSES_NAME] + list(report.CLASS_COLUMNS)
SERIES_LABEL = list(range(T)) + [t for t, _ in report.COLUMN_PAIRS]
DEFAULT_CHUNK = 1024  # replicates per launch: a choice (1024 x 32 x 64 x 3 int64 = 48 MiB of bins at the most)
LOG2_BETA = (-6.0, 6.0)
HALVINGS = 60


def check_bins(bins, binning, who="calibration_report"):
    if not resample.is_int(bins) or not 1 <= bins <= MAX_BINS:
        raise ValueError(f"{who}: bins must be an integer in [1, {MAX_BINS}], got {bins!r}")
    if binning not in BINNINGS:
        raise ValueError(f"{who}: binning must be one of {BINNINGS}, got {binning!r}")


def check_temperature(temperature, who="calibration_report"):
    """None or 8 positive finite numbers -> a list of 8 floats."""
    if temperature is None:
        return [1.0] * T
    if isinstance(temperature, torch.Tensor):
        temperature = temperature.tolist()
    temperature = list(temperature)
    if len(temperature) != T or not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0
                                        for v in temperature):
        raise ValueError(f"{who}: temperature must be None or {T} positive finite numbers, got {temperature!r}")
    return [float(v) for v in temperature]


def _q32(x):
    return torch.round(x * float(ONE)).to(torch.int64)


def fixed_point(preds, targets, temperature=None):
    """The plumbing around the kernel, on the device of preds: (q [32, N] int64, ev [32, N] uint8, xq [16, N] int64)."""
    temperature = check_temperature(temperature, "fixed_point")
    top, cls, etop, ecls, nll, br = [], [], [], [], [], []
    for t, pr in enumerate(preds):
        y = targets[:, t]
        z = pr.double() / temperature[t]
        p, lp = torch.softmax(z, dim=1), torch.log_softmax(z, dim=1)
        yhat = pr.argmax(dim=1)
        top.append(_q32(p.gather(1, yhat[:, None])[:, 0]))
        etop.append(yhat == y)
        nll.append(_q32(torch.clamp(-lp.gather(1, y[:, None])[:, 0], max=NLL_CLAMP)))
        b = torch.zeros_like(p[:, 0])
        for c in range(p.shape[1]):
            hit = y == c
            b = b + (p[:, c] - hit.double()) ** 2
            cls.append(_q32(p[:, c]))
            ecls.append(hit)
        br.append(_q32(b))
    return (torch.stack(top + cls).contiguous(), torch.stack(etop + ecls).to(torch.uint8).contiguous(),
            torch.stack(nll + br).contiguous())


def _div(num, den):
    return resample.safe_div(num, den)[0]


def values_from_counts(bins, sums, N):
    """bins [..., 32, M, 3] int64 (n_b, E_b, Q_b), sums [..., 16] int64 -> {"label_values" [..., 4, 9], "class_values" [..., 1,
    29], "diagram" [..., 32, M, 3] fp64, "diagram_undefined" [..., 32, M, 3] bool}."""
    bins, sums = np.asarray(bins, dtype=np.int64), np.asarray(sums, dtype=np.int64)
    n, E, Q = bins[..., 0], bins[..., 1], bins[..., 2]
    gap = np.abs(Q - E * ONE)
    den = np.int64(N) * ONE
    ece = _div(gap.sum(axis=-1), den)                                    # [..., 32]
    mce = _div(gap, n * ONE).max(axis=-1)                                # an empty bin holds gap 0 and gives 0
    lead = bins.shape[:-3]
    label = np.zeros(lead + (len(LABEL_METRICS), T + 1), dtype=np.float64)
    label[..., 0, :T] = _div(sums[..., :T], den)
    label[..., 1, :T] = _div(sums[..., T:], den)
    label[..., 2, :T] = ece[..., :T]
    label[..., 3, :T] = mce[..., :T]
    acc = np.zeros(lead + (len(LABEL_METRICS),), dtype=np.float64)
    for t in range(T):
        acc = acc + label[..., t]
    label[..., T] = acc / float(T)
    cw = np.zeros(lead + (1, report.NV), dtype=np.float64)
    cw[..., 0, :K] = ece[..., T:]
    cw[..., 0, K:] = report.averages(ece[..., T:])
    diagram = np.stack([n.astype(np.float64), _div(E, n), _div(Q, n * ONE)], axis=-1)
    undefined = np.zeros(diagram.shape, dtype=bool)
    undefined[..., 1] = undefined[..., 2] = n == 0
    return {"label_values": label, "class_values": cw, "diagram": diagram, "diagram_undefined": undefined}


def calibration_report(preds, targets, temperature=None, bins=DEFAULT_BINS, binning="width", bootstrap=0, confidence=0.95, seed=0,
                       chunk=None):
    """The calibration report of one set of predictions.

    preds, targets: as report.evaluation_report.  temperature: None or 8 positive numbers, the logits of label t are divided by
    temperature[t].  bins: M.  binning: "width" or "mass".  bootstrap, confidence, seed, chunk: as evaluation_report (chunk None:
    at most DEFAULT_CHUNK replicates per launch; every chunk gives the same bits).
    Returns {"bins" [32, M, 3] int64 (n_b, E_b, Q_b), "sums" [16] int64, "label_values" [4, 9] fp64 (rows NLL, Brier, ECE, MCE;
    columns the 8 labels, AVG), "class_values" [1, 29] fp64 (class-wise ECE of the 24 columns, the five averages), "diagram"
    [32, M, 3] fp64 (n_b, acc_b, conf_b), "label_metrics", "label_columns", "class_metrics", "class_columns", "series",
    "temperature", "n_bins", "binning", "targets", "n"} and, with bootstrap > 0, for each table x of "label", "class", "diagram":
    x_replicates [B, ...] fp64, x_lo, x_hi fp64 and x_undefined int64 of the table's shape, and "bootstrap", "seed",
    "confidence".  All tensors on the CPU.  The inputs are not modified."""
    who = "calibration_report"
    report.check_settings(bootstrap, confidence, seed, chunk, who)
    check_bins(bins, binning, who)
    temperature = check_temperature(temperature, who)
    N = report.check_inputs(preds, targets, who)
    dev = resample.device_for(preds, who)
    B, M = bootstrap, bins
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        q, ev, xq = fixed_point([p.detach().to(dev) for p in preds], targets.to(dev), temperature)
        order = torch.sort(q, dim=1, stable=True).indices.int().contiguous()
        slabel = torch.tensor(SERIES_LABEL, dtype=torch.int32, device=dev)
        (pb, ps), (rb, rs) = resample.replicate_tables(
            lambda outs, seed, r0, point: ops.calib_counts(q, ev, order, slabel, xq, outs[0], outs[1], T, binning, seed, r0,
                                                           point=point),
            [(S, M, 3), (X,)], B, seed, chunk, DEFAULT_CHUNK, dev)
    v = values_from_counts(pb, ps, N)
    out = {"bins": torch.from_numpy(pb), "sums": torch.from_numpy(ps), "label_values": torch.from_numpy(v["label_values"]),
           "class_values": torch.from_numpy(v["class_values"]), "diagram": torch.from_numpy(v["diagram"]),
           "label_metrics": list(LABEL_METRICS), "label_columns": list(LABEL_COLUMNS), "class_metrics": list(CLASS_METRICS),
           "class_columns": list(CLASS_COLUMNS), "series": list(SERIES), "temperature": list(temperature), "n_bins": M,
           "binning": binning, "targets": targets.detach().cpu().clone(), "n": N}
    if B:
        rv = values_from_counts(rb, rs, N)
        resample.pack_intervals(out, [("label_", rv["label_values"], np.zeros(rv["label_values"].shape[1:])),
                                      ("class_", rv["class_values"], np.zeros(rv["class_values"].shape[1:])),
                                      ("diagram_", rv["diagram"], rv["diagram_undefined"].sum(axis=0))], B, seed, confidence)
    return out


# ---- temperature scaling ---------------------------------------------------------------------------------------------------
def _g(z, zy, beta):
    """g(beta) = sum_n (sum_c p_nc(beta) z_nc - z_{n, y}), the derivative of the NLL sum by beta: fp64 per case, fsum over cases."""
    # z [N, C] fp64, zy [N] = z[n, y_n]
    a = z * beta
    a = a - a.max(axis=1, keepdims=True)
    w = np.exp(a)
    terms = (w * (z - zy[:, None])).sum(axis=1) / w.sum(axis=1)  # sum_c p_c (z_c - z_y): no cancellation against z_y
    return math.fsum(terms.tolist())


def fit_temperature(preds, targets):
    """Temperature scaling, one temperature per label: T_t = 1 / beta_t with g(beta_t) = 0 (the minimum of the label's NLL by
    beta; the NLL is convex in beta, so g is non-decreasing), by bisection on log2 beta in [-6, 6], 60 halvings, on the sign of
    g, which is computed on the host in fp64 per case as sum_c p_nc (z_nc - z_{n, y}) (the same number without the cancellation
    against z_{n, y}) and added with math.fsum over the cases (exactly rounded, hence free of the case order).  Where g has one
    sign over the whole interval -- a zero at an end included: on separable data g underflows to it -- the nearer end is
    returned (g >= 0 at 2^-6: the NLL grows with beta, beta = 2^-6; g <= 0 at 2^6, separable data: beta = 2^6) and flagged.
    Returns {"temperature": 8 floats, "beta": 8 floats, "clipped": 8 bools}.  Runs on the host: N <= MAX_CASES, C <= 5."""
    report.check_inputs(preds, targets, "fit_temperature")
    temps, betas, clipped = [], [], []
    for t, pr in enumerate(preds):
        z = pr.detach().double().cpu().numpy()
        zy = np.take_along_axis(z, targets[:, t].cpu().numpy()[:, None], axis=1)[:, 0]
        lo, hi = LOG2_BETA
        glo, ghi = _g(z, zy, 2.0 ** lo), _g(z, zy, 2.0 ** hi)
        if glo >= 0.0 or ghi <= 0.0:  # one sign throughout (a zero at an end included: on separable data g underflows to it)
            x, clip = (lo if glo >= 0.0 else hi), True
        else:
            for _ in range(HALVINGS):
                mid = 0.5 * (lo + hi)
                if _g(z, zy, 2.0 ** mid) > 0.0:
                    hi = mid
                else:
                    lo = mid
            x, clip = 0.5 * (lo + hi), False
        beta = 2.0 ** x
        betas.append(beta), temps.append(1.0 / beta), clipped.append(clip)
    return {"temperature": temps, "beta": betas, "clipped": clipped}


# ---- comparison and writers ------------------------------------------------------------------------------------------------
def compare(a, b):
    """The paired difference of two calibration reports of the SAME cases with the same settings: equal targets, bins, binning,
    bootstrap, seed and confidence (ValueError otherwise), so replicate r of both resamples the same cases.  Returns
    {"label_delta" [4, 9], "class_delta" [1, 29] = a - b, the metric and column names} and, with a bootstrap, x_lo, x_hi by the
    interval rule on the replicates' differences and x_frac_le_zero = the fraction of replicates with a difference <= 0, for x
    in "label", "class", and "bootstrap", "seed", "confidence"."""
    resample.check_paired(a, b, "calibration_report", ("label_values", "targets"),
                          (("n_bins", "bins differ ({} and {})"), ("binning", "binning differs ({} and {})")))
    out = {"label_delta": a["label_values"] - b["label_values"], "class_delta": a["class_values"] - b["class_values"],
           "label_metrics": list(LABEL_METRICS), "label_columns": list(LABEL_COLUMNS), "class_metrics": list(CLASS_METRICS),
           "class_columns": list(CLASS_COLUMNS)}
    return resample.paired_intervals(out, a, b, ("label_", "class_"))


def _tables(rep):
    """(table name, row names, column names, values key) of the two value tables."""
    return (("label", rep["label_metrics"], rep["label_columns"], "label_values"),
            ("class", rep["class_metrics"], rep["class_columns"], "class_values"))


def csv_rows(rep):
    """Long format: (table, row, column, value[, lo, hi, undefined]) of the two value tables, then of the diagram (table
    "diagram n" / "diagram acc" / "diagram conf", row = the series, column = the bin)."""
    boot = "label_lo" in rep
    rows = []
    for name, rnames, cnames, key in _tables(rep):
        for i, r in enumerate(rnames):
            for k, c in enumerate(cnames):
                row = [name, r, c, float(rep[key][i, k])]
                if boot:
                    row += [float(rep[f"{name}_lo"][i, k]), float(rep[f"{name}_hi"][i, k]), int(rep[f"{name}_undefined"][i, k])]
                rows.append(row)
    for e, part in enumerate(("n", "acc", "conf")):
        for s, sname in enumerate(rep["series"]):
            for b in range(rep["n_bins"]):
                row = [f"diagram {part}", sname, str(b), float(rep["diagram"][s, b, e])]
                if boot:
                    row += [float(rep["diagram_lo"][s, b, e]), float(rep["diagram_hi"][s, b, e]),
                            int(rep["diagram_undefined"][s, b, e])]
                rows.append(row)
    return rows


def to_csv(rep, path):
    """The long format of csv_rows with a header; repr of the fp64 values: they parse back exactly."""
    resample.write_long_csv(path, "table,row,column,value" + (",lo,hi,undefined" if "label_lo" in rep else ""), csv_rows(rep))


def to_json(rep, path):
    """Everything but the replicates and the targets, as lists (json writes repr of a float: the values parse back exactly)."""
    resample.write_json(rep, path, ("label_replicates", "class_replicates", "diagram_replicates", "targets"))


def format_table(rep):
    """The two tables as text: one line per metric and column, six decimals, the interval in brackets; repr would be unreadable
    here and is what the files hold."""
    lines = [f"calibration: {rep['n_bins']} {rep['binning']} bins, temperature " + " ".join(f"{v:.4f}" for v in rep["temperature"])]
    for name, rnames, cnames, key in _tables(rep):
        for i, r in enumerate(rnames):
            lines.append(r)
            for k, c in enumerate(cnames):
                s = f"  {c:<10} {float(rep[key][i, k]):9.6f}"
                if f"{name}_lo" in rep:
                    s += f"  [{float(rep[name + '_lo'][i, k]):9.6f}, {float(rep[name + '_hi'][i, k]):9.6f}]"
                lines.append(s)
    return "\n".join(lines)


def format_compare(cmp):
    lines = []
    for name in ("label", "class"):
        for i, r in enumerate(cmp[f"{name}_metrics"]):
            lines.append(f"{r} difference")
            for k, c in enumerate(cmp[f"{name}_columns"]):
                s = f"  {c:<10} {float(cmp[name + '_delta'][i, k]):+9.6f}"
                if f"{name}_lo" in cmp:
                    s += (f"  [{float(cmp[name + '_lo'][i, k]):+9.6f}, {float(cmp[name + '_hi'][i, k]):+9.6f}]"
                          f"  <= 0 in {float(cmp[name + '_frac_le_zero'][i, k]):.3f}")
                lines.append(s)
    return "\n".join(lines)


# ---- what the command-line tools share ----------------------------------------------------------------------------------
def add_flags(parser):
    """--calibration / --calib-bins / --calib-binning of the evaluation tools."""
    parser.add_argument("--calibration", action="store_true",
                        help="calibration report (NLL, Brier, ECE, MCE, class-wise ECE, reliability diagram) of the predictions")
    parser.add_argument("--calib-bins", type=int, default=DEFAULT_BINS, help=f"bins of the calibration report, 1 to {MAX_BINS}")
    parser.add_argument("--calib-binning", choices=BINNINGS, default="width", help="equal-width or equal-mass bins")
    return parser


def check_flags(args):
    """The refusals of the flags that argparse does not make, before any work is done."""
    check_bins(args.calib_bins, args.calib_binning, "--calib-bins")


def save(rep, log_path, stem="val_calibration"):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(rep, log_path, stem, to_json, to_csv)


def stats_line(rep):
    """The one printed line of the four top-label averages (with the interval when the report has one)."""
    if rep is None:
        return f"no calibration report: more than MAX_CASES = {report.MAX_CASES} cases"
    parts = []
    for i, m in enumerate(LABEL_METRICS):
        s = f"{m}_AVG {float(rep['label_values'][i, T]):.4f}"
        if "label_lo" in rep:
            s += f" [{float(rep['label_lo'][i, T]):.4f}, {float(rep['label_hi'][i, T]):.4f}]"
        parts.append(s)
    return " ".join(parts)


def validation_calibration(preds, targets, args, log_path):
    """What a tool does under --calibration after its last validation pass: the report at T = 1 with the tool's --bootstrap,
    --bootstrap-seed and --confidence, written as val_calibration.json / .csv under log_path.  Beyond MAX_CASES cases: None,
    which stats_line words."""
    if targets.shape[0] > report.MAX_CASES:
        return None
    rep = calibration_report(list(preds), targets, bins=args.calib_bins, binning=args.calib_binning, bootstrap=args.bootstrap,
                             confidence=args.confidence, seed=args.bootstrap_seed)
    save(rep, log_path)
    return rep
