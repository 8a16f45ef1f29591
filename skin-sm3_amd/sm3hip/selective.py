"""Selective-prediction report of the 8 derm7pt labels: the model keeps the cases it is sure of and refers the rest.  The
risk-coverage curve of a confidence ranking, its area (AURC, E-AURC), the error rate and the 2 x 2 values of the retained cases at
fixed coverages, the share of the positives that is sent away, the largest coverage that stays within a risk level, the same
counts at thresholds fitted on another split, and case-resampling bootstrap intervals of all of them.  This docstring is the
normative text; include/sm3_hip.h repeats the integer part.

Inputs.  preds (8 float tensors [N, n_t]) and targets [N, 8] int64 as report.check_inputs asks, 1 <= N <= report.MAX_CASES.
Optional temperature, 8 positive numbers as calibration.check_temperature asks (default 1).  Per label t and case n:

  * z = preds[t].double() / T_t;  yhat = the lowest index of the row maximum of preds[t], as in report;
    flags: err = [yhat != y], pos = [y == CLS_WEIGHTS[t]], call = [yhat == CLS_WEIGHTS[t]].
  * primary key, fp64, computed by torch on the device of preds (plumbing, like report.ranking); HIGHER = more confident:
        score = "msp":      z[yhat] - logsumexp over c != yhat of z[c].  Strictly increasing in p[yhat], and it does not saturate
                            where the softmax rounds to 1;
        score = "margin":   z[yhat] - max over c != yhat of z[c];
        score = "entropy":  sum_c p_c * log p_c (the negative entropy), from softmax and log_softmax in fp64;
        score = a float tensor [N, 8], finite or else refused: any outside signal (tools/eval_report.py feeds the range of the
                            test-time augmentation views through it).
  * ranking: descending by primary key, ties by descending "msp" key, then by ascending case index -- stable torch sorts, done
    ONCE: order [8, N] int32.  A tie group is the cases with an equal primary key; last[j] marks the sorted position that ends
    one.  ties[t] = the number of cases that share their (primary, msp) pair with another case: where the index order decided.
  * multiplicities m[n] >= 0, sum m = N.  The point estimate has m = 1; replicate r has the m_r of resample.py's rule on stream
    word 2: the same cases as replicate r of every other report.  The case at sorted position j owns the copy ranks C_j + 1 ..
    C_j + m_j, C_j = the copies before j; E_j = the error copies before j (TP_j, FP_j, FN_j alike: call & pos, call & !pos,
    !call & pos).
  * harmonic-tail table, a function of N alone, in Python integers (harmonic_table): f[k] = f[k + 1] + (2^64 // k) for k = N ..
    1 with f[N + 1] = 0; t[r] = (f[r] + 2^31) >> 32; PH[r] = PH[r - 1] + t[r], PH[0] = 0.  t[r] / 2^32 is within 2^-32 of
    sum_{k = r .. N} 1 / k (each floor loses less than 1 of 2^64, N <= 2^13 of them, and the rounding shift at most half of
    2^32), and PH[N] is about N * 2^32 < 2^46.
  * the record of a (replicate, label), int64, so that no summation order shows:
        A = the sum over the error positions j of PH[C_j + m_j] - PH[C_j].  A / (N * 2^32) is the area under the risk-coverage
            curve, (1 / N) sum_{k = 1 .. N} err(k) / k with err(k) = the errors among the first k copies, to within 2^-32: an
            error copy at rank r is counted in err(k) for every k >= r, so sum_k err(k) / k = the sum over the error copies of
            sum_{k >= r} 1 / k;
        E, P = the error copies and the positive copies;
        per coverage level (1 to MAX_COVERAGES), the exact rational of its decimal string, 0 < gamma <= 1, denominator at most
            MAX_DENOMINATOR: k = ceil(gamma * N) in integers, and err, TP, FP, FN among the first k copies; a case that straddles
            k contributes k - C_j copies;
        per risk level rho = a / b (0 to MAX_RISKS, 0 <= rho <= 1): the largest cut C_{j+1} over the positions j with last[j]
            and C_{j+1} >= 1 such that E_{j+1} * b <= a * C_{j+1}, and the E there; 0 and 0 when no cut qualifies.  A threshold
            on the primary key can only cut between tie groups: only group ends are admissible;
        per position cut p (0 to MAX_THRESHOLDS per label, 0 <= p <= N), p = the number of cases whose primary key is >= a given
            threshold: C_p, E_p, TP_p, FP_p, FN_p.
  * values, fp64, on the host, ONE IEEE division of two integers each through resample.safe_div; a zero denominator gives the
    value 0 and is counted in `undefined`:
        summary [4, 9]: AURC = A / (N * 2^32); AURC optimal = (PH[N] - PH[N - E]) / (N * 2^32), the errors ranked last; E-AURC
            = (A - (PH[N] - PH[N - E])) / (N * 2^32), exactly 0 for a ranking that puts every error last; risk = E / N;
        coverage [G, 6, 9]: selective risk err / k, then sensitivity TP / (TP + FN), specificity TN / (TN + FP), PPV TP / (TP +
            FP), NPV TN / (TN + FN) of the selected class among the retained copies (TN = k - TP - FP - FN), and referred
            positives (P - TP - FN) / P, the share of the positives that is sent away;
        risk [H, 2, 9]: coverage k* / N and the risk attained E* / k*;
        threshold [Pc, 6, 9]: coverage C_p / N, risk E_p / C_p and the four 2 x 2 values;
    columns the 8 labels and "AVG": summed in ascending label order, then one division by 8; undefined where a label is.
  * intervals by resample.interval, unchanged.

Records come from sm3_selective_counts (csrc/selective.hip): one workgroup per replicate and label, integers only, so equal
inputs give equal bits."""
import fractions

import numpy as np
import torch

from . import calibration, ops, report, resample
from .metrics import CLASSES_NAME, CLS_WEIGHTS, NUM_CLASSES

MAX_COVERAGES = ops.SELECTIVE_MAX_COVERAGES
MAX_RISKS = ops.SELECTIVE_MAX_RISKS
MAX_THRESHOLDS = ops.SELECTIVE_MAX_THRESHOLDS
MAX_DENOMINATOR = 10 ** 6
ONE = 1 << 32
SCORES = ("msp", "margin", "entropy")
DEFAULT_COVERAGES = (0.5, 0.6, 0.7, 0.8, 0.9, 1.0)
DEFAULT_RISKS = (0.05, 0.1, 0.2)
SUMMARY_METRICS = ("AURC", "AURC optimal", "E-AURC", "risk")
TWO_BY_TWO = ("sensitivity", "specificity", "PPV", "NPV")
COVERAGE_METRICS = ("selective risk",) + TWO_BY_TWO + ("referred positives",)
RISK_METRICS = ("coverage", "risk")
THRESHOLD_METRICS = ("coverage", "risk") + TWO_BY_TWO
COLUMNS = list(CLASSES_NAME) + ["AVG"]
T = len(NUM_CLASSES)
DEFAULT_CHUNK = 4096  # replicates per launch: a choice (4096 x 8 x 123 int64 = 31 MiB at the most)
TABLES = ("summary", "coverage", "risk", "threshold")
FLAG_ERR, FLAG_POS, FLAG_CALL, FLAG_LAST = 1, 2, 4, 8


# ---- settings --------------------------------------------------------------------------------------------------------------
def check_levels(levels, name, lowest, open_low, most, least=1, who="selective_report"):
    """`least` to `most` numbers or decimal strings, each in (lowest, 1] (open_low) or [lowest, 1] -> (the levels as strings,
    [(num, den), ...] of Fraction(string))."""
    rng = f"{'(' if open_low else '['}{lowest}, 1]"
    if isinstance(levels, (int, float, str)) and not isinstance(levels, bool):
        levels = (levels,)
    try:
        levels = list(levels)
    except TypeError:
        raise ValueError(f"{who}: {name} must be {least} to {most} numbers in {rng}, got {levels!r}") from None
    if not least <= len(levels) <= most:
        raise ValueError(f"{who}: {name} must be {least} to {most} numbers in {rng}, got {len(levels)} of them")
    names, pairs = [], []
    for v in levels:
        try:
            if isinstance(v, bool) or not isinstance(v, (int, float, str)):
                raise ValueError
            f = fractions.Fraction(str(v).strip())
        except (ValueError, ZeroDivisionError):
            raise ValueError(f"{who}: every level of {name} must be a number in {rng}, got {v!r}") from None
        if not (lowest < f if open_low else lowest <= f) or f > 1:
            raise ValueError(f"{who}: every level of {name} must be a number in {rng}, got {v!r}")
        if f.denominator > MAX_DENOMINATOR:
            raise ValueError(f"{who}: level {v!r} of {name} = {f} has too many digits: a denominator above {MAX_DENOMINATOR}")
        names.append(str(v).strip())
        pairs.append((f.numerator, f.denominator))
    return names, pairs


def check_coverages(coverages, who="selective_report"):
    return check_levels(coverages, "coverages", 0, True, MAX_COVERAGES, 1, who)


def check_risks(risks, who="selective_report"):
    return check_levels(risks, "risks", 0, False, MAX_RISKS, 0, who)


def check_score(score, N=None, who="selective_report"):
    """A name of SCORES, or a finite float tensor [N, 8]."""
    if isinstance(score, str):
        if score not in SCORES:
            raise ValueError(f"{who}: score must be one of {SCORES} or a float tensor [N, {T}], got {score!r}")
        return
    if not isinstance(score, torch.Tensor) or not score.is_floating_point() or score.dim() != 2 or score.shape[1] != T or \
            (N is not None and score.shape[0] != N):
        raise ValueError(f"{who}: score must be one of {SCORES} or a float tensor [{'N' if N is None else N}, {T}], got "
                         + (f"{tuple(score.shape)} {score.dtype}" if isinstance(score, torch.Tensor) else repr(score)))
    if not bool(torch.isfinite(score).all()):
        raise ValueError(f"{who}: the score tensor holds a value that is not finite (it has no rank)")


def check_thresholds(thresholds, who="selective_report"):
    """None, or primary-key thresholds [8] or [8, Pc], Pc <= MAX_THRESHOLDS, no NaN (inf: nothing or everything is kept) ->
    an fp64 CPU tensor [8, Pc]."""
    if thresholds is None:
        return torch.zeros((T, 0), dtype=torch.float64)
    try:
        thr = torch.as_tensor(thresholds).detach().cpu().double()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{who}: thresholds must be None or numbers [{T}] or [{T}, Pc], got {thresholds!r}") from None
    if thr.dim() == 1:
        thr = thr[:, None]
    if thr.dim() != 2 or thr.shape[0] != T or thr.shape[1] > MAX_THRESHOLDS:
        raise ValueError(f"{who}: thresholds must be None or numbers [{T}] or [{T}, Pc] with Pc <= {MAX_THRESHOLDS}, got "
                         f"{tuple(thr.shape)}")
    if bool(torch.isnan(thr).any()):
        raise ValueError(f"{who}: thresholds holds a NaN")
    return thr.contiguous()


def coverage_cuts(N, pairs):
    """k = ceil(gamma * N) of every level (num, den), in integers."""
    return [-((-num * N) // den) for num, den in pairs]


# ---- keys and ranking: torch on the device of the tensors, plumbing -------------------------------------------------------
def predicted(preds):
    """yhat [N, 8] int64, as report.ranking's."""
    return torch.stack([p.argmax(dim=1) for p in preds], dim=1)


def keys(preds, score="msp", temperature=None):
    """The primary keys [8, N] fp64 on the device of preds (of the tensor, for a score tensor [N, 8])."""
    check_score(score, preds[0].shape[0], "keys")
    if isinstance(score, torch.Tensor):
        return score.detach().double().t().contiguous()
    temperature = calibration.check_temperature(temperature, "keys")
    out = []
    for t, pr in enumerate(preds):
        z = pr.detach().double() / temperature[t]
        if score == "entropy":
            p, lp = torch.softmax(z, dim=1), torch.log_softmax(z, dim=1)
            out.append(torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(dim=1))  # a class of probability 0 adds nothing
            continue
        yhat = pr.argmax(dim=1)
        top = z.gather(1, yhat[:, None])[:, 0]
        rest = z.masked_fill(torch.nn.functional.one_hot(yhat, z.shape[1]).bool(), float("-inf"))
        out.append(top - (torch.logsumexp(rest, dim=1) if score == "msp" else rest.max(dim=1).values))
    return torch.stack(out).contiguous()


def ranking(keys, msp_keys):
    """keys, msp_keys [8, N] fp64 -> (order [8, N] int32: descending primary key, ties by descending msp key, then ascending
    case index; last [8, N] bool: the sorted position ends a tie group of the primary key; ties [8] int64: the cases that share
    their (primary, msp) pair with another case; the sorted primary keys [8, N])."""
    first = torch.sort(msp_keys, dim=1, descending=True, stable=True).indices
    second = torch.sort(keys.gather(1, first), dim=1, descending=True, stable=True).indices
    order = first.gather(1, second)
    ks, ms = keys.gather(1, order), msp_keys.gather(1, order)
    edge = torch.ones((ks.shape[0], 1), dtype=torch.bool, device=ks.device)
    last = torch.cat([ks[:, 1:] != ks[:, :-1], edge], dim=1)
    same = (ks[:, 1:] == ks[:, :-1]) & (ms[:, 1:] == ms[:, :-1])     # position j and j + 1 share the pair
    none = torch.zeros_like(edge)
    tied = torch.cat([same, none], dim=1) | torch.cat([none, same], dim=1)
    return order.int().contiguous(), last, tied.sum(dim=1), ks


def pack_flags(preds, targets, order, last):
    """packed [8, N] int32 = err | pos << 1 | call << 2 | last << 3 per (label, case); `last` is moved from the sorted position
    to the case that stands there."""
    yhat = predicted(preds).to(targets.device)
    sel = torch.tensor(CLS_WEIGHTS, device=targets.device)[None, :]
    flags = (yhat != targets).int() * FLAG_ERR + (targets == sel).int() * FLAG_POS + (yhat == sel).int() * FLAG_CALL
    at_case = torch.zeros_like(last).scatter_(1, order.long(), last)
    return (flags.t() + at_case.int() * FLAG_LAST).int().contiguous()


def position_cuts(keys, thresholds):
    """p [8, Pc] int32: the number of cases whose primary key is >= the threshold."""
    thr = thresholds.to(keys.device)
    return (keys[:, None, :] >= thr[:, :, None]).sum(dim=2).int().contiguous()


def cut_thresholds(sorted_keys, cuts):
    """The primary-key threshold [8] fp64 that keeps exactly the first cuts[t] cases of the point ranking (a cut at a group end):
    the key of the last case kept; +inf where the cut is 0."""
    sorted_keys = np.asarray(sorted_keys, dtype=np.float64)
    return np.array([sorted_keys[t, int(k) - 1] if int(k) >= 1 else np.inf for t, k in enumerate(cuts)], dtype=np.float64)


def harmonic_table(N):
    """PH [N + 1] int64 of the module text, in Python integers."""
    f, tails = 0, [0] * (N + 1)
    for k in range(N, 0, -1):
        f += (1 << 64) // k
        tails[k] = (f + (1 << 31)) >> 32
    ph, acc = [0], 0
    for r in range(1, N + 1):
        acc += tails[r]
        ph.append(acc)
    return np.array(ph, dtype=np.int64)


# ---- values --------------------------------------------------------------------------------------------------------------
def _averaged(rows):
    """[(num, den) per row], each [..., 8] -> (values [..., rows, 9], undefined [..., rows, 9])."""
    lead = np.broadcast(*[np.asarray(x) for nd in rows for x in nd]).shape[:-1]
    vals = np.zeros(lead + (len(rows), T + 1), dtype=np.float64)
    undef = np.zeros(vals.shape, dtype=bool)
    for i, (num, den) in enumerate(rows):
        v, u = resample.safe_div(num, den)
        vals[..., i, :T], undef[..., i, :T] = np.broadcast_to(v, lead + (T,)), np.broadcast_to(u, lead + (T,))
    acc = np.zeros(lead + (len(rows),), dtype=np.float64)
    for t in range(T):
        acc = acc + vals[..., t]
    vals[..., T] = acc / float(T)
    undef[..., T] = undef[..., :T].any(axis=-1)
    return vals, undef


def _two_by_two(k, TP, FP, FN):
    TN = k - TP - FP - FN
    return [(TP, TP + FN), (TN, TN + FP), (TP, TP + FP), (TN, TN + FN)]


def values_from_counts(counts, N, kcuts, H, Pc, table=None):
    """counts [..., 8, 3 + 4 G + 2 H + 5 Pc] int64, kcuts the G coverage cuts -> {"summary_values" [..., 4, 9], "coverage_values"
    [..., G, 6, 9], "risk_values" [..., H, 2, 9], "threshold_values" [..., Pc, 6, 9] fp64 and "<table>_undefined" bool of the
    same shapes}."""
    counts = np.asarray(counts, dtype=np.int64)
    table = harmonic_table(N) if table is None else np.asarray(table, dtype=np.int64)
    G = len(kcuts)
    lead = counts.shape[:-2]
    den = np.int64(N) * np.int64(ONE)
    n = np.int64(N)
    A, E, P = counts[..., 0], counts[..., 1], counts[..., 2]
    A_opt = table[N] - table[N - E]
    out = {}
    out["summary_values"], out["summary_undefined"] = _averaged([(A, den), (A_opt, den), (A - A_opt, den), (E, n)])
    cov = np.zeros(lead + (G, len(COVERAGE_METRICS), T + 1), dtype=np.float64)
    out["coverage_undefined"] = np.zeros(cov.shape, dtype=bool)
    for g, k in enumerate(kcuts):
        err, TP, FP, FN = (counts[..., 3 + 4 * g + e] for e in range(4))
        k = np.full(err.shape, k, dtype=np.int64)
        cov[..., g, :, :], out["coverage_undefined"][..., g, :, :] = _averaged([(err, k)] + _two_by_two(k, TP, FP, FN)
                                                                                + [(P - TP - FN, P)])
    out["coverage_values"] = cov
    rsk = np.zeros(lead + (H, len(RISK_METRICS), T + 1), dtype=np.float64)
    out["risk_undefined"] = np.zeros(rsk.shape, dtype=bool)
    for h in range(H):
        k, e = (counts[..., 3 + 4 * G + 2 * h + i] for i in range(2))
        rsk[..., h, :, :], out["risk_undefined"][..., h, :, :] = _averaged([(k, n), (e, k)])
    out["risk_values"] = rsk
    thr = np.zeros(lead + (Pc, len(THRESHOLD_METRICS), T + 1), dtype=np.float64)
    out["threshold_undefined"] = np.zeros(thr.shape, dtype=bool)
    for i in range(Pc):
        C, e, TP, FP, FN = (counts[..., 3 + 4 * G + 2 * H + 5 * i + f] for f in range(5))
        thr[..., i, :, :], out["threshold_undefined"][..., i, :, :] = _averaged([(C, n), (e, C)] + _two_by_two(C, TP, FP, FN))
    out["threshold_values"] = thr
    return out


# ---- the report ----------------------------------------------------------------------------------------------------------
def _device_inputs(preds, targets, score, temperature, dev):
    """(keys [8, N], sorted keys, order, ties, packed) on dev."""
    preds = [p.detach().to(dev) for p in preds]
    key = keys(preds, score.to(dev) if isinstance(score, torch.Tensor) else score, temperature)
    msp = key if isinstance(score, str) and score == "msp" else keys(preds, "msp", temperature)
    order, last, ties, sorted_keys = ranking(key, msp)
    return key, sorted_keys, order, ties, pack_flags(preds, targets.to(dev), order, last)


def _level_tensors(N, cov_pairs, risk_pairs, pcuts, dev):
    kcuts = coverage_cuts(N, cov_pairs)
    return (kcuts, torch.tensor(kcuts, dtype=torch.int32, device=dev), pcuts.to(dev).int().contiguous(),
            torch.tensor(risk_pairs, dtype=torch.int32, device=dev).reshape(len(risk_pairs), 2))


def _check_inputs(preds, targets, score, temperature, who):
    if not isinstance(score, (str, torch.Tensor)):
        raise ValueError(f"{who}: score must be one of {SCORES} or a float tensor [N, {T}], got {score!r}")
    if isinstance(score, str):
        check_score(score, None, who)
    temperature = calibration.check_temperature(temperature, who)
    N = report.check_inputs(preds, targets, who)
    check_score(score, N, who)
    return N, temperature


def selective_report(preds, targets, score="msp", temperature=None, coverages=DEFAULT_COVERAGES, risks=DEFAULT_RISKS,
                     thresholds=None, bootstrap=0, confidence=0.95, seed=0, chunk=None):
    """The selective-prediction report of one set of predictions.

    preds, targets: as report.evaluation_report.  score: "msp", "margin", "entropy" or a finite float tensor [N, 8], higher =
    more confident.  temperature: None or 8 positive numbers.  coverages: 1 to MAX_COVERAGES levels in (0, 1]; risks: 0 to
    MAX_RISKS levels in [0, 1]; numbers or decimal strings, taken as the exact rationals of their strings.  thresholds: None, or
    primary-key thresholds [8] or [8, Pc] (fit_thresholds) the split is also scored at.  bootstrap, confidence, seed, chunk: as
    evaluation_report (chunk None: at most DEFAULT_CHUNK replicates per launch; every chunk gives the same bits).
    Returns {"counts" [8, R] int64, "summary_values" [4, 9], "coverage_values" [G, 6, 9], "risk_values" [H, 2, 9],
    "threshold_values" [Pc, 6, 9] fp64, the row names "<table>_metrics", "columns", "coverages" and "risks" (the levels as
    strings), "coverage_cuts" (k per level), "thresholds" [8, Pc] fp64, "position_cuts" [8, Pc], "ties" [8], "score",
    "temperature", "targets", "n"} and, with bootstrap > 0, for each table x of TABLES: x_replicates [B, ...] fp64, x_lo, x_hi
    fp64 and x_undefined int64 of the table's shape, and "bootstrap", "seed", "confidence".  All tensors on the CPU.  The inputs
    are not modified."""
    who = "selective_report"
    report.check_settings(bootstrap, confidence, seed, chunk, who)
    cov_names, cov_pairs = check_coverages(coverages, who)
    risk_names, risk_pairs = check_risks(risks, who)
    thr = check_thresholds(thresholds, who)
    N, temperature = _check_inputs(preds, targets, score, temperature, who)
    dev = resample.device_for(preds, who)
    G, H, Pc = len(cov_pairs), len(risk_pairs), thr.shape[1]
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        key, _, order, ties, packed = _device_inputs(preds, targets, score, temperature, dev)
        pcuts = position_cuts(key, thr)
        kcuts, kc, pc, rk = _level_tensors(N, cov_pairs, risk_pairs, pcuts, dev)
        table = harmonic_table(N)
        tab = torch.from_numpy(table).to(dev)
        (point,), (reps,) = resample.replicate_tables(
            lambda outs, seed, r0, point: ops.selective_counts(packed, order, tab, kc, pc, rk, outs[0], seed, r0, point=point),
            [(T, ops.selective_record(G, H, Pc))], bootstrap, seed, chunk, DEFAULT_CHUNK, dev)
        ties, pcuts = ties.cpu(), pcuts.cpu()
    return assemble(point, reps, targets, cov_names, kcuts, risk_names, thr, pcuts, ties, score, temperature, bootstrap, seed,
                    confidence, table)


def assemble(counts, rep_counts, targets, coverages, kcuts, risks, thresholds, pcuts, ties, score, temperature, bootstrap=0, seed=0,
             confidence=0.95, table=None):
    """The report dict of selective_report from the point records [8, R] and (with a bootstrap) the replicate records [B, 8, R]:
    host arithmetic only."""
    N, H = targets.shape[0], len(risks)
    thresholds = torch.as_tensor(thresholds, dtype=torch.float64)
    Pc = thresholds.shape[1]
    table = harmonic_table(N) if table is None else table
    counts = np.asarray(counts, dtype=np.int64)
    v = values_from_counts(counts, N, kcuts, H, Pc, table)
    out = {"counts": torch.from_numpy(counts)}
    out.update({f"{x}_values": torch.from_numpy(v[f"{x}_values"]) for x in TABLES})
    out.update({"summary_metrics": list(SUMMARY_METRICS), "coverage_metrics": list(COVERAGE_METRICS),
                "risk_metrics": list(RISK_METRICS), "threshold_metrics": list(THRESHOLD_METRICS), "columns": list(COLUMNS),
                "coverages": list(coverages), "risks": list(risks), "coverage_cuts": [int(k) for k in kcuts],
                "thresholds": thresholds.clone(), "position_cuts": torch.as_tensor(pcuts).long().clone(),
                "ties": torch.as_tensor(ties).long().clone(), "score": score if isinstance(score, str) else "tensor",
                "temperature": list(temperature), "targets": targets.detach().cpu().clone(), "n": N})
    if bootstrap:
        rv = values_from_counts(rep_counts, N, kcuts, H, Pc, table)
        resample.pack_intervals(out, [(f"{x}_", rv[f"{x}_values"], rv[f"{x}_undefined"].sum(axis=0)) for x in TABLES],
                                bootstrap, seed, confidence)
    return out


def curve(preds, targets, score="msp", temperature=None):
    """The point estimate's full risk-coverage curve [8, N] fp64 (CPU) for plotting: entry k - 1 = the errors among the k most
    confident cases / k, on the host side of the ranking (torch on the device of preds; no kernel is needed for m = 1)."""
    who = "curve"
    _check_inputs(preds, targets, score, temperature, who)
    with torch.no_grad():
        dev = preds[0].device
        key, _, order, _, _ = _device_inputs(preds, targets, score, temperature, dev)
        err = (predicted(preds).to(dev) != targets.to(dev)).t().gather(1, order.long())
        k = torch.arange(1, err.shape[1] + 1, device=dev, dtype=torch.float64)
        return (err.long().cumsum(dim=1).double() / k[None, :]).cpu()


def fit_thresholds(preds, targets, risk="0.1", score="msp", temperature=None):
    """The primary-key thresholds [8] fp64 (CPU) of the risk cut on the point estimate: keeping the cases with key >= the
    threshold keeps the largest admissible cut whose error rate is at most `risk`; +inf where no cut qualifies.
    selective_report(other_preds, other_targets, thresholds=...) then scores another split at those fixed thresholds (the
    protocol of operating.fit_thresholds)."""
    who = "fit_thresholds"
    _, pairs = check_levels(risk, "risk", 0, False, 1, 1, who)
    N, temperature = _check_inputs(preds, targets, score, temperature, who)
    dev = resample.device_for(preds, who)
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        _, sorted_keys, order, _, packed = _device_inputs(preds, targets, score, temperature, dev)
        _, kc, pc, rk = _level_tensors(N, [(1, 1)], pairs, torch.zeros((T, 0), dtype=torch.int32), dev)
        out = torch.empty((1, T, ops.selective_record(1, 1, 0)), dtype=torch.int64, device=dev)
        ops.selective_counts(packed, order, torch.from_numpy(harmonic_table(N)).to(dev), kc, pc, rk, out, 0, 0, point=True)
        cuts, sorted_keys = out[0, :, 3 + 4].cpu().numpy(), sorted_keys.cpu().numpy()
    return torch.from_numpy(cut_thresholds(sorted_keys, cuts))


# ---- comparison and writers ----------------------------------------------------------------------------------------------
def compare(a, b):
    """The paired difference of two selective reports of the SAME cases (equal targets) -- two models, or two scores of one file --
    with the same coverages, risks, bootstrap, seed and confidence (ValueError otherwise), so replicate r of both resamples the
    same cases.  Returns {"summary_delta" [4, 9] (AURC, AURC optimal, E-AURC, risk), "coverage_delta" [G, 6, 9] (risk at coverage
    first), "risk_delta" [H, 2, 9] (coverage at risk first) = a - b, the names} and, with a bootstrap, x_lo, x_hi by the interval
    rule on the replicates' differences and x_frac_le_zero, and "bootstrap", "seed", "confidence"."""
    resample.check_paired(a, b, "selective_report", ("summary_values", "coverage_values", "risk_values", "targets"),
                          (("coverages", "coverages differ ({} and {})"), ("risks", "risks differ ({} and {})")))
    out = {f"{x}_delta": a[f"{x}_values"] - b[f"{x}_values"] for x in TABLES[:3]}
    out.update({"summary_metrics": list(SUMMARY_METRICS), "coverage_metrics": list(COVERAGE_METRICS),
                "risk_metrics": list(RISK_METRICS), "columns": list(COLUMNS), "coverages": list(a["coverages"]),
                "risks": list(a["risks"]), "scores": [a["score"], b["score"]]})
    return resample.paired_intervals(out, a, b, tuple(f"{x}_" for x in TABLES[:3]))


def _blocks(rep, tables=TABLES):
    """(table, level name, index prefix, row names) of every block of values."""
    out = []
    for x in tables:
        if x == "summary":
            out.append((x, "", (), rep["summary_metrics"]))
            continue
        names = rep["coverages"] if x == "coverage" else rep["risks"] if x == "risk" else \
            [str(i) for i in range(rep["thresholds"].shape[1])]
        out += [(x, name, (i,), rep[f"{x}_metrics"]) for i, name in enumerate(names)]
    return out


def csv_rows(rep):
    """Long format: (table, level, row, column, value[, lo, hi, undefined]); level = the coverage or risk level as given, the
    index of the threshold, empty for the summary."""
    boot = "summary_lo" in rep
    rows = []
    for x, level, pre, rnames in _blocks(rep):
        for i, r in enumerate(rnames):
            for k, c in enumerate(rep["columns"]):
                idx = pre + (i, k)
                row = [x, level, r, c, float(rep[f"{x}_values"][idx])]
                if boot:
                    row += [float(rep[f"{x}_lo"][idx]), float(rep[f"{x}_hi"][idx]), int(rep[f"{x}_undefined"][idx])]
                rows.append(row)
    return rows


def to_csv(rep, path):
    """The long format of csv_rows with a header; repr of the fp64 values: they parse back exactly."""
    resample.write_long_csv(path, "table,level,row,column,value" + (",lo,hi,undefined" if "summary_lo" in rep else ""), csv_rows(rep))


def to_json(rep, path):
    """Everything but the replicates and the targets, as lists."""
    resample.write_json(rep, path, tuple(f"{x}_replicates" for x in TABLES) + ("targets",))


def _lines(rep, tables, suffix, fmt, extra=None):
    lines = []
    for x, level, pre, rnames in _blocks(rep, tables):
        if level:
            lines.append(f"{x} {level}")
        for i, r in enumerate(rnames):
            lines.append(f" {r}{suffix}")
            for k, c in enumerate(rep["columns"]):
                idx = pre + (i, k)
                s = f"  {c:<10} {format(float(rep[x + fmt[0]][idx]), fmt[1])}"
                if f"{x}_lo" in rep:
                    s += f"  [{format(float(rep[x + '_lo'][idx]), fmt[1])}, {format(float(rep[x + '_hi'][idx]), fmt[1])}]"
                    if extra:
                        s += f"  <= 0 in {float(rep[x + extra][idx]):.3f}"
                lines.append(s)
    return lines


def format_table(rep):
    """The tables as text: one line per metric and column, six decimals, the interval in brackets."""
    head = (f"selective prediction: {rep['score']} ranking of {rep['n']} cases, temperature "
            + " ".join(f"{v:.4f}" for v in rep["temperature"]) + "; tied cases "
            + " ".join(f"{n} {int(v)}" for n, v in zip(CLASSES_NAME, rep["ties"])))
    return "\n".join([head] + _lines(rep, TABLES, "", ("_values", "9.6f")))


def format_compare(cmp):
    return "\n".join(_lines(cmp, TABLES[:3], " difference", ("_delta", "+9.6f"), "_frac_le_zero"))


# ---- what the command-line tool needs ------------------------------------------------------------------------------------
TOOL_SCORES = SCORES + ("tta-range",)


def add_flags(parser):
    """--selective and its settings (tools/eval_report.py)."""
    parser.add_argument("--selective", action="store_true",
                        help="selective-prediction report: risk-coverage, AURC, referral cuts of the predictions")
    parser.add_argument("--selective-score", choices=TOOL_SCORES, default="msp",
                        help="confidence ranking: top probability (msp), logit margin, negative entropy, or the range of the "
                             "test-time augmentation views saved with the predictions (tta-range)")
    parser.add_argument("--selective-coverage", nargs="+", default=[str(v) for v in DEFAULT_COVERAGES], metavar="GAMMA",
                        help=f"coverage levels, 1 to {MAX_COVERAGES} decimal numbers in (0, 1]")
    parser.add_argument("--selective-risk", nargs="*", default=[str(v) for v in DEFAULT_RISKS], metavar="RHO",
                        help=f"risk levels, at most {MAX_RISKS} decimal numbers in [0, 1]")
    parser.add_argument("--selective-rule", default="0.1", metavar="RISK",
                        help="with --fit-on: the risk level whose thresholds are fitted there and applied to the predictions")
    return parser


def check_flags(args):
    """The refusals of the flags that argparse does not make, before any work is done."""
    check_coverages(args.selective_coverage, "--selective-coverage")
    check_risks(args.selective_risk, "--selective-risk")
    check_levels(args.selective_rule, "the risk level", 0, False, 1, 1, "--selective-rule")


def flag_settings(args):
    """The keyword arguments of selective_report that the flags set (the tool makes the tensor of "tta-range" itself)."""
    kw = dict(coverages=args.selective_coverage, risks=args.selective_risk)
    if args.selective_score in SCORES:
        kw["score"] = args.selective_score
    return kw


def tta_range_score(preds, record):
    """The score tensor [N, 8] fp64 of "tta-range": -(max_q - min_q) of the view probabilities (sm3hip/tta.py's record) at the
    column of (t, yhat): the less the views move the predicted class, the more confident."""
    if not isinstance(record, dict) or "min_q" not in record or "max_q" not in record:
        raise ValueError("tta-range: the predictions file carries no 'tta' record with min_q and max_q (run the evaluation with --tta)")
    yhat = predicted(preds)
    first = torch.tensor([report.COLUMN_PAIRS.index((t, 0)) for t in range(T)], device=yhat.device)
    span = (record["max_q"] - record["min_q"]).to(yhat.device)
    return -(span.gather(1, yhat + first[None, :]).double())


def save(rep, log_path, stem="val_selective"):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(rep, log_path, stem, to_json, to_csv)


def stats_line(rep):
    """The one printed line: AURC, E-AURC and the coverage at each risk level, averaged over the labels (with the interval when
    the report has one)."""
    if rep is None:
        return f"no selective report: more than MAX_CASES = {report.MAX_CASES} cases"
    parts = []
    for x, idx, name in [("summary", (0, T), "AURC_AVG"), ("summary", (2, T), "E-AURC_AVG")] + \
            [("risk", (h, 0, T), f"coverage_AVG@risk{r}") for h, r in enumerate(rep["risks"])]:
        s = f"{name} {float(rep[x + '_values'][idx]):.4f}"
        if f"{x}_lo" in rep:
            s += f" [{float(rep[x + '_lo'][idx]):.4f}, {float(rep[x + '_hi'][idx]):.4f}]"
        parts.append(s)
    return " ".join(parts)
