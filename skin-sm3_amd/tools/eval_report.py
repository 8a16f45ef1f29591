"""The evaluation report of saved predictions on MI355X: AUROC, Recall, Spec and Prec of all 24 derm7pt classes and the five
averages of the reference's result tables (linear_results.csv / finetune_results.csv), with case-resampling bootstrap intervals,
and the paired comparison of two sets of predictions of the same cases.

    python tools/eval_report.py logs/linear/val_predictions.pt --bootstrap 2000
    python tools/eval_report.py logs/finetune/val_predictions.pt --against logs/linear/val_predictions.pt --bootstrap 2000

PRED.pt is a val_predictions.pt of backbone_eval / mlc_eval (logits) or a knn_predictions.pt of backbone_knn (votes, scored as
log of the vote fraction).  Prints the table, writes <name>_report.json and <name>_report.csv (the reference's layout, percent)
next to PRED.pt or under --out.  With --against OTHER.pt both files must hold the same cases (equal targets); the replicates
are a function of the seed, so replicate r resamples the same cases in both and the difference PRED - OTHER is paired:
its interval and the fraction of replicates with a difference <= 0 are printed and written to <name>_compare.json.

    python tools/eval_report.py logs/linear/val_predictions.pt --bootstrap 2000 --calibration --calib-binning mass
    python tools/eval_report.py logs/linear/test_predictions.pt --bootstrap 2000 --fit-on logs/linear/val_predictions.pt

--calibration adds the calibration report (sm3hip/calibration.py: NLL, Brier, ECE and MCE of the top label, class-wise ECE, the
reliability diagram; --calib-bins M, --calib-binning width|mass) with the SAME bootstrap replicates, written to
<name>_calibration.json / .csv.  --fit-on OTHER.pt (implies --calibration) fits one temperature per label on OTHER.pt, for
example the validation split's predictions, and reports PRED.pt both at T = 1 and at the fitted temperatures
(<name>_calibration_fitted.json / .csv), with the paired difference fitted - unscaled and its interval
(<name>_calibration_compare.json).

    python tools/eval_report.py logs/linear/test_predictions.pt --bootstrap 2000 --operating --operating-rule "spec>=0.9" \
        --fit-on logs/linear/val_predictions.pt

--operating adds the operating-point report (sm3hip/operating.py: average precision, the Youden and F1 optima, sensitivity at
--operating-spec floors, specificity at --operating-sens floors, net benefit at --operating-decision) with the SAME bootstrap
replicates, written to <name>_operating.json / .csv, and with --against the paired difference (<name>_operating_compare.json).
With --fit-on OTHER.pt the thresholds that --operating-rule (youden, f1, spec>=X, sens>=X) picks on OTHER.pt are applied to
PRED.pt: sens / spec / PPV / NPV at the transferred thresholds with their intervals (<name>_operating_fitted.json / .csv).

    python tools/eval_report.py logs/linear/test_predictions.pt --bootstrap 2000 --checklist --checklist-thresholds 1 3

--checklist adds the seven-point checklist report (sm3hip/checklist.py: melanoma by the score of the predicted criteria, beside
the DIAG head and the score of the annotated criteria; the rule "score >= k" at --checklist-thresholds; the agreement of the two
scores) with the SAME bootstrap replicates, written to <name>_checklist.json / .csv, and with --against the paired difference
(<name>_checklist_compare.json).

    python tools/eval_report.py logs/finetune/val_predictions.pt --against logs/linear/val_predictions.pt --significance \
        --permutations 10000 --permutation-seed 0

--significance (needs --against) adds the significance tests of PRED against OTHER (sm3hip/significance.py): the paired
randomisation test of every metric and column over --permutations swap replicates drawn from --permutation-seed, DeLong's test
of the 24 class AUCs with its intervals at --confidence, McNemar's exact test of the argmax decisions per label, and the
Holm-adjusted p-values; the table is printed and written to <name>_significance.json / .csv (long format).  Without the flag
neither file is written.

    python tools/eval_report.py logs/linear/test_predictions.pt --bootstrap 2000 --conformal --conformal-alpha 0.05 0.1 \
        --conformal-conditional class --fit-on logs/linear/val_predictions.pt

--conformal (needs --fit-on VAL.pt) adds the conformal prediction-set report (sm3hip/conformal.py): thresholds fitted on VAL.pt
at the --conformal-alpha levels by --conformal-method lac|aps, one per label or (--conformal-conditional class) one per class;
coverage, set size, empty and singleton sets and class-conditional coverage of PRED.pt.  The bootstrap resamples BOTH files and
refits the thresholds in every replicate (--conformal-fixed: keeps the point thresholds); the test replicates are the SAME as
every other report's.  --conformal-scaled divides the logits of both files by the temperatures fitted on VAL.pt.  Written to
<name>_conformal.json / .csv, and with --against OTHER.pt plus --against-fit-on OTHER_VAL.pt (the same cases as VAL.pt) the
paired difference to <name>_conformal_compare.json.

    python tools/eval_report.py logs/linear/test_predictions.pt --bootstrap 2000 --selective --selective-score margin \
        --selective-risk 0.05 0.1 --fit-on logs/linear/val_predictions.pt

--selective adds the selective-prediction report (sm3hip/selective.py: the cases ranked by --selective-score msp|margin|entropy|
tta-range, the area under the risk-coverage curve, selective risk and sens / spec / PPV / NPV of the retained cases and the
share of referred positives at the --selective-coverage levels, the largest coverage within each --selective-risk level) with
the SAME bootstrap replicates, written to <name>_selective.json / .csv.  tta-range ranks by the range of the test-time
augmentation views and needs PRED.pt to carry the "tta" record, as val_predictions_tta.pt does.  With --fit-on VAL.pt the
thresholds of the risk level --selective-rule (default 0.1) are fitted on VAL.pt and PRED.pt is also reported at them, in the
same files; with --against OTHER.pt the paired difference goes to <name>_selective_compare.json.  Without the flag nothing of
this is computed, printed or written.
"""
import argparse
import os
import sys

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import torch  # noqa: E402

import eval_cli  # noqa: E402
from sm3hip import calibration, checklist, conformal, operating, report, resample, selective, significance  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="SM3 evaluation report of saved predictions (MI355X)")
    p.add_argument("pred", metavar="PRED.pt", help="val_predictions.pt (backbone_eval, mlc_eval) or knn_predictions.pt")
    p.add_argument("--against", metavar="OTHER.pt", default=None, help="second file of the same cases: paired comparison")
    p.add_argument("--out", default=None, help="directory of the JSON / CSV files (default: next to PRED.pt)")
    p.add_argument("--chunk", type=int, default=None, help="bootstrap replicates per launch (any value gives the same bits)")
    report.add_flags(p)
    eval_cli.add_report_flags(p)
    p.add_argument("--significance", action="store_true",
                   help="with --against: permutation, DeLong and McNemar tests of PRED against OTHER, Holm-adjusted")
    p.add_argument("--permutations", type=int, default=significance.DEFAULT_PERMUTATIONS,
                   help="swap replicates of the paired randomisation test")
    p.add_argument("--permutation-seed", type=int, default=0, help="64-bit seed of the swap replicates")
    p.add_argument("--fit-on", metavar="OTHER.pt", default=None,
                   help="fit the temperatures on this predictions file; report PRED.pt at T = 1 and at the fitted T (implies --calibration)")
    conformal.add_flags(p)
    p.add_argument("--against-fit-on", metavar="OTHER_VAL.pt", default=None,
                   help="with --conformal and --against: the file OTHER.pt's thresholds are fitted on (the cases of --fit-on)")
    selective.add_flags(p)
    return p


def calibrate(args, preds, targets, kw, out, stem, dev):
    """The --calibration / --fit-on part: prints the tables, writes the files, returns what it computed."""
    if targets.shape[0] > report.MAX_CASES:
        print(calibration.stats_line(None), flush=True)
        return {}
    ckw = dict(kw, bins=args.calib_bins, binning=args.calib_binning)
    cal = calibration.calibration_report(preds, targets, **ckw)
    print(calibration.format_table(cal), flush=True)
    calibration.save(cal, out, stem + "_calibration")
    result = {"calibration": cal}
    if args.fit_on:
        fit = calibration.fit_temperature(*report.load_predictions(args.fit_on, dev))
        print(f"temperatures fitted on {args.fit_on}: " + " ".join(
            f"{n} {v:.4f}{' (clipped)' if c else ''}" for n, v, c in zip(calibration.CLASSES_NAME, fit["temperature"], fit["clipped"])),
            flush=True)
        fitted = calibration.calibration_report(preds, targets, temperature=fit["temperature"], **ckw)
        print(calibration.format_table(fitted), flush=True)
        calibration.save(fitted, out, stem + "_calibration_fitted")
        cmp = calibration.compare(fitted, cal)
        print("fitted - unscaled", flush=True)
        print(calibration.format_compare(cmp), flush=True)
        resample.write_json(dict(cmp, fit=fit), os.path.join(out, stem + "_calibration_compare.json"))
        result.update({"fit": fit, "calibration_fitted": fitted, "calibration_compare": cmp})
    return result


def operate(args, preds, targets, kw, out, stem, dev):
    """The --operating part: prints the tables, writes the files, returns what it computed."""
    if targets.shape[0] > report.MAX_CASES:
        print(operating.stats_line(None), flush=True)
        return {}
    okw = dict(kw, **operating.flag_settings(args))
    opr = operating.operating_report(preds, targets, **okw)
    print(operating.format_table(opr), flush=True)
    operating.save(opr, out, stem + "_operating")
    result = {"operating": opr}
    if args.against:
        cmp = operating.compare(opr, operating.operating_report(*report.load_predictions(args.against, dev), **okw))
        print(f"{args.pred} - {args.against}", flush=True)
        print(operating.format_compare(cmp), flush=True)
        resample.write_json(cmp, os.path.join(out, stem + "_operating_compare.json"))
        result["operating_compare"] = cmp
    if args.fit_on:
        thr = operating.fit_thresholds(*report.load_predictions(args.fit_on, dev), args.operating_rule)
        print(f"thresholds fitted on {args.fit_on} by {args.operating_rule}: " + " ".join(
            f"{n} {float(v):.4f}" for n, v in zip(report.CLASS_COLUMNS, thr)), flush=True)
        fitted = operating.operating_report(preds, targets, thresholds=thr, **okw)
        fitted.update({"rule": args.operating_rule, "fit_on": args.fit_on})
        print(operating.format_table(fitted), flush=True)
        operating.save(fitted, out, stem + "_operating_fitted")
        result.update({"operating_thresholds": thr, "operating_fitted": fitted})
    return result


def check(args, preds, targets, kw, out, stem, dev):
    """The --checklist part: prints the tables, writes the files, returns what it computed."""
    if targets.shape[0] > report.MAX_CASES:
        print(checklist.stats_line(None), flush=True)
        return {}
    ckw = dict(kw, **checklist.flag_settings(args))
    ckl = checklist.checklist_report(preds, targets, **ckw)
    print(checklist.format_table(ckl), flush=True)
    checklist.save(ckl, out, stem + "_checklist")
    result = {"checklist": ckl}
    if args.against:
        cmp = checklist.compare(ckl, checklist.checklist_report(*report.load_predictions(args.against, dev), **ckw))
        print(f"{args.pred} - {args.against}", flush=True)
        print(checklist.format_compare(cmp), flush=True)
        resample.write_json(cmp, os.path.join(out, stem + "_checklist_compare.json"))
        result["checklist_compare"] = cmp
    return result


def conform(args, preds, targets, kw, out, stem, dev, fit=None):
    """The --conformal part: prints the tables, writes the files, returns what it computed.  fit: what calibrate() fitted on
    --fit-on, when it ran."""
    cal_preds, cal_targets = report.load_predictions(args.fit_on, dev)
    if max(targets.shape[0], cal_targets.shape[0]) > report.MAX_CASES:
        print(conformal.stats_line(None), flush=True)
        return {}
    ckw = dict(kw, **conformal.flag_settings(args))
    if args.conformal_scaled:
        fit = fit or calibration.fit_temperature(cal_preds, cal_targets)
        ckw["temperature"] = fit["temperature"]
    cfm = conformal.conformal_report(preds, targets, cal_preds, cal_targets, **ckw)
    cfm["fit_on"] = args.fit_on
    print(conformal.format_table(cfm), flush=True)
    print(conformal.stats_line(cfm), flush=True)
    conformal.save(cfm, out, stem + "_conformal")
    result = {"conformal": cfm}
    if args.against and args.against_fit_on:
        other_cal = report.load_predictions(args.against_fit_on, dev)
        if args.conformal_scaled:
            ckw["temperature"] = calibration.fit_temperature(*other_cal)["temperature"]
        other = conformal.conformal_report(*report.load_predictions(args.against, dev), *other_cal, **ckw)
        cmp = conformal.compare(cfm, other)
        print(f"{args.pred} - {args.against}", flush=True)
        print(conformal.format_compare(cmp), flush=True)
        resample.write_json(cmp, os.path.join(out, stem + "_conformal_compare.json"))
        result.update({"conformal_other": other, "conformal_compare": cmp})
    return result


def _selective_score(args, path, preds, dev):
    """What --selective-score asks for of the predictions in `path`: a name, or the tensor of tta-range."""
    if args.selective_score != "tta-range":
        return args.selective_score
    return selective.tta_range_score(preds, torch.load(path, map_location=dev, weights_only=False).get("tta"))


def select(args, preds, targets, kw, out, stem, dev):
    """The --selective part: prints the tables, writes the files, returns what it computed."""
    if targets.shape[0] > report.MAX_CASES:
        print(selective.stats_line(None), flush=True)
        return {}
    skw = dict(kw, **selective.flag_settings(args))
    score = _selective_score(args, args.pred, preds, dev)
    thr = None
    if args.fit_on:
        fit_preds, fit_targets = report.load_predictions(args.fit_on, dev)
        thr = selective.fit_thresholds(fit_preds, fit_targets, args.selective_rule,
                                       _selective_score(args, args.fit_on, fit_preds, dev))
        print(f"thresholds fitted on {args.fit_on} at risk {args.selective_rule}: " + " ".join(
            f"{n} {float(v):.4f}" for n, v in zip(selective.CLASSES_NAME, thr)), flush=True)
    sel = selective.selective_report(preds, targets, **dict(skw, score=score, thresholds=thr))
    sel["score"] = args.selective_score
    if args.fit_on:
        sel.update({"rule": args.selective_rule, "fit_on": args.fit_on})
    print(selective.format_table(sel), flush=True)
    print(selective.stats_line(sel), flush=True)
    selective.save(sel, out, stem + "_selective")
    result = {"selective": sel}
    if args.against:
        other_preds, other_targets = report.load_predictions(args.against, dev)
        other = selective.selective_report(other_preds, other_targets,
                                           **dict(skw, score=_selective_score(args, args.against, other_preds, dev)))
        cmp = selective.compare(sel, other)
        print(f"{args.pred} - {args.against}", flush=True)
        print(selective.format_compare(cmp), flush=True)
        resample.write_json(cmp, os.path.join(out, stem + "_selective_compare.json"))
        result.update({"selective_other": other, "selective_compare": cmp})
    return result


def signify(args, preds, targets, out, stem, dev):
    """The --significance part: prints the table, writes the files, returns what it computed."""
    other, other_targets = report.load_predictions(args.against, dev)
    sig = significance.significance_report(preds, other, targets, permutations=args.permutations, seed=args.permutation_seed,
                                           confidence=args.confidence, chunk=None, targets_b=other_targets)
    print(f"significance of {args.pred} - {args.against}", flush=True)
    print(significance.format_table(sig), flush=True)
    significance.save(sig, out, stem + "_significance")
    return {"significance": sig}


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    if args.significance and not args.against:
        parser.error("--significance compares two sets of predictions: it needs --against OTHER.pt")
    if args.significance:
        try:
            significance.check_permutation_settings(args.permutations, args.permutation_seed, None, "--significance")
        except ValueError as e:
            parser.error(str(e))
    if args.conformal and not args.fit_on:
        parser.error("--conformal fits its thresholds on a second split: it needs --fit-on VAL.pt")
    if args.conformal:
        try:
            conformal.check_flags(args)
        except ValueError as e:
            parser.error(str(e))
    if args.selective:
        try:
            selective.check_flags(args)
        except ValueError as e:
            parser.error(str(e))
    eval_cli.check_report_flags(args)
    out = args.out or os.path.dirname(os.path.abspath(args.pred))
    stem = os.path.splitext(os.path.basename(args.pred))[0]
    kw = dict(bootstrap=args.bootstrap, confidence=args.confidence, seed=args.bootstrap_seed, chunk=args.chunk)
    dev = torch.device("cuda", 0)
    preds, targets = report.load_predictions(args.pred, dev)
    rep = report.evaluation_report(preds, targets, **kw)
    print(f"{args.pred}: {rep['n']} cases" + (f", {args.bootstrap} bootstrap replicates, seed {args.bootstrap_seed}, "
                                               f"confidence {args.confidence}" if args.bootstrap else ""), flush=True)
    print(report.format_table(rep), flush=True)
    report.save(rep, out, stem + "_report")
    result = {"report": rep}
    if args.against:
        other = report.evaluation_report(*report.load_predictions(args.against, dev), **kw)
        cmp = report.compare(rep, other)
        print(f"{args.pred} - {args.against}", flush=True)
        print(report.format_compare(cmp), flush=True)
        resample.write_json(cmp, os.path.join(out, stem + "_compare.json"))
        result.update({"other": other, "compare": cmp})
    if args.significance:
        result.update(signify(args, preds, targets, out, stem, dev))
    if args.calibration or args.fit_on:
        result.update(calibrate(args, preds, targets, kw, out, stem, dev))
    if args.operating:
        result.update(operate(args, preds, targets, kw, out, stem, dev))
    if args.checklist:
        result.update(check(args, preds, targets, kw, out, stem, dev))
    if args.conformal:
        result.update(conform(args, preds, targets, kw, out, stem, dev, result.get("fit")))
    if args.selective:
        result.update(select(args, preds, targets, kw, out, stem, dev))
    return result


if __name__ == "__main__":
    main()
