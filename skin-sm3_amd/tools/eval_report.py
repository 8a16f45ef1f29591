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
"""
import argparse
import json
import os
import sys

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
sys.path.insert(0, ROOT_PATH)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import torch  # noqa: E402

from sm3hip import report  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="SM3 evaluation report of saved predictions (MI355X)")
    p.add_argument("pred", metavar="PRED.pt", help="val_predictions.pt (backbone_eval, mlc_eval) or knn_predictions.pt")
    p.add_argument("--against", metavar="OTHER.pt", default=None, help="second file of the same cases: paired comparison")
    p.add_argument("--out", default=None, help="directory of the JSON / CSV files (default: next to PRED.pt)")
    p.add_argument("--chunk", type=int, default=None, help="bootstrap replicates per launch (any value gives the same bits)")
    report.add_flags(p)
    return p


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


def main(argv=None):
    args = get_parser().parse_args(argv)
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
        print(format_compare(cmp), flush=True)
        with open(os.path.join(out, stem + "_compare.json"), "w") as f:
            json.dump({k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in cmp.items()}, f, indent=1)
        result.update({"other": other, "compare": cmp})
    return result


if __name__ == "__main__":
    main()
