"""Weighted kNN evaluation of the SSL backbones on MI355X: no training, one eval-mode pass over the train split (the feature
bank) and one over the test split (the queries), scored by the reference's KNNOnlineEvaluator rule (Wu et al. 2018, sec. 3.4;
src/models/evaluator.py) for each of the 8 derm7pt labels.

    python tools/backbone_knn.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 128 -j 4 --img-sz 224 224 \
        --pretrain-path logs/backbone/ckp_399.pth --log-path logs/backbone/knn_399 --knn-k 200 --knn-t 0.07

Takes backbone_eval's command line (and eval_cli's subject, batches and features) plus --knn-k / --knn-t.  The encoders are
frozen and in eval mode (one fused conv + BN + ReLU kernel per layer); a case's feature is normalize(cat(derm_f, clinic_f))
(sm3_normalize_rows), both splits through the validation chain (Resize -> Normalize of the whole image).  Per label the votes
become fractions p = votes / sum(votes); AUC_AVG is sm3hip.metrics.auc_avg of log p (softmax(log p) = p) and top-1 is the
first of the stable descending order, as KNNOnlineEvaluator.predict ranks.  knn_predictions.pt goes to --log-path, and with it
val_report.json / val_report.csv: Recall / Spec / Prec and every class's AUROC of the same log p (sm3hip.report; --bootstrap B
adds case-resampling intervals); --operating adds val_operating.json / .csv of the same log p (sm3hip.operating),
--checklist val_checklist.json / .csv (sm3hip.checklist; --checklist-thresholds).
`--data-name synthetic`: --steps-per-epoch batches form the bank, --val-steps batches the queries; --random-features N B D
replaces the encoders by N bank and B query rows of unit-norm random features of width D (the kNN stage alone, at bank sizes
no encoder pass in a test reaches).
"""
import os
import sys
import time

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import torch  # noqa: E402

import backbone_eval  # noqa: E402
import eval_cli  # noqa: E402
from sm3hip import report  # noqa: E402
from sm3hip.metrics import CLASSES_NAME, NUM_CLASSES, auc_avg  # noqa: E402


def get_parser():
    p = backbone_eval.get_parser(calibration_flags=False, tta_flags=False)
    p.description = "SM3 weighted kNN evaluation (MI355X)"
    p.add_argument("--knn-k", default=200, type=int, help="neighbours per query (1..1024, at most the bank size)")
    p.add_argument("--knn-t", default=0.07, type=float, help="temperature of the exp(s / T) weights")
    p.add_argument("--random-features", type=int, nargs=3, default=None, metavar=("N", "B", "D"),
                   help="synthetic only: random unit-norm features for N bank rows and B queries of width D, no encoders")
    p.add_argument("--save-features", action="store_true", help="also store the bank and query features in knn_predictions.pt")
    return p


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    eval_cli.check_report_flags(args, calibration=False)

    def check(real):
        if real and args.random_features:
            raise SystemExit("backbone_knn: --random-features goes with --data-name synthetic")
    dev, gen, real = eval_cli.refuse_and_seed(args, parser, "backbone_knn", check)
    evaluator = None if args.random_features else eval_cli.baseline_subject(args, dev, freeze=True, eval_mode=True)
    from sm3hip.knn import KNNBank, knn_scores
    if real:
        store, aug = eval_cli.image_store(args, ["train", "test"], dev)
        bank_data, query_data = (eval_cli.split_batches(args, store, store.splits[m], aug) for m in ("train", "test"))
    elif not args.random_features:  # drawn inside the timed region: the bank, then the queries
        bank_data, query_data = (eval_cli.synthetic_batches([args.batch_size] * n, args.img_sz, dev, gen)
                                 for n in (args.steps_per_epoch, args.val_steps))
    torch.cuda.synchronize()
    t0 = time.time()
    with torch.no_grad():
        if args.random_features:
            n, b, d = args.random_features
            bank_f, bank_t = eval_cli.random_features(n, d, dev, gen, normalize=True)
            query_f, query_t = eval_cli.random_features(b, d, dev, gen, normalize=True)
        else:
            bank_f, bank_t = eval_cli.encode(evaluator, bank_data, normalize=True)
            query_f, query_t = eval_cli.encode(evaluator, query_data, normalize=True)
        bank = KNNBank(bank_f, bank_t, NUM_CLASSES)
        votes = knn_scores(query_f, bank, k=args.knn_k, temperature=args.knn_t)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    probs = [v.double() / v.double().sum(dim=1, keepdim=True) for v in votes]
    per, avg = auc_avg([p.log() for p in probs], query_t)
    top1 = [float((v.argsort(dim=1, descending=True, stable=True)[:, 0] == query_t[:, i]).double().mean())
            for i, v in enumerate(votes)]
    stat = {f"AUC_{n}": float(a) for n, a in zip(CLASSES_NAME, per)}
    stat.update({f"TOP1_{n}": a for n, a in zip(CLASSES_NAME, top1)})
    stat.update({"AUC_AVG": float(avg), "bank": bank.N, "queries": query_f.shape[0],
                 "pairs_per_s": (bank.N + query_f.shape[0]) / seconds})
    os.makedirs(args.log_path, exist_ok=True)
    new, rep = report.validation_stats([p.log() for p in probs], query_t, args, True, args.log_path)
    stat.update(new)
    saved = {"votes": [v.cpu() for v in votes], "targets": query_t.cpu(), "AUC_AVG": stat["AUC_AVG"],
             "AUC": [float(a) for a in per], "top1": top1, "k": args.knn_k, "temperature": args.knn_t, "bank_size": bank.N}
    if args.save_features:
        saved.update({"bank_features": bank_f.cpu(), "bank_targets": bank_t.cpu(), "query_features": query_f.cpu()})
    torch.save(saved, os.path.join(args.log_path, "knn_predictions.pt"))
    print(f"knn k={args.knn_k} T={args.knn_t}: AUC_AVG {stat['AUC_AVG']:.4f} | top-1 "
          + " ".join(f"{n} {a:.3f}" for n, a in zip(CLASSES_NAME, top1))
          + f" | bank {bank.N} queries {query_f.shape[0]} | {stat['pairs_per_s']:.0f} pairs/s", flush=True)
    print(f"knn k={args.knn_k} T={args.knn_t}: {report.stats_line(stat, rep)}", flush=True)
    eval_cli.optional_reports(f"knn k={args.knn_k} T={args.knn_t}: ", [p.log() for p in probs], query_t, args, args.log_path)
    return stat


if __name__ == "__main__":
    main()
