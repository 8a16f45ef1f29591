"""Linear probe / fine-tune of the SSL backbones on MI355X -- entry point mirroring the reference's
tools/backbone_eval.py (train :65-142, validate :145-212, checkpoint key split :278-296, run.sh:15-28).

    python tools/backbone_eval.py --data-name synthetic --data-path - -a resnet50 -b 128 -lr 1e-3 \
        --finetune fc --pretrain-path logs/backbone/ckp_50.pth --epochs 2 --steps-per-epoch 10

`--finetune fc`: encoders frozen and in eval mode (one fused conv+BN+ReLU kernel per layer), the 8 heads trained
with AdamW on the weighted cross-entropy sum/8; AUROC "8 avg" (sm3hip.metrics.auc_avg) on the validation pass, and with it the
reference's Recall / Spec / Prec of the 8 labels (sm3hip.report).  The validation pass of the last epoch writes val_report.json
and val_report.csv (the reference's table layout) to --log-path; --bootstrap B adds case-resampling intervals to them.
--calibration adds val_calibration.json / .csv of the same pass at T = 1 (sm3hip.calibration: NLL, Brier, ECE, MCE, class-wise ECE and
the reliability diagram; --calib-bins M, --calib-binning width|mass; the same bootstrap replicates).
--operating adds val_operating.json / .csv of the same pass (sm3hip.operating: average precision, the Youden and F1 optima,
sensitivity at --operating-spec floors, specificity at --operating-sens floors, net benefit at --operating-decision; the same
bootstrap replicates).
--checklist adds val_checklist.json / .csv of the same pass (sm3hip.checklist: melanoma by the seven-point checklist score of the
predicted criteria beside the DIAG head and the annotated score, the rule "score >= k" at --checklist-thresholds, the agreement
of the two scores; the same bootstrap replicates).
Any other value fine-tunes everything through the autograd bridge.

`--data-name SevenPCBaseDataset --data-path DIR`: derm7pt's train and test splits decoded once into the device image store
(sm3hip/imagestore.py); training one pass over the train split per epoch with the reference's chain (backbone_eval.py:234-262:
RandomResizedCrop(img_sz, scale=(0.5, 1)) -> flip -> Normalize) on the GPU, validation on the test split with Resize(img_sz)
-> Normalize and its real labels; the validation predictions of the last epoch are saved as val_predictions.pt.
--tta hflip|flips|d4 (sm3hip.tta) adds, after the last epoch's validation pass, one more pass over the same cases that averages the
predicted probabilities over the group's views of every case (--tta-crops 5: of a centre and four corner crops of --tta-crop-scale
each, real data only), prints its AUC_AVG and how much the predictions move across the views, and under real data saves
val_predictions_tta.pt in val_predictions.pt's format: `eval_report.py val_predictions_tta.pt --against val_predictions.pt
--significance` is the paired comparison.
--corrupt NAME [NAME ...] | all (sm3hip.corrupt; real data only) adds, after the last epoch's validation pass, one pass over the same
cases per image corruption and --corrupt-severity (default 1 .. 5; --corrupt-modality both|derm|clinic, --corrupt-seed): it saves
val_predictions_corrupt/<name>_<s>.pt in val_predictions.pt's format and val_robustness.json / .csv (the paired AUC differences with
the bootstrap's intervals, the flip rate and the mean |delta p| of every corruption), and prints one line per corruption.
`--data-name synthetic`: random images and labels, --steps-per-epoch / --val-steps steps.
"""
import argparse
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
import torch.nn as nn  # noqa: E402

import eval_cli  # noqa: E402
from sm3hip import corrupt, report, tta  # noqa: E402
from sm3hip.metrics import CLASSES_NAME, auc_avg  # noqa: E402


def get_parser(calibration_flags=True, tta_flags=True):
    """src/utils/misc.py:get_parser + tools/backbone_eval.py:434-440 of the reference, then this build's own flags
    (calibration_flags=False: without --calibration and its two settings, for backbone_knn, whose votes are not logits;
    tta_flags=False: without --tta and its two settings and without the --corrupt flags, for the tools on frozen features)."""
    from src.utils.misc import get_parser as base_parser
    p = base_parser("SM3 linear probe / fine-tune (MI355X)")
    p.add_argument("--arch-weights", type=str, default=None)
    p.add_argument("--num-labels", type=int, default=8)
    p.add_argument("--label-weights", type=float, nargs="*", default=[1.0] * 8)
    # this build (synthetic data: an epoch is a number of steps)
    p.add_argument("--steps-per-epoch", default=8, type=int)
    p.add_argument("--val-steps", default=4, type=int)
    report.add_flags(p)
    eval_cli.add_report_flags(p, calibration=calibration_flags)
    if tta_flags:
        tta.add_flags(p)
        corrupt.add_flags(p)
    p.set_defaults(arch="resnet50", epochs=50, batch_size=128)
    return p


def run_epoch(args, evaluator, criterion, optimizer, steps, gen, dev, train, data=None):
    if train and args.finetune != "fc":
        evaluator.train()
    else:
        evaluator.eval()
    all_preds, all_targets, total, t0 = [], [], 0.0, time.time()
    if data is None:
        data = eval_cli.synthetic_batches([args.batch_size] * steps, args.img_sz, dev, gen)
    steps, pairs = 0, 0
    for derm, clinic, labels in data:
        steps += 1
        pairs += labels.shape[0]
        with torch.set_grad_enabled(train):
            outputs = evaluator([derm, clinic])
            loss = sum(args.label_weights[i] * criterion(outputs[i], labels[:, i]) for i in range(args.num_labels))
            loss = loss / args.num_labels
        if train:
            optimizer.zero_grad(set_to_none=True)
            scaler = getattr(args, "scaler", None)  # backbone_eval.py:100-112 of the reference: GradScaler(enabled=args.amp)
            if scaler is None:
                loss.backward()
                optimizer.step()
            else:
                scaler.scale(loss).backward()
                scaler.step(optimizer)
                scaler.update()
        total += float(loss.detach())
        all_preds.append([o.detach() for o in outputs])
        all_targets.append(labels)
    preds = [torch.cat([p[i] for p in all_preds]) for i in range(args.num_labels)]
    per, avg = auc_avg(preds, torch.cat(all_targets))
    stat = {f"AUC_{n}": float(v) for n, v in zip(CLASSES_NAME, per)}
    stat.update({"AUC_AVG": float(avg), "loss": total / steps,
                 "pairs_per_s": pairs / (time.time() - t0)})
    stat["preds"], stat["targets"] = preds, torch.cat(all_targets)
    return stat


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    eval_cli.check_report_flags(args)
    from src.utils.misc import amp_dtype
    dev, gen, real = eval_cli.refuse_and_seed(args, parser, "backbone_eval", check=lambda real: (tta.check_flags(args, real),
                                                                                                  corrupt.check_flags(args, real)))
    evaluator = eval_cli.baseline_subject(args, dev, freeze=args.finetune == "fc", eval_mode=False)
    args.scaler = torch.amp.GradScaler("cuda", enabled=amp_dtype(args) == torch.float16)  # backbone_eval.py:271
    params = [p for p in evaluator.parameters() if p.requires_grad]
    optimizer = torch.optim.AdamW(params, lr=args.base_lr, weight_decay=args.wd)
    criterion = nn.CrossEntropyLoss()
    train_data = val_data = lambda epoch: None
    if real:
        from src.utils.data.sampler import train_batches
        store, aug = eval_cli.image_store(args, ["train", "test"], dev)
        tsplit, vsplit = store.splits["train"], store.splits["test"]
        aug_gen = torch.Generator().manual_seed(args.seed + 1000)
        train_data = lambda epoch: eval_cli.split_batches(
            args, store, tsplit, aug, train_batches(len(tsplit), 1, 0, epoch, args.batch_size), aug_gen, whole=False)
        val_data = lambda epoch: eval_cli.split_batches(args, store, vsplit, aug)
    best, history = -1.0, []
    os.makedirs(args.log_path, exist_ok=True)
    for epoch in range(args.epochs):
        tr = run_epoch(args, evaluator, criterion, optimizer, args.steps_per_epoch, gen, dev, True, train_data(epoch))
        va = run_epoch(args, evaluator, criterion, None, args.val_steps, gen, dev, False, val_data(epoch))
        history.append((tr, va))
        new, rep = report.validation_stats(va["preds"], va["targets"], args, epoch == args.epochs - 1, args.log_path)
        va.update(new)
        if real:
            torch.save({"epoch": epoch + 1, "preds": [p.cpu() for p in va["preds"]], "targets": va["targets"].cpu(),
                        "AUC_AVG": va["AUC_AVG"]}, os.path.join(args.log_path, "val_predictions.pt"))
        print(f"epoch {epoch}: train loss {tr['loss']:.4f} AUC_AVG {tr['AUC_AVG']:.4f} {tr['pairs_per_s']:.0f} pairs/s | "
              f"val loss {va['loss']:.4f} AUC_AVG {va['AUC_AVG']:.4f} {va['pairs_per_s']:.0f} pairs/s", flush=True)
        print(f"epoch {epoch}: val {report.stats_line(va, rep)}", flush=True)
        if epoch == args.epochs - 1:  # val_calibration / val_operating / val_checklist .json / .csv next to val_report.*
            eval_cli.optional_reports(f"epoch {epoch}: val ", va["preds"], va["targets"], args, args.log_path)
            if args.tta != "none":  # one more pass over the same validation cases, every view of each
                eval_cli.tta_pass(f"epoch {epoch}: ", evaluator, args, epoch, dev, gen, store if real else None,
                                  vsplit if real else None, args.img_sz)
            if args.corrupt is not None:  # one more pass per corruption and severity (real data: check_flags)
                eval_cli.corrupt_pass(f"epoch {epoch}: ", evaluator, args, epoch, store, vsplit, args.img_sz)
        if va["AUC_AVG"] > best:  # best by val/AUC_AVG (backbone_eval.py:386,405-411)
            best = va["AUC_AVG"]
            torch.save({"epoch": epoch + 1, "state_dict": evaluator.state_dict(), "optimizer": optimizer.state_dict()},
                       os.path.join(args.log_path, "best_linear.pth"))
    return history


if __name__ == "__main__":
    main()
