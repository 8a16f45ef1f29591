"""L-BFGS logistic-regression probe of the SSL backbones on MI355X: the "linear probe" protocol of the self-supervised-learning
papers (SimCLR, appendix B.9; CLIP, sec. 3.2) -- one eval-mode pass of the frozen encoders over train, valid and test, an
L2-regularised multinomial logistic regression per derm7pt label fitted to its optimum on the cached features (sm3hip.logreg,
csrc/logreg.hip), C swept and picked on held-out cases, the test split scored.  No learning rate, no epochs, no augmentation: the
score is a function of (features, labels, C).

    python tools/backbone_logreg.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 128 -j 4 --img-sz 224 224 \
        --pretrain-path logs/backbone/ckp_399.pth --log-path logs/backbone/logreg_399 --logreg-select val

Takes backbone_eval's command line (--bootstrap, --calibration, --operating, --checklist; eval_cli's subject, batches and features)
plus the --logreg-* flags (--logreg-solver workgroup | lockstep picks the kernels of the fit, recorded in logreg_predictions.pt),
--save-features and --random-features.  A case's feature is cat(derm_f, clinic_f) through the
validation chain, then --logreg-normalize (standardize: per-feature mean and deviation of the train rows).

  --logreg-select val   every (label, C) is fitted on train and scored on valid (--logreg-by auc | nll; ties: the smaller C); the
                        reported model is the train fit at the selected C -- the fit is a function of its inputs, so "refitting"
                        on train alone changes nothing and is not run; --logreg-refit-trainval refits on train + valid instead.
  --logreg-select cv    --logreg-folds K folds of train (sm3hip.logreg.folds), out-of-fold predictions pooled, then one fit on all
                        of train at the selected C.
  --logreg-select none  one --logreg-c, no selection.
  --logreg-fractions    label-efficiency: nested subsets of train (sm3hip.logreg.fractions); the model reported is the largest
                        fraction's, logreg_curve.csv holds every (label, C, fraction).

Under --log-path: logreg_predictions.pt ("preds" / "targets" of test as val_predictions.pt has them -- tools/eval_report.py and
the four reports read it -- plus the selected C, the selection tables and the status table), best_linear.pth (a Baseline
state_dict with the fitted heads, standardisation folded in; not written under l2, whose per-row scaling no Linear holds),
val_report.json / .csv (and val_calibration / val_operating / val_checklist when asked), logreg_curve.csv.
`--data-name synthetic`: --steps-per-epoch batches are train, --val-steps batches valid and as many test; --random-features N B D
replaces the encoders by N train and B valid / B test rows of random features of width D.
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
from sm3hip import logreg, report  # noqa: E402
from sm3hip.metrics import CLASSES_NAME, NUM_CLASSES, auc_avg  # noqa: E402

TOOL = "backbone_logreg"


def get_parser():
    p = backbone_eval.get_parser(tta_flags=False)
    p.description = "SM3 L-BFGS logistic-regression probe (MI355X)"
    p.add_argument("--logreg-c", type=float, nargs="+", default=list(logreg.DEFAULT_CS),
                   help="the grid of C (default: 16 values log-spaced over 1e-4 .. 1e4)")
    p.add_argument("--logreg-select", default="val", help="val | cv | none: how C is picked")
    p.add_argument("--logreg-folds", type=int, default=5, help="K of --logreg-select cv")
    p.add_argument("--logreg-by", default="auc", help="auc | nll: the selection score")
    p.add_argument("--logreg-shared-c", action="store_true", help="one C for all labels (the best mean score)")
    p.add_argument("--logreg-fractions", type=float, nargs="+", default=[1.0], help="fractions of the train labels to fit on")
    p.add_argument("--logreg-class-weight", default="none", help="none | balanced")
    p.add_argument("--logreg-normalize", default="standardize", help="none | l2 | standardize")
    p.add_argument("--logreg-gtol", type=float, default=1e-9, help="stop at |grad F|_inf <= gtol")
    p.add_argument("--logreg-max-iter", type=int, default=1000, help="L-BFGS iterations at most")
    p.add_argument("--logreg-solver", default="workgroup",
                   help="workgroup | lockstep: one workgroup a problem, or all problems side by side on batched f64-MFMA products")
    p.add_argument("--logreg-refit-trainval", action="store_true",
                   help="with --logreg-select val: the reported model is refitted on train + valid at the selected C")
    p.add_argument("--random-features", type=int, nargs=3, default=None, metavar=("N", "B", "D"),
                   help="synthetic only: random features for N train rows and B valid / B test rows of width D, no encoders")
    p.add_argument("--save-features", action="store_true", help="also store the features in logreg_predictions.pt: the encoders' own, before --logreg-normalize, which the "
                        "heads of best_linear.pth take")
    return p


def check_flags(args):
    """The refusals of the --logreg-* flags: before any kernel, before the device is touched."""
    for flag, value, allowed in (("--logreg-select", args.logreg_select, ("val", "cv", "none")),
                                 ("--logreg-by", args.logreg_by, ("auc", "nll")),
                                 ("--logreg-class-weight", args.logreg_class_weight, ("none", "balanced")),
                                 ("--logreg-normalize", args.logreg_normalize, logreg.NORMALIZE),
                                 ("--logreg-solver", args.logreg_solver, logreg.SOLVERS)):
        if value not in allowed:
            raise SystemExit(f"{TOOL}: {flag} {value} is not one of {', '.join(allowed)}")
    if not all(0.0 < c < float("inf") for c in args.logreg_c):
        raise SystemExit(f"{TOOL}: every --logreg-c must be positive and finite, got {args.logreg_c}")
    if len(set(args.logreg_c)) != len(args.logreg_c):
        raise SystemExit(f"{TOOL}: --logreg-c names a value twice")
    if args.logreg_select == "cv" and args.logreg_folds < 2:
        raise SystemExit(f"{TOOL}: --logreg-select cv needs --logreg-folds K >= 2, got {args.logreg_folds}")
    if not all(0.0 < f <= 1.0 for f in args.logreg_fractions):
        raise SystemExit(f"{TOOL}: every fraction of --logreg-fractions must lie in (0, 1], got {args.logreg_fractions}")
    if args.logreg_select == "cv" and sorted(set(args.logreg_fractions)) != [1.0]:
        raise SystemExit(f"{TOOL}: --logreg-select cv folds all of train: --logreg-fractions must be 1")
    if args.logreg_select == "none" and len(args.logreg_c) != 1:
        raise SystemExit(f"{TOOL}: --logreg-select none takes exactly one --logreg-c")
    if args.logreg_refit_trainval and args.logreg_select != "val":
        raise SystemExit(f"{TOOL}: --logreg-refit-trainval goes with --logreg-select val")
    if not 0.0 <= args.logreg_gtol < float("inf"):
        raise SystemExit(f"{TOOL}: --logreg-gtol must be finite and >= 0, got {args.logreg_gtol}")
    if args.logreg_max_iter < 1:
        raise SystemExit(f"{TOOL}: --logreg-max-iter must be >= 1, got {args.logreg_max_iter}")
    if not 0 <= args.seed < 2 ** 64:
        raise SystemExit(f"{TOOL}: --seed must lie in [0, 2^64): it also seeds the folds and the fractions")
    if args.random_features and not all(v >= 1 for v in args.random_features):
        raise SystemExit(f"{TOOL}: --random-features N B D must all be >= 1")
    if args.random_features and (args.random_features[0] > logreg.MAX_ROWS or args.random_features[2] > logreg.MAX_DIM):
        raise SystemExit(f"{TOOL}: --random-features: at most {logreg.MAX_ROWS} train rows of width {logreg.MAX_DIM}")


def score_tables(fit, Xval, tval):
    """(auc, nll) [R, labels, Cs] float64 of every problem on the validation rows."""
    R, nl, nc = fit.weights.shape[0], len(fit.labels), len(fit.Cs)
    z = logreg.predict_all(fit, Xval).reshape(R, nl, nc, Xval.shape[0], -1)
    tval = tval.to(z.device)
    auc, nll = torch.zeros(R, nl, nc, dtype=torch.float64), torch.zeros(R, nl, nc, dtype=torch.float64)
    for r in range(R):
        for a, t in enumerate(fit.labels):
            for j in range(nc):
                zz = z[r, a, j, :, :NUM_CLASSES[t]]
                auc[r, a, j] = logreg.score(zz, tval[:, t], t, "auc")
                nll[r, a, j] = -logreg.score(zz, tval[:, t], t, "nll")
    return auc, nll


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    eval_cli.check_report_flags(args)
    check_flags(args)

    def check(real):
        if real and args.random_features:
            raise SystemExit(f"{TOOL}: --random-features goes with --data-name synthetic")
        if not real and not args.random_features and args.steps_per_epoch * args.batch_size > logreg.MAX_ROWS:
            raise SystemExit(f"{TOOL}: {args.steps_per_epoch * args.batch_size} train rows, at most {logreg.MAX_ROWS} are supported")
    dev, gen, real = eval_cli.refuse_and_seed(args, parser, TOOL, check)
    evaluator = None if args.random_features else eval_cli.baseline_subject(args, dev, freeze=True, eval_mode=True)
    if real:
        store, aug = eval_cli.image_store(args, ["train", "valid", "test"], dev)
        data = [eval_cli.split_batches(args, store, store.splits[m], aug) for m in ("train", "valid", "test")]
    elif not args.random_features:  # drawn before the timer starts: train, valid, test
        data = [list(eval_cli.synthetic_batches([args.batch_size] * n, args.img_sz, dev, gen))
                for n in (args.steps_per_epoch, args.val_steps, args.val_steps)]
    torch.cuda.synchronize()
    t0 = time.time()
    with torch.no_grad():
        if args.random_features:
            n, b, d = args.random_features
            sets = [eval_cli.random_features(m, d, dev, gen) for m in (n, b, b)]
        else:
            sets = [eval_cli.encode(evaluator, part) for part in data]
    torch.cuda.synchronize()
    encode_seconds = time.time() - t0
    (Xtr, ttr), (Xva, tva), (Xte, tte) = sets
    if Xtr.shape[0] > logreg.MAX_ROWS:
        raise SystemExit(f"{TOOL}: {Xtr.shape[0]} train rows, at most {logreg.MAX_ROWS} are supported")
    norm = logreg.normalize_fit(Xtr, args.logreg_normalize)
    raw = (Xtr, Xva, Xte)  # what the heads of best_linear.pth take: the encoders' features, before --logreg-normalize
    Xtr, Xva, Xte = (logreg.normalize_apply(x, norm) for x in raw)

    # ---- fit, select, refit
    cw = None if args.logreg_class_weight == "none" else "balanced"
    kw = dict(class_weight=cw, gtol=args.logreg_gtol, max_iter=args.logreg_max_iter, solver=args.logreg_solver)
    Cs = sorted(args.logreg_c)
    fracs = sorted(set(args.logreg_fractions), reverse=True)  # weight row 0: the largest fraction, the one reported
    torch.cuda.synchronize()
    t1 = time.time()
    rows = logreg.fractions(ttr, fracs, args.seed)
    grid = logreg.fit(Xtr, ttr, Cs, weights=rows, **kw)
    fits = [grid]
    auc_tab, nll_tab = score_tables(grid, Xva, tva)
    by = auc_tab if args.logreg_by == "auc" else -nll_tab
    selection = {"mode": args.logreg_select, "by": args.logreg_by, "Cs": Cs, "fractions": fracs, "val_auc": auc_tab, "val_nll": nll_tab}
    if args.logreg_select == "cv":
        cv = logreg.fit(Xtr, ttr, Cs, weights=logreg.folds(Xtr.shape[0], args.logreg_folds, args.seed), **kw)
        fits.append(cv)
        sel = logreg.select(cv, by=args.logreg_by, per_label=not args.logreg_shared_c, X=Xtr, targets=ttr)
        selection["cv_table"], chosen = sel["table"], sel["C"]
    else:
        chosen = logreg.pick(by[0].numpy(), Cs, per_label=not args.logreg_shared_c)
    final, Xfit = grid, Xtr
    if args.logreg_refit_trainval:
        Xfit, tfit = torch.cat([Xtr, Xva]).contiguous(), torch.cat([ttr, tva])
        if Xfit.shape[0] > logreg.MAX_ROWS:
            raise SystemExit(f"{TOOL}: {Xfit.shape[0]} train + valid rows, at most {logreg.MAX_ROWS} are supported")
        final = logreg.fit(Xfit, tfit, sorted(set(chosen)), **kw)
        fits.append(final)
    which = [final.index(t, chosen[t], 0) for t in range(len(NUM_CLASSES))]
    preds = logreg.predict_logits(final, Xte, which)
    torch.cuda.synchronize()
    fit_seconds = time.time() - t1

    # ---- score, write
    per, avg = auc_avg(preds, tte)
    problems = sum(len(f.problems) for f in fits)
    iterations = int(sum(int(f.iterations.sum()) for f in fits))
    not_ok = int(sum(int((f.status != 0).sum()) for f in fits))
    n_cases = Xtr.shape[0] + Xva.shape[0] + Xte.shape[0]
    stat = {f"AUC_{n}": float(a) for n, a in zip(CLASSES_NAME, per)}
    stat.update({"AUC_AVG": float(avg), "C": chosen, "problems": problems, "iterations": iterations, "not_converged": not_ok,
                 "pairs_per_s": n_cases / max(encode_seconds, 1e-9), "fit_seconds": fit_seconds})
    os.makedirs(args.log_path, exist_ok=True)
    new, rep = report.validation_stats(preds, tte, args, True, args.log_path)
    stat.update(new)
    saved = {"preds": [p.cpu() for p in preds], "targets": tte.cpu(), "AUC_AVG": stat["AUC_AVG"], "AUC": [float(a) for a in per],
             "C": chosen, "selection": selection, "normalize": args.logreg_normalize, "class_weight": args.logreg_class_weight,
             "solver": args.logreg_solver,
             "status": [{"problems": f.problems, "status": f.status.cpu(), "iterations": f.iterations.cpu(),
                         "objective": f.objective.cpu(), "grad_norm": f.grad_norm.cpu()} for f in fits]}
    if args.save_features:
        saved.update({"train_features": raw[0].cpu(), "train_targets": ttr.cpu(), "valid_features": raw[1].cpu(),
                      "valid_targets": tva.cpu(), "test_features": raw[2].cpu()})
    torch.save(saved, os.path.join(args.log_path, "logreg_predictions.pt"))
    if args.logreg_normalize == "l2":
        print("logreg: best_linear.pth is not written under --logreg-normalize l2 (each row is divided by its own norm, which "
              "no Linear head holds)", flush=True)
    else:
        heads = logreg.to_baseline_state(final, which, norm)
        state = dict(evaluator.state_dict()) if evaluator is not None else {}
        state.update(heads)
        torch.save({"epoch": 0, "state_dict": {k: v.cpu() for k, v in state.items()}},
                   os.path.join(args.log_path, "best_linear.pth"))
    with open(os.path.join(args.log_path, "logreg_curve.csv"), "w") as f:
        f.write("label,C,fraction,val_auc,val_nll\n")
        for r, fr in enumerate(fracs):
            for a, t in enumerate(grid.labels):
                for j, c in enumerate(Cs):
                    f.write(f"{CLASSES_NAME[t]},{c!r},{fr!r},{float(auc_tab[r, a, j])!r},{float(nll_tab[r, a, j])!r}\n")
    print(f"logreg {args.logreg_select}/{args.logreg_by}: AUC_AVG {stat['AUC_AVG']:.4f} | C "
          + " ".join(f"{n} {c:.3g}" for n, c in zip(CLASSES_NAME, chosen))
          + f" | {problems} problems ({not_ok} not converged), {iterations} iterations | {stat['pairs_per_s']:.0f} pairs/s | "
          f"fit {fit_seconds:.2f} s", flush=True)
    print(f"logreg {args.logreg_select}/{args.logreg_by}: {report.stats_line(stat, rep)}", flush=True)
    eval_cli.optional_reports("logreg: ", preds, tte, args, args.log_path)  # under the short prefix, as they always were
    return stat


if __name__ == "__main__":
    main()
