"""What the evaluation tools (backbone_eval, mlc_eval, backbone_knn, backbone_logreg, backbone_retrieval, backbone_map,
eval_report) share: the registry of the optional validation reports, the linear-probe subject with every refusal before the
device is touched, the (derm, clinic, labels) batches of a real split or of the synthetic stream, and the cached encoder
features.  Imported by the tools, which are run as scripts and have put this directory on sys.path."""
import os

import torch

from sm3hip import calibration, checklist, knn, operating
from sm3hip.metrics import NUM_CLASSES

# (flag attribute, module, name of its validation function) in the order the lines are printed.  The function is looked up on
# the module when it is called; the printed line is the module's stats_line.  A new validation report is one entry here plus
# its module's add_flags / check_flags / validation_* / stats_line.
REPORTS = (("calibration", calibration, "validation_calibration"),
           ("operating", operating, "validation_operating"),
           ("checklist", checklist, "validation_checklist"))


def _modules(with_calibration):
    return [module for _, module, _ in REPORTS if with_calibration or module is not calibration]


def add_report_flags(parser, calibration=True):
    """Every report's flags (calibration=False: without calibration's, for backbone_knn, whose votes are not logits)."""
    for module in _modules(calibration):
        module.add_flags(parser)
    return parser


def check_report_flags(args, calibration=True):
    """The refusals of those flags: no device needed."""
    for module in _modules(calibration):
        module.check_flags(args)


def optional_reports(prefix, preds, targets, args, log_path):
    """Runs the reports whose flag is set (val_<report>.json / .csv next to val_report.*), prints prefix + the report's one
    line; {flag: report}."""
    done = {}
    for flag, module, validation in REPORTS:
        if getattr(args, flag, False):
            done[flag] = getattr(module, validation)(preds, targets, args, log_path)
            print(prefix + module.stats_line(done[flag]), flush=True)
    return done


# ---- the subject ------------------------------------------------------------------------------------------------------------
def ignored_notice(args, parser, real):
    from src.utils.misc import ignored_line
    if ignored_line(args, parser, real):
        print("accepted for compatibility, without effect in this build:", " ".join(ignored_line(args, parser, real)), flush=True)


def load_ssl_backbones(evaluator, path):
    """Split an SSL checkpoint's keys by the derm_backbone.encoder. / clinic_backbone.encoder. prefixes
    (backbone_eval.py:278-296)."""
    state = torch.load(path, map_location="cpu")["state_dict"]
    derm, clinic = {}, {}
    for k, v in state.items():
        k = k[7:] if k.startswith("module.") else k
        if k.startswith("derm_backbone.encoder."):
            derm[k[len("derm_backbone.encoder."):]] = v
        elif k.startswith("clinic_backbone.encoder."):
            clinic[k[len("clinic_backbone.encoder."):]] = v
    evaluator.derm_backbone.load_state_dict(derm)
    evaluator.clinic_backbone.load_state_dict(clinic)


def refuse_and_seed(args, parser, tool, check=None):
    """What a linear-probe tool does before its model: every refusal (check(real): the tool's own, after the data's), then the
    seeds -- torch's, then the device generator's.  (device, its generator, whether the data is real)."""
    from src.utils.misc import require_baseline_arch, require_data
    require_baseline_arch(args.arch, tool)
    real = require_data(args, tool)
    if check is not None:
        check(real)
    ignored_notice(args, parser, real)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    return dev, torch.Generator(device=dev).manual_seed(args.seed), real


def baseline_subject(args, dev, freeze, eval_mode):
    """The linear probe on the device: the model, the SSL weights of --pretrain-path, the frozen encoders (freeze) and their
    arithmetic mode; in eval mode when eval_mode."""
    from src.models.baseline import Baseline
    from src.utils.misc import amp_dtype
    evaluator = Baseline(args.arch, args.arch_weights)
    if args.pretrain_path and os.path.isfile(args.pretrain_path):
        load_ssl_backbones(evaluator, args.pretrain_path)
        print(f"loaded pre-trained model weights from '{args.pretrain_path}'")
    if freeze:
        evaluator.freeze_backbone()
    for m in (evaluator.derm_backbone, evaluator.clinic_backbone):
        m.sm3_dtype = amp_dtype(args)
    evaluator.to(dev)
    return evaluator.eval() if eval_mode else evaluator


# ---- batches ----------------------------------------------------------------------------------------------------------------
def image_store(args, modes, dev, size=None, name="backbone_eval"):
    """(the device image store of these splits, the chain `name` at `size`: --img-sz by default)."""
    from sm3hip.augment import chain
    from sm3hip.imagestore import build_for
    return build_for(args, modes, dev), chain(name, tuple(size or args.img_sz), args.mean, args.std)


def split_batches(args, store, split, aug, order=None, gen=None, whole=True, labels=True):
    """(derm, clinic, labels) of each batch of case indices of `order` (the whole split in its own order by default): one
    augmented view per modality, labels from the device; labels=False: (derm, clinic)."""
    if order is None:
        from src.utils.data.sampler import eval_batches
        order = eval_batches(len(split), args.batch_size)
    for sel in order:
        pair = tuple(store.augment(aug, ids[sel], gen, whole=whole)[0] for ids in (split.derm_ids, split.clinic_ids))
        if labels:
            pair += (split.labels.index_select(0, sel.to(split.labels.device, non_blocking=True)),)
        yield pair


def synthetic(bs, size, dev, gen):
    derm = torch.randn(bs, 3, size[0], size[1], device=dev, generator=gen)
    clinic = torch.randn(bs, 3, size[0], size[1], device=dev, generator=gen)
    labels = torch.stack([torch.randint(0, n, (bs,), device=dev, generator=gen) for n in NUM_CLASSES], dim=1)
    return derm, clinic, labels


def synthetic_batches(sizes, size, dev, gen):
    """One synthetic batch per entry of `sizes`, drawn from gen as it is consumed."""
    return (synthetic(bs, size, dev, gen) for bs in sizes)


# ---- test-time augmentation ---------------------------------------------------------------------------------------------------
def tta_pass(prefix, evaluator, args, epoch, dev, gen, store, split, size):
    """One pass of sm3hip.tta over the validation cases -- the split of the image store, or --val-steps further synthetic
    batches when store is None -- with the eval-mode model: prints prefix + "val-tta AUC_AVG ... | " + tta.stats_line and, with
    a store, saves val_predictions_tta.pt (val_predictions.pt's keys plus "tta").  Returns the record."""
    import os

    from sm3hip import tta
    from sm3hip.metrics import auc_avg
    evaluator.eval()
    if store is not None:
        rec = tta.predict_split(evaluator, store, split, tuple(size), args.mean, args.std, args.tta, args.tta_crops,
                                args.tta_crop_scale, args.batch_size)
    else:
        batches = list(synthetic_batches([args.batch_size] * args.val_steps, size, dev, gen))
        rec = tta.predict(evaluator, torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches]), args.tta,
                          chunk=args.batch_size)
        rec["targets"] = torch.cat([b[2] for b in batches])
    _, avg = auc_avg(rec["preds"], rec["targets"])
    rec["AUC_AVG"] = float(avg)
    if store is not None:
        torch.save({"epoch": epoch + 1, "preds": [p.cpu() for p in rec["preds"]], "targets": rec["targets"].cpu(),
                    "AUC_AVG": rec["AUC_AVG"], "tta": tta.tool_record(rec, args.tta_crop_scale)},
                   os.path.join(args.log_path, "val_predictions_tta.pt"))
    print(f"{prefix}val-tta AUC_AVG {rec['AUC_AVG']:.4f} | {tta.stats_line(rec)}", flush=True)
    return rec


# ---- robustness under image corruptions ---------------------------------------------------------------------------------------
def corrupt_pass(prefix, evaluator, args, epoch, store, split, size):
    """One pass of sm3hip.corrupt over the validation split of the image store per (--corrupt name, --corrupt-severity) with the
    eval-mode model: saves val_predictions_corrupt/<name>_<s>.pt (val_predictions.pt's keys plus "corrupt") and
    val_robustness.json / .csv under --log-path, prints prefix + one line per corruption and the summary.  Returns the report."""
    from sm3hip import corrupt
    from sm3hip.metrics import auc_avg
    evaluator.eval()
    rec = corrupt.predict_split(evaluator, store, split, tuple(size), args.mean, args.std, args.corrupt, args.corrupt_severity,
                                args.corrupt_modality, args.corrupt_seed, args.batch_size)
    out_dir = os.path.join(args.log_path, "val_predictions_corrupt")
    os.makedirs(out_dir, exist_ok=True)
    for (name, s), preds in rec["preds"].items():
        _, avg = auc_avg(preds, rec["targets"])
        torch.save({"epoch": epoch + 1, "preds": [p.cpu() for p in preds], "targets": rec["targets"].cpu(), "AUC_AVG": float(avg),
                    "corrupt": {"name": name, "severity": s, "modality": rec["modality"], "seed": rec["seed"]}},
                   os.path.join(out_dir, f"{name}_{s}.pt"))
    rep = corrupt.robustness_report(rec, bootstrap=args.bootstrap, confidence=args.confidence, seed=args.bootstrap_seed)
    corrupt.save(rep, args.log_path)
    for line in corrupt.stats_lines(rep) + [corrupt.stats_line(rep)]:
        print(prefix + "val-" + line, flush=True)
    return rep


# ---- features ---------------------------------------------------------------------------------------------------------------
def encode(evaluator, batches, normalize=False):
    """cat(derm_f, clinic_f) as float32 -- normalize=True: as unit rows (sm3hip.knn.normalize) -- and the labels of every
    batch, concatenated."""
    feats, labels = [], []
    for derm, clinic, lab in batches:
        f = torch.cat([evaluator.derm_backbone(derm), evaluator.clinic_backbone(clinic)], dim=1)
        feats.append(knn.normalize(f) if normalize else f.float())
        labels.append(lab)
    return torch.cat(feats).contiguous(), torch.cat(labels)


def random_features(n, d, dev, gen, normalize=False):
    labels = torch.stack([torch.randint(0, c, (n,), device=dev, generator=gen) for c in NUM_CLASSES], dim=1)
    f = torch.randn(n, d, device=dev, generator=gen)
    return (knn.normalize(f) if normalize else f), labels
