"""Per-label input-gradient (saliency) maps of a linear probe on MI355X: which pixels of the dermoscopic and the clinical
image drive each of the 8 derm7pt label predictions.

    python tools/backbone_saliency.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 32 -j 4 --img-sz 224 224 \
        --linear-path logs/eval/best_linear.pth --log-path logs/eval/saliency --split test --max-cases 64

Takes backbone_eval's command line (and its data helpers) plus --linear-path (backbone_eval's best_linear.pth, a Baseline
state_dict), --target, --split and --max-cases.  Every parameter is frozen and the model runs in eval mode; the images go
through the validation chain (Resize -> Normalize) and the encoders' backward is data-only (no weight gradients; the image
gradient comes from sm3_stem_dgrad_bn).  For label i the target is the logit of the argmax class (--target pred) or of the
class AUC_AVG scores (--target cls, sm3hip.metrics.CLS_WEIGHTS); its map is max_c |d logit / d x| of the derm and the clinic
image at network resolution.  One forward and backward per label.  saliency.pt goes to --log-path: maps [n, 8, 2, H, W]
fp16 (derm, clinic), logits (8 tensors [n, classes]), targets [n, 8], target_class [n, 8], indices [n] (positions in the
split; with --data-name synthetic, in the generated stream).
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
from sm3hip.metrics import CLASSES_NAME, CLS_WEIGHTS, NUM_CLASSES  # noqa: E402

TARGETS = ("pred", "cls")


def get_parser():
    p = backbone_eval.get_parser()
    p.description = "SM3 per-label input-gradient maps of a linear probe (MI355X)"
    p.add_argument("--linear-path", type=str, default=None,
                   help="backbone_eval's best_linear.pth (a Baseline state_dict); required with real data")
    p.add_argument("--target", default="pred", choices=TARGETS,
                   help="logit per label: pred = the argmax class, cls = the class AUC_AVG scores (CLS_WEIGHTS)")
    p.add_argument("--split", default="test", choices=("test", "valid"))
    p.add_argument("--max-cases", default=64, type=int, help="cases of the split (or synthetic images) to map")
    return p


def load_linear(model, path):
    """backbone_eval's best_linear.pth ({"state_dict": ...}) or a bare state_dict; a "module." prefix is dropped."""
    state = torch.load(path, map_location="cpu")
    state = state.get("state_dict", state)
    model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in state.items()})


def saliency_batch(model, derm, clinic, target_class):
    """maps [n, 8, 2, H, W] fp32 of max_c |d logit_i / d x| (i = label, target_class [n, 8]): one forward and backward per
    label.  Eval mode: each logit depends on its own image only, so the gradient of the batch sum is per image."""
    maps = []
    for i in range(len(NUM_CLASSES)):
        d = derm.detach().requires_grad_()
        c = clinic.detach().requires_grad_()
        logit = model([d, c])[i].gather(1, target_class[:, i:i + 1]).sum()
        gd, gc = torch.autograd.grad(logit, [d, c])
        maps.append(torch.stack([gd.abs().amax(dim=1), gc.abs().amax(dim=1)], dim=1))
    return torch.stack(maps, dim=1)


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from src.utils.misc import amp_dtype, ignored_line, require_baseline_arch, require_data
    require_baseline_arch(args.arch, "backbone_saliency")
    real = require_data(args, "backbone_saliency")
    if args.linear_path is not None and not os.path.isfile(args.linear_path):
        raise SystemExit(f"backbone_saliency: --linear-path {args.linear_path} does not exist")
    if real and args.linear_path is None:
        raise SystemExit("backbone_saliency: --linear-path (backbone_eval's best_linear.pth) is required with real data")
    if args.max_cases < 1:
        raise SystemExit("backbone_saliency: --max-cases must be at least 1")
    if ignored_line(args, parser, real):
        print("accepted for compatibility, without effect in this build:", " ".join(ignored_line(args, parser, real)), flush=True)
    from src.models.baseline import Baseline
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    model = Baseline(args.arch, args.arch_weights)
    if args.linear_path is not None:
        load_linear(model, args.linear_path)
        print(f"loaded linear probe from '{args.linear_path}'")
    for p in model.parameters():
        p.requires_grad_(False)
    for m in (model.derm_backbone, model.clinic_backbone):
        m.sm3_dtype = amp_dtype(args)
    model.to(dev).eval()
    if real:
        from sm3hip.augment import chain
        from sm3hip.imagestore import build_for
        from src.utils.data.sampler import eval_batches
        store = build_for(args, [args.split], dev)
        split = store.splits[args.split]
        n = min(args.max_cases, len(split))
        aug = chain("backbone_eval", tuple(args.img_sz), args.mean, args.std)
        sels = [s[s < n] for s in eval_batches(len(split), args.batch_size)]
        sels = [s for s in sels if s.numel()]
        data = backbone_eval.real_batches(store, split, aug, sels, None, True)
        indices = torch.cat(sels)
    else:
        n = args.max_cases
        sizes = [min(args.batch_size, n - s) for s in range(0, n, args.batch_size)]
        data = (backbone_eval.synthetic(b, args.img_sz, dev, gen) for b in sizes)
        indices = torch.arange(n)
    maps, logits, targets, tcls = [], [[] for _ in NUM_CLASSES], [], []
    torch.cuda.synchronize()
    t0 = time.time()
    for derm, clinic, lab in data:
        with torch.no_grad():
            outs = model([derm, clinic])
        if args.target == "pred":
            tc = torch.stack([o.argmax(dim=1) for o in outs], dim=1)
        else:
            tc = torch.tensor(CLS_WEIGHTS, dtype=torch.long, device=dev).expand(derm.shape[0], -1).contiguous()
        maps.append(saliency_batch(model, derm, clinic, tc).half().cpu())
        for i, o in enumerate(outs):
            logits[i].append(o.float().cpu())
        targets.append(lab.cpu())
        tcls.append(tc.cpu())
    torch.cuda.synchronize()
    seconds = time.time() - t0
    maps = torch.cat(maps)
    saved = {"maps": maps, "logits": [torch.cat(l) for l in logits], "targets": torch.cat(targets),
             "target_class": torch.cat(tcls), "indices": indices, "target": args.target, "labels": list(CLASSES_NAME),
             "split": args.split if real else "synthetic"}
    os.makedirs(args.log_path, exist_ok=True)
    torch.save(saved, os.path.join(args.log_path, "saliency.pt"))
    stat = {"cases": maps.shape[0], "images_per_s": 2 * maps.shape[0] / seconds, "seconds": seconds}  # derm + clinic
    print(f"saliency ({args.target}): {maps.shape[0]} cases x {len(NUM_CLASSES)} labels, maps "
          f"{tuple(maps.shape)} | {stat['images_per_s']:.1f} images/s", flush=True)
    return stat


if __name__ == "__main__":
    main()
