"""Integrated Gradients and SmoothGrad attributions of a linear probe on MI355X: which pixels of the dermoscopic and the clinical
image drive each of the 8 derm7pt label predictions (sm3hip/attr.py).

    python tools/backbone_attr.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 8 -j 4 --img-sz 224 224 \
        --linear-path logs/eval/best_linear.pth --log-path logs/eval/attr --method ig --steps 32 --split test --max-cases 64

Takes tools/backbone_cam.py's command line with --method ig|smoothgrad, --steps, --samples, --sigma, --squared, --attr-seed
and --chunk in the place of --cam-layer.  The model runs in eval mode on the validation chain (Resize -> Normalize); the IG
baseline is zero in normalised space (the dataset-mean image).  attr.pt goes to --log-path: maps [n, 8, 2, H, W] fp16 (the sum
over the colour channels of |attribution|; derm, clinic), logits (8 tensors [n, classes]), targets [n, 8], target_class [n, 8],
indices [n] and, for IG, delta [n, 8] fp64 (the completeness gap: sum of the attributions - (logit(x) - logit(baseline))).
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
from backbone_saliency import load_linear  # noqa: E402
from sm3hip.attr import METHODS  # noqa: E402
from sm3hip.cam import TARGETS  # noqa: E402
from sm3hip.metrics import CLASSES_NAME, NUM_CLASSES  # noqa: E402


def add_attr_args(p, method_help="ig (Integrated Gradients) or smoothgrad",
                  chunk_help="path points / samples per encoder forward (default: from the free device memory); any value gives "
                             "the same bits"):
    """The flags the two attribution tools share (the place --cam-layer takes in the Grad-CAM tools)."""
    p.add_argument("--target", default="pred", choices=TARGETS,
                   help="logit per label: pred = the argmax class, cls = the class AUC_AVG scores (CLS_WEIGHTS)")
    p.add_argument("--method", default="ig", help=method_help)
    p.add_argument("--steps", default=32, type=int, help="ig: points of the midpoint rule on the path from the baseline")
    p.add_argument("--samples", default=16, type=int, help="smoothgrad: noisy copies per image")
    p.add_argument("--sigma", default=0.15, type=float, help="smoothgrad: noise level relative to each image's max - min")
    p.add_argument("--squared", action="store_true", help="smoothgrad: average the squared gradients")
    p.add_argument("--attr-seed", default=0, type=int, help="smoothgrad: seed of the noise")
    p.add_argument("--chunk", default=None, type=int, help=chunk_help)
    p.add_argument("--split", default="test", choices=("test", "valid"))
    p.add_argument("--max-cases", default=64, type=int, help="cases of the split (or synthetic images) to attribute")
    return p


def check_attr_args(args, tool):
    """Refusals that need no device."""
    if args.method not in METHODS:
        raise SystemExit(f"{tool}: --method {args.method} is not available (one of {', '.join(METHODS)})")
    if args.max_cases < 1:
        raise SystemExit(f"{tool}: --max-cases must be at least 1")
    n = args.steps if args.method == "ig" else args.samples
    name = "--steps" if args.method == "ig" else "--samples"
    if n < 1:
        raise SystemExit(f"{tool}: {name} must be at least 1")
    if args.chunk is not None and not 1 <= args.chunk <= n:
        raise SystemExit(f"{tool}: --chunk must be between 1 and {name} ({n})")
    if args.sigma < 0:
        raise SystemExit(f"{tool}: --sigma must be non-negative")
    if args.attr_seed < 0:
        raise SystemExit(f"{tool}: --attr-seed must be non-negative")


def get_parser():
    p = backbone_eval.get_parser()
    p.description = "SM3 Integrated Gradients / SmoothGrad attributions of a linear probe (MI355X)"
    p.add_argument("--linear-path", type=str, default=None,
                   help="backbone_eval's best_linear.pth (a Baseline state_dict); required with real data")
    return add_attr_args(p)


def attribute(model, derm, clinic, args):
    from sm3hip.attr import integrated_gradients, smooth_grad
    if args.method == "ig":
        return integrated_gradients(model, derm, clinic, target=args.target, steps=args.steps, chunk=args.chunk)
    return smooth_grad(model, derm, clinic, target=args.target, samples=args.samples, sigma=args.sigma, squared=args.squared,
                       seed=args.attr_seed, chunk=args.chunk)


def run(model, data, args):
    """The attributions over the batches of `data`; the collected outputs (CPU) and the seconds it took."""
    maps, logits, targets, tcls, delta = [], [[] for _ in NUM_CLASSES], [], [], []
    torch.cuda.synchronize()
    t0 = time.time()
    for derm, clinic, lab in data:
        out = attribute(model, derm, clinic, args)
        maps.append(out["maps"].half().cpu())
        for i, o in enumerate(out["logits"]):
            logits[i].append(o.cpu())
        targets.append(lab.cpu())
        tcls.append(out["target_class"].cpu())
        if "delta" in out:
            delta.append(out["delta"].cpu())
    torch.cuda.synchronize()
    saved = {"maps": torch.cat(maps), "logits": [torch.cat(l) for l in logits], "targets": torch.cat(targets),
             "target_class": torch.cat(tcls)}
    if delta:
        saved["delta"] = torch.cat(delta)
    return saved, time.time() - t0


def save(saved, args, seconds, tool):
    os.makedirs(args.log_path, exist_ok=True)
    torch.save(saved, os.path.join(args.log_path, "attr.pt"))
    n = saved["maps"].shape[0]
    stat = {"cases": n, "images_per_s": 2 * n / seconds, "seconds": seconds}  # derm + clinic
    what = f"{args.steps} steps" if args.method == "ig" else f"{args.samples} samples, sigma {args.sigma}"
    print(f"{tool} ({args.method}, {what}, {args.target}): {n} cases x {len(NUM_CLASSES)} labels, maps "
          f"{tuple(saved['maps'].shape)} | {stat['images_per_s']:.2f} images/s", flush=True)
    if "delta" in saved:
        print(f"{tool}: completeness gap max |delta| = {float(saved['delta'].abs().max()):.3e}", flush=True)
    return stat


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from src.utils.misc import amp_dtype, ignored_line, require_baseline_arch, require_data
    require_baseline_arch(args.arch, "backbone_attr")
    check_attr_args(args, "backbone_attr")
    real = require_data(args, "backbone_attr")
    if args.linear_path is not None and not os.path.isfile(args.linear_path):
        raise SystemExit(f"backbone_attr: --linear-path {args.linear_path} does not exist")
    if real and args.linear_path is None:
        raise SystemExit("backbone_attr: --linear-path (backbone_eval's best_linear.pth) is required with real data")
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
    saved, seconds = run(model, data, args)
    saved.update(indices=indices, target=args.target, method=args.method, labels=list(CLASSES_NAME),
                 split=args.split if real else "synthetic")
    return save(saved, args, seconds, "backbone_attr")


if __name__ == "__main__":
    main()
