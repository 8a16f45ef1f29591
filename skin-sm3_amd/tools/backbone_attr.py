"""Integrated Gradients, SmoothGrad and RISE attributions of a linear probe on MI355X: which pixels of the dermoscopic and the
clinical image drive each of the 8 derm7pt label predictions (sm3hip/attr.py, sm3hip/rise.py).

    python tools/backbone_attr.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 8 -j 4 --img-sz 224 224 \
        --linear-path logs/eval/best_linear.pth --log-path logs/eval/attr --method ig --steps 32 --split test --max-cases 64

    python tools/backbone_attr.py ... --method rise --rise-masks 4000 --rise-cells 7 --rise-p 0.5 --attr-seed 0

Takes tools/backbone_cam.py's command line with --method ig|smoothgrad|rise, --steps, --samples, --sigma, --squared, --attr-seed,
--rise-masks, --rise-cells, --rise-p and --chunk in the place of --cam-layer.  The model runs in eval mode on the validation chain (Resize -> Normalize); the IG
baseline is zero in normalised space (the dataset-mean image).  attr.pt goes to --log-path: maps [n, 8, 2, H, W] fp16 (the sum
over the colour channels of |attribution|; derm, clinic), logits (8 tensors [n, classes]), targets [n, 8], target_class [n, 8],
indices [n] and, for IG, delta [n, 8] fp64 (the completeness gap: sum of the attributions - (logit(x) - logit(baseline))), for
RISE, scores [n, 8, masks] fp64 (the target class's probability under every mask; the masks are seeded by --attr-seed and are the
same for every case).
"""
import os
import sys

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import explain_cli as cli  # noqa: E402
from sm3hip import attr, rise  # noqa: E402
from sm3hip.metrics import NUM_CLASSES  # noqa: E402


def get_parser():
    return cli.add_attr_args(cli.backbone_parser(
        "SM3 Integrated Gradients / SmoothGrad / RISE attributions of a linear probe (MI355X)"))


def per_batch(model, derm, clinic, lab, args):
    if args.method == "ig":
        out = attr.integrated_gradients(model, derm, clinic, target=args.target, steps=args.steps, chunk=args.chunk)
    elif args.method == "rise":
        out = rise.rise(model, derm, clinic, target=args.target, masks=args.rise_masks, cells=args.rise_cells, p=args.rise_p,
                        seed=args.attr_seed, chunk=args.chunk)
    else:
        out = attr.smooth_grad(model, derm, clinic, target=args.target, samples=args.samples, sigma=args.sigma,
                               squared=args.squared, seed=args.attr_seed, chunk=args.chunk)
    got = {"maps": out["maps"].half(), "logits": out["logits"], "targets": lab, "target_class": out["target_class"]}
    for k in ("delta", "scores"):
        if k in out:
            got[k] = out[k]
    return got


def run(args, parser, tool, mlc):
    saved, stat = cli.explain(args, parser, tool, mlc, per_batch, "attr.pt",
                              check=lambda a, t: cli.check_attr_args(a, t, cli.image_size(a, mlc)), target=args.target,
                              method=args.method)
    what = {"ig": f"{args.steps} steps", "smoothgrad": f"{args.samples} samples, sigma {args.sigma}",
            "rise": f"{args.rise_masks} masks, {args.rise_cells} cells, p {args.rise_p}"}[args.method]
    print(f"{tool} ({args.method}, {what}, {args.target}): {stat['cases']} cases x {len(NUM_CLASSES)} labels, maps "
          f"{tuple(saved['maps'].shape)} | {stat['images_per_s']:.2f} images/s", flush=True)
    if "delta" in saved:
        print(f"{tool}: completeness gap max |delta| = {float(saved['delta'].abs().max()):.3e}", flush=True)
    return stat


def main(argv=None):
    parser = get_parser()
    return run(parser.parse_args(argv), parser, "backbone_attr", False)


if __name__ == "__main__":
    main()
