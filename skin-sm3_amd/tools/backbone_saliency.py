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

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import torch  # noqa: E402

import explain_cli as cli  # noqa: E402
from explain_cli import load_linear  # noqa: E402,F401  (kept reachable as backbone_saliency.load_linear)
from sm3hip.explain import target_class  # noqa: E402
from sm3hip.metrics import NUM_CLASSES  # noqa: E402


def get_parser():
    p = cli.backbone_parser("SM3 per-label input-gradient maps of a linear probe (MI355X)")
    return cli.add_cases_args(cli.add_target_arg(p))


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


def per_batch(model, derm, clinic, lab, args):
    with torch.no_grad():
        outs = model([derm, clinic])
    tc = target_class(outs, args.target, derm.shape[0], derm.device)
    return {"maps": saliency_batch(model, derm, clinic, tc).half(), "logits": [o.float() for o in outs], "targets": lab,
            "target_class": tc}


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    saved, stat = cli.explain(args, parser, "backbone_saliency", False, per_batch, "saliency.pt", freeze=True, target=args.target)
    print(f"saliency ({args.target}): {stat['cases']} cases x {len(NUM_CLASSES)} labels, maps "
          f"{tuple(saved['maps'].shape)} | {stat['images_per_s']:.1f} images/s", flush=True)
    return stat


if __name__ == "__main__":
    main()
